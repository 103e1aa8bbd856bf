/*
 * fa_gfx950_mla_prefill.h -- multi-head latent attention (MLA) prefill over packed sequences, for the
 * MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no existing version macro moves and no existing entry changes.
 * No reference counterpart; the call is the prompt pass of DeepSeek-V2 / V3 / R1 and Kimi-K2 in the
 * NON-absorbed form: per head 192 key / query columns (128 "nope", then 64 RoPE) and 128 value columns.
 *
 *   out[t, h, :] = softmax_n(scale q[t, h, :192] . k[n, h / g, :192]) v[n, h / g, :128],  g = Hq / Hkv,
 *
 * per sequence of a packed batch:
 *
 *   - q [total_q, Hq, 192], o [total_q, Hq, 128], v [total_k, Hkv, 128] by ELEMENT strides (row, head; the last
 *     dimension contiguous), one 16-bit dtype, bases 16-byte aligned, strides non-negative multiples of 8;
 *   - a key row is TWO column ranges, each with a base and (row, head) strides of its own: columns 0 .. 127 from
 *     k_nope_ptr, columns 128 .. 191 from k_rope_ptr. One tensor k [total_k, Hkv, 192] is k_rope_ptr =
 *     k_nope_ptr + 128 elements with the same strides; a RoPE stream shared by every head is a head stride 0;
 *   - cu_seqlens_q, cu_seqlens_k: int32 [B + 1] on the device, clamped there to [0, total] and to
 *     non-decreasing. Sequence b's queries are its LAST Sq_b positions: with `causal`, key n is visible to
 *     query m iff n <= m + Sk_b - Sq_b. Sq_b != Sk_b is allowed either way;
 *   - max_seqlen_q sizes the grid (blocks of 128 rows up to 128, of 256 above): rows of a sequence past the
 *     blocks it gives are not computed and their o / lse not written;
 *   - nothing outside a sequence reaches the result: a key tile that overhangs a sequence's end reads zeros,
 *     never the next sequence's rows or the bytes past total_k;
 *   - softmax_scale is the caller's scale TIMES log2(e) (as fa_fwd_params.softmax_scale), finite and > 0.
 *     There is no default: with YaRN it is not 192 ** -0.5;
 *   - a row without a visible key gives o = 0 and lse = -inf;
 *   - lse (or NULL): fp32 [Hq, total_q] by element strides, ln sum_n exp(scale q . k_n), natural log -- the
 *     packed-state layout of fa_merge_states_gfx950 (fa_gfx950_lse.h), so the causal pass over a new chunk and
 *     the non-causal pass over the cached context merge as they are.
 *
 * Only (headdim_qk, headdim_v) = (192, 128) is built; anything else is FA_ERR_UNSUPPORTED.
 */
#ifndef FA_GFX950_MLA_PREFILL_H
#define FA_GFX950_MLA_PREFILL_H

#include "fa_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_MLA_PREFILL_VERSION 1

typedef struct fa_mla_prefill_params {
    const void *q_ptr;
    const void *k_nope_ptr; /* key columns 0 .. 127 */
    const void *k_rope_ptr; /* key columns 128 .. 191 */
    const void *v_ptr;
    void *o_ptr;
    float *lse_ptr;              /* or NULL */
    const int32_t *cu_seqlens_q; /* [B + 1], device */
    const int32_t *cu_seqlens_k; /* [B + 1], device */
    int64_t batch_size, total_q, total_k, max_seqlen_q;
    int64_t num_heads_q, num_heads_kv, headdim_qk, headdim_v;
    int64_t q_row_stride, q_head_stride;
    int64_t k_nope_row_stride, k_nope_head_stride;
    int64_t k_rope_row_stride, k_rope_head_stride;
    int64_t v_row_stride, v_head_stride;
    int64_t o_row_stride, o_head_stride;
    int64_t lse_head_stride, lse_row_stride;
    float softmax_scale;
    int32_t causal;
} fa_mla_prefill_params;

/* Launch on `stream`: one kernel. Asynchronous, no host synchronisation, safe under hipGraph capture. */
int fa_mla_prefill_gfx950(const fa_mla_prefill_params *params, int dtype, void *stream);

/* Validate `params` exactly as fa_mla_prefill_gfx950 does, without touching the device. */
int fa_mla_prefill_gfx950_check(const fa_mla_prefill_params *params, int dtype);

/* FA_GFX950_MLA_PREFILL_VERSION of the loaded library. */
int fa_mla_prefill_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_MLA_PREFILL_H */
