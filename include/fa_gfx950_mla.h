/*
 * fa_gfx950_mla.h -- multi-head latent attention (MLA) decode over a paged latent KV cache, for the
 * MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no existing version macro moves and no existing entry changes.
 * No reference counterpart; the call is the decode step of DeepSeek-V2 / V3 / R1 and Kimi-K2 with absorbed
 * queries (FlashMLA's flash_mla_with_kvcache).
 *
 * One latent stream per sequence, shared by every q-head: a pool of pages [num_pages, page_size, 576] given
 * by ELEMENT strides (page, row; the last dimension contiguous). A row is the key (all 576 columns: 512
 * compressed-KV columns, then 64 RoPE columns) AND the value (its first 512 columns). Sequence b's key n is
 * row n % page_size of page block_table[b][n / page_size]; it has seqlens_k[b] keys. The pool is read in
 * place, each 32-key tile once per (batch, key split, group of 64 query rows).
 *
 *   - q [B, Hq, Sq, 576] (the absorbed queries q_nope W_UK || q_pe), o [B, Hq, Sq, 512], by element strides,
 *     last dimension contiguous, bases 16-byte aligned and strides multiples of 8;
 *   - page_size is a multiple of 32 (the key tile: a tile never straddles a page); the row stride is a
 *     multiple of 8 and at least 576;
 *   - seqlens_k[b] is clamped to [0, max_pages * page_size] and every page id into [0, num_pages) on the
 *     device; table entries of pages a sequence does not reach and pool rows past its end are never read;
 *   - the queries are each sequence's LAST seqlen_q positions: with `causal`, key n is visible to query m iff
 *     n <= m + seqlens_k[b] - seqlen_q. A row without a visible key gives o = 0 and lse = -inf;
 *   - softmax_scale is the caller's scale TIMES log2(e) (as fa_fwd_params.softmax_scale), finite and > 0.
 *     There is no default: 576 ** -0.5 is wrong for every model that uses this layout;
 *   - lse (or NULL): fp32 [B, Hq, Sq] by element strides, ln sum_n exp(scale q . k_n), natural log -- the
 *     convention of fa_gfx950_lse.h, so partial states go straight into fa_merge_states_gfx950;
 *   - num_splits: 0 lets the plan choose the key splits, n >= 1 forces n (capped at 256). A plan with more
 *     than one split needs `workspace` of fa_mla_decode_gfx950_ws_bytes() bytes, 16-byte aligned.
 *
 * Only (headdim_qk, headdim_v) = (576, 512) is built; anything else is FA_ERR_UNSUPPORTED.
 */
#ifndef FA_GFX950_MLA_H
#define FA_GFX950_MLA_H

#include "fa_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_MLA_VERSION 1

typedef struct fa_mla_params {
    const void *q_ptr;
    const void *kv_ptr;
    void *o_ptr;
    float *lse_ptr;             /* or NULL */
    const int32_t *block_table; /* [B, max_pages], device */
    const int32_t *seqlens_k;   /* [B], device */
    int64_t batch_size, num_heads_q, seqlen_q, headdim_qk, headdim_v;
    int64_t q_batch_stride, q_head_stride, q_seqlen_stride;
    int64_t o_batch_stride, o_head_stride, o_seqlen_stride;
    int64_t lse_batch_stride, lse_head_stride, lse_seqlen_stride;
    int64_t kv_page_stride, kv_row_stride;
    int64_t num_pages, page_size, max_pages, block_table_stride;
    int64_t num_splits;
    float softmax_scale;
    int32_t causal;
} fa_mla_params;

/* Launch on `stream`: the decode kernel, and the combine kernel when the plan splits the keys. Asynchronous,
 * no host synchronisation, safe under hipGraph capture. */
int fa_mla_decode_gfx950(const fa_mla_params *params, int dtype, void *workspace, int64_t workspace_bytes,
                         void *stream);

/* Validate `params` exactly as fa_mla_decode_gfx950 does, without touching the device. */
int fa_mla_decode_gfx950_check(const fa_mla_params *params, int dtype);

/* Workspace bytes of the plan (0: one split; -1: invalid parameters). Host-only. */
int64_t fa_mla_decode_gfx950_ws_bytes(const fa_mla_params *params);

/* FA_GFX950_MLA_VERSION of the loaded library. */
int fa_mla_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_MLA_H */
