/*
 * fa_gfx950_lse.h -- softmax log-sum-exp (LSE) output of the paged split-KV decode, and the merge of partial
 * attention states, for the MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no existing version macro moves and no existing entry changes.
 * No reference counterpart; the LSE is flash-attn's `return_softmax_lse`, the merge vLLM's
 * `merge_attn_states` / flashinfer's `merge_state`.
 *
 * With the LSE, attention results over DISJOINT key sets can be combined exactly: shared-prefix (cascade)
 * decode -- the prefix pages streamed once per group of sequences instead of once per sequence -- and
 * sequence-sharded decode across devices are both "run the decode on each key set, then fa_merge_states".
 *
 * LSE: one fp32 per (batch, q-head, position) row, element (b, h, m) at b * lse_batch_stride + h *
 * lse_head_stride + m * lse_seqlen_stride of `lse_ptr`:
 *
 *     lse = ln sum_n exp(scale * q . k_n)   over the row's visible keys, NATURAL log units,
 *
 * with scale = softmax_scale (as the caller means it, i.e. base.softmax_scale / log2(e)), times
 * k_descale[b, h] for an FP8 pool; v_descale does not enter. A row that sees no key gets -inf (its O is 0).
 * O is bit-identical to fa_fwd_gfx950_paged / _paged_fp8 on the same parameters.
 *
 * Two length options, so that a shared-prefix call needs no helper kernels:
 *
 *   - seqlen_offset: sequence b has L_b = clamp(seqlens_k[b] + seqlen_offset, 0, max_pages * page_size)
 *     keys; |seqlen_offset| <= 2^30;
 *   - seqlens_k == NULL: every sequence has clamp(seqlen_offset, 0, max_pages * page_size) keys.
 *
 * Everything else is fa_gfx950_paged.h's and fa_gfx950_fp8.h's (clamping, what is never read, the decode
 * rule head_q_per_group * seqlen_q <= 64, the workspace rules). There is no windowed LSE variant: the
 * entries take window_left for symmetry with fa_gfx950_paged_window.h and return FA_ERR_UNSUPPORTED for
 * window_left >= 0.
 */
#ifndef FA_GFX950_LSE_H
#define FA_GFX950_LSE_H

#include "fa_gfx950.h"
#include "fa_gfx950_fp8.h"
#include "fa_gfx950_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_LSE_VERSION 1

/* Most partial states one fa_merge_states_gfx950 call merges (a node of 8 devices, twice over). */
#define FA_MERGE_MAX_PARTS 16

typedef struct fa_paged_lse_params {
    fa_paged_params paged;      /* as for fa_fwd_gfx950_paged, except that seqlens_k may be NULL */
    float *lse_ptr;             /* [B, Hq, Sq] fp32, device, 4-byte aligned, by element strides */
    int64_t lse_batch_stride, lse_head_stride, lse_seqlen_stride; /* non-negative */
    int64_t seqlen_offset;
} fa_paged_lse_params;

typedef struct fa_paged_fp8_lse_params {
    fa_paged_fp8_params fp8;    /* as for fa_fwd_gfx950_paged_fp8, except that paged.seqlens_k may be NULL */
    float *lse_ptr;
    int64_t lse_batch_stride, lse_head_stride, lse_seqlen_stride;
    int64_t seqlen_offset;
} fa_paged_fp8_lse_params;

/*
 * The paged decode that also writes the LSE. Asynchronous, no host synchronisation, safe under hipGraph
 * capture. window_left < 0: no window; window_left >= 0: FA_ERR_UNSUPPORTED. Workspace as for
 * fa_fwd_gfx950_paged / _paged_fp8 (NULL: unsplit), of _workspace_size() bytes -- the same plan and the same
 * bytes as the entry without the LSE.
 */
int fa_fwd_gfx950_paged_lse(const fa_paged_lse_params *params, int dtype, int causal, int64_t window_left,
                            void *workspace, int64_t workspace_bytes, void *stream);
int64_t fa_fwd_gfx950_paged_lse_workspace_size(const fa_paged_lse_params *params, int dtype, int causal,
                                               int64_t window_left);
int fa_fwd_gfx950_paged_lse_check(const fa_paged_lse_params *params, int dtype, int causal, int64_t window_left);

int fa_fwd_gfx950_paged_lse_fp8(const fa_paged_fp8_lse_params *params, int dtype, int causal, int64_t window_left,
                                void *workspace, int64_t workspace_bytes, void *stream);
int64_t fa_fwd_gfx950_paged_lse_fp8_workspace_size(const fa_paged_fp8_lse_params *params, int dtype, int causal,
                                                   int64_t window_left);
int fa_fwd_gfx950_paged_lse_fp8_check(const fa_paged_fp8_lse_params *params, int dtype, int causal,
                                      int64_t window_left);

/*
 * fa_merge_states_gfx950: merge num_parts partial attention states over disjoint key sets.
 *
 *   outs  [N, B, Hq, Sq, D] of `dtype`, element strides (part, batch, head, seq), last dimension contiguous;
 *         base 16-byte aligned and every stride a multiple of 8 elements (16-byte loads)
 *   lses  [N, B, Hq, Sq] fp32, element strides (part, batch, head, seq), 4-byte aligned
 *   out   [B, Hq, Sq, D] of `dtype`, strides (batch, head, seq), aligned as outs; may not overlap outs
 *   lse   [B, Hq, Sq] fp32 by strides, or NULL
 *
 * Per row: Mx = max_i lse_i, w_i = exp(lse_i - Mx) (0 for lse_i = -inf), out = sum_i w_i o_i / sum_i w_i in
 * fp32, rounded once; lse = Mx + ln sum_i w_i. A row whose parts are all -inf gives out = 0, lse = -inf.
 * headdim % 8 == 0, 1 <= num_parts <= FA_MERGE_MAX_PARTS. One memory-bound pass, no workspace, no host
 * synchronisation, safe under hipGraph capture.
 */
typedef struct fa_merge_params {
    const void *outs;
    const float *lses;
    void *out;
    float *lse;                 /* or NULL */
    int64_t num_parts, batch_size, num_heads, seqlen, headdim;
    int64_t outs_part_stride, outs_batch_stride, outs_head_stride, outs_seqlen_stride;
    int64_t lses_part_stride, lses_batch_stride, lses_head_stride, lses_seqlen_stride;
    int64_t out_batch_stride, out_head_stride, out_seqlen_stride;
    int64_t lse_batch_stride, lse_head_stride, lse_seqlen_stride;
} fa_merge_params;

int fa_merge_states_gfx950(const fa_merge_params *params, int dtype, void *stream);
int fa_merge_states_gfx950_check(const fa_merge_params *params, int dtype);

/* FA_GFX950_LSE_VERSION of the loaded library. */
int fa_lse_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_LSE_H */
