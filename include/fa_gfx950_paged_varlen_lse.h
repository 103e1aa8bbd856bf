/*
 * fa_gfx950_paged_varlen_lse.h -- the softmax log-sum-exp (LSE) from the ragged paged prefill
 * (fa_gfx950_paged_varlen.h, with or without the sinks of fa_gfx950_paged_varlen_sink.h) for the MI355X (gfx950 /
 * CDNA4) FlashAttention-2 forward operator: a prompt chunk's partial attention state (out, lse), which
 * fa_merge_states_gfx950 (fa_gfx950_lse.h) combines with the states of other key sets -- keys sharded over devices,
 * keys in two pools, a prefix that a group of sequences shares.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no existing version macro moves and no existing entry changes.
 * The query side, the pool, the table, the lengths, the masks and the never-read guarantees are
 * fa_gfx950_paged_varlen.h's, per sequence, and `out` has the bits of fa_fwd_gfx950_paged_varlen_sink (of
 * fa_fwd_gfx950_paged_varlen when `sinks` is NULL).
 *
 * With s_n = softmax_scale * q . k_n over the row's visible keys (causal and window rules unchanged), the LSE of
 * packed row i of q-head h, in natural-log units, is
 *
 *     lse = ln( sum_n exp(s_n) + exp(sinks[h]) ),
 *
 * written as one fp32 at lse_ptr[h * lse_head_stride + i * lse_row_stride].
 *
 *   - The sink term is 0 when `sinks` is NULL, or sinks[h] is -inf or at or below -1e30.
 *   - A row without a visible key and without a sink gets -inf (and out = 0).
 *   - A row without a visible key and with a sink gets lse = sinks[h] (and out = 0): the sink's weight over a
 *     zero value, which is what a later merge needs. A sink is therefore in exactly ONE of the states that are
 *     merged: pass `sinks` to one launch and NULL to the others.
 *   - Only the elements of rows in [clamp(cu_seqlens_q[b]), clamp(cu_seqlens_q[b + 1])) are written, for each b;
 *     nothing else of the array is touched.
 *
 * 16-bit pools and page sizes that are multiples of 64 only, as the entries without the LSE. Not built: the LSE from
 * the dense, padded, varlen and uniform paged-prefill entries, and FP8 pools in this kernel.
 */
#ifndef FA_GFX950_PAGED_VARLEN_LSE_H
#define FA_GFX950_PAGED_VARLEN_LSE_H

#include "fa_gfx950.h"
#include "fa_gfx950_paged_varlen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_PAGED_VARLEN_LSE_VERSION 1

typedef struct fa_paged_varlen_lse_params {
    fa_paged_varlen_params varlen; /* as for fa_fwd_gfx950_paged_varlen */
    const float *sinks;            /* [num_heads_q] fp32 device, 4-byte aligned, or NULL: no sinks */
    float *lse_ptr;                /* fp32 device, 4-byte aligned; element (h, row) at
                                      h * lse_head_stride + row * lse_row_stride, row = the packed q row */
    int64_t lse_head_stride, lse_row_stride; /* non-negative, element units; the row stride at most 2^20 */
} fa_paged_varlen_lse_params;

/*
 * The ragged paged prefill that also writes the LSE. Asynchronous, no host synchronisation, safe under hipGraph
 * capture. Validation is fa_fwd_gfx950_paged_varlen's (its codes and messages) plus: lse_ptr NULL or not 4-byte
 * aligned, a negative stride, a row stride above 2^20, or a non-NULL sinks that is not 4-byte aligned is
 * FA_ERR_INVALID_ARGUMENT. The launch keeps nothing in the workspace (_workspace_size is 0 and `workspace` may be
 * NULL); workspace_bytes below _workspace_size, a negative one included, is FA_ERR_INVALID_ARGUMENT.
 * total_q == 0 launches nothing.
 */
int fa_fwd_gfx950_paged_varlen_lse(const fa_paged_varlen_lse_params *params, int dtype, int causal,
                                   int64_t window_left, void *workspace, int64_t workspace_bytes, void *stream);

/* Workspace bytes fa_fwd_gfx950_paged_varlen_lse wants (0; -1: invalid parameters). Host-only. */
int64_t fa_fwd_gfx950_paged_varlen_lse_workspace_size(const fa_paged_varlen_lse_params *params, int dtype, int causal,
                                                      int64_t window_left);

/* Validate exactly as fa_fwd_gfx950_paged_varlen_lse does, without touching the device:
 * fa_fwd_gfx950_paged_varlen_check (called, not copied), then the rules of this header. */
int fa_fwd_gfx950_paged_varlen_lse_check(const fa_paged_varlen_lse_params *params, int dtype, int causal);

/* FA_GFX950_PAGED_VARLEN_LSE_VERSION of the loaded library. */
int fa_paged_varlen_lse_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_PAGED_VARLEN_LSE_H */
