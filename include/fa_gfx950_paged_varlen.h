/*
 * fa_gfx950_paged_varlen.h -- ragged query blocks over the paged KV cache for the MI355X (gfx950 / CDNA4)
 * FlashAttention-2 forward operator: one step of a continuous batch, a prompt chunk of one sequence beside a
 * short tail of another, in ONE launch of the paged prefill kernel with the pool read in place. What
 * flash-attn's flash_attn_varlen_func(..., block_table=...) gives an engine.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no other version moves and the entry points of the other headers
 * are untouched. The pool, the table and the lengths are fa_gfx950_paged.h's fa_paged_params with the same
 * meaning; what changes is the query side:
 *
 *   - q / o are PACKED [total_q, Hq, D]: row r of q-head h at q_ptr + r * q_seqlen_stride + h * q_head_stride
 *     (elements; the last dimension contiguous, every stride a multiple of 8, the bases 16-byte aligned, so a
 *     slice of a fused QKV projection is read in place). base.q_batch_stride / o_batch_stride are ignored;
 *   - sequence b owns rows [cu_seqlens_q[b], cu_seqlens_q[b + 1]) (int32 [batch_size + 1], device). Both
 *     bounds are clamped on the device, q0 = clamp(cu[b], 0, total_q), q1 = clamp(cu[b + 1], q0, total_q), so a
 *     bad array never reads or writes outside q / o. Rows of o outside every sequence's range are not written;
 *   - base.seqlen_q is max_seqlen_q, a host-side UPPER BOUND of every Sq_b = q1 - q0 that sizes the grid
 *     (ceil(max_seqlen_q / 256) q-tiles per sequence and q-head). Larger than the true maximum only launches
 *     empty q-tiles; smaller leaves the rows past it unwritten.
 *
 * Semantics are fa_gfx950_paged_prefill.h's, PER SEQUENCE with its own Sq_b: with L_b = clamp(seqlens_k[b], 0,
 * max_pages * page_size), the rows are the sequence's LAST Sq_b positions and
 *
 *     key n is visible to query m  iff  (window_left < 0 or n >= m + L_b - Sq_b - window_left)
 *                                  and, when causal, n <= m + L_b - Sq_b
 *
 * Rows that see no key are 0. Sq_b == 0 and L_b == 0 are valid. The never-read guarantees hold per sequence:
 * table entries at or past ceil(L_b / page_size) are never read, and with a window the pages wholly below
 * max(0, L_b - Sq_b - window_left) / 64 * 64, and their entries, are never read. Page ids are clamped into the
 * pool. page_size is a multiple of 64; 16-bit pools only.
 *
 * The result is bit-identical to fa_fwd_gfx950_varlen(_window) on the gathered keys packed densely: the same
 * kernel body walks the same 256-row blocks and 64-key tiles in the same order. Every sequence costs at least
 * one 256-row block per q-head: a batch of one-token sequences belongs to fa_fwd_gfx950_paged.
 */
#ifndef FA_GFX950_PAGED_VARLEN_H
#define FA_GFX950_PAGED_VARLEN_H

#include "fa_gfx950.h"
#include "fa_gfx950_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_PAGED_VARLEN_VERSION 1

typedef struct fa_paged_varlen_params {
    fa_paged_params paged;       /* base.seqlen_q = max_seqlen_q; q / o batch strides ignored */
    const int32_t *cu_seqlens_q; /* [batch_size + 1], device */
    int64_t total_q;             /* rows of q / o */
} fa_paged_varlen_params;

/*
 * Launch on `stream`. Asynchronous, no host synchronisation, safe under hipGraph capture (cu_seqlens_q, the
 * table, the lengths and the pool are read when the kernel runs). The launch keeps nothing in the workspace
 * (_workspace_size is 0 and `workspace` may be NULL); workspace_bytes below _workspace_size, a negative one
 * included, is FA_ERR_INVALID_ARGUMENT. total_q == 0 launches nothing.
 */
int fa_fwd_gfx950_paged_varlen(const fa_paged_varlen_params *params, int dtype, int causal, int64_t window_left,
                               void *workspace, int64_t workspace_bytes, void *stream);

/* Workspace bytes fa_fwd_gfx950_paged_varlen wants (-1: invalid parameters). Host-only. */
int64_t fa_fwd_gfx950_paged_varlen_workspace_size(const fa_paged_varlen_params *params, int dtype, int causal,
                                                  int64_t window_left);

/*
 * Validate `params` exactly as fa_fwd_gfx950_paged_varlen does, without touching the device: the rules of
 * fa_fwd_gfx950_paged_prefill_check (called, not copied) on the packed layout, plus cu_seqlens_q non-NULL and
 * 4-byte aligned, 0 <= total_q < 2^31 and max_seqlen_q (base.seqlen_q) < 2^30.
 */
int fa_fwd_gfx950_paged_varlen_check(const fa_paged_varlen_params *params, int dtype, int causal);

/* FA_GFX950_PAGED_VARLEN_VERSION of the loaded library. */
int fa_paged_varlen_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_PAGED_VARLEN_H */
