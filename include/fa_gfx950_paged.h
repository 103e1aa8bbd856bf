/*
 * fa_gfx950_paged.h -- paged KV-cache decode for the MI355X (gfx950 / CDNA4) FlashAttention-2
 * forward operator: block-table attention on the split-KV decode kernel.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own so that FA_GFX950_ABI_VERSION does not move.
 * No reference counterpart (the reference has neither a KV cache nor a split-KV kernel); the layout is
 * the one of vLLM-style engines and flash-attn's flash_attn_with_kvcache(..., block_table=...).
 *
 * The KV cache is a pool of fixed-size pages, [num_pages, Hkv, page_size, D] given by ELEMENT strides
 * (page, head, row; the last dimension contiguous), so any stride order works -- flash-attn's
 * [num_pages, page_size, Hkv, D] is a transposed view. Sequence b's key n is row n % page_size of page
 * block_table[b][n / page_size]; it has seqlens_k[b] keys, positions [0, seqlens_k[b]). The kernel
 * reads the pool in place: no gather into a dense tensor.
 *
 *   - page_size is a multiple of 32 (the kernel's key tile: a tile never straddles a page);
 *   - seqlens_k[b] is clamped to [0, max_pages * page_size] on the device, and every page id into
 *     [0, num_pages), so neither can address outside the table row or the pool (the policy of
 *     fa_fwd_gfx950_padded's range clamping);
 *   - table entries of pages past ceil(seqlens_k[b] / page_size) are never read, and rows of a last
 *     page past the sequence end are never read from memory: stale data there cannot reach the output;
 *   - the queries are each sequence's LAST seqlen_q positions: causal masking is bottom-right aligned
 *     per sequence (key n visible to query m iff n <= m + seqlens_k[b] - seqlen_q), rows with no
 *     visible key are 0, seqlens_k[b] == 0 gives 0 rows;
 *   - decode shapes only: head_q_per_group * seqlen_q <= 64 (the rule of the split-KV decode kernel,
 *     after the Sq == 1 q-head pack if the caller applies it). Larger query blocks return
 *     FA_ERR_UNSUPPORTED: the caller gathers the pages and uses fa_fwd_gfx950_padded.
 */
#ifndef FA_GFX950_PAGED_H
#define FA_GFX950_PAGED_H

#include "fa_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_PAGED_VERSION 1

typedef struct fa_paged_params {
    fa_fwd_params base;         /* q / o dense as for fa_fwd_gfx950. k_ptr / v_ptr = pool bases,
                                   k/v_batch_stride = PAGE stride, k/v_head_stride, k/v_seqlen_stride
                                   within a page. seqlen_kv = max_pages * page_size */
    const int32_t *block_table; /* [B, max_pages], device */
    int64_t block_table_stride; /* elements between rows */
    int64_t max_pages, num_pages, page_size;
    const int32_t *seqlens_k;   /* [B], device */
} fa_paged_params;

/*
 * Launch the paged decode on `stream`. Asynchronous, no host synchronisation, safe under hipGraph
 * capture (the table, the lengths and the pool are read when the kernel runs). Workspace as for
 * fa_fwd_gfx950_padded's decode path: NULL runs every (batch, kv-head) unsplit; otherwise it must hold
 * fa_fwd_gfx950_paged_workspace_size() bytes (16-byte aligned; a smaller one is an error) and the keys
 * are split over more workgroups, every split taking an equal share of its sequence's tiles. The result
 * is bit-identical to fa_fwd_gfx950_padded on the gathered dense cache with k_start = 0, k_end =
 * seqlens_k.
 */
int fa_fwd_gfx950_paged(const fa_paged_params *params, int dtype, int causal, void *workspace,
                        int64_t workspace_bytes, void *stream);

/* Workspace bytes fa_fwd_gfx950_paged wants (0: no split; -1: invalid parameters): those of
 * fa_fwd_gfx950_padded for dense k / v of max_pages * page_size keys. Host-only. */
int64_t fa_fwd_gfx950_paged_workspace_size(const fa_paged_params *params, int dtype, int causal);

/* Validate `params` exactly as fa_fwd_gfx950_paged does, without touching the device (the device
 * arrays are not read). */
int fa_fwd_gfx950_paged_check(const fa_paged_params *params, int dtype, int causal);

/* FA_GFX950_PAGED_VERSION of the loaded library. */
int fa_paged_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_PAGED_H */
