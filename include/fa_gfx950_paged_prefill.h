/*
 * fa_gfx950_paged_prefill.h -- prefill-sized query blocks over the paged KV cache for the MI355X (gfx950 /
 * CDNA4) FlashAttention-2 forward operator: block-table attention on the prefill kernel (fa_fwd_w4), the pool
 * read in place. What a chunked prefill over a cached prefix, a prefix-cache hit or a long speculative block
 * needs from flash-attn's flash_attn_with_kvcache(..., block_table=...).
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: FA_GFX950_ABI_VERSION, FA_GFX950_PAGED_VERSION,
 * FA_GFX950_KVCACHE_VERSION, FA_GFX950_FP8_VERSION and FA_GFX950_PAGED_WINDOW_VERSION do not move and the
 * entry points of those headers are untouched. The parameter struct is fa_gfx950_paged.h's fa_paged_params,
 * with the same meaning: a pool [num_pages, Hkv, page_size, D] given by element strides, sequence b's key n
 * in row n % page_size of page block_table[b][n / page_size], seqlens_k[b] keys.
 *
 * Semantics are those of fa_fwd_gfx950_paged and fa_fwd_gfx950_paged_window, for sequence b with L_b =
 * clamp(seqlens_k[b], 0, max_pages * page_size) keys and Sq = seqlen_q (the queries are the sequence's LAST Sq
 * positions):
 *
 *     key n is visible to query m  iff  (window_left < 0 or n >= m + L_b - Sq - window_left)
 *                                  and, when causal, n <= m + L_b - Sq
 *
 * Rows that see no key are 0 (causal with L_b < Sq: the first Sq - L_b rows); L_b == 0 gives 0 rows.
 * window_left < 0 is no window; values above 2^30 count as 2^30, which covers any capacity.
 *
 *   - page_size is a multiple of 64 (the prefill kernel's key tile: a tile never straddles a page). Other
 *     multiples of 32 are valid pools for the decode entries but FA_ERR_UNSUPPORTED here: the caller gathers
 *     the pages and uses fa_fwd_gfx950_padded, as it does for FP8 pools, which this entry does not read;
 *   - ANY head_q_per_group * seqlen_q: this entry always runs the prefill kernel (one workgroup per 256
 *     query rows of a q-head). The caller picks: fa_fwd_gfx950_paged / _paged_window for decode shapes
 *     (head_q_per_group * seqlen_q <= 64), this entry above;
 *   - seqlens_k[b] is clamped to [0, max_pages * page_size] on the device and every page id into
 *     [0, num_pages); the page term of an address is 64-bit, offsets inside a page are bounded to 32 bits by
 *     _check;
 *   - what is read: the 64-key tiles [j_lo, n_end) of each 256-row query block, where n_end is the block's
 *     last visible tile (ceil(L_b / 64), or the causal diagonal's) and j_lo the tile of the lowest key its
 *     first row sees (0 without a window). A table row is indexed only at [j_lo * 64 / page_size,
 *     (n_end - 1) * 64 / page_size]: entries at or past ceil(L_b / page_size) are never read, and with a
 *     window the PAGES WHOLLY BELOW max(0, L_b - Sq - window_left) / 64 * 64, AND THEIR TABLE ENTRIES, ARE
 *     NEVER READ (the guarantee of fa_gfx950_paged_window.h). Rows of a last page past L_b are cut by the
 *     descriptor bound and never read from memory. L_b == 0 reads no entry at all;
 *   - the result is bit-identical to fa_fwd_gfx950_padded (window_left the same) on the gathered dense cache
 *     with k_start = 0, k_end = seqlens_k: the same tiles in the same order through the same arithmetic.
 */
#ifndef FA_GFX950_PAGED_PREFILL_H
#define FA_GFX950_PAGED_PREFILL_H

#include "fa_gfx950.h"
#include "fa_gfx950_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_PAGED_PREFILL_VERSION 1

/*
 * Launch the paged prefill on `stream`. Asynchronous, no host synchronisation, safe under hipGraph capture
 * (the table, the lengths and the pool are read when the kernel runs). The launch keeps nothing in the
 * workspace today (_workspace_size is 0 and `workspace` may be NULL), but the rule is the other entries':
 * workspace_bytes below _workspace_size, a negative one included, is FA_ERR_INVALID_ARGUMENT.
 */
int fa_fwd_gfx950_paged_prefill(const fa_paged_params *params, int dtype, int causal, int64_t window_left,
                                void *workspace, int64_t workspace_bytes, void *stream);

/* Workspace bytes fa_fwd_gfx950_paged_prefill wants (-1: invalid parameters). Host-only. */
int64_t fa_fwd_gfx950_paged_prefill_workspace_size(const fa_paged_params *params, int dtype, int causal,
                                                   int64_t window_left);

/*
 * Validate `params` exactly as fa_fwd_gfx950_paged_prefill does, without touching the device. The pool, the
 * table and the strides take fa_fwd_gfx950_paged_check (called, not copied; its decode-shape rule is asked of
 * a one-position, one-q-head-per-group copy, since this entry has no such rule) and q / o take
 * fa_fwd_gfx950_check; for a decode-shaped parameter set the result is fa_fwd_gfx950_paged_check's. New here:
 * page_size % 64 != 0 and a page whose rows span 2^31 bytes or more are FA_ERR_UNSUPPORTED.
 */
int fa_fwd_gfx950_paged_prefill_check(const fa_paged_params *params, int dtype, int causal);

/* FA_GFX950_PAGED_PREFILL_VERSION of the loaded library. */
int fa_paged_prefill_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_PAGED_PREFILL_H */
