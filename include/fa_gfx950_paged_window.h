/*
 * fa_gfx950_paged_window.h -- sliding-window decode over the paged KV cache (16-bit and FP8 e4m3 pools)
 * for the MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator: fa_fwd_gfx950_paged and
 * fa_fwd_gfx950_paged_fp8 with the local window of fa_fwd_gfx950_window, applied per sequence. What
 * flash-attn's flash_attn_with_kvcache(..., window_size=(window_left, ...)) does on a paged cache, for
 * Mistral- / Qwen2-style models.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: FA_GFX950_ABI_VERSION, FA_GFX950_PAGED_VERSION,
 * FA_GFX950_KVCACHE_VERSION and FA_GFX950_FP8_VERSION do not move and the entry points of those headers are
 * untouched. The parameter structs are theirs.
 *
 * Semantics, for sequence b with L_b = clamp(seqlens_k[b], 0, max_pages * page_size) keys, Sq = seqlen_q (the
 * queries are the sequence's last Sq positions):
 *
 *     key n is visible to query m  iff  n >= m + L_b - Sq - window_left
 *                                  and, when causal, n <= m + L_b - Sq
 *
 * i.e. a window of window_left + 1 keys ending at the bottom-right diagonal (transformers' sliding_window W
 * is window_left = W - 1). window_left < 0 means no window: the call is then fa_fwd_gfx950_paged /
 * fa_fwd_gfx950_paged_fp8 itself, the same plan and the same bits. Every non-negative value is valid; values
 * above 2^30 count as 2^30, which covers any capacity. Rows that see no key are 0; L_b == 0 gives 0 rows.
 *
 * The window is relative to seqlen_q AS PASSED: a caller that packs the q-heads of a one-position decode step
 * into seqlen_q (head_q_per_group 1, seqlen_q = the group size, as fa_fwd_gfx950_paged's callers may) must
 * not do so here; pass seqlen_q 1 and head_q_per_group = the group size instead. The kernel and its
 * arithmetic are the same either way.
 *
 * What is read: with lo0_b = max(0, L_b - Sq - window_left), the lowest key any row of the sequence sees,
 * the kernel reads the 32-key tiles [lo0_b / 32, ceil(L_b / 32)) of the sequence and nothing else. Pages that
 * lie wholly below tile lo0_b / 32, and THEIR BLOCK-TABLE ENTRIES, ARE NEVER READ: an engine may free those
 * pages and leave anything in the entries. Keys of that first tile below a row's bound are read and masked;
 * they sit in a page that holds a visible key. Everything else is fa_gfx950_paged.h's: lengths and page ids
 * are clamped on the device, entries past a sequence's end and rows past it in its last page are never read.
 *
 * Split plan and workspace: the plan of fa_fwd_gfx950_paged (fa_fwd_gfx950_paged_fp8: with its own workgroup
 * target) made for min(max_pages * page_size, 32 * (ceil((window_left + seqlen_q) / 32) + 1)) keys, the most
 * a window can intersect, instead of the capacity; every split takes an equal share of the tiles its
 * sequence reads. The workspace follows that plan: never larger than the unwindowed entry's, equal to it
 * for window_left < 0 or a window that covers the capacity, 0 when the plan does not split.
 */
#ifndef FA_GFX950_PAGED_WINDOW_H
#define FA_GFX950_PAGED_WINDOW_H

#include "fa_gfx950.h"
#include "fa_gfx950_fp8.h"
#include "fa_gfx950_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_PAGED_WINDOW_VERSION 1

/*
 * Launch the windowed paged decode on `stream`. Asynchronous, no host synchronisation, safe under hipGraph
 * capture. Validation, the decode rule (head_q_per_group * seqlen_q <= 64, else FA_ERR_UNSUPPORTED) and the
 * workspace rules (NULL: unsplit; 16-byte aligned; smaller than _workspace_size: FA_ERR_INVALID_ARGUMENT) are
 * fa_fwd_gfx950_paged's.
 */
int fa_fwd_gfx950_paged_window(const fa_paged_params *params, int dtype, int causal, int64_t window_left,
                               void *workspace, int64_t workspace_bytes, void *stream);

/* Workspace bytes fa_fwd_gfx950_paged_window wants (0: no split; -1: invalid parameters). */
int64_t fa_fwd_gfx950_paged_window_workspace_size(const fa_paged_params *params, int dtype, int causal,
                                                  int64_t window_left);

/* Validate exactly as fa_fwd_gfx950_paged_window does (fa_fwd_gfx950_paged_check: every window_left is
 * valid), without touching the device. */
int fa_fwd_gfx950_paged_window_check(const fa_paged_params *params, int dtype, int causal, int64_t window_left);

/* The same three over an FP8 (e4m3) pool: fa_fwd_gfx950_paged_fp8 (include/fa_gfx950_fp8.h) with the window. */
int fa_fwd_gfx950_paged_window_fp8(const fa_paged_fp8_params *params, int dtype, int causal, int64_t window_left,
                                   void *workspace, int64_t workspace_bytes, void *stream);
int64_t fa_fwd_gfx950_paged_window_fp8_workspace_size(const fa_paged_fp8_params *params, int dtype, int causal,
                                                      int64_t window_left);
int fa_fwd_gfx950_paged_window_fp8_check(const fa_paged_fp8_params *params, int dtype, int causal,
                                         int64_t window_left);

/* FA_GFX950_PAGED_WINDOW_VERSION of the loaded library. */
int fa_paged_window_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_PAGED_WINDOW_H */
