/*
 * fa_gfx950_mla_sparse.h -- sparse MLA decode: attention over top-k token indices of the paged latent KV
 * cache, for the MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator.
 *
 * An addition to the boundary of fa_gfx950_mla.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no existing version macro moves and no existing entry changes.
 * No reference counterpart; the call is the attention core of DeepSeek Sparse Attention (DeepSeek-V3.2):
 * a lightning indexer picks, for every query token, the `topk` cache positions the token may attend to, and
 * absorbed-query MLA runs over exactly those rows (FlashMLA's flash_mla_with_kvcache(..., indices=)). With
 * seqlen_q > 1 and one list per prompt token it is also that model's prefill.
 *
 *   - q, o, kv (the pool [num_pages, page_size, 576]), block_table, seqlens_k, lse, softmax_scale, num_splits
 *     and the workspace: exactly as in fa_gfx950_mla.h (16-bit q and pool of one dtype; seqlens_k clamped to
 *     [0, max_pages * page_size] and page ids into [0, num_pages) on the device; page_size a multiple of 32,
 *     the row stride a multiple of 8; softmax_scale is the caller's scale TIMES log2(e));
 *   - indices: int32 [B, Sq, topk] on the device, last stride 1, batch and position strides in ELEMENTS. The
 *     kernel reads a list 32 entries at a time with 128-byte scalar loads, so the base must be 4-byte aligned
 *     and topk a positive multiple of 32 (the caller pads with -1); anything else is FA_ERR_INVALID_ARGUMENT.
 *     Negative strides are FA_ERR_INVALID_ARGUMENT, topk above 2^24 is FA_ERR_UNSUPPORTED;
 *   - an entry is a LOGICAL position of sequence b (what the indexer produces); the kernel translates it
 *     through block_table on the device: position n is row n % page_size of page block_table[b][n / page_size];
 *   - visibility: entry j of (b, pos) is a key of that position's rows iff 0 <= idx <= lim, where
 *     lim = seqlens_k[b] - 1 without `causal` and min(seqlens_k[b] - 1, pos + seqlens_k[b] - seqlen_q) with it
 *     (the dense kernel's bottom-right limit). Every other value (-1, INT32_MAX, >= seqlens_k[b], beyond the
 *     causal limit) is not a key: no pool row is read for it, no block-table entry is looked up with it, and
 *     it contributes exactly nothing, whatever the pool holds there. (Its lookup slot reads block_table[b][0],
 *     and only in a 32-entry tile that has a visible entry, that is when the sequence has that page.);
 *   - the list is unsorted; a duplicate entry counts once per occurrence;
 *   - o [B, Hq, Sq, 512]; a row with no visible entry is 0, its lse -inf. lse is the natural-log convention of
 *     fa_gfx950_lse.h: the states of a list sharded over devices go straight into fa_merge_states_gfx950;
 *   - addressing is 64-bit: a pool may span more than 2^32 bytes;
 *   - num_splits: 0 lets the plan choose the splits of a list's topk / 32 tiles, n >= 1 forces n (capped at
 *     256). A plan with more than one split needs `workspace` of fa_mla_sparse_decode_gfx950_ws_bytes()
 *     bytes, 16-byte aligned: num_splits * B * Hq * Sq * (512 * 4 + 4).
 */
#ifndef FA_GFX950_MLA_SPARSE_H
#define FA_GFX950_MLA_SPARSE_H

#include "fa_gfx950_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_MLA_SPARSE_VERSION 1

typedef struct fa_mla_sparse_params {
    fa_mla_params base;     /* every field as in fa_gfx950_mla.h */
    const int32_t *indices; /* [B, Sq, topk], device */
    int64_t topk;
    int64_t indices_batch_stride, indices_seqlen_stride;
} fa_mla_sparse_params;

/* Launch on `stream`: the sparse decode kernel, and fa_mla_decode's combine kernel when the plan splits the
 * lists. Asynchronous, no host synchronisation, safe under hipGraph capture. */
int fa_mla_sparse_decode_gfx950(const fa_mla_sparse_params *params, int dtype, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* Validate `params` exactly as fa_mla_sparse_decode_gfx950 does, without touching the device. */
int fa_mla_sparse_decode_gfx950_check(const fa_mla_sparse_params *params, int dtype);

/* Workspace bytes of the plan (0: one split; -1: invalid parameters). Host-only. */
int64_t fa_mla_sparse_decode_gfx950_ws_bytes(const fa_mla_sparse_params *params);

/* FA_GFX950_MLA_SPARSE_VERSION of the loaded library. */
int fa_mla_sparse_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_MLA_SPARSE_H */
