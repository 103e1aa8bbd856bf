/*
 * fa_gfx950_kvcache_varlen.h -- ragged in-place KV-cache append with fused rotate-half RoPE for the MI355X
 * (gfx950 / CDNA4) FlashAttention-2 forward operator: the write side of one step of a continuous batch, where
 * every sequence brings its own number of new tokens. The read side is fa_gfx950_paged_varlen.h.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no other version moves and fa_gfx950_kvcache.h is untouched. The
 * rules are that header's TO THE LETTER, with a per-sequence token count in place of seqlen_new / seqlen_q.
 * For every sequence b with len_b = clamp(seqlens_k[b], 0, cap), cap = max_pages * page_size:
 *
 *   - k_new / v_new are PACKED [total_new, Hkv, D]. Sequence b owns rows [n0, n1), n0 = clamp(cu_seqlens_new[b],
 *     0, total_new), n1 = clamp(cu_seqlens_new[b + 1], n0, total_new): a bad array never reads outside them;
 *   - token i of sequence b (row n0 + i) has position n = len_b + i. Its K row goes to row n % page_size of
 *     page block_table[b][n / page_size], rotated with table row min(n, max_pos - 1) when cos / sin are given;
 *     its V row goes to the same place of the V pool, unrotated;
 *   - a write is DROPPED, never redirected: a token with n >= cap is not written, and neither is one whose
 *     page id lies outside [0, num_pages);
 *   - seqlens_out[b] = min(len_b + (n1 - n0), cap), written by exactly one thread per b; it must not overlap
 *     seqlens_k;
 *   - q is PACKED [total_q, Hq, D] with its own cu_seqlens_q (clamped the same way against total_q). Row i of
 *     sequence b's Sq_b rows is rotated at max(seqlens_out[b] - Sq_b + i, 0), clamped to max_pos - 1 -- the
 *     sequence's LAST Sq_b positions after the append, the convention of fa_fwd_gfx950_paged_varlen -- and
 *     written to q_out (packed, its own strides). q needs the tables;
 *   - table entries of pages that no new token lands in are never read; cache rows other than the ones written
 *     are never touched (not even read); rows of q_out outside every sequence's range are not written.
 *
 * Paged 16-bit caches only: block_table is required and page_size is a multiple of 32. The rotation is
 * fa_rope_gfx950's, bit for bit. All strides are in ELEMENTS and the last dimension of every tensor is
 * contiguous; the 16-byte path and the element paths are chosen as in fa_gfx950_kvcache.h.
 */
#ifndef FA_GFX950_KVCACHE_VARLEN_H
#define FA_GFX950_KVCACHE_VARLEN_H

#include "fa_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_KVCACHE_VARLEN_VERSION 1

typedef struct fa_kvcache_varlen_params {
    /* new keys / values [total_new, Hkv, D]; both NULL iff total_new == 0 */
    const void *k_new, *v_new;
    int64_t kn_row_stride, kn_head_stride;
    int64_t vn_row_stride, vn_head_stride;
    const int32_t *cu_seqlens_new; /* [B + 1], device */
    int64_t total_new;
    /* optional queries [total_q, Hq, D] and their rotated output; both NULL iff total_q == 0 */
    const void *q;
    void *q_out;
    int64_t q_row_stride, q_head_stride;
    int64_t qo_row_stride, qo_head_stride;
    const int32_t *cu_seqlens_q; /* [B + 1], device; NULL iff total_q == 0 */
    int64_t total_q;
    /* optional RoPE tables [max_pos, D], both or neither; row r at r * cs_row_stride */
    const void *cos, *sin;
    int64_t cs_row_stride, max_pos;
    /* the page pool, as fa_paged_params describes it */
    void *k_cache, *v_cache;
    int64_t k_page_stride, k_head_stride, k_row_stride;
    int64_t v_page_stride, v_head_stride, v_row_stride;
    const int32_t *block_table; /* [B, max_pages], device */
    int64_t block_table_stride; /* elements between rows */
    int64_t max_pages, num_pages, page_size;
    const int32_t *seqlens_k;   /* [B], device */
    int32_t *seqlens_out;       /* [B], device, or NULL; must not overlap seqlens_k */
    int64_t batch_size, num_heads_q, num_heads_kv, headdim;
} fa_kvcache_varlen_params;

/*
 * Launch the append on `stream`: K, V and q in ONE kernel over the packed rows (a row finds its sequence by a
 * binary search of the cumulative array). Asynchronous, no host synchronisation and no allocation, safe under
 * hipGraph capture. Nothing is launched when batch_size == 0.
 */
int fa_kvcache_append_varlen_gfx950(const fa_kvcache_varlen_params *params, int dtype, void *stream);

/* Validate `params` exactly as fa_kvcache_append_varlen_gfx950 does, without touching the device. Host-only. */
int fa_kvcache_append_varlen_gfx950_check(const fa_kvcache_varlen_params *params, int dtype);

/* FA_GFX950_KVCACHE_VARLEN_VERSION of the loaded library. */
int fa_kvcache_varlen_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_KVCACHE_VARLEN_H */
