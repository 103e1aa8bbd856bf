/*
 * fa_gfx950_kvcache.h -- in-place KV-cache append with fused rotate-half RoPE for the MI355X (gfx950 /
 * CDNA4) FlashAttention-2 forward operator: the WRITE side of the cache that fa_gfx950_paged.h (page pool)
 * and fa_fwd_gfx950_padded (dense cache) read.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own so that FA_GFX950_ABI_VERSION and FA_GFX950_PAGED_VERSION do
 * not move. No reference counterpart (the reference has no KV cache); the semantics are the append half
 * of flash-attn's flash_attn_with_kvcache(q, k_cache, v_cache, k, v, rotary_cos, rotary_sin,
 * cache_seqlens, block_table).
 *
 * One launch, for every sequence b with len_b = clamp(seqlens_k[b], 0, cap), cap = max_pages * page_size:
 *
 *   - new token i (0 <= i < seqlen_new) has position n = len_b + i. K row i goes to row n % page_size of
 *     page block_table[b][n / page_size] of the K pool, rotated with table row min(n, max_pos - 1) when
 *     cos / sin are given; V row i goes to the same place of the V pool, unrotated;
 *   - a write is DROPPED, never redirected: a token with n >= cap is not written, and neither is one whose
 *     page id lies outside [0, num_pages). This is deliberately NOT the clamp of the read path
 *     (fa_gfx950_paged.h clamps page ids into the pool, which is harmless for a read): a clamped write
 *     would land in a page that belongs to another sequence;
 *   - seqlens_out[b] = min(len_b + seqlen_new, cap), written by exactly one thread per b. seqlens_out
 *     must not overlap seqlens_k (other workgroups of the launch are still reading seqlens_k; the check
 *     rejects an overlap of the two [B] address ranges);
 *   - q row i (0 <= i < seqlen_q) is rotated at position max(seqlens_out[b] - seqlen_q + i, 0), clamped
 *     to max_pos - 1 -- the sequence's LAST seqlen_q positions after the append, the convention of
 *     fa_fwd_gfx950_paged -- and written to q_out. q needs the tables;
 *   - table entries of pages that no new token lands in are never read; cache rows other than the ones
 *     written are never touched (not even read);
 *   - two sequences whose tables send a new token to the same physical row are the caller's error: which
 *     one stays is undefined.
 *
 * block_table == NULL describes a dense cache [B, Hkv, Smax, D]: page = batch row, page_size = Smax (any
 * positive value), max_pages = 1; num_pages is ignored. With a table, page_size is a multiple of 32 as in
 * fa_gfx950_paged.h.
 *
 * The rotation is fa_rope_gfx950's, bit for bit: out = fma(x, cos, rot * sin) in fp32, rot =
 * -x[d + D/2] (d < D/2) or x[d - D/2], one RNE rounding. cos / sin are [max_pos, D] tables of the k / q
 * dtype (the full-width rotate-half convention: both halves of a row are read).
 *
 * All strides are in ELEMENTS and the last dimension of every tensor is contiguous. When headdim is a
 * multiple of 16 and every base is 16-byte aligned and every stride a multiple of 8 elements, the kernel
 * moves 16 bytes per load / store; any other even (with tables) or arbitrary (without) headdim and
 * alignment takes an element path. Nothing is ever copied to fix alignment.
 */
#ifndef FA_GFX950_KVCACHE_H
#define FA_GFX950_KVCACHE_H

#include "fa_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_KVCACHE_VERSION 1

typedef struct fa_kvcache_params {
    /* new keys / values [B, Hkv, seqlen_new, D]; both NULL iff seqlen_new == 0 */
    const void *k_new, *v_new;
    int64_t kn_batch_stride, kn_head_stride, kn_seqlen_stride;
    int64_t vn_batch_stride, vn_head_stride, vn_seqlen_stride;
    /* optional queries [B, Hq, seqlen_q, D] and their rotated output; both NULL iff seqlen_q == 0 */
    const void *q;
    void *q_out;
    int64_t q_batch_stride, q_head_stride, q_seqlen_stride;
    int64_t qo_batch_stride, qo_head_stride, qo_seqlen_stride;
    /* optional RoPE tables [max_pos, D], both or neither; row r at r * cs_row_stride */
    const void *cos, *sin;
    int64_t cs_row_stride, max_pos;
    /* the cache, as fa_paged_params describes it: pool bases and page / head / row strides */
    void *k_cache, *v_cache;
    int64_t k_page_stride, k_head_stride, k_row_stride;
    int64_t v_page_stride, v_head_stride, v_row_stride;
    const int32_t *block_table; /* [B, max_pages], device; NULL: dense cache */
    int64_t block_table_stride; /* elements between rows */
    int64_t max_pages, num_pages, page_size;
    const int32_t *seqlens_k;   /* [B], device */
    int32_t *seqlens_out;       /* [B], device, or NULL; must not overlap seqlens_k */
    int64_t batch_size, num_heads_q, num_heads_kv, seqlen_new, seqlen_q, headdim;
} fa_kvcache_params;

/*
 * Launch the append on `stream`: K, V and q in ONE kernel. Asynchronous, no host synchronisation and no
 * allocation, safe under hipGraph capture (the table, the lengths and the inputs are read when the kernel
 * runs). Nothing is launched, and seqlens_out is not written, when batch_size == 0 or when there is
 * neither a new token nor a query (seqlen_new == 0 and seqlen_q == 0).
 */
int fa_kvcache_append_gfx950(const fa_kvcache_params *params, int dtype, void *stream);

/* Validate `params` exactly as fa_kvcache_append_gfx950 does, without touching the device (the device
 * arrays are not read). Host-only. */
int fa_kvcache_append_gfx950_check(const fa_kvcache_params *params, int dtype);

/* FA_GFX950_KVCACHE_VERSION of the loaded library. */
int fa_kvcache_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_KVCACHE_H */
