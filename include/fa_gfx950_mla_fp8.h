/*
 * fa_gfx950_mla_fp8.h -- the FP8 (OCP e4m3) latent KV cache of the MLA decode, and the latent cache's write
 * side, for the MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator.
 *
 * An addition to the boundary of fa_gfx950_mla.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no existing version macro moves and no existing entry changes.
 *
 * 1. fa_mla_decode_fp8_gfx950: fa_mla_decode_gfx950 over a pool of e4m3 BYTES, read in place. `base` is the
 *    16-bit call's parameter block with these differences:
 *      - kv_ptr is [num_pages, page_size, 576] bytes; kv_page_stride and kv_row_stride count bytes (elements).
 *        The base is 16-byte aligned, the row stride at least 576 and both strides multiples of 16;
 *      - `dtype` is the dtype of q and o (fp16 / bf16), which stay 16-bit;
 *      - kv_descale (device, fp32, or NULL for 1.0) holds one DESCALE per batch row at element stride
 *        kv_descale_stride >= 0 (0: one scalar for the batch). It is read on the device:
 *            out = descale * softmax((softmax_scale * descale) * q . T(kv8)^T) . T(kv8)[:, :512]
 *            lse = ln sum_n exp(softmax_scale * descale * q . T(kv8)_n)
 *        where T widens a byte to the q dtype (exact: every e4m3 value is a fp16 and a bf16 value). The result
 *        is that of the 16-bit call over the dequantised pool, to the 16-bit call's own accuracy.
 *    Everything else is the contract of fa_gfx950_mla.h: lengths and page ids clamped on the device, nothing read
 *    that a sequence does not reach (rows past its end read as 0, whatever bytes the pool holds), bottom-right
 *    `causal`, any num_heads_q * seqlen_q, num_splits, the workspace layout and its size rule, the LSE
 *    convention, no host synchronisation, safe under hipGraph capture.
 *
 * 2. fa_mla_append_gfx950: appends seqlen_new latent rows per sequence to the paged latent cache (vLLM's
 *    concat_and_cache_mla under fa_kvcache_append_gfx950's rules). Token i of sequence b goes to position
 *    n = max(seqlens_k[b], 0) + i: c_kv[b, i, 0..511] to columns 0..511 and k_pe[b, i, 0..63] (ALREADY rotated) to
 *    columns 512..575 of row n % page_size of page block_table[b][n / page_size].
 *      - a write at n >= max_pages * page_size, or through a page id outside [0, num_pages), is dropped, never
 *        redirected; seqlens_out[b] (or NULL) = min(max(seqlens_k[b], 0) + seqlen_new, max_pages * page_size), a
 *        NEW array (seqlens_k is not written);
 *      - cache_dtype == `dtype` (FA_DTYPE_F16 / FA_DTYPE_BF16): the bits are copied; strides count elements;
 *      - cache_dtype == FA_MLA_CACHE_E4M3: byte = e4m3_rne(clamp(fp32(x) / descale[b], -448, 448)), an IEEE
 *        division; the cache strides count bytes and are multiples of 16, kv_descale as above;
 *      - c_kv / k_pe by element strides (batch, token), last dimension contiguous, bases 16-byte aligned and
 *        strides multiples of 8; the cache base 16-byte aligned, its strides multiples of 8 (16 for e4m3).
 */
#ifndef FA_GFX950_MLA_FP8_H
#define FA_GFX950_MLA_FP8_H

#include "fa_gfx950_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_MLA_FP8_VERSION 1

/* cache_dtype of fa_mla_append_params for an e4m3 pool (the 16-bit values are FA_DTYPE_F16 / FA_DTYPE_BF16) */
#define FA_MLA_CACHE_E4M3 8

typedef struct fa_mla_fp8_params {
    fa_mla_params base;
    const float *kv_descale; /* device, or NULL for 1.0 */
    int64_t kv_descale_stride;
} fa_mla_fp8_params;

typedef struct fa_mla_append_params {
    void *kv_ptr;               /* [num_pages, page_size, 576], 16-bit or e4m3 */
    const void *c_kv;           /* [B, seqlen_new, 512] */
    const void *k_pe;           /* [B, seqlen_new, 64] */
    const int32_t *block_table; /* [B, max_pages], device */
    const int32_t *seqlens_k;   /* [B], device */
    int32_t *seqlens_out;       /* [B], device, or NULL */
    const float *kv_descale;    /* device, or NULL for 1.0 (e4m3 only) */
    int64_t kv_descale_stride;
    int64_t batch_size, seqlen_new;
    int64_t ckv_batch_stride, ckv_seqlen_stride;
    int64_t kpe_batch_stride, kpe_seqlen_stride;
    int64_t kv_page_stride, kv_row_stride;
    int64_t num_pages, page_size, max_pages, block_table_stride;
    int32_t cache_dtype;
} fa_mla_append_params;

/* Launch on `stream`, as fa_mla_decode_gfx950. */
int fa_mla_decode_fp8_gfx950(const fa_mla_fp8_params *params, int q_dtype, void *workspace, int64_t workspace_bytes,
                             void *stream);

/* Validate `params` exactly as fa_mla_decode_fp8_gfx950 does, without touching the device. */
int fa_mla_decode_fp8_gfx950_check(const fa_mla_fp8_params *params, int q_dtype);

/* Workspace bytes of the plan (0: one split; -1: invalid parameters). Host-only. */
int64_t fa_mla_decode_fp8_gfx950_ws_bytes(const fa_mla_fp8_params *params);

/* One launch on `stream`; asynchronous, no host synchronisation, safe under hipGraph capture. `dtype` is the
 * dtype of c_kv and k_pe. */
int fa_mla_append_gfx950(const fa_mla_append_params *params, int dtype, void *stream);

/* Validate `params` exactly as fa_mla_append_gfx950 does, without touching the device. */
int fa_mla_append_gfx950_check(const fa_mla_append_params *params, int dtype);

/* FA_GFX950_MLA_FP8_VERSION of the loaded library. */
int fa_mla_fp8_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_MLA_FP8_H */
