/*
 * fa_gfx950_mla_mixed.h -- sparse MLA decode and append on the MIXED FP8 latent row of DeepSeek-V3.2, for the
 * MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator.
 *
 * An addition to the boundary of fa_gfx950_mla_sparse.h and fa_gfx950_mla_fp8.h (same library, same conventions,
 * error codes and fa_last_error()), versioned on its own: no existing version macro moves and no existing entry
 * changes. The row is the one FlashMLA's sparse decode reads and vLLM calls fp8_ds_mla, 656 bytes a token:
 *
 *     [  0, 512)  the 512 compressed-KV columns as OCP e4m3
 *     [512, 528)  four fp32 scales, little endian; scale j covers columns [128 j, 128 j + 128): value = e4m3 * scale[j]
 *     [528, 656)  the 64 RoPE columns as bf16, not quantised
 *
 * 1. fa_mla_sparse_mixed_decode_gfx950: fa_mla_sparse_decode_gfx950 over a pool [num_pages, page_size, 656] of such
 *    rows, gathered in place. The parameter block is fa_mla_sparse_params with these differences:
 *      - base.kv_ptr is the byte pool; base.kv_page_stride and base.kv_row_stride count BYTES. The base is 16-byte
 *        aligned, the row stride at least 656, and both strides multiples of 16;
 *      - `dtype` (of q and o) is FA_DTYPE_BF16; anything else is FA_ERR_UNSUPPORTED;
 *      - headdim_qk / headdim_v stay 576 / 512: the row dequantises to 576 columns, the first 512 are the value.
 *    The result is that of the bf16 sparse call over the dequantised rows, to that call's own accuracy (the scale
 *    of a 128-column tile is applied in fp32 to the tile's partial score and, on the value side, to P before its
 *    rounding to bf16). Everything else is the contract of fa_gfx950_mla_sparse.h: logical indices translated on
 *    the device, the visibility rule, no pool byte read for an entry that is not a key (scales included), topk a
 *    positive multiple of 32, 64-bit addressing, num_splits, the workspace layout and ITS SIZE (the plan is the
 *    16-bit sparse entry's), the LSE convention, no host synchronisation, safe under hipGraph capture.
 *
 * 2. fa_mla_append_mixed_gfx950: fa_mla_append_gfx950's placement and drop rules (fa_gfx950_mla_fp8.h), writing
 *    mixed rows. Per token and 128-column tile j of c_kv: scale[j] = max(amax_j / 448, FLT_MIN) in fp32 (vLLM's
 *    rule), byte = e4m3_rne(clamp(fp32(x) / scale[j], -448, 448)) with an IEEE division, then the four scales and
 *    the bits of the ALREADY rotated k_pe. A dropped token writes nothing. The parameter block is
 *    fa_mla_append_params with cache_dtype == FA_MLA_CACHE_MIXED, kv_descale NULL (the row carries its scales;
 *    anything else is FA_ERR_INVALID_ARGUMENT), `dtype` FA_DTYPE_BF16, the cache strides in bytes, multiples of 16,
 *    the row stride at least 656.
 */
#ifndef FA_GFX950_MLA_MIXED_H
#define FA_GFX950_MLA_MIXED_H

#include "fa_gfx950_mla_fp8.h"
#include "fa_gfx950_mla_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_MLA_MIXED_VERSION 1

/* bytes of a mixed latent row */
#define FA_MLA_MIXED_ROW_BYTES 656

/* cache_dtype of fa_mla_append_params for a pool of mixed rows */
#define FA_MLA_CACHE_MIXED 9

/* Launch on `stream`: the mixed-row sparse decode kernel, and fa_mla_decode's combine kernel when the plan splits
 * the lists. Asynchronous, no host synchronisation, safe under hipGraph capture. */
int fa_mla_sparse_mixed_decode_gfx950(const fa_mla_sparse_params *params, int dtype, void *workspace,
                                      int64_t workspace_bytes, void *stream);

/* Validate `params` exactly as fa_mla_sparse_mixed_decode_gfx950 does, without touching the device. */
int fa_mla_sparse_mixed_decode_gfx950_check(const fa_mla_sparse_params *params, int dtype);

/* Workspace bytes of the plan (0: one split; -1: invalid parameters). Host-only. */
int64_t fa_mla_sparse_mixed_decode_gfx950_ws_bytes(const fa_mla_sparse_params *params);

/* One launch on `stream`; asynchronous, no host synchronisation, safe under hipGraph capture. */
int fa_mla_append_mixed_gfx950(const fa_mla_append_params *params, int dtype, void *stream);

/* Validate `params` exactly as fa_mla_append_mixed_gfx950 does, without touching the device. */
int fa_mla_append_mixed_gfx950_check(const fa_mla_append_params *params, int dtype);

/* FA_GFX950_MLA_MIXED_VERSION of the loaded library. */
int fa_mla_mixed_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_MLA_MIXED_H */
