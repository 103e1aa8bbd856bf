/*
 * fa_gfx950_fp8.h -- FP8 (OCP e4m3, torch.float8_e4m3fn) KV cache for the MI355X (gfx950 / CDNA4)
 * FlashAttention-2 forward operator: a quantizing in-place append (the write side) and a split-KV paged
 * decode that reads the 8-bit pool in place (the read side). q and the output stay fp16 / bf16.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: FA_GFX950_ABI_VERSION, FA_GFX950_PAGED_VERSION and
 * FA_GFX950_KVCACHE_VERSION do not move, and the 16-bit entry points are untouched. No reference
 * counterpart; the cache format is the one of vLLM-style engines and of flash-attn's k_descale / v_descale.
 *
 * Scales are DESCALES: fp32, positive and finite, one per (batch row, kv-head), element (b, h) at
 * b * descale_batch_stride + h * descale_head_stride of a device array (any strides, 0 included: a single
 * value with both strides 0 is the per-tensor case). A NULL array means 1.0. They are read by the kernels,
 * never by the host. A non-positive or non-finite descale gives undefined values, never an out-of-bounds
 * access.
 *
 * Read, for sequence b and kv-head h (T = the q dtype, T(x) the exact widening of an e4m3 byte):
 *
 *     out = v_descale[b,h] * softmax((softmax_scale * k_descale[b,h]) * q . T(K8)^T) . T(V8)
 *
 * Every e4m3 value is exact in fp16 and in bf16, so this is "dequantize, then fa_fwd_gfx950_paged" with
 * the two scales folded into the softmax scale and the final normalisation. Everything else is
 * fa_gfx950_paged.h's: the queries are each sequence's last seqlen_q positions, causal masks are
 * bottom-right aligned per sequence, seqlens_k and page ids are clamped on the device, rows without a
 * visible key are 0, unused table entries and rows past a sequence's end are never read.
 *
 * Write, for new token i of sequence b at position n (fa_gfx950_kvcache.h's placement and drop rules):
 *
 *     byte = e4m3_rne(clamp(fp32(x) / descale[b,h], -448, 448))
 *
 * with x the rotated key ALREADY ROUNDED to the input dtype (bit for bit fa_rope_gfx950's value) for K and
 * the input for V; the clamp is done in fp32 before the conversion and the division is IEEE fp32. q rows
 * are rotated and stay 16-bit, seqlens_out as in fa_gfx950_kvcache.h.
 *
 * The cache is caller-owned and read / written in place, nothing is padded or copied, so: headdim is a
 * multiple of 16 and at most 128, the K / V pool bases are 16-byte aligned and their page / head / row
 * strides (in 1-byte ELEMENTS) multiples of 16; page_size is a multiple of 32 when there is a table.
 */
#ifndef FA_GFX950_FP8_H
#define FA_GFX950_FP8_H

#include "fa_gfx950.h"
#include "fa_gfx950_kvcache.h"
#include "fa_gfx950_paged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_FP8_VERSION 1

typedef struct fa_paged_fp8_params {
    fa_paged_params paged;      /* as for fa_fwd_gfx950_paged; k_ptr / v_ptr and the k / v strides
                                   describe 1-byte e4m3 elements, q / o the 16-bit `dtype` */
    const float *k_descale;     /* [B, Hkv] fp32, device, or NULL (1.0) */
    const float *v_descale;
    int64_t descale_batch_stride, descale_head_stride; /* elements, of both arrays */
} fa_paged_fp8_params;

/*
 * Launch the paged decode over an e4m3 pool on `stream`; `dtype` is the type of q and o. Asynchronous, no
 * host synchronisation, safe under hipGraph capture. Workspace rules and the decode rule
 * (head_q_per_group * seqlen_q <= 64, else FA_ERR_UNSUPPORTED) are fa_fwd_gfx950_paged's; the split plan is
 * its rule aiming at 256 workgroups (one per CU) instead of 160.
 */
int fa_fwd_gfx950_paged_fp8(const fa_paged_fp8_params *params, int dtype, int causal, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* Workspace bytes fa_fwd_gfx950_paged_fp8 wants (0: no split; -1: invalid parameters): units * n_split * 32
 * fp32 rows of the head-dim tile (64 / 128) plus one fp32 each, the layout of fa_fwd_gfx950_paged's, with
 * n_split from the plan above -- equal to fa_fwd_gfx950_paged_workspace_size of the same shape wherever the
 * workgroup target does not bind (short sequences, large batches). */
int64_t fa_fwd_gfx950_paged_fp8_workspace_size(const fa_paged_fp8_params *params, int dtype, int causal);

/* Validate `params` exactly as fa_fwd_gfx950_paged_fp8 does, without touching the device. */
int fa_fwd_gfx950_paged_fp8_check(const fa_paged_fp8_params *params, int dtype, int causal);

typedef struct fa_kvcache_fp8_params {
    fa_kvcache_params base;     /* as for fa_kvcache_append_gfx950; k_cache / v_cache and their strides
                                   describe 1-byte e4m3 elements, every other tensor the 16-bit `dtype` */
    const float *k_descale;     /* [B, Hkv] fp32, device, or NULL (1.0) */
    const float *v_descale;
    int64_t descale_batch_stride, descale_head_stride;
} fa_kvcache_fp8_params;

/* Launch the quantizing append on `stream`: K (rotated, then quantized), V (quantized) and q (rotated,
 * 16-bit) in ONE kernel; `dtype` is the type of k_new / v_new / q / the tables. Asynchronous, no host
 * synchronisation and no allocation, safe under hipGraph capture. */
int fa_kvcache_append_fp8_gfx950(const fa_kvcache_fp8_params *params, int dtype, void *stream);

/* Validate `params` exactly as fa_kvcache_append_fp8_gfx950 does, without touching the device. */
int fa_kvcache_append_fp8_gfx950_check(const fa_kvcache_fp8_params *params, int dtype);

/* FA_GFX950_FP8_VERSION of the loaded library. */
int fa_fp8_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_FP8_H */
