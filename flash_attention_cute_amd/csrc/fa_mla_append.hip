// fa_mla_append.hip -- the write side of the paged latent (MLA) KV cache for gfx950 (C-ABI fa_mla_append_gfx950,
// include/fa_gfx950_mla_fp8.h): vLLM's concat_and_cache_mla under fa_kvcache.hip's placement and drop rules.
//
// Token i of sequence b goes to position n = len_b + i: its 512 compressed-KV columns and its 64 (already
// rotated) RoPE columns become the 576 columns of row n % page_size of page block_table[b][n / page_size]. A
// write at n >= max_pages * page_size or through a page id outside [0, num_pages) is dropped, never redirected;
// negative lengths count as 0; seqlens_out = min(len + seqlen_new, capacity) is written by the first B threads.
//
// One kernel, templated on the cache element: the input dtype (the bits are copied, 16 bytes a thread) or e4m3,
//
//     byte = e4m3_rne(clamp(fp32(x) / descale[b], -448, 448))
//
// with fa_kvcache_fp8.hip's arithmetic: an IEEE fp32 division (this file is built without fast-math
// reciprocals), the clamp in fp32 ahead of v_cvt_pk_fp8_f32 (nothing rests on the convert's overflow
// behaviour). An item is (b, i, chunk): a row is 72 chunks of 8 elements, 64 from c_kv and 8 from k_pe; one
// thread loads 16 bytes and stores 16 (16-bit) or 8 (e4m3), and consecutive lanes take consecutive chunks, so a
// row is one contiguous run of stores. Every page term is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_mla_fp8.h"
#include "fa_launch.h"

namespace fa {
namespace {

typedef uint32_t u32x4a __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2a __attribute__((ext_vector_type(2)));

constexpr int kLatCols = 576, kLatCkv = 512, kLatChunks = kLatCols / 8;  // 72 chunks of 8 elements

template <bool kF16>
__device__ __forceinline__ float ld16(const uint16_t v) {
    if constexpr (kF16) return (float)__builtin_bit_cast(_Float16, v);
    else return (float)__builtin_bit_cast(__bf16, v);
}

// 8 elements of the input dtype -> 8 e4m3 bytes: IEEE division, fp32 clamp, RNE convert
template <bool kF16>
__device__ __forceinline__ u32x2a quant8(const u32x4a v, const float descale) {
    const uint16_t *e = (const uint16_t *)&v;
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = fminf(fmaxf(ld16<kF16>(e[i]) / descale, -448.f), 448.f);
    u32x2a w;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int x = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i], f[4 * i + 1], 0, false);
        x = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i + 2], f[4 * i + 3], x, true);
        w[i] = (uint32_t)x;
    }
    return w;
}

// items: (b, i, chunk) row-major, n_items = B * seqlen_new * 72. Threads [0, B) also write seqlens_out (the
// launch has at least B threads).
template <bool kF16, bool kFp8>
__global__ __launch_bounds__(256) void fa_mla_append_kernel(const fa_mla_append_params p, const int64_t n_items) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t cap = p.max_pages * p.page_size;
    if (p.seqlens_out && i < p.batch_size) {
        int64_t len = p.seqlens_k[i];
        len = len < 0 ? 0 : len > cap ? cap : len;
        const int64_t out = len + p.seqlen_new;
        p.seqlens_out[i] = (int32_t)(out > cap ? cap : out);
    }
    if (i >= n_items) return;
    const int c = (int)(i % kLatChunks);
    const int64_t row = i / kLatChunks;
    const int64_t s = row % p.seqlen_new, b = row / p.seqlen_new;
    int64_t len = p.seqlens_k[b];
    len = len < 0 ? 0 : len > cap ? cap : len;
    const int64_t pos = len + s;
    if (pos >= cap) return;  // past the table's capacity: dropped
    const int64_t page = p.block_table[b * p.block_table_stride + pos / p.page_size];
    if (page < 0 || page >= p.num_pages) return;  // outside the pool: dropped, never clamped
    const int64_t dst = page * p.kv_page_stride + (pos % p.page_size) * p.kv_row_stride + 8 * c;
    const uint16_t *x = 8 * c < kLatCkv
                            ? (const uint16_t *)p.c_kv + b * p.ckv_batch_stride + s * p.ckv_seqlen_stride + 8 * c
                            : (const uint16_t *)p.k_pe + b * p.kpe_batch_stride + s * p.kpe_seqlen_stride +
                                  (8 * c - kLatCkv);
    const u32x4a v = *(const u32x4a *)x;
    if constexpr (kFp8) {
        const float descale = p.kv_descale ? p.kv_descale[b * p.kv_descale_stride] : 1.f;
        *(u32x2a *)((uint8_t *)p.kv_ptr + dst) = quant8<kF16>(v, descale);
    } else {
        *(u32x4a *)((uint16_t *)p.kv_ptr + dst) = v;
    }
}

int mla_append_check(const fa_mla_append_params *p, int dtype) {
    if (!p) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return set_err(FA_ERR_UNSUPPORTED, "the MLA append takes fp16 / bf16 rows only (dtype %d)", dtype);
    if (p->cache_dtype != dtype && p->cache_dtype != FA_MLA_CACHE_E4M3)
        return set_err(FA_ERR_UNSUPPORTED, "the latent cache must have the dtype of the new rows or be e4m3 (got %d)",
                       (int)p->cache_dtype);
    const bool fp8 = p->cache_dtype == FA_MLA_CACHE_E4M3;
    if (p->batch_size < 0 || p->seqlen_new < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "batch_size and seqlen_new must be non-negative");
    if (p->batch_size > 0x7fffffLL || p->seqlen_new > 0xffffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "batch or new rows too large");
    if (!p->kv_ptr || !p->block_table || !p->seqlens_k)
        return set_err(FA_ERR_INVALID_ARGUMENT, "kv, block_table and seqlens_k must be non-NULL");
    if (p->seqlen_new > 0 && (!p->c_kv || !p->k_pe))
        return set_err(FA_ERR_INVALID_ARGUMENT, "c_kv and k_pe must be non-NULL");
    if (((uintptr_t)p->block_table & 3) || ((uintptr_t)p->seqlens_k & 3) || ((uintptr_t)p->seqlens_out & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table, seqlens_k and seqlens_out must be 4-byte aligned");
    if (p->page_size <= 0) return set_err(FA_ERR_INVALID_ARGUMENT, "page_size must be positive");
    if (p->num_pages < 1 || p->max_pages < 1)
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_pages and max_pages must be at least 1");
    if (p->num_pages > 0x7fffffffLL || p->max_pages > 0x3fffffffLL / p->page_size)
        return set_err(FA_ERR_UNSUPPORTED, "page pool or block table too large");
    if (p->block_table_stride < 0 || (p->batch_size > 1 && p->block_table_stride < p->max_pages))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table_stride must be at least max_pages");
    const int64_t unit = fp8 ? 16 : 8;
    if (((uintptr_t)p->kv_ptr & 15) || ((uintptr_t)p->c_kv & 15) || ((uintptr_t)p->k_pe & 15))
        return set_err(FA_ERR_INVALID_ARGUMENT, "kv, c_kv and k_pe must be 16-byte aligned");
    if (p->kv_row_stride < kLatCols || p->kv_row_stride % unit != 0 || p->kv_page_stride < 0 ||
        p->kv_page_stride % unit != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT,
                       "the latent row stride (%lld) must be at least %d and, like the page stride, a multiple of %d",
                       (long long)p->kv_row_stride, kLatCols, (int)unit);
    const int64_t st[4] = {p->ckv_batch_stride, p->ckv_seqlen_stride, p->kpe_batch_stride, p->kpe_seqlen_stride};
    for (int i = 0; i < 4; ++i)
        if (st[i] < 0 || st[i] % 8 != 0)
            return set_err(FA_ERR_INVALID_ARGUMENT,
                           "the strides of c_kv and k_pe must be non-negative multiples of 8 elements");
    if (p->kv_descale_stride < 0) return set_err(FA_ERR_INVALID_ARGUMENT, "kv_descale_stride must be non-negative");
    if ((uintptr_t)p->kv_descale & 3)
        return set_err(FA_ERR_INVALID_ARGUMENT, "kv_descale must be a 4-byte aligned fp32 array");
    if (!fp8 && p->kv_descale)
        return set_err(FA_ERR_INVALID_ARGUMENT, "kv_descale is for an e4m3 latent cache only");
    return FA_OK;
}

int mla_append_launch(const fa_mla_append_params *params, int dtype, hipStream_t stream) {
    const int rc = mla_append_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_append_params &p = *params;
    if (p.batch_size == 0) return FA_OK;
    const int64_t items = p.batch_size * p.seqlen_new * kLatChunks;
    const int64_t threads = items > p.batch_size ? items : p.batch_size;
    const dim3 grid((uint32_t)((threads + 255) / 256));
    const bool f16 = dtype == FA_DTYPE_F16;
    if (p.cache_dtype == FA_MLA_CACHE_E4M3) {
        if (f16) hipLaunchKernelGGL((fa_mla_append_kernel<true, true>), grid, dim3(256), 0, stream, p, items);
        else hipLaunchKernelGGL((fa_mla_append_kernel<false, true>), grid, dim3(256), 0, stream, p, items);
    } else {  // the bits are copied: one instantiation serves both 16-bit dtypes
        hipLaunchKernelGGL((fa_mla_append_kernel<true, false>), grid, dim3(256), 0, stream, p, items);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

}  // namespace
}  // namespace fa

extern "C" int fa_mla_append_gfx950(const fa_mla_append_params *params, int dtype, void *stream) {
    return fa::mla_append_launch(params, dtype, (hipStream_t)stream);
}
extern "C" int fa_mla_append_gfx950_check(const fa_mla_append_params *params, int dtype) {
    return fa::mla_append_check(params, dtype);
}
