// fa_mla_append_mixed.hip -- the write side of a paged latent cache of MIXED rows for gfx950 (C-ABI
// fa_mla_append_mixed_gfx950, include/fa_gfx950_mla_mixed.h): fa_mla_append.hip's placement and drop rules, writing
// the 656-byte row of DeepSeek-V3.2's FP8 cache (512 e4m3 bytes, four fp32 tile scales, 64 bf16 RoPE columns).
//
// One wave64 per token: lane l loads c_kv columns 8 l .. 8 l + 7 (16 bytes), so the 16 lanes 16 j .. 16 j + 15 hold
// 128-column tile j. Per tile
//
//     scale = max(amax / 448, FLT_MIN)                        (amax: a 4-step xor reduction over the 16 lanes)
//     byte  = e4m3_rne(clamp(fp32(x) / scale, -448, 448))
//
// with fa_mla_append.hip's arithmetic: IEEE fp32 divisions (this file is built without fast-math reciprocals), the
// clamp in fp32 ahead of v_cvt_pk_fp8_f32. A lane stores its 8 bytes (the row's first 512 bytes are one contiguous
// run of the wave's stores), the first lane of each tile its scale, and lanes 0 .. 7 copy the 128 bytes of the
// already rotated k_pe. The drop decision is wave-uniform: a dropped token writes nothing. Every page term is 64-bit.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_mla_mixed.h"
#include "fa_launch.h"

namespace fa {
namespace {

typedef uint32_t u32x4a __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2a __attribute__((ext_vector_type(2)));

constexpr int kRowBytes = FA_MLA_MIXED_ROW_BYTES, kScaleOff = 512, kRopeOff = 528;

// tokens: (b, i) row-major, one wave each. Threads [0, B) also write seqlens_out (the launch has at least B threads).
__global__ __launch_bounds__(256) void fa_mla_append_mixed_kernel(const fa_mla_append_params p, const int64_t n_tokens) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int64_t cap = p.max_pages * p.page_size;
    if (p.seqlens_out && i < p.batch_size) {
        int64_t len = p.seqlens_k[i];
        len = len < 0 ? 0 : len > cap ? cap : len;
        const int64_t out = len + p.seqlen_new;
        p.seqlens_out[i] = (int32_t)(out > cap ? cap : out);
    }
    const int64_t tok = i >> 6;
    if (tok >= n_tokens) return;
    const int64_t s = tok % p.seqlen_new, b = tok / p.seqlen_new;
    int64_t len = p.seqlens_k[b];
    len = len < 0 ? 0 : len > cap ? cap : len;
    const int64_t pos = len + s;
    if (pos >= cap) return;  // past the table's capacity: dropped
    const int64_t page = p.block_table[b * p.block_table_stride + pos / p.page_size];
    if (page < 0 || page >= p.num_pages) return;  // outside the pool: dropped, never clamped
    uint8_t *row = (uint8_t *)p.kv_ptr + page * p.kv_page_stride + (pos % p.page_size) * p.kv_row_stride;

    const u32x4a v = *(const u32x4a *)((const uint16_t *)p.c_kv + b * p.ckv_batch_stride + s * p.ckv_seqlen_stride +
                                       8 * lane);
    const uint16_t *e = (const uint16_t *)&v;
    float f[8], amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        f[k] = (float)__builtin_bit_cast(__bf16, e[k]);
        amax = fmaxf(amax, fabsf(f[k]));
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
    const float scale = fmaxf(amax / 448.f, FLT_MIN);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = fminf(fmaxf(f[k] / scale, -448.f), 448.f);
    u32x2a w;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int x = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * k], f[4 * k + 1], 0, false);
        x = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * k + 2], f[4 * k + 3], x, true);
        w[k] = (uint32_t)x;
    }
    *(u32x2a *)(row + 8 * lane) = w;
    if ((lane & 15) == 0) *(float *)(row + kScaleOff + 4 * (lane >> 4)) = scale;
    if (lane < 8)
        *(u32x4a *)(row + kRopeOff + 16 * lane) =
            *(const u32x4a *)((const uint16_t *)p.k_pe + b * p.kpe_batch_stride + s * p.kpe_seqlen_stride + 8 * lane);
}

int mla_append_mixed_check(const fa_mla_append_params *p, int dtype) {
    if (!p) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (dtype != FA_DTYPE_BF16)
        return set_err(FA_ERR_UNSUPPORTED, "the mixed-row MLA append takes bf16 rows only (dtype %d)", dtype);
    if (p->cache_dtype != FA_MLA_CACHE_MIXED)
        return set_err(FA_ERR_UNSUPPORTED, "cache_dtype must be FA_MLA_CACHE_MIXED (got %d)", (int)p->cache_dtype);
    if (p->kv_descale)
        return set_err(FA_ERR_INVALID_ARGUMENT, "kv_descale must be NULL: a mixed row carries its scales");
    fa_mla_append_params q = *p;  // every other rule is the e4m3 append's over a byte pool
    q.cache_dtype = FA_MLA_CACHE_E4M3;
    const int rc = fa_mla_append_gfx950_check(&q, dtype);
    if (rc != FA_OK) return rc;
    if (p->batch_size * p->seqlen_new > (1LL << 31))  // (a wave per token in one launch)
        return set_err(FA_ERR_UNSUPPORTED, "batch * new rows too large for one launch");
    if (p->kv_row_stride < kRowBytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "the mixed latent row stride (%lld) must be at least %d bytes",
                       (long long)p->kv_row_stride, kRowBytes);
    return FA_OK;
}

int mla_append_mixed_launch(const fa_mla_append_params *params, int dtype, hipStream_t stream) {
    const int rc = mla_append_mixed_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_append_params &p = *params;
    if (p.batch_size == 0) return FA_OK;
    const int64_t tokens = p.batch_size * p.seqlen_new;
    const int64_t threads = tokens * 64 > p.batch_size ? tokens * 64 : p.batch_size;
    hipLaunchKernelGGL(fa_mla_append_mixed_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, p,
                       tokens);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

}  // namespace
}  // namespace fa

extern "C" int fa_mla_append_mixed_gfx950(const fa_mla_append_params *params, int dtype, void *stream) {
    return fa::mla_append_mixed_launch(params, dtype, (hipStream_t)stream);
}
extern "C" int fa_mla_append_mixed_gfx950_check(const fa_mla_append_params *params, int dtype) {
    return fa::mla_append_mixed_check(params, dtype);
}
