// fa_merge.hip -- fa_merge_states_gfx950 (include/fa_gfx950_lse.h): merge N partial attention states (O_i,
// lse_i) over disjoint key sets into one, gfx950. The counterpart of vLLM's merge_attn_states / flashinfer's
// merge_state; what shared-prefix decode and sequence-sharded decode end with.
//
// Per (batch, head, position) row: Mx = max_i lse_i, w_i = exp(lse_i - Mx), O = sum_i w_i O_i / sum_i w_i in
// fp32, rounded once (RNE) to T; lse = Mx + ln sum_i w_i. A part whose lse is -inf weighs 0; a row whose parts
// all are gives O = 0 and lse = -inf.
//
// Memory-bound, one pass, no LDS: one thread per (row, 8-element chunk) reads the row's N lse values (4 bytes
// each, shared by the row's D / 8 threads through the cache) twice -- the max, then the weights -- and one
// 16-byte chunk per part, and writes one 16-byte chunk: N * (2 D + 4) + 2 D bytes per row.
//
// The build is -ffinite-math-only, so an lse never enters float arithmetic as an infinity: -inf is recognised
// by its bit pattern and replaced by kNegLse, and the -inf result is stored as a bit pattern.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_lse.h"
#include "fa_launch.h"

namespace fa {
namespace {

typedef uint32_t u32x4m __attribute__((ext_vector_type(4)));
typedef float f2m __attribute__((ext_vector_type(2)));

constexpr float kNegLse = -1.0e30f;   // stands for an lse of -inf
constexpr uint32_t kNegInfBits = 0xff800000u;
constexpr float kLog2e = 1.44269504088896341f, kLn2 = 0.69314718055994531f;

template <bool kF16>
__device__ __forceinline__ float widen(const uint16_t v) {
    if constexpr (kF16) return (float)__builtin_bit_cast(_Float16, v);
    else return __uint_as_float((uint32_t)v << 16);
}
template <bool kF16>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    if constexpr (kF16) {
        typedef _Float16 hh2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector((f2m){lo, hi}, hh2));
    } else {
        typedef __bf16 bb2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector((f2m){lo, hi}, bb2));
    }
}

__device__ __forceinline__ float load_lse(const float *ptr) {
    const uint32_t bits = *(const uint32_t *)ptr;
    return bits == kNegInfBits ? kNegLse : __uint_as_float(bits);
}

template <bool kF16>
__global__ __launch_bounds__(256) void fa_merge_states_kernel(const fa_merge_params p, const int64_t n_items) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int per_row = (int)p.headdim / 8;
    const int c = (int)(i % per_row);
    const int64_t row = i / per_row;  // (b, h, s) row-major
    const int64_t s = row % p.seqlen, bh = row / p.seqlen;
    const int64_t h = bh % p.num_heads, b = bh / p.num_heads;
    const int n = (int)p.num_parts;
    const float *lp = p.lses + b * p.lses_batch_stride + h * p.lses_head_stride + s * p.lses_seqlen_stride;
    const uint16_t *op = (const uint16_t *)p.outs + b * p.outs_batch_stride + h * p.outs_head_stride +
                         s * p.outs_seqlen_stride + 8 * c;

    float mx = kNegLse;
    for (int k = 0; k < n; ++k) mx = fmaxf(mx, load_lse(lp + k * p.lses_part_stride));
    float acc[8], sum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int k = 0; k < n; ++k) {
        const float l = load_lse(lp + k * p.lses_part_stride);
        const float w = (l <= 0.5f * kNegLse) ? 0.f : __builtin_amdgcn_exp2f((l - mx) * kLog2e);
        sum += w;
        const u32x4m x = *(const u32x4m *)(op + k * p.outs_part_stride);
        const uint16_t *x_ = (const uint16_t *)&x;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(w, widen<kF16>(x_[e]), acc[e]);
    }
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= inv;
    // keep the fp32 product: one rounding to T, whatever the compiler would fuse
    asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]),
                 "+v"(acc[7]));
    const u32x4m o = {pack2<kF16>(acc[0], acc[1]), pack2<kF16>(acc[2], acc[3]), pack2<kF16>(acc[4], acc[5]),
                      pack2<kF16>(acc[6], acc[7])};
    uint16_t *dst = (uint16_t *)p.out + b * p.out_batch_stride + h * p.out_head_stride + s * p.out_seqlen_stride + 8 * c;
    *(u32x4m *)dst = o;
    if (p.lse && c == 0) {
        const float v = mx + __builtin_amdgcn_logf(sum) * kLn2;
        uint32_t *ld = (uint32_t *)p.lse + b * p.lse_batch_stride + h * p.lse_head_stride + s * p.lse_seqlen_stride;
        *ld = sum > 0.f ? __float_as_uint(v) : kNegInfBits;
    }
}

}  // namespace

int merge_check(const fa_merge_params *p, int dtype) {
    if (!p) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return set_err(FA_ERR_UNSUPPORTED, "merge_states supports fp16 / bf16 partial outputs only (dtype %d)", dtype);
    if (!p->outs || !p->lses || !p->out)
        return set_err(FA_ERR_INVALID_ARGUMENT, "outs, lses and out must be non-NULL");
    if (p->num_parts < 1 || p->num_parts > FA_MERGE_MAX_PARTS)
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_parts (%lld) must be in [1, %d]", (long long)p->num_parts,
                       FA_MERGE_MAX_PARTS);
    if (p->batch_size < 0 || p->num_heads < 0 || p->seqlen < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "sizes must be non-negative");
    if (p->headdim <= 0 || p->headdim % 8 != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "hidden dimension (%lld) must be a positive multiple of 8",
                       (long long)p->headdim);
    if (((uintptr_t)p->outs & 15) || ((uintptr_t)p->out & 15))
        return set_err(FA_ERR_INVALID_ARGUMENT, "outs and out must be 16-byte aligned");
    if (((uintptr_t)p->lses & 3) || ((uintptr_t)p->lse & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "lses and lse must be 4-byte aligned fp32 arrays");
    const int64_t st16[7] = {p->outs_part_stride, p->outs_batch_stride, p->outs_head_stride, p->outs_seqlen_stride,
                             p->out_batch_stride, p->out_head_stride, p->out_seqlen_stride};
    for (int i = 0; i < 7; ++i)
        if (st16[i] < 0 || st16[i] % 8 != 0)
            return set_err(FA_ERR_INVALID_ARGUMENT,
                           "the strides of outs and out must be non-negative multiples of 8 elements (16 bytes)");
    const int64_t st4[7] = {p->lses_part_stride, p->lses_batch_stride, p->lses_head_stride, p->lses_seqlen_stride,
                            p->lse_batch_stride, p->lse_head_stride, p->lse_seqlen_stride};
    for (int i = 0; i < 7; ++i)
        if (st4[i] < 0) return set_err(FA_ERR_INVALID_ARGUMENT, "the strides of lses and lse must be non-negative");
    const int64_t lim = int64_t(1) << 31;
    if (p->batch_size >= lim || p->num_heads >= lim || p->seqlen >= lim ||
        (double)p->batch_size * (double)p->num_heads * (double)p->seqlen * (double)(p->headdim / 8) >= 256.0 * (double)lim)
        return set_err(FA_ERR_UNSUPPORTED, "too many rows for one merge launch");
    return FA_OK;
}

int merge_launch(const fa_merge_params *p, int dtype, hipStream_t stream) {
    const int rc = merge_check(p, dtype);
    if (rc != FA_OK) return rc;
    const int64_t items = p->batch_size * p->num_heads * p->seqlen * (p->headdim / 8);
    if (items == 0) return FA_OK;
    const dim3 grid((uint32_t)((items + 255) / 256));
    if (dtype == FA_DTYPE_F16) hipLaunchKernelGGL((fa_merge_states_kernel<true>), grid, dim3(256), 0, stream, *p, items);
    else hipLaunchKernelGGL((fa_merge_states_kernel<false>), grid, dim3(256), 0, stream, *p, items);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

}  // namespace fa

extern "C" int fa_merge_states_gfx950(const fa_merge_params *params, int dtype, void *stream) {
    return fa::merge_launch(params, dtype, (hipStream_t)stream);
}
extern "C" int fa_merge_states_gfx950_check(const fa_merge_params *params, int dtype) {
    return fa::merge_check(params, dtype);
}
