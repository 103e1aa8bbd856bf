// fa_kvcache_fp8.hip -- quantizing in-place KV-cache append for gfx950 (C-ABI fa_kvcache_append_fp8_gfx950,
// include/fa_gfx950_fp8.h): the write side of the FP8 (OCP e4m3) cache that fa_paged_fp8_gfx950.hip reads.
//
// fa_kvcache.hip's launch with an 8-bit destination: the same item decomposition (K rows, V rows, q rows,
// seqlens_out by the first B threads), the same placement and drop rules, the same rotation -- K is rotated
// with fa_rope.hip's arithmetic behind its fp32 pin and ROUNDED to the input dtype first, so the value
// that is quantized is bit for bit what the 16-bit cache would hold -- and then
//
//     byte = e4m3_rne(clamp(fp32(x) / descale[b, h], -448, 448))
//
// with an IEEE fp32 division (this file is built without fast-math reciprocals) and the clamp in fp32
// ahead of v_cvt_pk_fp8_f32, so nothing rests on the convert instruction's overflow behaviour. One thread
// owns the 8-element chunk d0 of the first half of a row and its partner d0 + D/2 (two 16-B loads) and
// stores 8 bytes per half; consecutive lanes take consecutive chunks, so each half of a row is one
// contiguous run of 8-B stores. q rows are rotated and stay 16-bit. Every page term is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_fp8.h"
#include "fa_launch.h"

namespace fa {

int kvcache_check(const fa_kvcache_params *p, int dtype);  // fa_kvcache.hip

namespace {

typedef uint32_t u32x4q __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2q __attribute__((ext_vector_type(2)));
typedef float f2q __attribute__((ext_vector_type(2)));

template <bool kF16>
__device__ __forceinline__ float ld(const uint16_t v) {
    if constexpr (kF16) return (float)__builtin_bit_cast(_Float16, v);
    else return (float)__builtin_bit_cast(__bf16, v);
}
template <bool kF16>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    if constexpr (kF16) {
        typedef _Float16 hh2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector((f2q){lo, hi}, hh2));
    } else {
        typedef __bf16 bb2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector((f2q){lo, hi}, bb2));
    }
}

// the chunk pair (d0, d1 = d0 + D/2) of a row, rotated as fa_kvcache.hip's move_vec does (fa_rope.hip's
// arithmetic, bit for bit) when cs != nullptr, else as loaded: 2 x 8 elements of the input dtype
template <bool kF16>
__device__ __forceinline__ void load_rot(const uint16_t *x, const uint16_t *cs, const uint16_t *sn, const int d0,
                                         const int d1, u32x4q &oa, u32x4q &ob) {
    const u32x4q xa = *(const u32x4q *)(x + d0), xb = *(const u32x4q *)(x + d1);
    if (!cs) {
        oa = xa;
        ob = xb;
        return;
    }
    const u32x4q ca = *(const u32x4q *)(cs + d0), cb = *(const u32x4q *)(cs + d1);
    const u32x4q sa = *(const u32x4q *)(sn + d0), sb = *(const u32x4q *)(sn + d1);
    const uint16_t *xa_ = (const uint16_t *)&xa, *xb_ = (const uint16_t *)&xb;
    const uint16_t *ca_ = (const uint16_t *)&ca, *cb_ = (const uint16_t *)&cb;
    const uint16_t *sa_ = (const uint16_t *)&sa, *sb_ = (const uint16_t *)&sb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a[2], bb[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = 2 * j + t;
            const float u = ld<kF16>(xa_[e]), w = ld<kF16>(xb_[e]);
            a[t] = __builtin_fmaf(u, ld<kF16>(ca_[e]), -w * ld<kF16>(sa_[e]));
            bb[t] = __builtin_fmaf(w, ld<kF16>(cb_[e]), u * ld<kF16>(sb_[e]));
        }
        asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(bb[0]), "+v"(bb[1]));  // fp32 step kept (fa_rope.hip)
        oa[j] = pack2<kF16>(a[0], a[1]);
        ob[j] = pack2<kF16>(bb[0], bb[1]);
    }
}

// 8 elements of the input dtype -> 8 e4m3 bytes: IEEE division, fp32 clamp, RNE convert
template <bool kF16>
__device__ __forceinline__ u32x2q quant8(const u32x4q v, const float descale) {
    const uint16_t *e = (const uint16_t *)&v;
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = fminf(fmaxf(ld<kF16>(e[i]) / descale, -448.f), 448.f);
    u32x2q w;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int x = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i], f[4 * i + 1], 0, false);
        x = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i + 2], f[4 * i + 3], x, true);
        w[i] = (uint32_t)x;
    }
    return w;
}

// items: [0, n_kv) K rows, [n_kv, 2 n_kv) V rows, [2 n_kv, 2 n_kv + n_q) q rows, each (b, h, s, chunk)
// row-major, per_row = D / 16 chunk pairs. Threads [0, B) of the launch also write seqlens_out.
template <bool kF16>
__global__ __launch_bounds__(256) void fa_kvcache_append_fp8_kernel(const fa_kvcache_fp8_params q, const int64_t n_kv,
                                                                    const int64_t n_items, const int per_row) {
    const fa_kvcache_params &p = q.base;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int64_t cap = p.max_pages * p.page_size;
    if (p.seqlens_out && i < p.batch_size) {
        int64_t len = p.seqlens_k[i];
        len = len < 0 ? 0 : len > cap ? cap : len;
        const int64_t out = len + p.seqlen_new;
        p.seqlens_out[i] = (int32_t)(out > cap ? cap : out);
    }
    const int kind = i < n_kv ? 0 : i < 2 * n_kv ? 1 : 2;  // K, V, q
    const int64_t j = i - (kind == 0 ? 0 : kind == 1 ? n_kv : 2 * n_kv);
    const int c = (int)(j % per_row);
    const int64_t row = j / per_row;  // (b, h, s) row-major
    const int64_t rows_s = kind == 2 ? p.seqlen_q : p.seqlen_new;
    const int64_t heads = kind == 2 ? p.num_heads_q : p.num_heads_kv;
    const int64_t s = row % rows_s, bh = row / rows_s;
    const int64_t h = bh % heads, b = bh / heads;
    int64_t len = p.seqlens_k[b];
    len = len < 0 ? 0 : len > cap ? cap : len;

    const uint16_t *x;
    uint16_t *o16 = nullptr;  // q
    uint8_t *o8 = nullptr;    // K / V
    int64_t pos;
    if (kind == 2) {
        const int64_t end = len + p.seqlen_new > cap ? cap : len + p.seqlen_new;  // seqlens_out[b], recomputed
        pos = end - p.seqlen_q + s;
        pos = pos < 0 ? 0 : pos;
        x = (const uint16_t *)p.q + b * p.q_batch_stride + h * p.q_head_stride + s * p.q_seqlen_stride;
        o16 = (uint16_t *)p.q_out + b * p.qo_batch_stride + h * p.qo_head_stride + s * p.qo_seqlen_stride;
    } else {
        pos = len + s;
        if (pos >= cap) return;  // past the table's capacity: dropped
        int64_t page = b;
        if (p.block_table) {
            page = p.block_table[b * p.block_table_stride + pos / p.page_size];
            if (page < 0 || page >= p.num_pages) return;  // outside the pool: dropped, never clamped
        }
        const int64_t r = pos % p.page_size;
        if (kind == 0) {
            x = (const uint16_t *)p.k_new + b * p.kn_batch_stride + h * p.kn_head_stride + s * p.kn_seqlen_stride;
            o8 = (uint8_t *)p.k_cache + page * p.k_page_stride + h * p.k_head_stride + r * p.k_row_stride;
        } else {
            x = (const uint16_t *)p.v_new + b * p.vn_batch_stride + h * p.vn_head_stride + s * p.vn_seqlen_stride;
            o8 = (uint8_t *)p.v_cache + page * p.v_page_stride + h * p.v_head_stride + r * p.v_row_stride;
        }
    }
    const uint16_t *cs = nullptr, *sn = nullptr;
    if (kind != 1 && p.cos) {
        pos = pos > p.max_pos - 1 ? p.max_pos - 1 : pos;  // a table shorter than the position: its last row
        cs = (const uint16_t *)p.cos + pos * p.cs_row_stride;
        sn = (const uint16_t *)p.sin + pos * p.cs_row_stride;
    }
    const int d0 = c * 8, d1 = d0 + (int)p.headdim / 2;
    u32x4q va, vb;
    load_rot<kF16>(x, cs, sn, d0, d1, va, vb);
    if (kind == 2) {
        *(u32x4q *)(o16 + d0) = va;
        *(u32x4q *)(o16 + d1) = vb;
    } else {
        const float *ds = kind == 0 ? q.k_descale : q.v_descale;
        const float descale = ds ? ds[b * q.descale_batch_stride + h * q.descale_head_stride] : 1.f;
        *(u32x2q *)(o8 + d0) = quant8<kF16>(va, descale);
        *(u32x2q *)(o8 + d1) = quant8<kF16>(vb, descale);
    }
}

bool al16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

int kvcache_fp8_check(const fa_kvcache_fp8_params *v, int dtype) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    const int rc = kvcache_check(&v->base, dtype);
    if (rc != FA_OK) return rc;
    const fa_kvcache_params &p = v->base;
    if (p.headdim > 128) return set_err(FA_ERR_UNSUPPORTED, "only support hidden dimension <= 128");
    if (p.headdim % 16 != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "an fp8 KV cache needs a head dim that is a multiple of 16 (got %lld)",
                       (long long)p.headdim);
    if (v->descale_batch_stride < 0 || v->descale_head_stride < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "descale strides must be non-negative");
    if (((uintptr_t)v->k_descale & 3) || ((uintptr_t)v->v_descale & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "k_descale and v_descale must be 4-byte aligned fp32 arrays");
    // the cache is written in place by 8-byte stores at multiples of 8 bytes, read by 16-byte chunks
    if (p.seqlen_new > 0) {
        if (!al16(p.k_cache) || !al16(p.v_cache))
            return set_err(FA_ERR_INVALID_ARGUMENT, "the fp8 K / V pool bases must be 16-byte aligned");
        const int64_t st[6] = {p.k_page_stride, p.k_head_stride, p.k_row_stride,
                               p.v_page_stride, p.v_head_stride, p.v_row_stride};
        for (int i = 0; i < 6; ++i)
            if (st[i] % 16 != 0)
                return set_err(FA_ERR_INVALID_ARGUMENT,
                               "the fp8 K / V page, head and row strides must be multiples of 16 elements (16 bytes)");
        const int64_t sn[6] = {p.kn_batch_stride, p.kn_head_stride, p.kn_seqlen_stride,
                               p.vn_batch_stride, p.vn_head_stride, p.vn_seqlen_stride};
        bool ok = al16(p.k_new) && al16(p.v_new);
        for (int i = 0; i < 6; ++i) ok = ok && sn[i] % 8 == 0;
        if (!ok)
            return set_err(FA_ERR_INVALID_ARGUMENT,
                           "k_new / v_new must be 16-byte aligned with strides that are multiples of 8 elements");
    }
    if (p.seqlen_q > 0) {
        const int64_t sq[6] = {p.q_batch_stride,  p.q_head_stride,  p.q_seqlen_stride,
                               p.qo_batch_stride, p.qo_head_stride, p.qo_seqlen_stride};
        bool ok = al16(p.q) && al16(p.q_out);
        for (int i = 0; i < 6; ++i) ok = ok && sq[i] % 8 == 0;
        if (!ok)
            return set_err(FA_ERR_INVALID_ARGUMENT,
                           "q / q_out must be 16-byte aligned with strides that are multiples of 8 elements");
    }
    if (p.cos && (p.cs_row_stride % 8 != 0 || !al16(p.cos) || !al16(p.sin)))
        return set_err(FA_ERR_INVALID_ARGUMENT,
                       "cos / sin must be 16-byte aligned with a row stride that is a multiple of 8 elements");
    return set_err(FA_OK, "%s", "");
}

int kvcache_fp8_launch(const fa_kvcache_fp8_params *v, int dtype, hipStream_t stream) {
    const int rc = kvcache_fp8_check(v, dtype);
    if (rc != FA_OK) return rc;
    const fa_kvcache_params &p = v->base;
    if (p.batch_size == 0 || (p.seqlen_new == 0 && p.seqlen_q == 0)) return FA_OK;
    const int per_row = (int)(p.headdim / 16);
    const int64_t n_kv = p.batch_size * p.num_heads_kv * p.seqlen_new * per_row;
    // (at least B items: seqlens_out is written by the first B threads)
    const int64_t items = 2 * n_kv + p.batch_size * p.num_heads_q * p.seqlen_q * per_row;
    const dim3 grid((uint32_t)((items + 255) / 256));
    if (dtype == FA_DTYPE_F16)
        hipLaunchKernelGGL((fa_kvcache_append_fp8_kernel<true>), grid, dim3(256), 0, stream, *v, n_kv, items, per_row);
    else
        hipLaunchKernelGGL((fa_kvcache_append_fp8_kernel<false>), grid, dim3(256), 0, stream, *v, n_kv, items, per_row);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

}  // namespace
}  // namespace fa

extern "C" int fa_kvcache_append_fp8_gfx950(const fa_kvcache_fp8_params *params, int dtype, void *stream) {
    return fa::kvcache_fp8_launch(params, dtype, (hipStream_t)stream);
}

extern "C" int fa_kvcache_append_fp8_gfx950_check(const fa_kvcache_fp8_params *params, int dtype) {
    return fa::kvcache_fp8_check(params, dtype);
}
