// fa_kvcache_move.h -- the row movers of the KV-cache append kernels (fa_kvcache.hip: one seqlen_new per
// batch; fa_kvcache_varlen.hip: packed ragged rows): copy or rotate one chunk pair / element pair of a row.
// The rotation is fa_rope.hip's arithmetic, bit for bit: fma(x, cos, rot * sin) in fp32 behind the same pin,
// one RNE rounding. Both kernels include this one definition, so they cannot drift apart.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "fa_launch.h"

namespace fa {
namespace kvmove {

typedef uint32_t u32x4k __attribute__((ext_vector_type(4)));
typedef float f2k __attribute__((ext_vector_type(2)));

template <bool kF16>
__device__ __forceinline__ float ld(const uint16_t v) {
    if constexpr (kF16) return (float)__builtin_bit_cast(_Float16, v);
    else return (float)__builtin_bit_cast(__bf16, v);
}
template <bool kF16>
__device__ __forceinline__ uint16_t st(const float f) {
    if constexpr (kF16) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else return __builtin_bit_cast(uint16_t, (__bf16)f);
}
template <bool kF16>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    if constexpr (kF16) {
        typedef _Float16 hh2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector((f2k){lo, hi}, hh2));
    } else {
        typedef __bf16 bb2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_convertvector((f2k){lo, hi}, bb2));
    }
}

// thread mappings: kVec 16-B chunk pairs (d0, d0 + D/2), D % 16 == 0, everything 16-B aligned;
// kPair element pairs (d0, d0 + D/2), any even D; kElem single elements (no tables, any D)
enum Mode { kVec = 0, kPair = 1, kElem = 2 };

// the chunk pair of fa_rope_kernel<kF16, true>: rotates when cs != nullptr, else copies
template <bool kF16>
__device__ __forceinline__ void move_vec(const uint16_t *x, uint16_t *o, const uint16_t *cs, const uint16_t *sn,
                                         const int d0, const int d1) {
    const u32x4k xa = *(const u32x4k *)(x + d0), xb = *(const u32x4k *)(x + d1);
    if (!cs) {
        *(u32x4k *)(o + d0) = xa;
        *(u32x4k *)(o + d1) = xb;
        return;
    }
    const u32x4k ca = *(const u32x4k *)(cs + d0), cb = *(const u32x4k *)(cs + d1);
    const u32x4k sa = *(const u32x4k *)(sn + d0), sb = *(const u32x4k *)(sn + d1);
    const uint16_t *xa_ = (const uint16_t *)&xa, *xb_ = (const uint16_t *)&xb;
    const uint16_t *ca_ = (const uint16_t *)&ca, *cb_ = (const uint16_t *)&cb;
    const uint16_t *sa_ = (const uint16_t *)&sa, *sb_ = (const uint16_t *)&sb;
    u32x4k oa, ob;
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
    *(u32x4k *)(o + d0) = oa;
    *(u32x4k *)(o + d1) = ob;
}

// the element pair of fa_rope_kernel<kF16, false>
template <bool kF16>
__device__ __forceinline__ void move_pair(const uint16_t *x, uint16_t *o, const uint16_t *cs, const uint16_t *sn,
                                          const int d0, const int d1) {
    if (!cs) {
        o[d0] = x[d0];
        o[d1] = x[d1];
        return;
    }
    const float u = ld<kF16>(x[d0]), w = ld<kF16>(x[d1]);
    float a = __builtin_fmaf(u, ld<kF16>(cs[d0]), -w * ld<kF16>(sn[d0]));
    float bb = __builtin_fmaf(w, ld<kF16>(cs[d1]), u * ld<kF16>(sn[d1]));
    // keep the fp32 rounding step (fa_rope.hip: without the pin hipcc folds it into a mixed-precision fma)
    asm volatile("" : "+v"(a), "+v"(bb));
    o[d0] = st<kF16>(a);
    o[d1] = st<kF16>(bb);
}

// ---- host side: what both launchers decide and check the same way, whatever the layout of the new rows -------

inline bool al16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

// threads per row of a mapping
inline int per_row_of(int64_t headdim, int mode) {
    return (int)(mode == kVec ? headdim / 16 : mode == kPair ? headdim / 2 : headdim);
}

// the 16-B path needs every chunk of every tensor the launch touches 16-B aligned: these strides (elements) and bases
inline bool vec_ok(std::initializer_list<int64_t> strides, std::initializer_list<const void *> bases) {
    bool ok = true;
    for (const int64_t st : strides) ok = ok && st % 8 == 0;
    for (const void *b : bases) ok = ok && al16(b);
    return ok;
}

inline int mode_of(bool vec, int64_t headdim) { return vec ? kVec : headdim % 2 == 0 ? kPair : kElem; }

// the rules of the RoPE tables and of seqlens_out, after the launcher's own: FA_OK, or the error (set_err)
inline int check_tables_and_lengths(const void *cos, int64_t headdim, int64_t max_pos,
                                    const int32_t *seqlens_k, const int32_t *seqlens_out, int64_t batch_size) {
    if (cos) {
        if (headdim & 1) return set_err(FA_ERR_INVALID_ARGUMENT, "RoPE needs an even head dim (got %lld)",
                                        (long long)headdim);
        if (max_pos < 1) return set_err(FA_ERR_INVALID_ARGUMENT, "max_pos must be at least 1 (the tables' rows)");
    }
    if (seqlens_out) {
        const uintptr_t a = (uintptr_t)seqlens_k, b = (uintptr_t)seqlens_out;
        const uintptr_t n = (uintptr_t)batch_size * 4;
        if ((a <= b ? b - a : a - b) < n)  // (the distance, so nothing wraps at the ends of the address space)
            return set_err(FA_ERR_INVALID_ARGUMENT,
                           "seqlens_out must not overlap seqlens_k (the launch is still reading it)");
    }
    return FA_OK;
}

}  // namespace kvmove
}  // namespace fa
