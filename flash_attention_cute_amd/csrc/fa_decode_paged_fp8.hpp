#pragma once
// fa_decode_paged_fp8.hpp -- fa_decode_paged over an FP8 (OCP e4m3) page pool (include/fa_gfx950_fp8.h),
// gfx950: q and o stay fp16 / bf16, K / V are read as bytes, widened to the q dtype IN REGISTERS (every
// e4m3 value is exact in fp16 and bf16) and multiplied by DT::mfma (32x32x16) exactly as fa_decode does.
// The two descales cost nothing in the key loop: k_descale folds into the softmax scale, v_descale into
// the final 1 / l.
//
// The kernel is decode_body (fa_decode.hpp) with the PagedKv8 policy below: the work decode, the scalar page
// id fetched one tile ahead (PagedWalk<1>), the per-wave LDS ring filled by LDS-DMA and retired by counted
// vmcnt waits (no barrier in the key loop), the online softmax with the deferred rescale, the four-wave LDS
// merge and the fp32 partials with the fused (decode_merge) / unfused (fa_decode_combine) combine are the
// 16-bit kernels' own code. What the policy changes is the K / V image and its fragments:
//
//   * a row is kD BYTES (128 / 64), a 32-key tile 4 / 2 KiB, a 16-byte LDS-DMA chunk 16 elements;
//   * K (A operand of S^T = K.Q^T): lane (h, r) reads ONE ds_read_b128 per pair of k-steps (2j, 2j + 1):
//     the 16 bytes d = 32 j + 16 h .. + 15 of key r, the low 8 for k-step 2j and the high 8 for 2j + 1.
//     The contraction index of an MFMA may be permuted as long as both operands agree, so Q's fragments
//     are loaded to match: qf[2j] = Q[r][32 j + 16 h .. + 7], qf[2j + 1] = the next 8. Swizzle: chunk
//     c ^ ((r >> 1) & 7) on 128-B rows (the byte image of Geo<64>::k_off), c ^ ((r >> 2) & 3) on 64-B
//     rows -- the 16 lanes of every ds_read_b128 lane group on 16 distinct 16-B bank slots;
//   * V (A operand of O^T += V^T.P^T): ds_read_b64_tr_b8. Per 16-lane group it reads 8 rows x 16 byte
//     columns: lane 2 q + p of the group supplies the address of row q, columns 8 p .. 8 p + 7, and lane i
//     receives column i, row q in byte q. With group g4 = lane >> 4 on rows 16 kk + 4 h + (q & 3) +
//     8 (q >> 2), h = g4 >> 1, and columns 32 dt + 16 (g4 & 1) + .., lane (h, m) receives V[those 8
//     keys][32 dt + m] in the key order of the rounded P^T fragment: ONE read per (key step, d tile),
//     half the transposed reads of the 16-bit kernel. A 32-lane half reads 8 rows x 32 B; the swizzle
//     (chunk ^ 2 x, x = row bit 1 | row bit 3 << 1 on 128-B rows, x = row bit 3 on 64-B rows) puts the
//     eight 32-B pieces on the eight 32-B slots of the 256-B bank row;
//   * bytes are widened by v_cvt_scalef32_pk_{f16,bf16}_fp8 with scale 1.0 (two bytes -> one packed pair);
//   * columns >= D of a tile that D does not fill read 0 through the out-of-range source offset, as in
//     fa_decode (byte 0 is 0.0).
//
// Ring depth (kFp8Ring): a tile carries half the bytes of a 16-bit one, so a four-slot ring would hold the
// 16-bit kernel's bytes in flight per wave in the same 128 KiB of LDS. Measured (same process, -DFA_FP8_RING=4
// against 2, profiles/fp8_decode_ab.json), the two-slot ring is 5-6 % FASTER on both shapes, so the ring
// stays two slots deep (64 KiB of LDS); DESIGN.md "FP8 KV cache" has the A/B.
#include "fa_decode_paged.hpp"

#ifndef FA_FP8_RING
#define FA_FP8_RING 2
#endif

namespace fa {

constexpr int kFp8Ring = FA_FP8_RING;  // slots of a wave's LDS ring: 2 or 4
static_assert(kFp8Ring == 2 || kFp8Ring == 4, "the ring is 2 or 4 slots (slot = tile & (ring - 1))");

template <int kD>
struct Fp8Geo {
    static constexpr int RB = kD;                   // bytes of a K / V row
    static constexpr int kTile = kDecKeys * RB;     // bytes of one K (or V) tile: 4 / 2 KiB
    static constexpr int kPieces = kTile / 1024;    // LDS-DMA pieces per K (or V) tile
    static constexpr int kSlot = 2 * kTile;         // K + V
    static constexpr int kWaveLds = kFp8Ring * kSlot;
    static constexpr int kLds = kDecWaves * kWaveLds;
    static constexpr int kPairs = kD / 32;          // pairs of k-steps: ds_read_b128 per K tile and lane
    static_assert(kLds >= kDecWaves * kDecRows * kD * 4, "the four-wave merge reuses the rings");

    static __device__ __forceinline__ int k_off(int row, int ch) {
        return kD == 128 ? row * 128 + 16 * (ch ^ ((row >> 1) & 7)) : row * 64 + 16 * (ch ^ ((row >> 2) & 3));
    }
    static __device__ __forceinline__ int v_off(int row, int ch) {
        return kD == 128 ? row * 128 + 16 * (ch ^ (2 * (((row >> 1) & 1) | (((row >> 3) & 1) << 1))))
                         : row * 64 + 16 * (ch ^ (2 * ((row >> 3) & 1)));
    }
};

// two e4m3 bytes of w (the low or the high pair) -> one packed pair of DT, exact
template <class DT, bool kHi>
__device__ __forceinline__ uint32_t widen2(const uint32_t w) {
    if constexpr (DT::kIsF16)
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, kHi));
    else
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, kHi));
}
// eight bytes -> one 32x32x16 operand
template <class DT>
__device__ __forceinline__ u32x4 widen8(const uint32_t lo, const uint32_t hi) {
    return (u32x4){widen2<DT, false>(lo), widen2<DT, true>(lo), widen2<DT, false>(hi), widen2<DT, true>(hi)};
}

__device__ __forceinline__ u32x2 tr8_read(const char *lds_ptr) {
    typedef int i32x2_ __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) i32x2_ lds_i32x2;
    const i32x2_ v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2 *)(lds_ptr));
    return __builtin_bit_cast(u32x2, v);
}

// `n` tiles (of kPer LDS-DMA pieces each) may still be in flight
template <int kPer>
__device__ __forceinline__ void wait_tiles(const int n) {
    if (n <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (n == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPer) : "memory");
    else if (n == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kPer) : "memory");
    else if (n == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * kPer) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * kPer) : "memory");
}

// The paged FP8 pool (ArgsT: PagedFp8DecArgs, or PagedFp8WinDecArgs for the windowed kernel)
template <int kD, class ArgsT = PagedFp8DecArgs>
struct PagedKv8 : Fp8Geo<kD>, PagedSeq<1, ArgsT> {
    using PagedSeq<1, ArgsT>::PagedSeq;
    using FG = Fp8Geo<kD>;
    using FG::RB;
    using FG::kPieces;
    static constexpr int kElem = 1;         // bytes of a K / V element
    static constexpr int kRing = kFp8Ring;  // slots of a wave's LDS ring
    static constexpr int KS = Geo<kD>::kKSteps, KP = FG::kPairs, DTL = Geo<kD>::kDTiles;
    typedef const __attribute__((address_space(4))) float *scale_t;  // (constant space: scalar loads)

    // the descales of this (batch row, kv-head): k folds into the softmax scale, v into the final 1 / l
    static __device__ __forceinline__ void scale(const fa_fwd_params &p, const ArgsT &a, const int b, const int hkv,
                                                 float &sc, float &vds) {
        const int64_t dso = (int64_t)b * a.descale_batch_stride + (int64_t)hkv * a.descale_head_stride;
        const float kds = a.k_descale ? ((scale_t)a.k_descale)[dso] : 1.f;
        vds = a.v_descale ? ((scale_t)a.v_descale)[dso] : 1.f;
        sc = p.softmax_scale * kds;
    }
    // bytes of the first `rows` rows of a [rows, D] slab of 1-byte elements with row stride `stride`
    static __device__ __forceinline__ uint32_t slab(int rows, int stride, int D) {
        return rows <= 0 ? 0u : (uint32_t)((rows - 1) * stride + D);
    }
    // B operand of S^T = K.Q^T in K's d order: lane (h, r) holds Q[row r][32 j + 16 h + 8 e .. + 7] for
    // k-step 2 j + e
    static __device__ __forceinline__ int q_chunk(int ks, int h) { return 4 * (ks >> 1) + 2 * h + (ks & 1); }

    // after the ring's first n_pre tiles (decode_body issues them): the counted wait retires the Q pieces
    // (issued first) and leaves the tiles in flight
    static constexpr bool kStraightPrefill = false;
    static __device__ __forceinline__ void wait_prefill(const int n_pre) { wait_tiles<2 * kPieces>(n_pre); }
    // tile t landed (the younger tiles of the ring may still be in flight)
    static __device__ __forceinline__ void wait_tile(const int t, const int t_hi) {
        wait_tiles<2 * kPieces>(min(t_hi - 1 - t, kRing - 1));
    }

    struct Frags {
        int v_addr[DTL], k_addr[KP];
        u32x4 k8[KP];
        u32x2 v8[2][DTL];

        __device__ __forceinline__ Frags(const int lane) {
            const int r = lane & 31, h = lane >> 5;
            const int g4 = lane >> 4, q = (lane >> 1) & 7, pp = lane & 1;
            const int row0 = 4 * (g4 >> 1) + (q & 3) + 8 * (q >> 2);
#pragma unroll
            for (int dt = 0; dt < DTL; ++dt) v_addr[dt] = FG::v_off(row0, 2 * dt + (g4 & 1)) + 8 * pp;
#pragma unroll
            for (int j = 0; j < KP; ++j) k_addr[j] = FG::k_off(r, 2 * j + h);
        }
        __device__ __forceinline__ void load(const char *K, const char *V) {
#pragma unroll
            for (int j = 0; j < KP; ++j) k8[j] = *(const u32x4 *)(K + k_addr[j]);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int dt = 0; dt < DTL; ++dt) v8[kk][dt] = tr8_read(V + kk * 16 * RB + v_addr[dt]);
        }
        template <class DT>
        __device__ __forceinline__ f32x16 qk(const u32x4 (&qf)[KS]) const {
            f32x16 s = {};
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                s = DT::mfma(widen8<DT>(k8[j][0], k8[j][1]), qf[2 * j], s);
                s = DT::mfma(widen8<DT>(k8[j][2], k8[j][3]), qf[2 * j + 1], s);
            }
            return s;
        }
        template <class DT>
        __device__ __forceinline__ void pv(const u32x4 (&pf)[2], f32x16 (&o)[DTL]) const {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int dt = 0; dt < DTL; ++dt)
                    o[dt] = DT::mfma(widen8<DT>(v8[kk][dt][0], v8[kk][dt][1]), pf[kk], o[dt]);
        }
    };
};

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_fp8kv(const fa_fwd_params p, const PagedFp8DecArgs a) {
    decode_body<PagedKv8<kD>, false, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8(const fa_fwd_params &p, PagedFp8DecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_fp8kv<DT, C, kD, kExact, true>,
                                                 &fa_decode_fp8kv<DT, C, kD, kExact, false>, kPathDecodePagedFp8,
                                                 kPathDecodePagedFp8Split);
}

}  // namespace fa
