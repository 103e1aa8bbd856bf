#pragma once
// fa_decode_paged_fp8.hpp -- fa_decode_paged over an FP8 (OCP e4m3) page pool (include/fa_gfx950_fp8.h),
// gfx950: q and o stay fp16 / bf16, K / V are read as bytes, widened to the q dtype IN REGISTERS (every
// e4m3 value is exact in fp16 and bf16) and multiplied by DT::mfma (32x32x16) exactly as fa_decode does.
// The two descales cost nothing in the key loop: k_descale folds into the softmax scale, v_descale into
// the final 1 / l.
//
// Carried over from fa_decode_body.inc / PagedKv unchanged in structure: the work decode, the scalar page
// id fetched one tile ahead, the per-wave LDS ring filled by LDS-DMA and retired by counted vmcnt waits
// (no barrier in the key loop), the online softmax with the deferred rescale, the four-wave LDS merge and
// the fp32 partials with the fused (decode_merge) / unfused (fa_decode_combine) combine, which are shared
// functions. What differs is the K / V image and its fragments:
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
#include "fa_decode.hpp"
#include "fa_paged_fp8_launch.h"

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

// PagedKv over 1-byte elements: the same walk (one call per tile in increasing t, the next page's id
// fetched by a scalar load one tile ahead, the id clamped into the pool, a 64-bit page term).
struct PagedKv8 {
    typedef const __attribute__((address_space(4))) int32_t *table_t;  // (constant space: a scalar load)
    const char *kh, *vh;  // the pool at this kv-head
    int64_t kps, vps;     // page strides, bytes
    int ks_, vs_;
    table_t row;
    int tpp, last_page, t_hi;
    int pi, tip, phys;

    __device__ __forceinline__ PagedKv8(const fa_fwd_params &p, const PagedDecArgs &a, int b, int hkv, int t_lo,
                                        int t_hi_)
        : kps(p.k_batch_stride), vps(p.v_batch_stride), ks_((int)p.k_seqlen_stride), vs_((int)p.v_seqlen_stride),
          tpp(a.tiles_per_page), last_page(a.num_pages - 1), t_hi(t_hi_) {
        kh = (const char *)p.k_ptr + (int64_t)hkv * p.k_head_stride;
        vh = (const char *)p.v_ptr + (int64_t)hkv * p.v_head_stride;
        row = (table_t)(a.block_table + (int64_t)b * a.block_table_stride);
        pi = t_lo / tpp;
        tip = t_lo - pi * tpp;
        phys = t_lo < t_hi ? row[pi] : 0;  // (a wave without tiles reads no entry)
    }
    __device__ __forceinline__ void tile(int t, const char *&k, const char *&v) {
        const int64_t page = min(max(phys, 0), last_page);
        const int64_t r0 = (int64_t)(tip * kDecKeys);
        k = kh + page * kps + r0 * ks_;
        v = vh + page * vps + r0 * vs_;
        if (++tip == tpp) {
            tip = 0;
            ++pi;
            if (t + 1 < t_hi) phys = row[pi];  // the next tile's page, one tile ahead of its use
        }
    }
};

// bytes of the first `rows` rows of a [rows, D] slab of 1-byte elements with row stride `stride`
__device__ __forceinline__ uint32_t slab_bytes8(int rows, int stride, int D) {
    return rows <= 0 ? 0u : (uint32_t)((rows - 1) * stride + D);
}

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_fp8kv(const fa_fwd_params p, const PagedFp8DecArgs a) {
    using G = Geo<kD>;  // the 16-bit Q image
    using FG = Fp8Geo<kD>;
    constexpr int KS = G::kKSteps;
    constexpr int KP = FG::kPairs;
    constexpr int DTL = G::kDTiles;
    constexpr int QRB = G::kRowBytes;
    constexpr int RB = FG::RB;
    constexpr int NP = FG::kPieces;
    constexpr int R = kFp8Ring;
    typedef const __attribute__((address_space(4))) float *scale_t;  // (constant space: scalar loads)
    typedef const __attribute__((address_space(4))) int32_t *len_t;
    __shared__ __attribute__((aligned(1024))) char lds[FG::kLds];
    __shared__ __attribute__((aligned(1024))) char qlds[kDecRows * QRB];
    __shared__ float ml[kDecWaves][kDecRows][2];
    __shared__ uint32_t last_wg;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;

    // ---- work: (unit = (b, hkv, rb), split), as fa_decode ---------------------------------------
    int split, unit;
    if constexpr (kFuse) {
        const int k = (int)(blockIdx.x >> 3);
        unit = ((k / a.n_split) << 3) | (int)(blockIdx.x & 7);
        split = k % a.n_split;
        if (unit >= (int)p.batch_size * (int)p.num_heads_kv * a.n_rb) return;
    } else {
        split = blockIdx.x % a.n_split;
        unit = blockIdx.x / a.n_split;
    }
    const int rb = unit % a.n_rb;
    const int hkv = (unit / a.n_rb) % (int)p.num_heads_kv;
    const int b = unit / (a.n_rb * (int)p.num_heads_kv);
    const int Sq = (int)p.seqlen_q, D = (int)p.headdim;
    // the descales of this (batch row, kv-head): k folds into the softmax scale, v into the final 1 / l
    const int64_t dso = (int64_t)b * a.descale_batch_stride + (int64_t)hkv * a.descale_head_stride;
    const float kds = a.k_descale ? ((scale_t)a.k_descale)[dso] : 1.f;
    const float vds = a.v_descale ? ((scale_t)a.v_descale)[dso] : 1.f;
    const float sc = p.softmax_scale * kds;
    const float thr_raw = kRescaleThr / sc;
    const int Sk = min(max(((len_t)a.seqlens_k)[b], 0), (int)p.seqlen_kv);
    const int diag = Sk - Sq;

    // this lane's row
    const int rg = rb * kDecRows + r;
    const bool row_ok = rg < a.rows;
    const int pos = row_ok ? rg % Sq : 0;
    const int lim = (kCausal && row_ok) ? min(Sk - 1, pos + diag) : Sk - 1;  // last visible key

    // ---- this wave's tiles: a contiguous quarter of the split's equal share of the sequence ------
    const int n_tiles = (Sk + kDecKeys - 1) / kDecKeys;
    const int tps = (n_tiles + a.n_split - 1) / a.n_split;
    const int s_lo = min(split * tps, n_tiles), s_hi = min(s_lo + tps, n_tiles);
    const int per_wave = (s_hi - s_lo + kDecWaves - 1) / kDecWaves;
    const int t_lo = min(s_lo + wave * per_wave, s_hi), t_hi = min(t_lo + per_wave, s_hi);

    const int ks_ = (int)p.k_seqlen_stride, vs_ = (int)p.v_seqlen_stride;
    PagedKv8 pages(p, a, b, hkv, t_lo, t_hi);

    // ---- LDS-DMA source offsets (lane-linear destination, swizzle on the source) ---------------
    constexpr int ROWS_PER_PIECE = 1024 / RB;
    int kvo[NP], vvo[NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        const int row = n * ROWS_PER_PIECE + (16 * lane) / RB;
        const int slot = ((16 * lane) % RB) / 16;
        const int kch = FG::k_off(row, slot) % RB / 16;  // (the XOR swizzles are involutions)
        const int vch = FG::v_off(row, slot) % RB / 16;
        kvo[n] = (kExactD || kch * 16 < D) ? row * ks_ + 16 * kch : 0x7ffffff0;
        vvo[n] = (kExactD || vch * 16 < D) ? row * vs_ + 16 * vch : 0x7ffffff0;
    }
    char *ring = lds + wave * FG::kWaveLds;
    const uint32_t ring_u = lds_u32(ring);
    auto issue = [&](const int t) {
        const int key0 = t * kDecKeys;
        const int rows = min(Sk - key0, kDecKeys);
        const uint32_t dst = ring_u + (t & (R - 1)) * FG::kSlot;
        const char *kt, *vt;
        pages.tile(t, kt, vt);
        const rsrc_t kr = make_rsrc(kt, slab_bytes8(rows, ks_, D));
        const rsrc_t vr = make_rsrc(vt, slab_bytes8(rows, vs_, D));
        if (a.flags & kDecNt) {
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one_nt(kr, dst + n * 1024, kvo[n], n == 0);
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one_nt(vr, dst + FG::kTile + n * 1024, vvo[n], n == 0);
        } else {
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one(kr, dst + n * 1024, kvo[n], n == 0);
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one(vr, dst + FG::kTile + n * 1024, vvo[n], n == 0);
        }
    };
    // ---- Q: the row block's 32 rows by LDS-DMA into a shared K-swizzled 16-bit image, as fa_decode ----
    {
        constexpr int QROWS_PER_PIECE = 1024 / QRB;
        constexpr int QPW = kDecRows * QRB / 1024 / kDecWaves;
        const int64_t qspan = ((int64_t)(a.g - 1) * p.q_head_stride + (int64_t)(Sq - 1) * p.q_seqlen_stride + D) * 2;
        const rsrc_t qr = make_rsrc((const char *)p.q_ptr + 2 * ((int64_t)b * p.q_batch_stride +
                                                                 (int64_t)hkv * a.g * p.q_head_stride),
                                    (uint32_t)qspan);
#pragma unroll
        for (int n = 0; n < QPW; ++n) {
            const int piece = wave * QPW + n;
            const int row = piece * QROWS_PER_PIECE + (16 * lane) / QRB;
            const int slot = ((16 * lane) % QRB) / 16;
            const int ch = G::k_off(row, slot) % QRB / 16;
            const int rq = rb * kDecRows + row;
            const int off = (rq < a.rows && (kExactD || ch * 8 < D))
                                ? 2 * ((rq / Sq) * (int)p.q_head_stride + (rq % Sq) * (int)p.q_seqlen_stride) + 16 * ch
                                : 0x7ffffff0;
            dma_one(qr, lds_u32(qlds) + piece * 1024, off, n == 0);
        }
    }
    // the ring's first tiles; the counted wait retires the Q pieces (issued first) and leaves them in flight
    const int n_pre = min(t_hi - t_lo, R);
    for (int i = 0; i < n_pre; ++i) issue(t_lo + i);
    wait_tiles<2 * NP>(n_pre);
    __syncthreads();  // every wave's Q pieces landed
    // B operand of S^T = K.Q^T in K's d order: lane (h, r) holds Q[row r][32 j + 16 h + 8 e .. + 7] for
    // k-step 2 j + e
    u32x4 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const u32x4 *)(qlds + G::k_off(r, 4 * (ks >> 1) + 2 * h + (ks & 1)));

    // ---- per-lane LDS fragment addresses --------------------------------------------------------
    int v_addr[DTL];
    {
        const int g4 = lane >> 4, q = (lane >> 1) & 7, pp = lane & 1;
        const int row0 = 4 * (g4 >> 1) + (q & 3) + 8 * (q >> 2);
#pragma unroll
        for (int dt = 0; dt < DTL; ++dt) v_addr[dt] = FG::v_off(row0, 2 * dt + (g4 & 1)) + 8 * pp;
    }
    int k_addr[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) k_addr[j] = FG::k_off(r, 2 * j + h);

    f32x16 o[DTL];
#pragma unroll
    for (int dt = 0; dt < DTL; ++dt) o[dt] = (f32x16){};
    float m_use = kNeg, msc = 0.f, l_run = 0.f;

    for (int t = t_lo; t < t_hi; ++t) {
        // tile t landed (the younger tiles of the ring may still be in flight)
        wait_tiles<2 * NP>(min(t_hi - 1 - t, R - 1));
        const char *K = ring + (t & (R - 1)) * FG::kSlot;
        const char *V = K + FG::kTile;
        u32x4 k8[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) k8[j] = *(const u32x4 *)(K + k_addr[j]);
        u32x2 v8[2][DTL];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int dt = 0; dt < DTL; ++dt) v8[kk][dt] = tr8_read(V + kk * 16 * RB + v_addr[dt]);
        // the slot is free once its bytes are in registers: refill it with tile t + R
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t + R < t_hi) issue(t + R);

        f32x16 s = {};
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            s = DT::mfma(widen8<DT>(k8[j][0], k8[j][1]), qf[2 * j], s);
            s = DT::mfma(widen8<DT>(k8[j][2], k8[j][3]), qf[2 * j + 1], s);
        }

        const int key0 = t * kDecKeys;
        // lane (h, r) holds keys key0 + (i & 3) + 8 (i >> 2) + 4 h of row r
        if (__builtin_amdgcn_ballot_w64(key0 + kDecKeys - 1 > lim)) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (key0 + (i & 3) + 8 * (i >> 2) + 4 * h > lim) s[i] = kNeg;
        }
        float mx = fmaxf(s[0], s[1]);
#pragma unroll
        for (int i = 2; i < 16; ++i) mx = fmaxf(mx, s[i]);
        if (__builtin_amdgcn_ballot_w64(mx > m_use + thr_raw)) {
            const float m_new = fmaxf(m_use, pair_max(mx));
            const float msc_new = (m_new <= 0.5f * kNeg) ? 0.f : m_new * sc;
            const float alpha = (m_use <= 0.5f * kNeg) ? 0.f : __builtin_amdgcn_exp2f(msc - msc_new);
            m_use = m_new;
            msc = msc_new;
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < DTL; ++dt) o[dt] *= alpha;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], sc, -msc));
        float ls = s[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) ls += s[i];
        l_run += ls;
        u32x4 pf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
            pf[kk] = (u32x4){DT::pack(s[8 * kk + 0], s[8 * kk + 1]), DT::pack(s[8 * kk + 2], s[8 * kk + 3]),
                             DT::pack(s[8 * kk + 4], s[8 * kk + 5]), DT::pack(s[8 * kk + 6], s[8 * kk + 7])};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int dt = 0; dt < DTL; ++dt) o[dt] = DT::mfma(widen8<DT>(v8[kk][dt][0], v8[kk][dt][1]), pf[kk], o[dt]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- merge the 4 wave partials in LDS (fa_decode's, with v_descale in the final 1 / l) --------
    __syncthreads();  // every wave is done with its ring
    float *ow = (float *)lds;  // [wave][row][kD]
    {
        const float l_tot = pair_sum(l_run);
        if (h == 0) {
            ml[wave][r][0] = (m_use <= 0.5f * kNeg) ? kNeg : msc;
            ml[wave][r][1] = l_tot;
        }
#pragma unroll
        for (int dt = 0; dt < DTL; ++dt)
#pragma unroll
            for (int grp = 0; grp < 4; ++grp) {
                const int d = dt * 32 + 8 * grp + 4 * h;
                *(float4 *)(ow + (wave * kDecRows + r) * kD + d) =
                    make_float4(o[dt][4 * grp], o[dt][4 * grp + 1], o[dt][4 * grp + 2], o[dt][4 * grp + 3]);
            }
    }
    __syncthreads();

    constexpr int DPT = kD / 8;  // d values per thread: thread (row = tid / 8, part = tid % 8)
    const int row = tid >> 3, part = tid & 7;
    float M = kNeg;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) M = fmaxf(M, ml[w][row][0]);
    float wgt[kDecWaves], L = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) {
        const float mw = ml[w][row][0];
        wgt[w] = (mw <= 0.5f * kNeg) ? 0.f : __builtin_amdgcn_exp2f(mw - M);
        L += wgt[w] * ml[w][row][1];
    }
    float acc[DPT];
#pragma unroll
    for (int i = 0; i < DPT; ++i) acc[i] = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) {
        const float *src = ow + (w * kDecRows + row) * kD + part * DPT;
#pragma unroll
        for (int i = 0; i < DPT; i += 4) {
            const float4 x = *(const float4 *)(src + i);
            acc[i] += wgt[w] * x.x;
            acc[i + 1] += wgt[w] * x.y;
            acc[i + 2] += wgt[w] * x.z;
            acc[i + 3] += wgt[w] * x.w;
        }
    }
    const float inv = L > 0.f ? vds / L : 0.f;
    const int rg2 = rb * kDecRows + row;
    if (a.n_split == 1) {
        if (rg2 < a.rows) {
            const int hq2 = hkv * a.g + rg2 / Sq, pos2 = rg2 % Sq;
            char *orow = (char *)p.o_ptr + 2 * ((int64_t)b * p.o_batch_stride + (int64_t)hq2 * p.o_head_stride +
                                                (int64_t)pos2 * p.o_seqlen_stride);
#pragma unroll
            for (int i = 0; i < DPT; i += 8) {
                const int d = part * DPT + i;
                if (kExactD || d < D) {
                    const u32x4 w4 = {DT::pack(acc[i] * inv, acc[i + 1] * inv), DT::pack(acc[i + 2] * inv, acc[i + 3] * inv),
                                      DT::pack(acc[i + 4] * inv, acc[i + 5] * inv),
                                      DT::pack(acc[i + 6] * inv, acc[i + 7] * inv)};
                    *(u32x4 *)(orow + 2 * d) = w4;
                }
            }
        }
    } else {
        if (rg2 < a.rows) {
            const size_t slot = ((size_t)unit * a.n_split + split) * kDecRows + row;
            float *dst = a.ws_o + slot * kD + part * DPT;
#pragma unroll
            for (int i = 0; i < DPT; i += 4)
                *(float4 *)(dst + i) = make_float4(acc[i] * inv, acc[i + 1] * inv, acc[i + 2] * inv, acc[i + 3] * inv);
            if (part == 0) a.ws_lse[slot] = L > 0.f ? M + __builtin_amdgcn_logf(L) : kNeg;  // log2
        }
        if constexpr (kFuse) {
            // fused merge, as fa_decode: the last arrival of the unit merges its splits' partials
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                const uint32_t old = __hip_atomic_fetch_add(a.cnt + unit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last_wg = old + 1 == (uint32_t)a.n_split;
                if (last_wg) __hip_atomic_store(a.cnt + unit, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            if (last_wg) decode_merge<DT, kD, kExactD>(p, a, unit, b, hkv, rb);
        }
    }
}

// as launch_decode_paged: the FP8 kernel (+ the split combine when a.n_split > 1 and the merge is not fused)
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8(const fa_fwd_params &p, PagedFp8DecArgs a, void *ws, hipStream_t stream) {
    const int64_t units = decode_units(p, a);
    if (a.n_split > 1) {
        const int64_t slots = units * a.n_split * kDecRows;
        a.ws_o = (float *)ws;
        a.ws_lse = (float *)((char *)ws + slots * kD * 4);
    }
    if (a.n_split > 1 && knobs().dec_fuse && same_xcd_placement()) {
        unsigned *err = nullptr;
        a.cnt = split_sync_area(stream, units * 4, &err);
    }
    set_last_dec_fused(a.cnt != nullptr);
    const int64_t grid = a.cnt ? 8 * ((units + 7) / 8) * a.n_split : units * a.n_split;
    if (a.cnt)
        hipLaunchKernelGGL((fa_decode_fp8kv<DT, C, kD, kExact, true>), dim3((uint32_t)grid), dim3(256), 0, stream, p, a);
    else
        hipLaunchKernelGGL((fa_decode_fp8kv<DT, C, kD, kExact>), dim3((uint32_t)grid), dim3(256), 0, stream, p, a);
    if (a.n_split > 1 && !a.cnt)
        hipLaunchKernelGGL((fa_decode_combine<DT, kD, kExact>),
                           dim3((uint32_t)(p.batch_size * p.num_heads_kv * ((a.rows + 3) / 4))), dim3(256), 0, stream,
                           p, static_cast<const DecArgs &>(a));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    set_last_path(a.n_split > 1 ? kPathDecodePagedFp8Split : kPathDecodePagedFp8);
    return FA_OK;
}

}  // namespace fa
