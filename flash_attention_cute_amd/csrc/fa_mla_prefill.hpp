#pragma once
// fa_mla_prefill.hpp -- multi-head latent attention (MLA) prefill over packed sequences, gfx950
// (include/fa_gfx950_mla_prefill.h). No reference counterpart.
//
// The prompt pass of an MLA model runs in the NON-absorbed form: per head 192 score columns (128 "nope" + 64
// RoPE) and 128 value columns, multi-head, packed, causal (bottom-right) or not. fa_fwd_w4 is built around
// Dqk == Dv <= 128; this kernel is built around the 192 / 128 split and around a key row that comes from TWO
// places (the nope columns of one tensor, the RoPE columns of another, possibly shared by every head):
//
//   * work: a workgroup of 4 wave64s takes (sequence b, q-head, block of 128 kNRB query rows); wave w owns the
//     kNRB blocks of 32 rows [32 kNRB w, 32 kNRB (w + 1)) of it and runs the whole key loop for them: S^T = K.Q^T
//     (Q fragments as the B operand, in registers for the whole loop: 12 k-steps x 4 VGPRs per row block) and
//     O^T += V^T.P^T (4 d-tiles x 16 fp32 per row block), decode_softmax of fa_decode.hpp per 32-key half of a
//     64-key tile. No wave needs another's scores: ONE barrier per tile ("tile landed"). With kNRB = 2 a K / V
//     fragment read from LDS feeds two MFMAs instead of one;
//   * the tile ring (kMpRing = 3 stages of 40 KiB) is shared by the four waves, filled by LDS-DMA, two tiles in
//     flight while one is computed on. A stage is THREE images, because a buffer descriptor bounds one range
//     and a key row has two: nope [64][256 B] (Geo<128>::k_off), rope [64][128 B] (Geo<64>::k_off) -- both read
//     by ds_read_b128 with lane r on key row r -- and V [64][256 B] (Geo<128>::v_off), read transposed by
//     ds_read_b64_tr_b16. All three swizzles are fa_fwd_w4's, conflict-free for exactly these reads (DESIGN.md
//     section 4). Each wave issues 10 of a tile's 40 pieces (4 nope, 2 rope, 4 V); one k tensor of 192 columns is
//     the case rope base = nope base + 128 elements with the same strides;
//   * every descriptor is bounded to the rows of the tile that belong to the sequence: the rows past its end
//     read 0 for K and V (never the next sequence's rows, never past total_k: no 0 * NaN in P.V);
//   * causal: a workgroup runs the tiles up to its last row's diagonal, a wave only those up to ITS last row's
//     (it still meets the barriers of the rest), and decode_mask touches a half tile only where a lane's bound
//     cuts it (a wave-uniform ballot): interior tiles run unmasked;
//   * grid: 1-D, one item per (sequence, q-head, block), a sequence's last block -- the heaviest -- first, decoded
//     XCD-aware: XCD blockIdx & 7 takes a contiguous eighth of the items, so every XCD gets whole heads (the same
//     load) and the blocks of a head, and the q-heads of a kv group, share one L2;
//   * epilogue: O^T / l rounded once to T, 8-byte stores; the LSE as ln 2 (m s' + log2 l), -inf and O = 0 for a
//     row without a visible key. Rows past Sq_b, and blocks past a sequence's last row, load and store nothing.
#include "fa_decode.hpp"
#include "fa_gfx950_mla_prefill.h"

namespace fa {

constexpr int kMpDqk = 192, kMpDv = 128, kMpNope = 128, kMpRope = 64;
constexpr int kMpKeys = 64;  // keys per tile: two 32-key halves, each one decode_softmax step
constexpr int kMpRing = 3;
constexpr int kMpNopeOff = 0, kMpRopeOff = kMpKeys * kMpNope * 2, kMpVOff = kMpRopeOff + kMpKeys * kMpRope * 2;
constexpr int kMpStage = kMpVOff + kMpKeys * kMpDv * 2;                 // 40 KiB
constexpr int kMpNopeP = 4, kMpRopeP = 2, kMpVP = 4;                    // LDS-DMA pieces per wave per tile
constexpr int kMpPieces = kMpNopeP + kMpRopeP + kMpVP;                  // 10
constexpr int kMpKSteps = kMpDqk / 16, kMpNopeSteps = kMpNope / 16;     // 12, 8
constexpr int kMpDTiles = kMpDv / 32;                                   // 4
static_assert(kMpPieces * 4 * 1024 == kMpStage, "the four waves' pieces are one stage");

// the kernel's arguments: fa_mla_prefill_params narrowed to what the device reads (strides in elements)
struct MlaPrefillArgs {
    const char *q, *kn, *kr, *v;
    char *o;
    float *lse;
    const int32_t *cu_q, *cu_k;
    int64_t q_rs, q_hs, kn_hs, kr_hs, v_hs, o_rs, o_hs, lse_hs, lse_rs;
    int kn_rs, kr_rs, v_rs;
    int total_q, total_k, hq, g, causal;
    int n_blk, n_items, per;  // the plan: blocks per (sequence, q-head), items in all, items per XCD
    float sc;
};

template <class DT, int kNRB>
__global__ __launch_bounds__(256, 1) void fa_mla_prefill(const MlaPrefillArgs a) {
    __shared__ __attribute__((aligned(1024))) char ring[kMpRing * kMpStage];
    constexpr int kWaveRows = kDecRows * kNRB, kRows = 4 * kWaveRows;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    // the sequence: both cu arrays clamped to [0, total] and to non-decreasing (scalar loads)
    typedef const __attribute__((address_space(4))) int32_t *sload_t;
    // work item: XCD (blockIdx & 7, how the hardware deals workgroups) takes a contiguous range of a.per items of
    // the order (sequence, q-head, block with the sequence's last block first), so the blocks of a head -- and the
    // q-heads of a kv group -- stream one K / V through one L2, and every XCD gets heads whole: the same load
    const int item = (int)(blockIdx.x & 7) * a.per + (int)(blockIdx.x >> 3);
    if (item >= a.n_items) return;
    const int unit = item / a.n_blk;
    const int b = unit / a.hq, hq = unit % a.hq, hkv = hq / a.g;
    const int q0 = min(max(((sload_t)a.cu_q)[b], 0), a.total_q);
    const int Sq = min(max(((sload_t)a.cu_q)[b + 1], q0), a.total_q) - q0;
    const int k0 = min(max(((sload_t)a.cu_k)[b], 0), a.total_k);
    const int Sk = min(max(((sload_t)a.cu_k)[b + 1], k0), a.total_k) - k0;
    // the sequence's last block first: with a causal mask it is the longest
    const int m0 = (a.n_blk - 1 - item % a.n_blk) * kRows;
    if (m0 >= Sq) return;
    const int diag = Sk - Sq;
    const float sc = a.sc, thr_raw = kRescaleThr / sc;

    // tiles of the workgroup (up to its last row's bound) and of this wave (up to its own last row's)
    const int top = a.causal ? min(Sk - 1, min(m0 + kRows, Sq) - 1 + diag) : Sk - 1;
    const int n_t = top >= 0 ? top / kMpKeys + 1 : 0;
    const int mw0 = m0 + wave * kWaveRows;
    const int wtop = a.causal ? min(Sk - 1, min(mw0 + kWaveRows, Sq) - 1 + diag) : Sk - 1;
    const int w_nt = (mw0 < Sq && wtop >= 0) ? wtop / kMpKeys + 1 : 0;

    // this lane's row of each block, and Q: the B operand of S^T = K.Q^T, lane (h, r) holds
    // Q[row r][16 ks + 8 h .. + 7], straight from global memory (rows past the end are 0)
    int lim[kNRB];
    bool row_ok[kNRB];
    u32x4 qf[kNRB][kMpKSteps];
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
        const int m = mw0 + rb * kDecRows + r;
        row_ok[rb] = m < Sq;
        lim[rb] = a.causal ? min(Sk - 1, m + diag) : Sk - 1;
        const char *qrow = a.q + 2 * ((int64_t)(q0 + m) * a.q_rs + (int64_t)hq * a.q_hs) + 16 * h;
#pragma unroll
        for (int ks = 0; ks < kMpKSteps; ++ks)
            qf[rb][ks] = row_ok[rb] ? *(const u32x4 *)(qrow + 32 * ks) : (u32x4){0u, 0u, 0u, 0u};
    }
    // Q landed, and the compiler knows it (see fa_mla_decode): from here on only LDS-DMA counts in vmcnt
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
        for (int ks = 0; ks < kMpKSteps; ++ks) asm volatile("" : "+v"(qf[rb][ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- LDS-DMA: lane-linear destination, the swizzles on the source offsets (each an XOR: its own inverse) ----
    using GN = Geo<kMpNope>;
    using GR = Geo<kMpRope>;
    using GV = Geo<kMpDv>;
    const int kn_rs2 = a.kn_rs * 2, kr_rs2 = a.kr_rs * 2, v_rs2 = a.v_rs * 2;  // row strides, bytes
    int voff[kMpPieces];
#pragma unroll
    for (int n = 0; n < kMpNopeP; ++n) {
        const int byte = (wave * kMpNopeP + n) * 1024 + 16 * lane, row = byte >> 8;
        voff[n] = row * kn_rs2 + (GN::k_off(row, (byte >> 4) & 15) - row * 256);
    }
#pragma unroll
    for (int n = 0; n < kMpRopeP; ++n) {
        const int byte = (wave * kMpRopeP + n) * 1024 + 16 * lane, row = byte >> 7;
        voff[kMpNopeP + n] = row * kr_rs2 + (GR::k_off(row, (byte >> 4) & 7) - row * 128);
    }
#pragma unroll
    for (int n = 0; n < kMpVP; ++n) {
        const int byte = (wave * kMpVP + n) * 1024 + 16 * lane, row = byte >> 8;
        voff[kMpNopeP + kMpRopeP + n] = row * v_rs2 + (GV::v_off(row, (byte >> 4) & 15) - row * 256);
    }
    const uint32_t ring_u = lds_u32(ring);
    const char *kn_seq = a.kn + 2 * ((int64_t)k0 * a.kn_rs + (int64_t)hkv * a.kn_hs);
    const char *kr_seq = a.kr + 2 * ((int64_t)k0 * a.kr_rs + (int64_t)hkv * a.kr_hs);
    const char *v_seq = a.v + 2 * ((int64_t)k0 * a.v_rs + (int64_t)hkv * a.v_hs);
    auto issue = [&](const int t, const int slot) {
        const int key0 = t * kMpKeys, rows = min(Sk - key0, kMpKeys);
        const rsrc_t nr = make_rsrc_u(kn_seq + (int64_t)key0 * kn_rs2, slab_bytes(rows, a.kn_rs, kMpNope));
        const rsrc_t rr = make_rsrc_u(kr_seq + (int64_t)key0 * kr_rs2, slab_bytes(rows, a.kr_rs, kMpRope));
        const rsrc_t vr = make_rsrc_u(v_seq + (int64_t)key0 * v_rs2, slab_bytes(rows, a.v_rs, kMpDv));
        const uint32_t dst = ring_u + slot * kMpStage;
#pragma unroll
        for (int n = 0; n < kMpNopeP; ++n)
            dma_one(nr, dst + kMpNopeOff + (wave * kMpNopeP + n) * 1024, voff[n], n == 0);
#pragma unroll
        for (int n = 0; n < kMpRopeP; ++n)
            dma_one(rr, dst + kMpRopeOff + (wave * kMpRopeP + n) * 1024, voff[kMpNopeP + n], n == 0);
#pragma unroll
        for (int n = 0; n < kMpVP; ++n)
            dma_one(vr, dst + kMpVOff + (wave * kMpVP + n) * 1024, voff[kMpNopeP + kMpRopeP + n], n == 0);
    };

    // fragment addresses within a stage: K (ds_read_b128, lane r on key row r of a 32-key half; the swizzles read
    // row bits below 16, so the second half is a constant further) and V^T (ds_read_b64_tr_b16)
    int k_addr[kMpKSteps], v_addr[kMpDTiles];
    {
        const int g4 = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
        for (int ks = 0; ks < kMpNopeSteps; ++ks) k_addr[ks] = kMpNopeOff + GN::k_off(r, 2 * ks + h);
#pragma unroll
        for (int ks = kMpNopeSteps; ks < kMpKSteps; ++ks)
            k_addr[ks] = kMpRopeOff + GR::k_off(r, 2 * (ks - kMpNopeSteps) + h);
#pragma unroll
        for (int dt = 0; dt < kMpDTiles; ++dt)
            v_addr[dt] = kMpVOff + GV::v_off(4 * (g4 >> 1) + qq, dt * 4 + 2 * (g4 & 1) + (pp >> 1)) + 8 * (pp & 1);
    }

    f32x16 o[kNRB][kMpDTiles];
    float m_use[kNRB], msc[kNRB], l_run[kNRB];
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
#pragma unroll
        for (int dt = 0; dt < kMpDTiles; ++dt) o[rb][dt] = (f32x16){};
        m_use[rb] = kNeg, msc[rb] = 0.f, l_run[rb] = 0.f;
    }

    // the ring's first two tiles
    if (0 < n_t) issue(0, 0);
    if (1 < n_t) issue(1, 1);
    int slot = 0, slot_in = 2;  // slot of tile t; slot tile t + 2 goes to
    for (int t = 0; t < n_t; ++t) {
        // this wave's pieces of tile t landed (tile t + 1's, the youngest 10, may still be in flight); after the
        // barrier every wave's have, and every wave is done with tile t - 1: its slot takes tile t + 2
        if (t + 1 < n_t) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kMpPieces) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 2 < n_t) issue(t + 2, slot_in);
        const char *T = ring + slot * kMpStage;

        if (t < w_nt) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                // S^T of 32 keys: nope rows are 256 bytes, rope rows 128
                u32x4 kf[kMpKSteps];
#pragma unroll
                for (int ks = 0; ks < kMpKSteps; ++ks)
                    kf[ks] = *(const u32x4 *)(T + half * kDecKeys * (ks < kMpNopeSteps ? 256 : 128) + k_addr[ks]);
                u32x4 pf[kNRB][2];
#pragma unroll
                for (int rb = 0; rb < kNRB; ++rb) {
                    f32x16 s = {};
#pragma unroll
                    for (int ks = 0; ks < kMpKSteps; ++ks) s = DT::mfma(kf[ks], qf[rb][ks], s);
                    decode_mask<false>(s, t * kMpKeys + half * kDecKeys, h, lim[rb], 0, 0);
                    decode_softmax<DT, kMpDTiles>(s, o[rb], m_use[rb], msc[rb], l_run[rb], sc, thr_raw, pf[rb]);
                }
                // O^T += V^T.P^T over the half's 32 keys, V^T read transposed
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    u32x4 va[kMpDTiles];
#pragma unroll
                    for (int dt = 0; dt < kMpDTiles; ++dt) {
                        const char *vrow = T + (half * kDecKeys + kk * 16) * 256 + v_addr[dt];
                        const u32x2 lo = tr_read(vrow), hi = tr_read(vrow + 8 * 256);
                        va[dt] = (u32x4){lo[0], lo[1], hi[0], hi[1]};
                    }
#pragma unroll
                    for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
                        for (int dt = 0; dt < kMpDTiles; ++dt) o[rb][dt] = DT::mfma(va[dt], pf[rb][kk], o[rb][dt]);
                }
            }
        }
        slot = slot == kMpRing - 1 ? 0 : slot + 1;
        slot_in = slot_in == kMpRing - 1 ? 0 : slot_in + 1;
    }

    // ---- epilogue: lane (h, r) holds o[dt][4 grp + j] = O^T[d = 32 dt + 8 grp + 4 h + j][row r] ----
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
        const float L = pair_sum(l_run[rb]);
        const float M = (m_use[rb] <= 0.5f * kNeg) ? kNeg : msc[rb];
        const float inv = L > 0.f ? 1.f / L : 0.f;
        if (!row_ok[rb]) continue;
        const int64_t row = q0 + mw0 + rb * kDecRows + r;
        char *orow = a.o + 2 * (row * a.o_rs + (int64_t)hq * a.o_hs) + 8 * h;
#pragma unroll
        for (int dt = 0; dt < kMpDTiles; ++dt)
#pragma unroll
            for (int grp = 0; grp < 4; ++grp) {
                const u32x2 w2 = {DT::pack(o[rb][dt][4 * grp] * inv, o[rb][dt][4 * grp + 1] * inv),
                                  DT::pack(o[rb][dt][4 * grp + 2] * inv, o[rb][dt][4 * grp + 3] * inv)};
                *(u32x2 *)(orow + 2 * (32 * dt + 8 * grp)) = w2;
            }
        if (a.lse && h == 0) {
            const float v = (M + __builtin_amdgcn_logf(L)) * 0.69314718055994531f;
            *((uint32_t *)a.lse + (int64_t)hq * a.lse_hs + row * a.lse_rs) = L > 0.f ? __float_as_uint(v) : 0xff800000u;
        }
    }
}

}  // namespace fa
