#pragma once
// fa_mla_sparse_mixed.hpp -- fa_mla_sparse_decode (fa_mla_sparse.hpp) over the MIXED latent row of DeepSeek-V3.2's
// FP8 cache (FlashMLA's sparse-decode row, vLLM's fp8_ds_mla), gfx950 (include/fa_gfx950_mla_mixed.h). A token is
// 656 BYTES: 512 e4m3 bytes (the compressed-KV columns), four fp32 scales (scale j covers columns [128 j, 128 j +
// 128): value = e4m3 * scale[j]) and 64 bf16 RoPE columns that are not quantised. q and o are bf16.
//
// The work split (batch, position, split of the list's topk / 32 tiles dealt round-robin, group of up to 64 heads;
// XCD placement), the scalar scan of a tile's entries into the visibility mask, the skip of a tile without a key,
// the translation through the block table, the per-lane 64-bit LDS-DMA addresses, sparse_mask, the four-wave
// column split with the partial-S^T exchange, the ring over ISSUED tiles with counted vmcnt waits, the epilogue and
// the workspace are fa_mla_sparse_decode's (included, not edited). What the mixed row changes:
//
//   * the LDS image. 656 bytes are 41 16-byte chunks: no whole number of 1 KiB LDS-DMA pieces per wave, and no
//     whole or quarter number of 256-byte bank rows. The source addresses are per lane, so the three parts of a
//     row land in three REGIONS of a tile's image (20.5 KiB), each with the swizzle its reads need:
//       - nope, 32 rows x 512 bytes at 0 (mix_nope_off): chunk c of row r at r * 512 + 16 (c ^ f(r)), f(r) =
//         r2 | r0 << 1 | r1 << 2 | r3 << 3 (bits of r; a permutation of r's low four bits). A row is exactly two
//         bank rows, so every row starts at bank slot 0 and the XOR alone spreads the rows. (a) The key read is
//         ds_read_b128, lane r on key r, one chunk c per half-wave: the 16 rows of a lane group (in either order
//         the hardware may take them: 16 consecutive rows, or {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}) have 16
//         distinct r & 15, so 16 distinct f(r) and 16 distinct 16-byte bank slots (c ^ f(r)) & 15. (b) The V^T read
//         is ds_read_b64_tr_b8: a 32-lane half reads rows R + {0..3, 8..11} (R a multiple of 4), an aligned pair
//         of chunks (32 bytes) each; the pair sits at 32-byte slot ((c >> 1) ^ (f(r) >> 1)) & 7, and f(r) >> 1 =
//         r0 | r1 << 1 | r3 << 2 takes its eight values once over those rows (bit 0 of f, r2, is the same for all
//         eight and only swaps the chunks of a pair): the eight 32-byte slots once each. Rows 16 further down have
//         the same f: a transposed read's second key step is a constant offset;
//       - RoPE, 32 rows x 128 bytes at 16 KiB (mix_rope_off): the 1 KiB of wave w's eight rows holds chunk c of row
//         r = 8 w + j at 128 (c ^ (w & 1)) + 16 j -- the rows interleaved chunk by chunk, so that LDS-DMA lane l
//         carries row l & 7, the same row pick as the scale piece. The key read (ds_read_b128, lane r on key r, one
//         chunk per half-wave) lands on bank slot 8 ((c ^ r3) & 1) + (r & 7): 16 rows with distinct r & 15 take the
//         16 slots once each;
//       - scales, 32 rows x 16 bytes at 20 KiB: lane (h, r) reads scale[key][wave] of its 16 keys, one address per
//         half-wave and read (a broadcast), the two halves 64 bytes apart;
//   * the gather: wave w brings tile rows 8 w .. 8 w + 7 as SIX LDS-DMA issues: four nope pieces (two rows each:
//     the lower half-wave one row, the upper the next), one RoPE piece (lane l: row l & 7, chunk l >> 3) and one
//     scale piece of 128 bytes with EXEC narrowed to lanes 0 .. 7 (lane l: row l). The ring is three tiles (61.5
//     KiB), two in flight while one is computed on; the counted wait is vmcnt(6);
//   * the score columns: wave w takes nope columns [128 w, 128 w + 128) -- scale tile w -- as four ds_read_b128
//     widened (widen8, exact) into eight 32x32x16 k-steps, multiplies the lane's 16 partial scores by
//     scale[key][w] in fp32, and then runs the RoPE k-step (columns [16 w, 16 w + 16), bf16) with that as its
//     accumulator: nine k-steps and nine Q fragments per wave, as in fa_mla_sparse_decode. Q's fragments are
//     loaded in K's byte order (fa_mla_fp8.hpp);
//   * the value columns: wave w owns output columns [128 w, 128 w + 128), scale tile w again, so the scale rides on
//     P: mixed_softmax is decode_softmax with a per-key factor applied where P is packed (the row sum takes the
//     unscaled p), and the e4m3 V^T bytes are widened exactly. The same 16 scale registers serve both uses;
//   * an entry that is not a key points at mla_mixed_zero_row, 656 zero bytes of this translation unit: its bytes,
//     its scales and its RoPE columns read 0, and no pool byte is read for it.
#include "fa_decode_paged_fp8.hpp"
#include "fa_gfx950_mla_mixed.h"
#include "fa_mla_sparse.hpp"

namespace fa {

constexpr int kMixRowBytes = 656;                       // a token of the pool
constexpr int kMixScaleSrc = 512, kMixRopeSrc = 528;    // byte offsets within it
constexpr int kMixNopeRow = 512;                        // bytes of a row of the nope region
constexpr int kMixRopeOff = kDecKeys * kMixNopeRow;     // 16 KiB: the RoPE region
constexpr int kMixScaleOff = kMixRopeOff + kDecKeys * 128;  // 20 KiB: the scale region
constexpr int kMixTile = kMixScaleOff + kDecKeys * 16;  // 20.5 KiB
constexpr int kMixRing = 3;
constexpr int kMixPieces = 6;                           // LDS-DMA issues per wave and tile: 4 nope, RoPE, scales
constexpr int kMixPairs = 4;                            // b128 pairs of nope k-steps per wave

__device__ __attribute__((aligned(16))) uint32_t mla_mixed_zero_row[kMixRowBytes / 4];

// the nope region's swizzle: a permutation of the row's low four bits
__device__ __forceinline__ int mix_f(const int row) {
    return ((row >> 2) & 1) | ((row & 3) << 1) | (((row >> 3) & 1) << 3);
}
// byte offset of 16-byte chunk ch (0 .. 31) of row `row` in the nope region of a tile's image
__device__ __forceinline__ int mix_nope_off(const int row, const int ch) {
    return row * kMixNopeRow + 16 * (ch ^ mix_f(row));
}
// byte offset of 16-byte chunk ch (0 .. 7) of row `row` in the RoPE region
__device__ __forceinline__ int mix_rope_off(const int row, const int ch) {
    return kMixRopeOff + 1024 * (row >> 3) + 128 * (ch ^ ((row >> 3) & 1)) + 16 * (row & 7);
}

// decode_softmax (fa_decode.hpp: the same max / rescale / l arithmetic) with a per-key factor ks on P where it is
// packed: P^T[key] = bf16(p[key] * ks[key]); the row sum takes p
template <int DTL>
__device__ __forceinline__ void mixed_softmax(f32x16 &s, f32x16 (&o)[DTL], float &m_use, float &msc, float &l_run,
                                              const float sc, const float thr_raw, const float (&ks)[16],
                                              u32x4 (&pf)[2]) {
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
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] *= ks[i];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
        pf[kk] = (u32x4){BF16::pack(s[8 * kk + 0], s[8 * kk + 1]), BF16::pack(s[8 * kk + 2], s[8 * kk + 3]),
                         BF16::pack(s[8 * kk + 4], s[8 * kk + 5]), BF16::pack(s[8 * kk + 6], s[8 * kk + 7])};
}

// sa.m.kv_ps / kv_rs count BYTES; q and o are bf16
template <int kNRB>
__global__ __launch_bounds__(256, 1) void fa_mla_sparse_decode_mixed(const MlaSparseArgs sa) {
    using DT = BF16;
    __shared__ __attribute__((aligned(1024))) char ring[kMixRing * kMixTile];
    __shared__ __attribute__((aligned(1024))) char xch[kNRB * kDecWaves * 4096];
    const MlaArgs &a = sa.m;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    // (b, pos, split) and head group hg: the head groups of one list are 8 workgroup ids apart
    const int kq = (int)(blockIdx.x >> 3);
    const int hg = kq % a.n_rg;
    const int u3 = ((kq / a.n_rg) << 3) | (int)(blockIdx.x & 7);
    if (u3 >= a.batch * a.Sq * a.n_split) return;
    const int split = u3 % a.n_split, bp = u3 / a.n_split;
    const int b = bp / a.Sq, pos = bp % a.Sq;
    const int u = b * a.n_split + split;  // the workspace's unit

    typedef const __attribute__((address_space(4))) int32_t *sload_t;  // (constant space: scalar loads)
    const int Sk = min(max(((sload_t)a.seqlens_k)[b], 0), a.cap_keys);
    const int lim = a.causal ? min(Sk - 1, pos + Sk - a.Sq) : Sk - 1;  // one limit: one position
    const uint32_t ulim = (uint32_t)lim;  // visible: (uint32_t)idx <= ulim, for lim >= 0
    const int t_end = lim >= 0 ? sa.n_tiles : 0;  // this split's tiles: split, split + n_split, ... below t_end
    const float sc = a.sc, thr_raw = kRescaleThr / sc;

    // this lane's head of each block, and Q: the B operand of S^T = K.Q^T in K's byte order, straight from global
    // memory: qf[2 j + e] = Q[row][128 wave + 32 j + 16 h + 8 e .. + 7], qf[8] = Q[row][512 + 16 wave + 8 h .. + 7]
    bool row_ok[kNRB];
    int hq_of[kNRB];
    u32x4 qf[kNRB][kMlaKSteps];
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
        const int hq = hg * kMlaGroupRows + rb * kDecRows + r;
        row_ok[rb] = hq < sa.Hq;
        hq_of[rb] = row_ok[rb] ? hq : 0;
        const char *qrow = a.q + 2 * ((int64_t)b * a.q_bs + (int64_t)hq_of[rb] * a.q_hs + (int64_t)pos * a.q_ss);
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks) {
            const int col = ks < 2 * kMixPairs ? 128 * wave + 32 * (ks >> 1) + 16 * h + 8 * (ks & 1)
                                               : kMlaDv + 16 * wave + 8 * h;
            qf[rb][ks] = row_ok[rb] ? *(const u32x4 *)(qrow + 2 * col) : (u32x4){0u, 0u, 0u, 0u};
        }
    }
    // Q landed, and the compiler knows it: from here on only LDS-DMA counts in vmcnt (see fa_mla_decode)
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks) asm volatile("" : "+v"(qf[rb][ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- the gather: this wave's six pieces of a tile are tile rows 8 wave .. 8 wave + 7. Nope piece n is rows 8
    // wave + 2 n (lanes 0 .. 31) and + 2 n + 1 (lanes 32 .. 63), image slot lane & 31, from source chunk slot ^
    // f(row); in the RoPE and scale pieces lane l carries row 8 wave + (l & 7) ----
    int nope_in[kMixPairs];
#pragma unroll
    for (int n = 0; n < kMixPairs; ++n) nope_in[n] = 16 * (r ^ mix_f(8 * wave + 2 * n + h));
    const int rope_in = kMixRopeSrc + 16 * ((lane >> 3) ^ (wave & 1));
    const sload_t list = (sload_t)(sa.indices + (int64_t)b * sa.idx_bs + (int64_t)pos * sa.idx_ss);
    const sload_t table = (sload_t)(a.block_table + (int64_t)b * a.bt_stride);
    const int last_page = a.num_pages - 1;
    const uint64_t zero_row = (uint64_t)(uintptr_t)mla_mixed_zero_row;
    const uint32_t ring_u = lds_u32(ring);
    auto issue = [&](const int t, const int slot) {
        uint64_t ra[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = list[kDecKeys * t + 8 * wave + j];
            const bool ok = (uint32_t)idx <= ulim;
            const int pi = !ok ? 0 : sa.page_shift >= 0 ? idx >> sa.page_shift : idx / sa.page_size;
            const int64_t page = min(max(table[pi], 0), last_page);
            const int64_t off = page * a.kv_ps + (int64_t)(idx - pi * sa.page_size) * a.kv_rs;
            ra[j] = ok ? (uint64_t)(uintptr_t)(a.kv + off) : zero_row;
        }
        uint64_t mine = ra[0];  // row 8 wave + (lane & 7)
#pragma unroll
        for (int j = 1; j < 8; ++j) mine = (lane & 7) == j ? ra[j] : mine;
        const uint32_t dst = ring_u + slot * kMixTile;
#pragma unroll
        for (int n = 0; n < kMixPairs; ++n)
            gather_one_nt((h ? ra[2 * n + 1] : ra[2 * n]) + (uint64_t)nope_in[n],
                          dst + (wave * kMixPairs + n) * 1024, n == 0);
        gather_one_nt(mine + (uint64_t)rope_in, dst + kMixRopeOff + wave * 1024, false);
        if (lane < 8) gather_one_nt(mine + (uint64_t)kMixScaleSrc, dst + kMixScaleOff + wave * 128, false);
    };
    // the visibility mask of tile t, from scalars
    auto scan = [&](const int t) {
        uint32_t vis = 0;
#pragma unroll
        for (int i = 0; i < kDecKeys; ++i) vis |= (uint32_t)list[kDecKeys * t + i] <= ulim ? 1u << i : 0u;
        return vis;
    };
    // the next live tile from the cursor on goes to `slot`: its mask, or 0 when the split has no more
    int t_next = split;
    auto fetch = [&](const int slot) {
        while (t_next < t_end) {
            const uint32_t vis = scan(t_next);
            t_next += a.n_split;
            if (vis) {
                issue(t_next - a.n_split, slot);
                return vis;
            }
        }
        return 0u;
    };

    // fragment addresses within a tile: K (ds_read_b128, lane r on key row r: four nope pairs and the RoPE
    // k-step), V^T (ds_read_b64_tr_b8, fa_mla_fp8.hpp's lane map) and the lane's 16 scales
    int k_addr[kMixPairs], v_addr[kMlaDTiles];
    const int rope_addr = mix_rope_off(r, 2 * wave + h);
    const int scale_addr = kMixScaleOff + 64 * h + 4 * wave;  // + 16 (key - 4 h)
    {
        const int g4 = lane >> 4, q = (lane >> 1) & 7, pp = lane & 1;
        const int row0 = 4 * (g4 >> 1) + (q & 3) + 8 * (q >> 2);
#pragma unroll
        for (int j = 0; j < kMixPairs; ++j) k_addr[j] = mix_nope_off(r, 8 * wave + 2 * j + h);
#pragma unroll
        for (int dt = 0; dt < kMlaDTiles; ++dt)
            v_addr[dt] = mix_nope_off(row0, 8 * wave + 2 * dt + (g4 & 1)) + 8 * pp;
    }

    f32x16 o[kNRB][kMlaDTiles];
    float m_use[kNRB], msc[kNRB], l_run[kNRB];
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
#pragma unroll
        for (int dt = 0; dt < kMlaDTiles; ++dt) o[rb][dt] = (f32x16){};
        m_use[rb] = kNeg, msc[rb] = 0.f, l_run[rb] = 0.f;
    }

    // the ring's first two live tiles; vis0: the tile computed on, vis1: the one behind it (0: none)
    uint32_t vis0 = fetch(0);
    uint32_t vis1 = vis0 ? fetch(1) : 0u;
    int slot = 0, slot_in = 2;
    while (vis0) {
        // this wave's pieces of the tile landed (the next live tile's, the youngest 6, may still be in flight);
        // after the barrier every wave's have, and every wave is done with the tile before: its slot is free
        if (vis1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kMixPieces) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const uint32_t vis2 = vis1 ? fetch(slot_in) : 0u;
        const char *T = ring + slot * kMixTile;

        // scale[key][wave] of this lane's keys (i & 3) + 8 (i >> 2) + 4 h: for the scores and for P
        float ksc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) ksc[i] = *(const float *)(T + scale_addr + 16 * ((i & 3) + 8 * (i >> 2)));

        // partial S^T over this wave's nine k-steps, to the exchange buffer (lane-linear 16-byte pieces)
        {
            u32x4 kf[kMixPairs];
#pragma unroll
            for (int j = 0; j < kMixPairs; ++j) kf[j] = *(const u32x4 *)(T + k_addr[j]);
            const u32x4 kr = *(const u32x4 *)(T + rope_addr);
#pragma unroll
            for (int rb = 0; rb < kNRB; ++rb) {
                f32x16 s = {};
#pragma unroll
                for (int j = 0; j < kMixPairs; ++j) {
                    s = DT::mfma(widen8<DT>(kf[j][0], kf[j][1]), qf[rb][2 * j], s);
                    s = DT::mfma(widen8<DT>(kf[j][2], kf[j][3]), qf[rb][2 * j + 1], s);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) s[i] *= ksc[i];
                s = DT::mfma(kr, qf[rb][2 * kMixPairs], s);
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4)
                    *(float4 *)(xch + ((rb * kDecWaves + wave) * 4 + q4) * 1024 + 16 * lane) =
                        make_float4(s[4 * q4], s[4 * q4 + 1], s[4 * q4 + 2], s[4 * q4 + 3]);
            }
        }
        __syncthreads();

        u32x4 pf[kNRB][2];
#pragma unroll
        for (int rb = 0; rb < kNRB; ++rb) {
            // the four partials in wave order: the same sum, bit for bit, in every wave
            f32x16 s;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                float4 x = *(const float4 *)(xch + ((rb * kDecWaves + 0) * 4 + q4) * 1024 + 16 * lane);
#pragma unroll
                for (int w = 1; w < kDecWaves; ++w) {
                    const float4 y = *(const float4 *)(xch + ((rb * kDecWaves + w) * 4 + q4) * 1024 + 16 * lane);
                    x.x += y.x, x.y += y.y, x.z += y.z, x.w += y.w;
                }
                s[4 * q4] = x.x, s[4 * q4 + 1] = x.y, s[4 * q4 + 2] = x.z, s[4 * q4 + 3] = x.w;
            }
            sparse_mask(s, vis0, h);
            mixed_softmax<kMlaDTiles>(s, o[rb], m_use[rb], msc[rb], l_run[rb], sc, thr_raw, ksc, pf[rb]);
        }

        // O^T += V^T.P^T over this wave's 128 value columns, V^T read transposed from the nope region
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            u32x4 va[kMlaDTiles];
#pragma unroll
            for (int dt = 0; dt < kMlaDTiles; ++dt) {
                const u32x2 v8 = tr8_read(T + kk * 16 * kMixNopeRow + v_addr[dt]);
                va[dt] = widen8<DT>(v8[0], v8[1]);
            }
#pragma unroll
            for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
                for (int dt = 0; dt < kMlaDTiles; ++dt) o[rb][dt] = DT::mfma(va[dt], pf[rb][kk], o[rb][dt]);
        }
        vis0 = vis1, vis1 = vis2;
        slot = slot == kMixRing - 1 ? 0 : slot + 1;
        slot_in = slot_in == kMixRing - 1 ? 0 : slot_in + 1;
    }

    // ---- epilogue, fa_mla_sparse_decode's: lane (h, r) holds o[dt][4 grp + j] = O^T[d = 128 wave + 32 dt + 8 grp +
    // 4 h + j] of head r of the block; a split without a live tile writes the empty partial (0, kNeg) ----
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
        const float L = pair_sum(l_run[rb]);
        const float M = (m_use[rb] <= 0.5f * kNeg) ? kNeg : msc[rb];
        const float inv = L > 0.f ? 1.f / L : 0.f;
        if (!row_ok[rb]) continue;
        if (a.n_split == 1) {
            const int64_t o_off = (int64_t)b * a.o_bs + (int64_t)hq_of[rb] * a.o_hs + (int64_t)pos * a.o_ss;
            char *orow = a.o + 2 * o_off + 2 * (128 * wave + 4 * h);
#pragma unroll
            for (int dt = 0; dt < kMlaDTiles; ++dt)
#pragma unroll
                for (int grp = 0; grp < 4; ++grp) {
                    const u32x2 w2 = {DT::pack(o[rb][dt][4 * grp] * inv, o[rb][dt][4 * grp + 1] * inv),
                                      DT::pack(o[rb][dt][4 * grp + 2] * inv, o[rb][dt][4 * grp + 3] * inv)};
                    *(u32x2 *)(orow + 2 * (32 * dt + 8 * grp)) = w2;
                }
            if (a.lse && wave == 0 && h == 0) {
                const float v = (M + __builtin_amdgcn_logf(L)) * 0.69314718055994531f;
                *((uint32_t *)a.lse + (int64_t)b * a.lse_bs + (int64_t)hq_of[rb] * a.lse_hs + (int64_t)pos * a.lse_ss) =
                    L > 0.f ? __float_as_uint(v) : 0xff800000u;
            }
        } else {
            const size_t srow = (size_t)u * a.rows + (size_t)(hq_of[rb] * a.Sq + pos);
            float *dst = a.ws_o + srow * kMlaDv + 128 * wave + 4 * h;
#pragma unroll
            for (int dt = 0; dt < kMlaDTiles; ++dt)
#pragma unroll
                for (int grp = 0; grp < 4; ++grp)
                    *(float4 *)(dst + 32 * dt + 8 * grp) =
                        make_float4(o[rb][dt][4 * grp] * inv, o[rb][dt][4 * grp + 1] * inv,
                                    o[rb][dt][4 * grp + 2] * inv, o[rb][dt][4 * grp + 3] * inv);
            if (wave == 0 && h == 0) a.ws_lse[srow] = L > 0.f ? M + __builtin_amdgcn_logf(L) : kNeg;  // log2
        }
    }
}

}  // namespace fa
