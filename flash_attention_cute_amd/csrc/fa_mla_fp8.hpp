#pragma once
// fa_mla_fp8.hpp -- fa_mla_decode (fa_mla_decode.hpp) over an FP8 (OCP e4m3) latent pool, gfx950
// (include/fa_gfx950_mla_fp8.h). q and o stay fp16 / bf16; a latent row is 576 BYTES, read in place, widened to
// the q dtype IN REGISTERS (every e4m3 value is exact in fp16 and bf16: v_cvt_scalef32_pk_{f16,bf16}_fp8, scale
// 1.0) and multiplied by DT::mfma (32x32x16) exactly as fa_mla_decode does. The descale (one per batch row, a
// scalar load) folds into the softmax scale and into the final 1 / l, which also scales the split partials: the
// key loop pays nothing for it. The work split (batch, key split, group of 64 rows; XCD placement), the column
// split over the four waves, the partial-S^T exchange, decode_mask / decode_softmax, the epilogue, the workspace
// and fa_mla_combine are fa_mla_decode's. What the byte rows change:
//
//   * the ring. A 32-key tile is 18 KiB = 18 LDS-DMA pieces of 1 KiB, which four waves do not divide, so a
//     ring STEP is a PAIR of tiles (36 pieces): waves 0 / 1 issue the two halves (9 pieces each) of the even
//     tile, waves 2 / 3 those of the odd tile -- every wave 9 pieces of ONE tile, so one buffer descriptor and
//     one scalar page id per wave and step, and a pair may straddle a page. The ring is two steps (four tiles,
//     72 KiB, half of fa_mla_decode's 108 KiB): one pair is in flight while one is computed on, the same two
//     tile-times of cover fa_mla_decode gives its loads. The LDS that frees pays for a second partial-S^T
//     exchange buffer (one per tile of a pair), which removes the "tile landed" barrier of every second tile:
//     three barriers per pair instead of four. The wait is vmcnt(0) (only the step being waited on is
//     outstanding), so a wave whose tile does not exist (an odd tile count) simply issues nothing;
//   * the LDS image (mla8_off): row r at r * 576, 16-byte chunk c at slot c ^ x(r), x(r) = (r >> 2) & 3 -- the XOR
//     stays inside an aligned group of 4 chunks (a row is 36 = 9 * 4). 576 = 2.25 bank rows of 256 bytes, so row
//     r starts at 16-byte bank slot 4 (r & 3): chunk c of row r sits at slot 4 ((r + (c >> 2)) & 3) + ((c & 3) ^
//     x(r)). (a) The key read is ds_read_b128, lane r on key row r, one chunk c per half-wave; its 16-lane groups
//     are rows {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}: in each, r & 3 takes every value once per run of
//     four rows and the runs' (r >> 2) & 3 are {0, 3, 1, 2} / {1, 2, 0, 3} -- 16 distinct slots, conflict-free.
//     (b) The V^T read is ds_read_b64_tr_b8 (semantics: fa_decode_paged_fp8.hpp); a 32-lane half reads rows R +
//     {0..3, 8..11} (R a multiple of 4), an aligned 32-byte chunk pair each. The XOR keeps or swaps the two
//     chunks of a pair (bit 0) or moves the pair within its aligned 64 bytes (bit 1): rows R .. R + 3 take the
//     four 64-byte quarters of the bank row (r & 3), rows R + 8 .. have x ^ 2, the other 32-byte half of each
//     quarter -- the eight 32-byte slots once each, conflict-free. ONE image serves both reads; rows 16 further
//     down have the same x, so a transposed read's second key step is a constant offset;
//   * the score columns. The 36 chunks are 18 b128 pairs of k-steps (lane (h, r) reads chunk 2 P + h of key r:
//     its low 8 bytes are k-step 2 j, its high 8 bytes k-step 2 j + 1). Wave w takes pairs 4 w .. 4 w + 3 (latent
//     columns [128 w, 128 w + 128)) and ONE k-step of the RoPE columns' two pairs: half (w & 1) of pair 16 + (w >>
//     1). Nine k-steps and nine Q fragments per wave as in fa_mla_decode, five ds_read_b128 instead of nine (the
//     fifth used by half). The contraction index of an MFMA may be permuted as long as both operands agree, so
//     the Q fragments are loaded in that order: qf[2 j + e] = Q[row][32 P + 16 h + 8 e .. + 7];
//   * the value columns. Wave w owns output columns [128 w, 128 w + 128): 4 d-tiles x 2 key steps, ONE
//     ds_read_b64_tr_b8 per (key step, d-tile) -- half fa_mla_decode's transposed reads -- in the key order of
//     the rounded P^T fragment, so the accumulators have fa_mla_decode's layout and its epilogue.
//
// Rows of a tile past the sequence end are cut off by the buffer descriptor's bound (they read 0, never the
// page, so a NaN-byte pool cannot leak), table entries past a sequence's last page are never read, page ids are
// clamped.
#include "fa_decode_paged_fp8.hpp"
#include "fa_gfx950_mla_fp8.h"
#include "fa_mla_decode.hpp"

namespace fa {

constexpr int kMla8RowBytes = kMlaDqk;                   // 576
constexpr int kMla8Tile = kDecKeys * kMla8RowBytes;      // 18 KiB
constexpr int kMla8Step = 2 * kMla8Tile;                 // a ring step: a pair of tiles, 36 KiB
constexpr int kMla8Ring = 2;                             // steps
constexpr int kMla8Pieces = kMla8Step / 1024 / 4;        // LDS-DMA pieces per wave per step: 9 (half a tile)
constexpr int kMla8Pairs = 4;                            // whole b128 pairs of k-steps per wave (+ one k-step)
static_assert(kMla8Pieces * 2 * 1024 == kMla8Tile, "two waves issue one tile");

// byte offset of 16-byte chunk ch of row `row` in a tile's LDS image
__device__ __forceinline__ int mla8_off(const int row, const int ch) {
    return row * kMla8RowBytes + 16 * (ch ^ ((row >> 2) & 3));
}

template <class DT, int kNRB>
__global__ __launch_bounds__(256, 1) void fa_mla_decode_fp8kv(const MlaArgs a, const float *kv_descale,
                                                              const int64_t descale_stride) {
    __shared__ __attribute__((aligned(1024))) char ring[kMla8Ring * kMla8Step];
    __shared__ __attribute__((aligned(1024))) char xch[2 * kNRB * kDecWaves * 4096];  // one per tile of a pair

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    // (b, split) unit u and row group rg: the row groups of a unit are 8 workgroup ids apart
    const int kq = (int)(blockIdx.x >> 3);
    const int rg = kq % a.n_rg;
    const int u = ((kq / a.n_rg) << 3) | (int)(blockIdx.x & 7);
    if (u >= a.batch * a.n_split) return;
    const int b = u / a.n_split, split = u % a.n_split;

    typedef const __attribute__((address_space(4))) int32_t *sload_t;  // (constant space: scalar loads)
    typedef const __attribute__((address_space(4))) float *scale_t;
    const int Sk = min(max(((sload_t)a.seqlens_k)[b], 0), a.cap_keys);
    const float ds = kv_descale ? ((scale_t)kv_descale)[(int64_t)b * descale_stride] : 1.f;
    const int Sq = a.Sq, diag = Sk - Sq;
    const int n_tiles = (Sk + kDecKeys - 1) / kDecKeys;
    const int tps = (n_tiles + a.n_split - 1) / a.n_split;
    const int t_lo = min(split * tps, n_tiles), t_hi = min(t_lo + tps, n_tiles);
    const int n_steps = (t_hi - t_lo + 1) >> 1;
    const float sc = a.sc * ds, thr_raw = kRescaleThr / sc;

    // the b128 pairs of this wave: four whole ones, and the one it takes a half of
    const int pair0 = kMla8Pairs * wave, pair_x = 4 * kMla8Pairs + (wave >> 1), half_x = wave & 1;

    // this lane's row of each block, and Q: the B operand of S^T = K.Q^T in K's byte order, straight from global
    // memory (rows past the end are 0)
    int lim[kNRB];
    bool row_ok[kNRB];
    int64_t o_off[kNRB], lse_off[kNRB];
    u32x4 qf[kNRB][kMlaKSteps];
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
        const int row = rg * kMlaGroupRows + rb * kDecRows + r;
        row_ok[rb] = row < a.rows;
        const int hq = row_ok[rb] ? row / Sq : 0, pos = row_ok[rb] ? row % Sq : 0;
        lim[rb] = (a.causal && row_ok[rb]) ? min(Sk - 1, pos + diag) : Sk - 1;
        o_off[rb] = (int64_t)b * a.o_bs + (int64_t)hq * a.o_hs + (int64_t)pos * a.o_ss;
        lse_off[rb] = (int64_t)b * a.lse_bs + (int64_t)hq * a.lse_hs + (int64_t)pos * a.lse_ss;
        const char *qrow = a.q + 2 * ((int64_t)b * a.q_bs + (int64_t)hq * a.q_hs + (int64_t)pos * a.q_ss) + 32 * h;
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks) {
            const int col2 = ks < 2 * kMla8Pairs ? 64 * (pair0 + (ks >> 1)) + 16 * (ks & 1) : 64 * pair_x + 16 * half_x;
            qf[rb][ks] = row_ok[rb] ? *(const u32x4 *)(qrow + col2) : (u32x4){0u, 0u, 0u, 0u};
        }
    }
    // Q landed, and the compiler knows it (fa_mla_decode): from here on only LDS-DMA counts in vmcnt
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks) asm volatile("" : "+v"(qf[rb][ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- LDS-DMA: lane-linear destination, the swizzle on the source offsets (an XOR: its own inverse). This
    // wave fills half (wave & 1) of tile (wave >> 1) of a step ----
    const int rs = a.kv_rs;  // row stride, bytes
    const int tile_w = wave >> 1;
    int voff[kMla8Pieces];
#pragma unroll
    for (int n = 0; n < kMla8Pieces; ++n) {
        const int byte = ((wave & 1) * kMla8Pieces + n) * 1024 + 16 * lane;
        const int row = byte / kMla8RowBytes, slot = (byte % kMla8RowBytes) / 16;
        voff[n] = row * rs + (mla8_off(row, slot) - row * kMla8RowBytes);
    }
    const uint32_t ring_u = lds_u32(ring) + tile_w * kMla8Tile + (wave & 1) * kMla8Pieces * 1024;
    const sload_t table = (sload_t)(a.block_table + (int64_t)b * a.bt_stride);
    const int tpp = a.tiles_per_page, last_page = a.num_pages - 1;
    auto issue = [&](const int step, const int slot) {
        const int t = t_lo + 2 * step + tile_w;
        if (t >= t_hi) return;  // (wave-uniform) the odd tile of the last pair does not exist
        const int pi = __builtin_amdgcn_readfirstlane(t / tpp);
        const int64_t page = min(max(table[pi], 0), last_page);
        const char *src = a.kv + page * a.kv_ps + (int64_t)((t - pi * tpp) * kDecKeys) * rs;
        const int rows = min(Sk - t * kDecKeys, kDecKeys);
        const rsrc_t kr = make_rsrc_u(src, (uint32_t)((rows - 1) * rs + kMla8RowBytes));
        const uint32_t dst = ring_u + slot * kMla8Step;
#pragma unroll
        for (int n = 0; n < kMla8Pieces; ++n) dma_one_nt(kr, dst + n * 1024, voff[n], n == 0);
    };

    // fragment addresses within a tile: K (ds_read_b128, lane r on key row r) and V^T (ds_read_b64_tr_b8)
    int k_addr[kMla8Pairs + 1], v_addr[kMlaDTiles];
    {
        const int g4 = lane >> 4, q = (lane >> 1) & 7, pp = lane & 1;
        const int row0 = 4 * (g4 >> 1) + (q & 3) + 8 * (q >> 2);
#pragma unroll
        for (int j = 0; j < kMla8Pairs; ++j) k_addr[j] = mla8_off(r, 2 * (pair0 + j) + h);
        k_addr[kMla8Pairs] = mla8_off(r, 2 * pair_x + h);
#pragma unroll
        for (int dt = 0; dt < kMlaDTiles; ++dt) v_addr[dt] = mla8_off(row0, 8 * wave + 2 * dt + (g4 & 1)) + 8 * pp;
    }

    f32x16 o[kNRB][kMlaDTiles];
    float m_use[kNRB], msc[kNRB], l_run[kNRB];
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
#pragma unroll
        for (int dt = 0; dt < kMlaDTiles; ++dt) o[rb][dt] = (f32x16){};
        m_use[rb] = kNeg, msc[rb] = 0.f, l_run[rb] = 0.f;
    }

    if (n_steps > 0) issue(0, 0);
    int slot = 0;
    for (int st = 0; st < n_steps; ++st) {
        // this wave's pieces of step st landed; after the barrier every wave's have, and every wave is done with
        // step st - 1: its slot takes step st + 1
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (st + 1 < n_steps) issue(st + 1, slot ^ 1);

#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int t = t_lo + 2 * st + sub;
            if (t >= t_hi) break;  // (uniform over the workgroup)
            const char *T = ring + slot * kMla8Step + sub * kMla8Tile;
            char *X = xch + sub * (kNRB * kDecWaves * 4096);

            // partial S^T over this wave's nine k-steps, to the exchange buffer (lane-linear 16-byte pieces)
            {
                u32x4 kf[kMla8Pairs + 1];
#pragma unroll
                for (int j = 0; j <= kMla8Pairs; ++j) kf[j] = *(const u32x4 *)(T + k_addr[j]);
                const uint32_t x_lo = half_x ? kf[kMla8Pairs][2] : kf[kMla8Pairs][0];
                const uint32_t x_hi = half_x ? kf[kMla8Pairs][3] : kf[kMla8Pairs][1];
#pragma unroll
                for (int rb = 0; rb < kNRB; ++rb) {
                    f32x16 s = {};
#pragma unroll
                    for (int j = 0; j < kMla8Pairs; ++j) {
                        s = DT::mfma(widen8<DT>(kf[j][0], kf[j][1]), qf[rb][2 * j], s);
                        s = DT::mfma(widen8<DT>(kf[j][2], kf[j][3]), qf[rb][2 * j + 1], s);
                    }
                    s = DT::mfma(widen8<DT>(x_lo, x_hi), qf[rb][2 * kMla8Pairs], s);
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4)
                        *(float4 *)(X + ((rb * kDecWaves + wave) * 4 + q4) * 1024 + 16 * lane) =
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
                    float4 x = *(const float4 *)(X + ((rb * kDecWaves + 0) * 4 + q4) * 1024 + 16 * lane);
#pragma unroll
                    for (int w = 1; w < kDecWaves; ++w) {
                        const float4 y = *(const float4 *)(X + ((rb * kDecWaves + w) * 4 + q4) * 1024 + 16 * lane);
                        x.x += y.x, x.y += y.y, x.z += y.z, x.w += y.w;
                    }
                    s[4 * q4] = x.x, s[4 * q4 + 1] = x.y, s[4 * q4 + 2] = x.z, s[4 * q4 + 3] = x.w;
                }
                decode_mask<false>(s, t * kDecKeys, h, lim[rb], 0, 0);
                decode_softmax<DT, kMlaDTiles>(s, o[rb], m_use[rb], msc[rb], l_run[rb], sc, thr_raw, pf[rb]);
            }

            // O^T += V^T.P^T over this wave's 128 value columns, V^T read transposed from the same image
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                u32x4 va[kMlaDTiles];
#pragma unroll
                for (int dt = 0; dt < kMlaDTiles; ++dt) {
                    const u32x2 v8 = tr8_read(T + kk * 16 * kMla8RowBytes + v_addr[dt]);
                    va[dt] = widen8<DT>(v8[0], v8[1]);
                }
#pragma unroll
                for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
                    for (int dt = 0; dt < kMlaDTiles; ++dt) o[rb][dt] = DT::mfma(va[dt], pf[rb][kk], o[rb][dt]);
            }
        }
        slot ^= 1;
    }

    // ---- epilogue: lane (h, r) holds o[dt][4 grp + j] = O^T[d = 128 wave + 32 dt + 8 grp + 4 h + j][row r]; the
    // descale rides on 1 / l ----
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
        const float L = pair_sum(l_run[rb]);
        const float M = (m_use[rb] <= 0.5f * kNeg) ? kNeg : msc[rb];
        const float inv = L > 0.f ? ds / L : 0.f;
        if (!row_ok[rb]) continue;
        const int row = rg * kMlaGroupRows + rb * kDecRows + r;
        if (a.n_split == 1) {
            char *orow = a.o + 2 * o_off[rb] + 2 * (128 * wave + 4 * h);
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
                *((uint32_t *)a.lse + lse_off[rb]) = L > 0.f ? __float_as_uint(v) : 0xff800000u;
            }
        } else {
            const size_t srow = (size_t)u * a.rows + row;
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
