#pragma once
// fa_mla_decode.hpp -- multi-head latent attention (MLA) decode over a paged latent KV cache, gfx950
// (include/fa_gfx950_mla.h). No reference counterpart.
//
// An MLA decode step attends with absorbed queries of kDqk = 576 columns over ONE latent stream per sequence
// that every q-head shares (MQA), and the value is the first kDv = 512 columns of the same rows that form
// the key. So the kernel is built around one rule: a 32-key tile of the latent (32 x 1152 bytes) goes HBM ->
// LDS once and is read twice from the same LDS image, as K for S^T = K.Q^T and as V^T for O^T += V^T.P^T.
//
//   * work: a workgroup of 4 wave64s takes (batch b, key split, row group): up to kMlaGroupRows = 64 of the
//     b's Hq * Sq (q-head, position) rows, as one or two 32-row blocks (kNRB), and the split's share of the
//     sequence's tiles. The row groups of one (b, split) get workgroup ids congruent mod 8 (one XCD, the
//     hardware deals workgroups to XCDs by id mod 8), so their repeated tile reads meet in that XCD's L2;
//   * the tile ring (kMlaRing = 3 slots of 36 KiB) is SHARED by the four waves: each wave issues 9 of a
//     tile's 36 LDS-DMA pieces (non-temporal), two tiles are in flight while one is computed on, and the key
//     loop has two barriers per tile (tile landed / partial scores exchanged);
//   * the LDS image (mla_off): row r at r * 1152, 16-byte chunk c at slot c ^ g(r), g(r) = r3 r2 | r1 << 2
//     (bits of r). 1152 = 4.5 bank rows of 256 bytes, so row r starts at bank slot 8 (r & 1): the 16 rows of
//     a ds_read_b128 lane group (one chunk each) cover 16 distinct slots -- the low three slot bits are c ^
//     g(r), a bijection of (r1, r2, r3), the fourth is c3 ^ r0 --, and the four rows R .. R+3 of a half-wave's
//     ds_read_b64_tr_b16 (64 aligned bytes each; the XOR keeps an aligned group of four chunks together) fall
//     into the four 64-byte quarters (quarter bits c2 ^ r1 and c3 ^ r0): both reads are conflict-free, one
//     image serves both;
//   * the four waves split the columns: wave w owns latent columns [144 w, 144 w + 144) of the scores (9
//     k-steps of v_mfma_f32_32x32x16, Q fragments in registers for the whole split: 36 VGPRs per row block)
//     and output columns [128 w, 128 w + 128) (4 d-tiles x 2 k-steps, 64 fp32 accumulators per row block).
//     A wave's partial S^T goes to an LDS exchange buffer; after the barrier every wave sums the four
//     partials in the same order, so all four hold bit-identical scores and run the online-softmax step
//     (decode_softmax of fa_decode.hpp: deferred max, exp2, fp32 row sums, P rounded RNE to T) redundantly,
//     with bit-identical rescale decisions and P;
//   * epilogue: one split -> each wave writes its column slice of O / l in T, wave 0 the LSE; more splits ->
//     fp32 O / l and the log2-unit lse to the workspace, merged by fa_mla_combine (fa_decode_combine's
//     arithmetic: weights 2^(lse - M), an empty split weighs 0, one rounding to T; the splits are summed in a
//     fixed order spread over the workgroup, see there).
//
// Rows of a tile past the sequence end are cut off by the buffer descriptor's bound (they read 0, never the
// page: no 0 * NaN in P.V), table entries past a sequence's last page are never read, page ids are clamped.
// The page id is a scalar load (the loop's counted vmcnt waits see LDS-DMA only).
#include "fa_decode.hpp"
#include "fa_gfx950_mla.h"

namespace fa {

constexpr int kMlaDqk = 576, kMlaDv = 512;
constexpr int kMlaGroupRows = 2 * kDecRows;  // rows of a workgroup
constexpr int kMlaRing = 3;
constexpr int kMlaRowBytes = kMlaDqk * 2;              // 1152
constexpr int kMlaTile = kDecKeys * kMlaRowBytes;      // 36 KiB
constexpr int kMlaPieces = kMlaTile / 1024 / 4;        // LDS-DMA pieces per wave per tile: 9
constexpr int kMlaKSteps = kMlaDqk / 16 / 4;           // k-steps of a wave's score columns: 9
constexpr int kMlaDTiles = kMlaDv / 32 / 4;            // d-tiles of a wave's output columns: 4
// The plan (mla_plan, fa_mla_host.h): about one workgroup per CU of an MI355X (the ring admits one per CU, and a
// workgroup's tile rate is bound by its own barrier-separated phases, not by HBM: 256 measured faster than the
// decode kernels' 160 on every shape, and 64 slower), a split at least 8 tiles of the table's capacity, at most
// 256 splits (one long sequence still fills the device; fa_mla_combine has one thread per split)
constexpr int kMlaTargetWgs = 256;
constexpr int kMlaMinTilesPerSplit = 8;
constexpr int kMlaMaxSplit = 256;

// the kernel's arguments: fa_mla_params narrowed to what the device reads, and the plan
struct MlaArgs {
    const char *q, *kv;
    char *o;
    float *lse;
    const int32_t *block_table, *seqlens_k;
    int64_t q_bs, q_hs, q_ss, o_bs, o_hs, o_ss, lse_bs, lse_hs, lse_ss, kv_ps;
    int kv_rs, batch, Sq, rows, n_rg, n_split, num_pages, tiles_per_page, cap_keys, bt_stride, causal;
    float sc;
    float *ws_o;    // [batch * n_split][rows][512] fp32 O / l   (n_split > 1)
    float *ws_lse;  // [batch * n_split][rows] fp32 m s' + log2 l (n_split > 1)
};

// byte offset of 16-byte chunk ch of row `row` in a tile's LDS image
__device__ __forceinline__ int mla_off(const int row, const int ch) {
    return row * kMlaRowBytes + 16 * (ch ^ (((row >> 2) & 3) | (((row >> 1) & 1) << 2)));
}

template <class DT, int kNRB>
__global__ __launch_bounds__(256, 1) void fa_mla_decode(const MlaArgs a) {
    __shared__ __attribute__((aligned(1024))) char ring[kMlaRing * kMlaTile];
    __shared__ __attribute__((aligned(1024))) char xch[kNRB * kDecWaves * 4096];

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
    const int Sk = min(max(((sload_t)a.seqlens_k)[b], 0), a.cap_keys);
    const int Sq = a.Sq, diag = Sk - Sq;
    const int n_tiles = (Sk + kDecKeys - 1) / kDecKeys;
    const int tps = (n_tiles + a.n_split - 1) / a.n_split;
    const int t_lo = min(split * tps, n_tiles), t_hi = min(t_lo + tps, n_tiles);
    const float sc = a.sc, thr_raw = kRescaleThr / sc;

    // this lane's row of each block, and Q: the B operand of S^T = K.Q^T, lane (h, r) holds
    // Q[row r][144 wave + 16 ks + 8 h .. + 7], straight from global memory (rows past the end are 0)
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
        const char *qrow = a.q + 2 * ((int64_t)b * a.q_bs + (int64_t)hq * a.q_hs + (int64_t)pos * a.q_ss) +
                           2 * (144 * wave + 8 * h);
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks)
            qf[rb][ks] = row_ok[rb] ? *(const u32x4 *)(qrow + 32 * ks) : (u32x4){0u, 0u, 0u, 0u};
    }
    // Q landed, and the compiler knows it (the fragments are operands of the empty asm: it places its own wait
    // here, not a vmcnt(0) at their first use inside the key loop): from here on only LDS-DMA counts in vmcnt
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks) asm volatile("" : "+v"(qf[rb][ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- LDS-DMA: lane-linear destination, the swizzle on the source offsets (an XOR: its own inverse) ----
    const int rs2 = a.kv_rs * 2;  // row stride, bytes
    int voff[kMlaPieces];
#pragma unroll
    for (int n = 0; n < kMlaPieces; ++n) {
        const int byte = (wave * kMlaPieces + n) * 1024 + 16 * lane;
        const int row = byte / kMlaRowBytes, slot = (byte % kMlaRowBytes) / 16;
        voff[n] = row * rs2 + (mla_off(row, slot) - row * kMlaRowBytes);
    }
    const uint32_t ring_u = lds_u32(ring) + wave * kMlaPieces * 1024;
    const sload_t table = (sload_t)(a.block_table + (int64_t)b * a.bt_stride);
    const int tpp = a.tiles_per_page, last_page = a.num_pages - 1;
    auto issue = [&](const int t, const int slot) {
        const int pi = __builtin_amdgcn_readfirstlane(t / tpp);
        const int64_t page = min(max(table[pi], 0), last_page);
        const char *src = a.kv + 2 * (page * a.kv_ps + (int64_t)((t - pi * tpp) * kDecKeys) * a.kv_rs);
        const int rows = min(Sk - t * kDecKeys, kDecKeys);
        const rsrc_t kr = make_rsrc_u(src, slab_bytes(rows, a.kv_rs, kMlaDqk));
        const uint32_t dst = ring_u + slot * kMlaTile;
#pragma unroll
        for (int n = 0; n < kMlaPieces; ++n) dma_one_nt(kr, dst + n * 1024, voff[n], n == 0);
    };

    // fragment addresses within a tile: K (ds_read_b128, lane r on key row r) and V^T (ds_read_b64_tr_b16)
    // (the swizzle reads row bits 1 .. 3: the rows 8 further down have an address of their own; 16 further not)
    int k_addr[kMlaKSteps], v_addr[2][kMlaDTiles];
    {
        const int g4 = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks) k_addr[ks] = mla_off(r, 18 * wave + 2 * ks + h);
#pragma unroll
        for (int dt = 0; dt < kMlaDTiles; ++dt)
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
                v_addr[hi][dt] = mla_off(8 * hi + 4 * (g4 >> 1) + qq, 16 * wave + dt * 4 + 2 * (g4 & 1) + (pp >> 1)) +
                                 8 * (pp & 1);
    }

    f32x16 o[kNRB][kMlaDTiles];
    float m_use[kNRB], msc[kNRB], l_run[kNRB];
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
#pragma unroll
        for (int dt = 0; dt < kMlaDTiles; ++dt) o[rb][dt] = (f32x16){};
        m_use[rb] = kNeg, msc[rb] = 0.f, l_run[rb] = 0.f;
    }

    // the ring's first two tiles
    if (t_lo < t_hi) issue(t_lo, 0);
    if (t_lo + 1 < t_hi) issue(t_lo + 1, 1);
    int slot = 0, slot_in = 2;  // slot of tile t; slot tile t + 2 goes to
    for (int t = t_lo; t < t_hi; ++t) {
        // this wave's pieces of tile t landed (tile t + 1's, the youngest 9, may still be in flight); after the
        // barrier every wave's have, and every wave is done with tile t - 1: its slot takes tile t + 2
        if (t + 1 < t_hi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kMlaPieces) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 2 < t_hi) issue(t + 2, slot_in);
        const char *T = ring + slot * kMlaTile;

        // partial S^T over this wave's 144 columns, to the exchange buffer (lane-linear 16-byte pieces)
        {
            u32x4 kf[kMlaKSteps];
#pragma unroll
            for (int ks = 0; ks < kMlaKSteps; ++ks) kf[ks] = *(const u32x4 *)(T + k_addr[ks]);
#pragma unroll
            for (int rb = 0; rb < kNRB; ++rb) {
                f32x16 s = {};
#pragma unroll
                for (int ks = 0; ks < kMlaKSteps; ++ks) s = DT::mfma(kf[ks], qf[rb][ks], s);
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
            decode_mask<false>(s, t * kDecKeys, h, lim[rb], 0, 0);
            decode_softmax<DT, kMlaDTiles>(s, o[rb], m_use[rb], msc[rb], l_run[rb], sc, thr_raw, pf[rb]);
        }

        // O^T += V^T.P^T over this wave's 128 value columns, V^T read transposed from the same image
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            u32x4 va[kMlaDTiles];
#pragma unroll
            for (int dt = 0; dt < kMlaDTiles; ++dt) {
                const u32x2 lo = tr_read(T + kk * 16 * kMlaRowBytes + v_addr[0][dt]);
                const u32x2 hi = tr_read(T + kk * 16 * kMlaRowBytes + v_addr[1][dt]);
                va[dt] = (u32x4){lo[0], lo[1], hi[0], hi[1]};
            }
#pragma unroll
            for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
                for (int dt = 0; dt < kMlaDTiles; ++dt) o[rb][dt] = DT::mfma(va[dt], pf[rb][kk], o[rb][dt]);
        }
        slot = slot == kMlaRing - 1 ? 0 : slot + 1;
        slot_in = slot_in == kMlaRing - 1 ? 0 : slot_in + 1;
    }

    // ---- epilogue: lane (h, r) holds o[dt][4 grp + j] = O^T[d = 128 wave + 32 dt + 8 grp + 4 h + j][row r] ----
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
        const float L = pair_sum(l_run[rb]);
        const float M = (m_use[rb] <= 0.5f * kNeg) ? kNeg : msc[rb];
        const float inv = L > 0.f ? 1.f / L : 0.f;
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

// Merge of the n_split partials of one (batch, row): a workgroup per (batch, row, 128-column chunk) -- few rows and
// many splits is the common case (one long sequence), so the splits are spread over the workgroup too: the lse
// values, their max and the weights 2^(lse - M) (an empty split weighs 0) go through LDS once, then thread
// (group g = tid / 32, c = tid % 32) accumulates columns 4 c .. 4 c + 3 of the chunk over splits g, g + 8, ...
// with independent 16-byte loads, and group 0 adds the eight partial sums in group order: a fixed order, one
// rounding to T. fa_decode_combine's arithmetic otherwise; the chunk-0 workgroup also writes the row's lse.
template <class DT>
__global__ __launch_bounds__(256) void fa_mla_combine(const MlaArgs a) {
    static_assert(kMlaMaxSplit <= 256, "one thread per split loads its lse");
    __shared__ float wt[kMlaMaxSplit];
    __shared__ float4 part[8][32];
    const int chunk = blockIdx.x & 3, br = blockIdx.x >> 2;
    const int b = br / a.rows, row = br % a.rows;
    const int tid = threadIdx.x, ns = a.n_split;
    const size_t base = (size_t)b * ns * a.rows + row;
    if (tid < ns) wt[tid] = a.ws_lse[base + (size_t)tid * a.rows];
    __syncthreads();
    float M = kNeg;
    for (int s = 0; s < ns; ++s) M = fmaxf(M, wt[s]);
    __syncthreads();
    if (tid < ns) wt[tid] = (wt[tid] <= 0.5f * kNeg) ? 0.f : __builtin_amdgcn_exp2f(wt[tid] - M);
    __syncthreads();
    float L = 0.f;
    for (int s = 0; s < ns; ++s) L += wt[s];
    const int grp = tid >> 5, c = tid & 31;
    const float *src = a.ws_o + base * kMlaDv + 128 * chunk + 4 * c;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int s = grp; s < ns; s += 8) {
        const float w = wt[s];
        const float4 x = *(const float4 *)(src + (size_t)s * a.rows * kMlaDv);
        acc.x = __builtin_fmaf(w, x.x, acc.x), acc.y = __builtin_fmaf(w, x.y, acc.y);
        acc.z = __builtin_fmaf(w, x.z, acc.z), acc.w = __builtin_fmaf(w, x.w, acc.w);
    }
    part[grp][c] = acc;
    __syncthreads();
    if (grp != 0) return;
#pragma unroll
    for (int g = 1; g < 8; ++g) {
        const float4 x = part[g][c];
        acc.x += x.x, acc.y += x.y, acc.z += x.z, acc.w += x.w;
    }
    const float inv = L > 0.f ? 1.f / L : 0.f;
    const int hq = row / a.Sq, pos = row % a.Sq;
    char *orow = a.o + 2 * ((int64_t)b * a.o_bs + (int64_t)hq * a.o_hs + (int64_t)pos * a.o_ss);
    const u32x2 w2 = {DT::pack(acc.x * inv, acc.y * inv), DT::pack(acc.z * inv, acc.w * inv)};
    *(u32x2 *)(orow + 2 * (128 * chunk + 4 * c)) = w2;
    if (a.lse && chunk == 0 && c == 0) {
        const float v = (M + __builtin_amdgcn_logf(L)) * 0.69314718055994531f;
        *((uint32_t *)a.lse + (int64_t)b * a.lse_bs + (int64_t)hq * a.lse_hs + (int64_t)pos * a.lse_ss) =
            L > 0.f ? __float_as_uint(v) : 0xff800000u;
    }
}

}  // namespace fa
