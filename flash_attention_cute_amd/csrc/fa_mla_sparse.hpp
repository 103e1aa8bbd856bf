#pragma once
// fa_mla_sparse.hpp -- sparse MLA decode: absorbed-query MLA over top-k token indices of the paged latent KV
// cache, gfx950 (include/fa_gfx950_mla_sparse.h). No reference counterpart; the attention core of DeepSeek
// Sparse Attention (DeepSeek-V3.2).
//
// The compute half is fa_mla_decode's (fa_mla_decode.hpp, included and not edited): the LDS image mla_off read
// twice, as K and as V^T, the four-wave column split, the partial-S^T exchange, decode_softmax, the epilogue and
// the workspace layout (row = hq * Sq + pos, unit = b * n_split + split), so fa_mla_combine merges the splits
// as it is. What a tile IS differs: its 32 rows are 32 entries of one query position's index list, each a
// logical position of the sequence with a page and a row of its own, or no key at all.
//
//   * work: a workgroup takes (batch b, position pos, split of the list's topk / 32 tiles, group of up to 64
//     q-HEADS, as one or two 32-row blocks). A list belongs to one position, so only heads share a tile, and
//     the visibility limit lim is one number per workgroup. The head groups of one (b, pos, split) get
//     workgroup ids congruent mod 8 (one XCD's L2). Split s takes tiles s, s + n_split, ...: the live tiles of
//     a padded list (its front) are dealt evenly over the splits, where contiguous shares would leave them to
//     the first splits (fa_mla_combine does not care which tiles a split took);
//   * the list: every wave reads the tile's 32 entries with scalar loads (the list is contiguous; the mask
//     needs all of them) and forms the wave-uniform 32-bit visibility mask vis (bit i: 0 <= idx_i <= lim, one
//     unsigned compare). vis == 0: the tile is SKIPPED -- no loads, no MFMA, no barrier; all four waves decide
//     on the same scalars, so the barriers stay matched. The ring and the counted vmcnt waits run over ISSUED
//     tiles: the loop carries the masks of the tile being computed and of the one behind it, `fetch` scans
//     forward to the next live tile;
//   * the gather: wave w's 9 LDS-DMA pieces of a tile (9 KiB) are exactly tile rows 8 w .. 8 w + 7 (8 x 1152
//     bytes). The wave loads its own 8 entries once more as scalars, translates them through the block table
//     with scalar loads (all eight in flight together) and forms 8 64-bit row addresses in SGPRs. A piece
//     covers parts of at most two neighbouring rows: each lane picks its row's address, adds its in-row byte
//     offset (the swizzle on the source side, the LDS destination lane-linear, as in fa_mla_decode) and the
//     piece goes out as global_load_lds_dwordx4 with per-lane 64-bit addresses -- no buffer descriptor, so no
//     32-bit offset from the pool base: a pool may span any number of bytes;
//   * an entry that is not visible is pointed at mla_sparse_zero_row, 1152 zero bytes of this translation
//     unit: its LDS row is 0 (P = 0 times a NaN of the pool would be NaN), no pool row is read for it, and its
//     block-table slot reads entry 0 (branch-free, so the eight lookups overlap), which the sequence has,
//     since the tile has a visible entry;
//   * the mask: key i of the score fragment goes to kNeg iff bit i of vis is clear (sparse_mask, beside
//     decode_mask).
#include "fa_gfx950_mla_sparse.h"
#include "fa_mla_decode.hpp"

namespace fa {

// The plan (fa_mla_sparse_gfx950.hip): fa_mla_decode's constants over B * Sq * ceil(Hq / 64) workgroups and
// the list's topk / 32 tiles, which are the same for every list -- but a split may be as short as 2 tiles: a list
// has few tiles (64 at topk 2048), and at B = 1 the 32 splits of 2 tiles measured 0.57-0.58 of the time of 8
// splits of 8 (at B = 32 the workgroup target decides, not this bound)
constexpr int kMlaSparseMinTilesPerSplit = 2;

struct MlaSparseArgs {
    MlaArgs m;               // as fa_mla_decode's; n_rg counts the head groups, rows = Hq * Sq
    const int32_t *indices;  // [B, Sq, topk]
    int64_t idx_bs, idx_ss;
    int Hq, n_tiles, page_size, page_shift;  // page_shift: log2 page_size, or -1 (not a power of two)
};

__device__ __attribute__((aligned(16))) uint32_t mla_sparse_zero_row[kMlaRowBytes / 4];

// LDS-DMA of one 1 KiB piece from per-lane 64-bit addresses, non-temporal (dma_one_nt's waits before it)
__device__ __forceinline__ void gather_one_nt(const uint64_t addr, const uint32_t lds, const bool nop) {
    if (nop) asm volatile("s_nop 4\n\tglobal_load_lds_dwordx4 %0, off nt" ::"v"(addr), "{m0}"(lds) : "memory");
    else asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, off nt" ::"v"(addr), "{m0}"(lds) : "memory");
}

// lane (h, r) holds keys (i & 3) + 8 (i >> 2) + 4 h of the tile: key k is visible iff bit k of vis is set
__device__ __forceinline__ void sparse_mask(f32x16 &s, const uint32_t vis, const int h) {
    if (vis != 0xffffffffu) {
        const uint32_t v = vis >> (4 * h);
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (!((v >> ((i & 3) + 8 * (i >> 2))) & 1u)) s[i] = kNeg;
    }
}

template <class DT, int kNRB>
__global__ __launch_bounds__(256, 1) void fa_mla_sparse_decode(const MlaSparseArgs sa) {
    __shared__ __attribute__((aligned(1024))) char ring[kMlaRing * kMlaTile];
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

    // this lane's head of each block, and Q as in fa_mla_decode
    bool row_ok[kNRB];
    int hq_of[kNRB];
    u32x4 qf[kNRB][kMlaKSteps];
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb) {
        const int hq = hg * kMlaGroupRows + rb * kDecRows + r;
        row_ok[rb] = hq < sa.Hq;
        hq_of[rb] = row_ok[rb] ? hq : 0;
        const char *qrow = a.q + 2 * ((int64_t)b * a.q_bs + (int64_t)hq_of[rb] * a.q_hs + (int64_t)pos * a.q_ss) +
                           2 * (144 * wave + 8 * h);
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks)
            qf[rb][ks] = row_ok[rb] ? *(const u32x4 *)(qrow + 32 * ks) : (u32x4){0u, 0u, 0u, 0u};
    }
    // Q landed, and the compiler knows it: from here on only LDS-DMA counts in vmcnt (see fa_mla_decode)
#pragma unroll
    for (int rb = 0; rb < kNRB; ++rb)
#pragma unroll
        for (int ks = 0; ks < kMlaKSteps; ++ks) asm volatile("" : "+v"(qf[rb][ks]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- the gather: piece n of this wave is bytes [1024 n, 1024 n + 1024) of tile rows 8 wave .. 8 wave + 7;
    // lane l's 16 bytes lie in row rl at image slot sl, and come from source chunk sl ^ g(row) of that row ----
    int inrow[kMlaPieces];
#pragma unroll
    for (int n = 0; n < kMlaPieces; ++n) {
        const int byte = n * 1024 + 16 * lane;
        const int row = 8 * wave + byte / kMlaRowBytes, slot = (byte % kMlaRowBytes) / 16;
        inrow[n] = mla_off(row, slot) - row * kMlaRowBytes;
    }
    const sload_t list = (sload_t)(sa.indices + (int64_t)b * sa.idx_bs + (int64_t)pos * sa.idx_ss);
    const sload_t table = (sload_t)(a.block_table + (int64_t)b * a.bt_stride);
    const int last_page = a.num_pages - 1;
    const uint64_t zero_row = (uint64_t)(uintptr_t)mla_sparse_zero_row;
    const uint32_t ring_u = lds_u32(ring) + wave * kMlaPieces * 1024;
    auto issue = [&](const int t, const int slot) {
        uint64_t ra[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = list[kDecKeys * t + 8 * wave + j];
            const bool ok = (uint32_t)idx <= ulim;
            const int pi = !ok ? 0 : sa.page_shift >= 0 ? idx >> sa.page_shift : idx / sa.page_size;
            const int64_t page = min(max(table[pi], 0), last_page);
            const int64_t off = page * a.kv_ps + (int64_t)(idx - pi * sa.page_size) * a.kv_rs;
            ra[j] = ok ? (uint64_t)(uintptr_t)(a.kv + 2 * off) : zero_row;
        }
        const uint32_t dst = ring_u + slot * kMlaTile;
#pragma unroll
        for (int n = 0; n < kMlaPieces; ++n) {
            constexpr int kRow = kMlaRowBytes;
            const int lo = n * 1024 / kRow, hi = (n * 1024 + 1023) / kRow;  // the piece's one or two rows
            const bool up = 16 * lane >= hi * kRow - n * 1024;
            gather_one_nt((up ? ra[hi] : ra[lo]) + (uint64_t)(int64_t)inrow[n], dst + n * 1024, n == 0);
        }
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

    // fragment addresses within a tile, as in fa_mla_decode
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

    // the ring's first two live tiles; vis0: the tile computed on, vis1: the one behind it (0: none)
    uint32_t vis0 = fetch(0);
    uint32_t vis1 = vis0 ? fetch(1) : 0u;
    int slot = 0, slot_in = 2;
    while (vis0) {
        // this wave's pieces of the tile landed (the next live tile's, the youngest 9, may still be in flight);
        // after the barrier every wave's have, and every wave is done with the tile before: its slot is free
        if (vis1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kMlaPieces) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const uint32_t vis2 = vis1 ? fetch(slot_in) : 0u;
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
            sparse_mask(s, vis0, h);
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
        vis0 = vis1, vis1 = vis2;
        slot = slot == kMlaRing - 1 ? 0 : slot + 1;
        slot_in = slot_in == kMlaRing - 1 ? 0 : slot_in + 1;
    }

    // ---- epilogue, fa_mla_decode's: lane (h, r) holds o[dt][4 grp + j] = O^T[d = 128 wave + 32 dt + 8 grp + 4 h + j]
    // of head r of the block; a split without a live tile writes the empty partial (0, kNeg) ----
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
