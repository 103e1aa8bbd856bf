#pragma once
// fa_decode.hpp -- split-KV ("flash-decoding") forward for few query rows per kv-head, gfx950.
//
// The reference has no split-KV kernel (TODO at reference README.md:20). Its decode path is the
// q-head pack of reference csrc/flash_attention_api.cpp:72-83: with Sq == 1 the group of q-heads
// that share one kv-head becomes the rows of one problem, and the prefill kernel then runs one
// 128-row CTA per (batch, kv-head) over the whole K/V stream -- B * Hkv CTAs, most rows empty.
// Decode is HBM-bound (every K/V byte is read once per step), so this kernel is built around the
// K/V stream instead of the MFMA:
//
//   * a row block is up to 32 (q-head, position) rows of one (batch, kv-head): rows_total =
//     head_q_per_group * Sq, row r -> q-head hkv * g + r / Sq, position r % Sq. The host's Sq == 1
//     pack (g' = 1, Sq' = g) and unpacked GQA with a few query positions (speculative decode,
//     causal per position) map onto the same rows; K/V are read once per group either way;
//   * one workgroup = 4 wave64s on one (batch, kv-head, row block, key split); each wave owns a
//     contiguous quarter of the split's 32-key tiles and streams them through its OWN 2-slot
//     LDS ring by LDS-DMA (buffer_load ... lds, 1 KiB per wave-instruction, XOR swizzle applied
//     on the source offsets as in fa_fwd_w4). No barrier in the key loop: a wave only waits for
//     its own DMA (vmcnt);
//   * per tile S^T = K.Q^T and O^T += V^T.P^T with v_mfma_f32_32x32x16 (fragment layouts of
//     fa_fwd_w8: each lane owns one row, the rounded P^T is directly the B operand); MFMA time is
//     ~1/4 of the tile's HBM time at 1 wave per SIMD, so padding rows to 32 costs nothing;
//   * the 4 wave partials are merged in LDS (log-sum-exp weights); with n_split == 1 the
//     workgroup writes O, otherwise fp32 partials (O / l and lse) go to a caller-provided
//     workspace and fa_decode_combine merges the splits.
//
// Numerics: S in fp32, P = exp2(S*s' - m*s') rounded (RNE) to T before P.V, row sums of the fp32
// P, deferred max (guide T13, as fa_fwd_w4). The split changes only which running max a P is
// rounded against, which is within the stated fp16 / bf16 tolerance (tests/test_gpu_parity.py).
// Rows that see no key are 0 (DESIGN.md quirk iii).
#include "fa_fwd_kernels.hpp"

namespace fa {

// LDS-DMA with the non-temporal policy (K/V of a decode step are read once)
__device__ __forceinline__ void dma_one_nt(const rsrc_t &rs, const uint32_t lds, const int voff, const bool nop) {
    if (nop)
        asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, 0 offen nt lds" ::"v"(voff), "s"(rs), "{m0}"(lds)
                     : "memory");
    else
        asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen nt lds" ::"v"(voff), "s"(rs), "{m0}"(lds)
                     : "memory");
}

template <int kD>
struct DecGeo {
    using G = Geo<kD>;
    static constexpr int RB = G::kRowBytes;
    static constexpr int kTile = kDecKeys * RB;     // bytes of one K (or V) tile: 8 / 4 KiB
    static constexpr int kPieces = kTile / 1024;    // LDS-DMA pieces per K (or V) tile
    static constexpr int kSlot = 2 * kTile;         // K + V
    static constexpr int kWaveLds = 2 * kSlot;      // 2-slot ring per wave
    static constexpr int kLds = kDecWaves * kWaveLds;
    static constexpr int kQPiecesPerWave = kDecRows * RB / 1024 / kDecWaves;  // 2 / 1
};

// Fused merge of a unit's n_split partials by the last of its workgroups (fa_decode, a.cnt): the same
// arithmetic as fa_decode_combine (weights 2^(lse - M) in split order, acc / L), spread over the
// workgroup: lse of every (split, row) into LDS, each row's weights by one thread, then a float4 of
// one valid row per thread per pass. Loads are device-scope (sc1: not from this CU's L1).
template <class DT, int kD, bool kExactD>
__device__ __forceinline__ void decode_merge(const fa_fwd_params &p, const DecArgs &a, const int unit, const int b,
                                          const int hkv, const int rb) {
    __shared__ float wt[kDecMaxSplit][kDecRows];
    __shared__ float linv[kDecRows];
    const int tid = threadIdx.x, ns = a.n_split;
    const size_t base = (size_t)unit * ns * kDecRows;  // slot of (split 0, row 0)
    const int nrow = min(a.rows - rb * kDecRows, kDecRows);  // valid rows of this unit
    const rsrc_t lr = make_rsrc((const char *)(a.ws_lse + base), (uint32_t)(ns * kDecRows * 4));
    const rsrc_t orr = make_rsrc((const char *)(a.ws_o + base * kD), (uint32_t)(ns * kDecRows * kD * 4));
    constexpr int kSc1 = 16;  // (CPol SC1: device scope, misses this CU's L1)
    for (int i = tid; i < ns * kDecRows; i += 256)
        wt[i / kDecRows][i % kDecRows] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(lr, 4 * i, 0, kSc1));
    __syncthreads();
    if (tid < nrow) {
        float M = kNeg, L = 0.f;
        for (int s = 0; s < ns; ++s) M = fmaxf(M, wt[s][tid]);
        for (int s = 0; s < ns; ++s) {
            const float ls = wt[s][tid];
            const float w = (ls <= 0.5f * kNeg) ? 0.f : __builtin_amdgcn_exp2f(ls - M);
            L += w;
            wt[s][tid] = w;
        }
        linv[tid] = L > 0.f ? 1.f / L : 0.f;
    }
    __syncthreads();
    constexpr int C4 = kD / 4;  // float4 chunks of a row
    const int Sq = (int)p.seqlen_q, D = (int)p.headdim;
    for (int it = tid; it < nrow * C4; it += 256) {
        const int row = it / C4, c = it % C4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
        for (int s = 0; s < ns; ++s) {
            const float w = wt[s][row];
            const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(orr, (((s * kDecRows) + row) * kD + 4 * c) * 4, 0, kSc1);
            acc.x += w * __uint_as_float(x[0]);
            acc.y += w * __uint_as_float(x[1]);
            acc.z += w * __uint_as_float(x[2]);
            acc.w += w * __uint_as_float(x[3]);
        }
        const float inv = linv[row];
        const int rg = rb * kDecRows + row;
        const int hq = hkv * a.g + rg / Sq, pos = rg % Sq;
        char *orow = (char *)p.o_ptr +
                     2 * ((int64_t)b * p.o_batch_stride + (int64_t)hq * p.o_head_stride + (int64_t)pos * p.o_seqlen_stride);
        const int d = 4 * c;
        if (kExactD || d < D) {
            const u32x2 w2 = {DT::pack(acc.x * inv, acc.y * inv), DT::pack(acc.z * inv, acc.w * inv)};
            *(u32x2 *)(orow + 2 * d) = w2;
        }
    }
}

// kFuse: the fused-merge body (a.cnt set; split launches only) -- a separate instantiation, so the
// unsplit launches keep the kernel without the merge code
template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode(const fa_fwd_params p, const DecArgs a) {
#define FA_DEC_PAGED 0
#include "fa_decode_body.inc"
#undef FA_DEC_PAGED
}

// Merge n_split partials (O / l and lse = m*s' + log2 l, log2 units): one wave per valid (q-head,
// position) row of a (batch, kv-head) -- a workgroup covers 4 of its a.rows rows, so the grid holds
// only valid rows (B * Hkv * ceil(rows / 4) workgroups) -- lane l owns d = 2l, 2l+1 (kD = 128) or
// d = l (kD = 64), so every partial row is one contiguous 512 / 256-B wave read.
template <class DT, int kD, bool kExactD>
__global__ __launch_bounds__(256) void fa_decode_combine(const fa_fwd_params p, const DecArgs a) {
    constexpr int DPL = kD / 64;  // d values per lane
    const int lane = threadIdx.x & 63;
    const int nb4 = (a.rows + 3) / 4;  // workgroups per (batch, kv-head)
    const int bh = blockIdx.x / nb4;
    const int rg = (blockIdx.x % nb4) * 4 + (threadIdx.x >> 6);  // row of the (batch, kv-head)
    if (bh >= (int)(p.batch_size * p.num_heads_kv) || rg >= a.rows) return;
    const int rb = rg / kDecRows, row = rg % kDecRows;
    const int unit = bh * a.n_rb + rb;
    const int hkv = bh % (int)p.num_heads_kv;
    const int b = bh / (int)p.num_heads_kv;
    const int Sq = (int)p.seqlen_q, D = (int)p.headdim;
    const size_t base = (size_t)unit * a.n_split * kDecRows + row;
    float M = kNeg;
    for (int s = 0; s < a.n_split; ++s) M = fmaxf(M, a.ws_lse[base + (size_t)s * kDecRows]);
    float acc[DPL], L = 0.f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
    for (int s = 0; s < a.n_split; ++s) {
        const size_t slot = base + (size_t)s * kDecRows;
        const float ls = a.ws_lse[slot];
        const float w = (ls <= 0.5f * kNeg) ? 0.f : __builtin_amdgcn_exp2f(ls - M);
        L += w;
        const float *src = a.ws_o + slot * kD + lane * DPL;
        if constexpr (DPL == 2) {
            const float2 x = *(const float2 *)src;
            acc[0] += w * x.x;
            acc[1] += w * x.y;
        } else {
            acc[0] += w * src[0];
        }
    }
    const float inv = L > 0.f ? 1.f / L : 0.f;
    const int hq = hkv * a.g + rg / Sq, pos = rg % Sq;
    char *orow = (char *)p.o_ptr +
                 2 * ((int64_t)b * p.o_batch_stride + (int64_t)hq * p.o_head_stride + (int64_t)pos * p.o_seqlen_stride);
    const int d = lane * DPL;
    if (kExactD || d < D) {
        if constexpr (DPL == 2) {
            *(uint32_t *)(orow + 2 * d) = DT::pack(acc[0] * inv, acc[1] * inv);
        } else {
            const uint32_t w2 = DT::pack(acc[0] * inv, 0.f);
            *(uint16_t *)(orow + 2 * d) = (uint16_t)(w2 & 0xffff);
        }
    }
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode(const fa_fwd_params &p, DecArgs a, void *ws, hipStream_t stream) {
    const int64_t units = decode_units(p, a);
    if (a.n_split > 1) {
        const int64_t slots = units * a.n_split * kDecRows;
        a.ws_o = (float *)ws;
        a.ws_lse = (float *)((char *)ws + slots * kD * 4);
    }
    // fused merge: the stream's zeroed per-unit counters (none under graph capture), and only where a
    // unit's splits share an XCD (same_xcd_placement)
    if (a.n_split > 1 && knobs().dec_fuse && same_xcd_placement()) {
        unsigned *err = nullptr;
        a.cnt = split_sync_area(stream, units * 4, &err);
    }
    set_last_dec_fused(a.cnt != nullptr);
    // (fused: every XCD holds ceil(units / 8) units' splits)
    const int64_t grid = a.cnt ? 8 * ((units + 7) / 8) * a.n_split : units * a.n_split;
    if (a.cnt)
        hipLaunchKernelGGL((fa_decode<DT, C, kD, kExact, true>), dim3((uint32_t)grid), dim3(256), 0, stream, p, a);
    else
        hipLaunchKernelGGL((fa_decode<DT, C, kD, kExact>), dim3((uint32_t)grid), dim3(256), 0, stream, p, a);
    if (a.n_split > 1 && !a.cnt)
        hipLaunchKernelGGL((fa_decode_combine<DT, kD, kExact>),
                           dim3((uint32_t)(p.batch_size * p.num_heads_kv * ((a.rows + 3) / 4))), dim3(256), 0, stream,
                           p, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    set_last_path(a.n_split > 1 ? kPathDecodeSplit : kPathDecode);
    return FA_OK;
}

}  // namespace fa
