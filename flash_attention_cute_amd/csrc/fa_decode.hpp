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
//
// One body for five kernels: fa_decode, fa_decode_paged, fa_decode_fp8kv and the two sliding-window variants
// are one-line calls of decode_body<Kv, kWindow, ...> below. The stages that do not depend on where K / V
// live (work decode, tile range, Q load, mask, online-softmax step, four-wave merge, epilogues, fused-merge
// arrival) are functions written once; a policy type Kv owns what differs (see "the K / V policies"), and the
// window is `if constexpr (kWindow)`. Everything is __forceinline__, so each kernel is still one flat function;
// that the kernels do the work they did before the seam is measured, not assumed
// (scripts/compare_decode_objs.py against the previous build, profiles/decode_unify_ab.json).
// Two more kernels, fa_decode_paged_lse and fa_decode_fp8kv_lse (fa_decode_paged_lse.hpp), are the same body over
// argument structs that carry an LSE output: `if constexpr (DecLse<Args>::value)` below, absent from the five.
// Four more (fa_decode_paged_sink.hpp) are the paged four over argument structs that carry attention sinks:
// `if constexpr (DecSink<Args>::value)`, at the same three final-row sites and absent from all the others.
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
};

// The LSE variant (fa_decode_paged_lse.hpp): an argument struct with a member `lse` (pointer and the (batch,
// q-head, position) element strides of an fp32 array) makes decode_body, the fused merge and the launcher also
// write every final row's log-sum-exp. Compile-time, as the window is: the kernels whose arguments carry no
// `lse` compile without any of it.
template <class A, class = void>
struct DecLse : std::false_type {};
template <class A>
struct DecLse<A, std::void_t<decltype(std::declval<const A &>().lse)>> : std::true_type {};

// lse of row rg of (b, hkv) from the kernel's log2-unit state: ln sum_n exp(scale q.k_n) = (M + log2 L) ln 2
// in NATURAL log units; a row without a visible key (L == 0) is -inf. (The -inf travels as its bit pattern: the
// build is -ffinite-math-only.)
template <class Lse>
__device__ __forceinline__ void decode_store_lse(const fa_fwd_params &p, const Lse &o, const int g, const int b,
                                                 const int hkv, const int rg, const float M, const float L) {
    const int Sq = (int)p.seqlen_q;
    const int hq = hkv * g + rg / Sq, pos = rg % Sq;
    const float v = (M + __builtin_amdgcn_logf(L)) * 0.69314718055994531f;
    uint32_t *dst = (uint32_t *)o.ptr + ((int64_t)b * o.batch_stride + (int64_t)hq * o.head_stride +
                                         (int64_t)pos * o.seqlen_stride);
    *dst = L > 0.f ? __float_as_uint(v) : 0xff800000u;
}

// The sink variant (fa_decode_paged_sink.hpp): an argument struct with a member `sinks` (const float *, one fp32
// logit per q-head, in final-logit units) makes the three places that produce a final row -- the unsplit
// epilogue, the fused merge and fa_decode_combine_sink -- add one key of that logit and value 0 to the row's
// softmax. Compile-time, as the LSE is: the kernels whose arguments carry no `sinks` compile without any of it.
template <class A, class = void>
struct DecSink : std::false_type {};
template <class A>
struct DecSink<A, std::void_t<decltype(std::declval<const A &>().sinks)>> : std::true_type {};

// What replaces num / L for a row of q-head hq whose state is (M, L), M in log2 units: with s2 = sinks[hq] log2 e,
// Ms = max(M, s2) and e = 2^(M - Ms), the row's sum becomes L' = L e + 2^(s2 - Ms) and its acc is scaled by
// e num / L'. The max is taken first, so neither exp2 can overflow. The sink's magnitude is clamped to |kNeg| on
// its BITS (-inf and +-3e38 included: no infinity enters float arithmetic, the build is -ffinite-math-only); a
// sink that far below every score has e == 1 and L' == L exactly, and e * (num / L') is then the unsinked
// division bit for bit. A row without a visible key (L == 0) stays 0. The load is a vector load: callers stand
// behind the key loop's last s_waitcnt vmcnt(0), whose counted waits it would break.
// No contraction in here: fused into fma(sink, log2 e, -Ms), the difference s2 - Ms is the rounding error of s2
// when s2 is the max -- half an ulp of 1.4e30 for a clamped sink, far outside exp2's range, instead of 0.
__device__ __forceinline__ float decode_sink_inv(const float *sinks, const int hq, const float M, const float L,
                                                 const float num) {
#pragma clang fp contract(off)
    const uint32_t u = *(const uint32_t *)(sinks + hq);
    const uint32_t mag = min(u & 0x7fffffffu, __float_as_uint(-kNeg));
    const float s2 = __uint_as_float(mag | (u & 0x80000000u)) * 1.4426950408889634f;
    const float Ms = fmaxf(M, s2);
    const float e = __builtin_amdgcn_exp2f(M - Ms);
    const float Ls = __builtin_fmaf(L, e, __builtin_amdgcn_exp2f(s2 - Ms));
    return L > 0.f ? e * (num / Ls) : 0.f;
}

// Fused merge of a unit's n_split partials by the last of its workgroups (fa_decode, a.cnt): the same
// arithmetic as fa_decode_combine (weights 2^(lse - M) in split order, acc / L), spread over the
// workgroup: lse of every (split, row) into LDS, each row's weights by one thread, then a float4 of
// one valid row per thread per pass. Loads are device-scope (sc1: not from this CU's L1).
template <class DT, int kD, bool kExactD, class A>
__device__ __forceinline__ void decode_merge(const fa_fwd_params &p, const A &a, const int unit, const int b,
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
        if constexpr (DecSink<A>::value)  // the partials are unsinked: the sink enters here, once per row
            linv[tid] = decode_sink_inv(a.sinks, hkv * a.g + (rb * kDecRows + tid) / (int)p.seqlen_q, M, L, 1.f);
        else
            linv[tid] = L > 0.f ? 1.f / L : 0.f;
        if constexpr (DecLse<A>::value) decode_store_lse(p, a.lse, a.g, b, hkv, rb * kDecRows + tid, M, L);
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

// ---- the stages of decode_body, each written once ----------------------------------------------

// The work of a workgroup: (unit = (b, hkv, rb), split). Fused merge (a.cnt): unit u's splits are the
// workgroups (u >> 3) * n_split + split of XCD u & 7 (the hardware deals workgroups to XCDs by id mod 8),
// so the last one reads the others' partials through its own L2; the grid pads every XCD to the same
// count (the extra workgroups leave: false).
struct DecWork {
    int split, unit, rb, hkv, b;
};
template <bool kFuse>
__device__ __forceinline__ bool decode_work(const fa_fwd_params &p, const DecArgs &a, DecWork &w) {
    if constexpr (kFuse) {
        const int k = (int)(blockIdx.x >> 3);
        w.unit = ((k / a.n_split) << 3) | (int)(blockIdx.x & 7);
        w.split = k % a.n_split;
        if (w.unit >= (int)p.batch_size * (int)p.num_heads_kv * a.n_rb) return false;
    } else {
        w.split = blockIdx.x % a.n_split;
        w.unit = blockIdx.x / a.n_split;
    }
    w.rb = w.unit % a.n_rb;
    w.hkv = (w.unit / a.n_rb) % (int)p.num_heads_kv;
    w.b = w.unit / (a.n_rb * (int)p.num_heads_kv);
    return true;
}

// This wave's tiles [t_lo, t_hi): a contiguous quarter of the split's share of the sequence's tiles.
// Sliding window (kWindow, a.window_left >= 0): row m sees keys n >= m + diag - window_left, so the
// sequence's tiles start at the tile of row 0's bound -- pages wholly below it, and their table
// entries, are never read -- and the splits share [t_first, n_tiles). All of it scalar.
template <class Kv, bool kWindow>
__device__ __forceinline__ void decode_tiles(const typename Kv::Args &a, const int split, const int wave, const int Sk,
                                             const int diag, int &t_lo, int &t_hi) {
    const int n_tiles = (Sk + kDecKeys - 1) / kDecKeys;
    int t_first = 0;
    if constexpr (kWindow) t_first = max(diag - a.window_left, 0) / kDecKeys;
    const int tps = Kv::tiles_per_split(a, n_tiles - t_first);
    const int s_lo = min(t_first + split * tps, n_tiles), s_hi = min(s_lo + tps, n_tiles);
    const int per_wave = (s_hi - s_lo + kDecWaves - 1) / kDecWaves;
    t_lo = min(s_lo + wave * per_wave, s_hi);
    t_hi = min(t_lo + per_wave, s_hi);
}

// Q: the row block's 32 rows by LDS-DMA into a shared K-swizzled 16-bit image (rows are scattered over
// q-heads / positions; a descriptor over the group's span bounds them, invalid rows and columns past D
// read 0). Issued before the K/V tiles so that the ring's first counted wait retires it.
template <int kD, bool kExactD>
__device__ __forceinline__ void decode_load_q(const fa_fwd_params &p, const DecArgs &a, const DecWork &w, char *qlds,
                                              const int wave, const int lane) {
    using G = Geo<kD>;
    constexpr int RB = G::kRowBytes;
    constexpr int ROWS_PER_PIECE = 1024 / RB;
    constexpr int QPW = kDecRows * RB / 1024 / kDecWaves;  // pieces per wave: 2 / 1
    const int Sq = (int)p.seqlen_q, D = (int)p.headdim;
    const int64_t qspan = ((int64_t)(a.g - 1) * p.q_head_stride + (int64_t)(Sq - 1) * p.q_seqlen_stride + D) * 2;
    const rsrc_t qr = make_rsrc((const char *)p.q_ptr + 2 * ((int64_t)w.b * p.q_batch_stride +
                                                             (int64_t)w.hkv * a.g * p.q_head_stride),
                                (uint32_t)qspan);
#pragma unroll
    for (int n = 0; n < QPW; ++n) {
        const int piece = wave * QPW + n;
        const int row = piece * ROWS_PER_PIECE + (16 * lane) / RB;
        const int slot = ((16 * lane) % RB) / 16;
        const int ch = G::k_off(row, slot) % RB / 16;
        const int rq = w.rb * kDecRows + row;
        const int off = (rq < a.rows && (kExactD || ch * 8 < D))
                            ? 2 * ((rq / Sq) * (int)p.q_head_stride + (rq % Sq) * (int)p.q_seqlen_stride) + 16 * ch
                            : 0x7ffffff0;
        dma_one(qr, lds_u32(qlds) + piece * 1024, off, n == 0);
    }
}

// The mask of the tile at key0: lane (h, r) holds keys key0 + (i & 3) + 8 (i >> 2) + 4 h of row r, visible
// up to lim. kWindow: the lower bound lo joins it -- only a sequence's first one or two tiles enter for it
// (lo_max: the last row's bound). A row whose window starts in a later tile than row 0's sees an all-masked
// tile first: its m_use stays kNeg, msc 0, every exp2 underflows to 0 and alpha is 0 at its first visible
// key, so O and l stay 0 through it.
template <bool kWindow>
__device__ __forceinline__ void decode_mask(f32x16 &s, const int key0, const int h, const int lim, const int lo,
                                            const int lo_max) {
    if constexpr (kWindow) {
        if (__builtin_amdgcn_ballot_w64(key0 + kDecKeys - 1 > lim) || key0 < lo_max) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = key0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (key > lim || key < lo) s[i] = kNeg;
            }
        }
    } else {
        if (__builtin_amdgcn_ballot_w64(key0 + kDecKeys - 1 > lim)) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (key0 + (i & 3) + 8 * (i >> 2) + 4 * h > lim) s[i] = kNeg;
        }
    }
}

// One online-softmax step on a masked S tile: the deferred rescale of o / l_run, P = exp2(S sc - msc) with
// its fp32 row sum, and P^T rounded to DT as the B operand of O^T += V^T.P^T.
template <class DT, int DTL>
__device__ __forceinline__ void decode_softmax(f32x16 &s, f32x16 (&o)[DTL], float &m_use, float &msc, float &l_run,
                                               const float sc, const float thr_raw, u32x4 (&pf)[2]) {
    float mx = fmaxf(s[0], s[1]);
#pragma unroll
    for (int i = 2; i < 16; ++i) mx = fmaxf(mx, s[i]);
    // both lane halves hold the same row's m_use: the check needs no cross-half reduction
    if (__builtin_amdgcn_ballot_w64(mx > m_use + thr_raw)) {
        const float m_new = fmaxf(m_use, pair_max(mx));
        const float msc_new = (m_new <= 0.5f * kNeg) ? 0.f : m_new * sc;
        // a row's first visible key: O and l are still 0, alpha must not overflow
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
    for (int kk = 0; kk < 2; ++kk)
        pf[kk] = (u32x4){DT::pack(s[8 * kk + 0], s[8 * kk + 1]), DT::pack(s[8 * kk + 2], s[8 * kk + 3]),
                         DT::pack(s[8 * kk + 4], s[8 * kk + 5]), DT::pack(s[8 * kk + 6], s[8 * kk + 7])};
}

// Merge of the 4 wave partials in LDS (ow: [wave][row][kD] fp32, the rings' memory, free after the
// barrier): thread (row = tid / 8, part = tid % 8) ends with the unnormalised acc of its kD / 8 d values
// and the row's max M (log2 units) and sum L.
template <int kD>
__device__ __forceinline__ void decode_wave_merge(float *ow, const f32x16 (&o)[kD / 32], const float m_use,
                                                  const float msc, const float l_run, const int wave, const int r,
                                                  const int h, const int row, const int part, float (&acc)[kD / 8],
                                                  float &M, float &L) {
    constexpr int DTL = kD / 32, DPT = kD / 8;
    __shared__ float ml[kDecWaves][kDecRows][2];
    __syncthreads();  // every wave is done with its ring
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

    M = kNeg;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) M = fmaxf(M, ml[w][row][0]);
    float wgt[kDecWaves];
    L = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) {
        const float mw = ml[w][row][0];
        wgt[w] = (mw <= 0.5f * kNeg) ? 0.f : __builtin_amdgcn_exp2f(mw - M);
        L += wgt[w] * ml[w][row][1];
    }
#pragma unroll
    for (int i = 0; i < DPT; ++i) acc[i] = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) {
        const float *src = ow + (w * kDecRows + row) * kD + part * DPT;
#pragma unroll
        for (int i = 0; i < DPT; i += 4) {
            const float4 x = *(const float4 *)(src + i);
            // acc += wgt * x as an explicit fma, in wave order: the first wave's product is rounded, every
            // later one is fused. Written `acc += wgt * x`, the first two waves give a sum of two products,
            // and which of them the compiler fuses depends on the code around it (the results then differ by
            // an ulp between kernels, and between builds)
            acc[i] = __builtin_fmaf(wgt[w], x.x, acc[i]);
            acc[i + 1] = __builtin_fmaf(wgt[w], x.y, acc[i + 1]);
            acc[i + 2] = __builtin_fmaf(wgt[w], x.z, acc[i + 2]);
            acc[i + 3] = __builtin_fmaf(wgt[w], x.w, acc[i + 3]);
        }
    }
}

// Epilogue of an unsplit launch: O row rg2 of the (batch, kv-head), acc * inv rounded to DT
template <class DT, int kD, bool kExactD>
__device__ __forceinline__ void decode_store_o(const fa_fwd_params &p, const DecArgs &a, const DecWork &w,
                                               const int rg2, const int part, const float (&acc)[kD / 8],
                                               const float inv) {
    constexpr int DPT = kD / 8;
    const int Sq = (int)p.seqlen_q, D = (int)p.headdim;
    const int hq2 = w.hkv * a.g + rg2 / Sq, pos2 = rg2 % Sq;
    char *orow = (char *)p.o_ptr + 2 * ((int64_t)w.b * p.o_batch_stride + (int64_t)hq2 * p.o_head_stride +
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

// Epilogue of a split launch: the fp32 partial O / l and lse = M + log2 L of (unit, split, row)
template <int kD>
__device__ __forceinline__ void decode_store_partial(const DecArgs &a, const DecWork &w, const int row, const int part,
                                                     const float (&acc)[kD / 8], const float inv, const float M,
                                                     const float L) {
    constexpr int DPT = kD / 8;
    const size_t slot = ((size_t)w.unit * a.n_split + w.split) * kDecRows + row;
    float *dst = a.ws_o + slot * kD + part * DPT;
#pragma unroll
    for (int i = 0; i < DPT; i += 4)
        *(float4 *)(dst + i) = make_float4(acc[i] * inv, acc[i + 1] * inv, acc[i + 2] * inv, acc[i + 3] * inv);
    if (part == 0) a.ws_lse[slot] = L > 0.f ? M + __builtin_amdgcn_logf(L) : kNeg;  // log2
}

// Fused merge, the arrival: every thread's partials are in L2 before the workgroup arrives; the last
// arrival merges the unit (the others' stores were drained before their arrivals, and its loads bypass
// its CU's L1) and re-zeroes the counter
template <class DT, int kD, bool kExactD, class A>
__device__ __forceinline__ void decode_arrive(const fa_fwd_params &p, const A &a, const DecWork &w) {
    __shared__ uint32_t last_wg;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t old = __hip_atomic_fetch_add(a.cnt + w.unit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_wg = old + 1 == (uint32_t)a.n_split;
        if (last_wg) __hip_atomic_store(a.cnt + w.unit, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (last_wg) decode_merge<DT, kD, kExactD>(p, a, w.unit, w.b, w.hkv, w.rb);
}

// ---- the K / V policies ---------------------------------------------------------------------------
// decode_body reads K / V through a policy type Kv that owns only what differs between the dense 16-bit
// cache (DenseKv), the paged 16-bit pool (fa_decode_paged.hpp) and the paged FP8 pool
// (fa_decode_paged_fp8.hpp):
//   Args                        the kernel's argument struct (a DecArgs)
//   kElem, RB, kTile, kPieces, kSlot, kRing, kLds, k_off / v_off
//                               the LDS image of a tile and the per-wave ring
//   key_range(p, a, b, k0, Sk)  the sequence's keys; tiles_per_split(a, n)
//   scale(p, a, b, hkv, sc, vds)   the softmax scale and the numerator of the final 1 / l
//   Kv(p, a, b, hkv, k0, t_lo, t_hi), tile(t, k, v), slab(rows, stride, D)
//                               where tile t's rows are and how many bytes of them may be read
//   kStraightPrefill, prefill(issue, t_lo, t_hi) | wait_prefill(n_pre), wait_tile(t, t_hi)
//                               the ring's first tiles with the counted vmcnt wait after them (or, for a ring
//                               whose first tiles the body issues in a loop, that wait alone), and the wait
//                               before tile t is read
//   q_chunk(ks, h)              the 16-byte chunk of Q's row that is k-step ks's B operand
//   Frags                       the per-lane fragment addresses, the K / V fragment loads of a tile and the
//                               two MFMA loops

// The 16-bit image and its fragments (fa_fwd_w8 layouts), shared by the dense and the paged policy
template <int kD>
struct Kv16 : DecGeo<kD> {
    using G = Geo<kD>;
    using DecGeo<kD>::RB;
    using DecGeo<kD>::kPieces;
    static constexpr int kElem = 2;  // bytes of a K / V element
    static constexpr int kRing = 2;  // slots of a wave's LDS ring
    static constexpr int KS = G::kKSteps, DTL = G::kDTiles;

    static __device__ __forceinline__ int k_off(int row, int ch) { return G::k_off(row, ch); }
    static __device__ __forceinline__ int v_off(int row, int ch) { return G::v_off(row, ch); }
    static __device__ __forceinline__ uint32_t slab(int rows, int stride, int D) { return slab_bytes(rows, stride, D); }
    // B operand of S^T = K.Q^T: lane (h, r) holds Q[row r][16 ks + 8 h .. +7]
    static __device__ __forceinline__ int q_chunk(int ks, int h) { return 2 * ks + h; }

    // the two-slot ring's first tiles and its fixed waits: the first one also retires the Q pieces
    static constexpr bool kStraightPrefill = true;
    template <class Issue>
    static __device__ __forceinline__ void prefill(Issue &&issue, const int t_lo, const int t_hi) {
        const bool has0 = t_lo < t_hi, has1 = t_lo + 1 < t_hi;
        if (has0) issue(t_lo);
        if (has1) issue(t_lo + 1);
        if (has1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * kPieces) : "memory");
        else if (has0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kPieces) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // tile t landed (the youngest 2 * kPieces pieces, tile t + 1, may still be in flight)
    static __device__ __forceinline__ void wait_tile(const int t, const int t_hi) {
        if (t + 1 < t_hi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kPieces) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    struct Frags {
        int v_addr[DTL], k_addr[KS];
        u32x4 kf[KS], va[2][DTL];

        __device__ __forceinline__ Frags(const int lane) {
            const int r = lane & 31, h = lane >> 5;
            const int g4 = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
            for (int dt = 0; dt < DTL; ++dt)
                v_addr[dt] = G::v_off(4 * (g4 >> 1) + qq, dt * 4 + 2 * (g4 & 1) + (pp >> 1)) + 8 * (pp & 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) k_addr[ks] = G::k_off(r, 2 * ks + h);
        }
        __device__ __forceinline__ void load(const char *K, const char *V) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[ks] = *(const u32x4 *)(K + k_addr[ks]);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int dt = 0; dt < DTL; ++dt) {
                    const u32x2 lo = tr_read(V + kk * 16 * RB + v_addr[dt]);
                    const u32x2 hi = tr_read(V + kk * 16 * RB + 8 * RB + v_addr[dt]);
                    va[kk][dt] = (u32x4){lo[0], lo[1], hi[0], hi[1]};
                }
        }
        template <class DT>
        __device__ __forceinline__ f32x16 qk(const u32x4 (&qf)[KS]) const {
            f32x16 s = {};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) s = DT::mfma(kf[ks], qf[ks], s);
            return s;
        }
        template <class DT>
        __device__ __forceinline__ void pv(const u32x4 (&pf)[2], f32x16 (&o)[DTL]) const {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int dt = 0; dt < DTL; ++dt) o[dt] = DT::mfma(va[kk][dt], pf[kk], o[dt]);
        }
    };
};

// The dense cache [B, Hkv, Sk, D] of fa_decode
template <int kD>
struct DenseKv : Kv16<kD> {
    using Args = DecArgs;
    const char *kb, *vb;  // this (batch row, kv-head)'s rows from key k0
    int ks_, vs_;

    // this batch row's keys: positions [k0, k0 + Sk) (a padded batch's key range, DecArgs), else every key
    // (clamped to [0, seqlen_kv]: out-of-range positions never address outside the K / V rows)
    static __device__ __forceinline__ void key_range(const fa_fwd_params &p, const Args &a, const int b, int &k0,
                                                     int &Sk) {
        k0 = 0;
        Sk = (int)p.seqlen_kv;
        if (a.k_lo) {
            const int sk_all = Sk;
            k0 = min(max(a.k_lo[b], 0), sk_all);
            Sk = min(max(a.k_hi[b], k0), sk_all) - k0;
        }
    }
    // splits of the plan's (maximum) length; with per-sequence key ranges every split takes an equal share
    // of THIS sequence's tiles instead, so a short sequence leaves no split empty and a long one no split
    // overfull
    static __device__ __forceinline__ int tiles_per_split(const Args &a, const int n_tiles) {
        return a.k_lo ? (n_tiles + a.n_split - 1) / a.n_split : a.tps;
    }
    static __device__ __forceinline__ void scale(const fa_fwd_params &p, const Args &, int, int, float &sc,
                                                 float &vds) {
        sc = p.softmax_scale;
        vds = 1.f;
    }
    __device__ __forceinline__ DenseKv(const fa_fwd_params &p, const Args &, const int b, const int hkv, const int k0,
                                       int, int)
        : ks_((int)p.k_seqlen_stride), vs_((int)p.v_seqlen_stride) {
        kb = (const char *)p.k_ptr +
             2 * ((int64_t)b * p.k_batch_stride + (int64_t)hkv * p.k_head_stride + (int64_t)k0 * ks_);
        vb = (const char *)p.v_ptr +
             2 * ((int64_t)b * p.v_batch_stride + (int64_t)hkv * p.v_head_stride + (int64_t)k0 * vs_);
    }
    __device__ __forceinline__ void tile(const int t, const char *&k, const char *&v) const {
        const int key0 = t * kDecKeys;
        k = kb + 2 * (int64_t)key0 * ks_;
        v = vb + 2 * (int64_t)key0 * vs_;
    }
};

// ---- the one split-KV decode body, behind all five kernels -------------------------------------------
// (kFuse: the fused-merge body, a.cnt set, split launches only -- a separate instantiation, so the unsplit
// launches keep the kernel without the merge code)
template <class Kv, bool kWindow, class DT, bool kCausal, int kD, bool kExactD, bool kFuse>
__device__ __forceinline__ void decode_body(const fa_fwd_params &p, const typename Kv::Args &a) {
    using G = Geo<kD>;  // the 16-bit Q image
    constexpr int KS = G::kKSteps;
    constexpr int DTL = G::kDTiles;
    constexpr int RB = Kv::RB;
    constexpr int NP = Kv::kPieces;
    constexpr int R = Kv::kRing;
    static_assert(Kv::kLds >= kDecWaves * kDecRows * kD * 4, "the four-wave merge reuses the rings");
    __shared__ __attribute__((aligned(1024))) char lds[Kv::kLds];
    __shared__ __attribute__((aligned(1024))) char qlds[kDecRows * G::kRowBytes];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;

    DecWork w;
    if (!decode_work<kFuse>(p, a, w)) return;
    const int Sq = (int)p.seqlen_q, D = (int)p.headdim;  // Sq: positions per q-head (row addressing)
    float sc, vds;
    Kv::scale(p, a, w.b, w.hkv, sc, vds);
    const float thr_raw = kRescaleThr / sc;
    int k0, Sk;
    Kv::key_range(p, a, w.b, k0, Sk);
    const int diag = Sk - Sq;

    // this lane's row
    const int rg = w.rb * kDecRows + r;
    const bool row_ok = rg < a.rows;
    const int pos = row_ok ? rg % Sq : 0;
    const int lim = (kCausal && row_ok) ? min(Sk - 1, pos + diag) : Sk - 1;  // last visible key
    int lo = 0, lo_max = 0;  // (kWindow) this lane's first visible key; the last row's
    if constexpr (kWindow) {
        lo = pos + diag - a.window_left;
        lo_max = Sq - 1 + diag - a.window_left;
    }

    int t_lo, t_hi;
    decode_tiles<Kv, kWindow>(a, w.split, wave, Sk, diag, t_lo, t_hi);

    const int ks_ = (int)p.k_seqlen_stride, vs_ = (int)p.v_seqlen_stride;
    Kv kv(p, a, w.b, w.hkv, k0, t_lo, t_hi);

    // ---- LDS-DMA source offsets (lane-linear destination, swizzle on the source; the XOR swizzles are
    // involutions) ------------------------------------------------------------------------------
    constexpr int ROWS_PER_PIECE = 1024 / RB;
    constexpr int kChunk = 16 / Kv::kElem;  // elements of a 16-byte chunk
    int kvo[NP], vvo[NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        const int row = n * ROWS_PER_PIECE + (16 * lane) / RB;
        const int slot = ((16 * lane) % RB) / 16;
        const int kch = Kv::k_off(row, slot) % RB / 16;
        const int vch = Kv::v_off(row, slot) % RB / 16;
        kvo[n] = (kExactD || kch * kChunk < D) ? row * ks_ * Kv::kElem + 16 * kch : 0x7ffffff0;
        vvo[n] = (kExactD || vch * kChunk < D) ? row * vs_ * Kv::kElem + 16 * vch : 0x7ffffff0;
    }
    char *ring = lds + wave * Kv::kWaveLds;
    const uint32_t ring_u = lds_u32(ring);
    auto issue = [&](const int t) {
        const int key0 = t * kDecKeys;
        const int rows = min(Sk - key0, kDecKeys);
        const uint32_t dst = ring_u + (t & (R - 1)) * Kv::kSlot;
        const char *kt, *vt;
        kv.tile(t, kt, vt);
        const rsrc_t kr = make_rsrc(kt, Kv::slab(rows, ks_, D));
        const rsrc_t vr = make_rsrc(vt, Kv::slab(rows, vs_, D));
        if (a.flags & kDecNt) {
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one_nt(kr, dst + n * 1024, kvo[n], n == 0);
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one_nt(vr, dst + Kv::kTile + n * 1024, vvo[n], n == 0);
        } else {
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one(kr, dst + n * 1024, kvo[n], n == 0);
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one(vr, dst + Kv::kTile + n * 1024, vvo[n], n == 0);
        }
    };
    decode_load_q<kD, kExactD>(p, a, w, qlds, wave, lane);
    // The ring's first tiles and the counted wait behind them, which also retires the Q pieces (issued first).
    // The 16-bit policies do both in one function (two straight-line issues, the fixed two-slot waits); for a
    // ring of any depth (FP8) the loop is spelled here, where `issue` is called directly, and the policy
    // waits. Not one interface, because the compiler's layout follows where this text stands: with the
    // loop behind a policy function it was no longer unrolled in the unfused FP8 kernels, and with the
    // 16-bit issues here and their waits in the policy the second issue moved behind the fused merge
    // (profiles/decode_unify_ab.json, the code-shape gate; tests/test_paged_abi.py, the load order).
    if constexpr (Kv::kStraightPrefill) {
        Kv::prefill(issue, t_lo, t_hi);
    } else {
        const int n_pre = min(t_hi - t_lo, R);
        for (int i = 0; i < n_pre; ++i) issue(t_lo + i);
        Kv::wait_prefill(n_pre);
    }
    __syncthreads();  // every wave's Q pieces landed
    u32x4 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const u32x4 *)(qlds + G::k_off(r, Kv::q_chunk(ks, h)));

    typename Kv::Frags fr(lane);
    f32x16 o[DTL];
#pragma unroll
    for (int dt = 0; dt < DTL; ++dt) o[dt] = (f32x16){};
    float m_use = kNeg, msc = 0.f, l_run = 0.f;

    for (int t = t_lo; t < t_hi; ++t) {
        Kv::wait_tile(t, t_hi);
        const char *K = ring + (t & (R - 1)) * Kv::kSlot;
        fr.load(K, K + Kv::kTile);
        // the slot is free once its fragments are in registers: refill it with tile t + R
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t + R < t_hi) issue(t + R);

        f32x16 s = fr.template qk<DT>(qf);
        decode_mask<kWindow>(s, t * kDecKeys, h, lim, lo, lo_max);
        u32x4 pf[2];
        decode_softmax<DT, DTL>(s, o, m_use, msc, l_run, sc, thr_raw, pf);
        fr.template pv<DT>(pf, o);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    constexpr int DPT = kD / 8;  // d values per thread: thread (row = tid / 8, part = tid % 8)
    const int row = tid >> 3, part = tid & 7;
    float acc[DPT], M, L;
    decode_wave_merge<kD>((float *)lds, o, m_use, msc, l_run, wave, r, h, row, part, acc, M, L);
    const float inv = L > 0.f ? vds / L : 0.f;
    const int rg2 = w.rb * kDecRows + row;
    if (a.n_split == 1) {
        if constexpr (DecSink<typename Kv::Args>::value) {
            if (rg2 < a.rows)
                decode_store_o<DT, kD, kExactD>(p, a, w, rg2, part, acc,
                                                decode_sink_inv(a.sinks, w.hkv * a.g + rg2 / Sq, M, L, vds));
        } else {
            if (rg2 < a.rows) decode_store_o<DT, kD, kExactD>(p, a, w, rg2, part, acc, inv);
        }
        if constexpr (DecLse<typename Kv::Args>::value)
            if (rg2 < a.rows && part == 0) decode_store_lse(p, a.lse, a.g, w.b, w.hkv, rg2, M, L);
    } else {
        if (rg2 < a.rows) decode_store_partial<kD>(a, w, row, part, acc, inv, M, L);
        if constexpr (kFuse) decode_arrive<DT, kD, kExactD>(p, a, w);
    }
}

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode(const fa_fwd_params p, const DecArgs a) {
    decode_body<DenseKv<kD>, false, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

// Merge n_split partials (O / l and lse = m*s' + log2 l, log2 units): one wave per valid (q-head,
// position) row of a (batch, kv-head) -- a workgroup covers 4 of its a.rows rows, so the grid holds
// only valid rows (B * Hkv * ceil(rows / 4) workgroups) -- lane l owns d = 2l, 2l+1 (kD = 128) or
// d = l (kD = 64), so every partial row is one contiguous 512 / 256-B wave read.
// (kLse, fa_decode_combine_lse: lane 0 also writes the row's lse to `lse`; kSink, fa_decode_combine_sink: the
// row's sink, `sinks`[q-head], joins its sum -- decode_sink_inv, once per row, the partials are unsinked)
struct NoLse {};
template <class DT, int kD, bool kExactD, bool kLse, class Lse, bool kSink = false>
__device__ __forceinline__ void decode_combine_body(const fa_fwd_params &p, const DecArgs &a, const Lse &lse,
                                                    const float *sinks = nullptr) {
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
    float inv = L > 0.f ? 1.f / L : 0.f;
    const int hq = hkv * a.g + rg / Sq, pos = rg % Sq;
    if constexpr (kSink) inv = decode_sink_inv(sinks, hq, M, L, 1.f);
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
    if constexpr (kLse)
        if (lane == 0) decode_store_lse(p, lse, a.g, b, hkv, rg, M, L);
}

template <class DT, int kD, bool kExactD>
__global__ __launch_bounds__(256) void fa_decode_combine(const fa_fwd_params p, const DecArgs a) {
    decode_combine_body<DT, kD, kExactD, false>(p, a, NoLse{});
}

template <class DT, int kD, bool kExactD, class Lse>
__global__ __launch_bounds__(256) void fa_decode_combine_lse(const fa_fwd_params p, const DecArgs a, const Lse lse) {
    decode_combine_body<DT, kD, kExactD, true>(p, a, lse);
}

template <class DT, int kD, bool kExactD>
__global__ __launch_bounds__(256) void fa_decode_combine_sink(const fa_fwd_params p, const DecArgs a,
                                                              const float *sinks) {
    decode_combine_body<DT, kD, kExactD, false, NoLse, true>(p, a, NoLse{}, sinks);
}

// The launcher of every decode kernel (`fused` / `plain`: its two instantiations; `path` / `path_split`: what
// fa_debug_last_path reports): the kernel, + the split combine when a.n_split > 1 and the merge is not fused
template <class DT, int kD, bool kExact, class Args, class Kernel>
int launch_decode_kernels(const fa_fwd_params &p, Args a, void *ws, hipStream_t stream, Kernel fused, Kernel plain,
                          int path, int path_split) {
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
    hipLaunchKernelGGL(a.cnt ? fused : plain, dim3((uint32_t)grid), dim3(256), 0, stream, p, a);
    if (a.n_split > 1 && !a.cnt) {
        const dim3 cgrid((uint32_t)(p.batch_size * p.num_heads_kv * ((a.rows + 3) / 4)));
        static_assert(!(DecLse<Args>::value && DecSink<Args>::value), "no kernel writes the LSE of a sinked row");
        if constexpr (DecLse<Args>::value)
            hipLaunchKernelGGL((fa_decode_combine_lse<DT, kD, kExact, decltype(a.lse)>), cgrid, dim3(256), 0, stream, p,
                               static_cast<const DecArgs &>(a), a.lse);
        else if constexpr (DecSink<Args>::value)
            hipLaunchKernelGGL((fa_decode_combine_sink<DT, kD, kExact>), cgrid, dim3(256), 0, stream, p,
                               static_cast<const DecArgs &>(a), a.sinks);
        else
            hipLaunchKernelGGL((fa_decode_combine<DT, kD, kExact>), cgrid, dim3(256), 0, stream, p,
                               static_cast<const DecArgs &>(a));
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    set_last_path(a.n_split > 1 ? path_split : path);
    return FA_OK;
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode(const fa_fwd_params &p, DecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode<DT, C, kD, kExact, true>,
                                                 &fa_decode<DT, C, kD, kExact, false>, kPathDecode, kPathDecodeSplit);
}

}  // namespace fa
