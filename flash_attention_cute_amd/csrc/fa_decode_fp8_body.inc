// fa_decode_fp8_body.inc -- the body of the fa_decode_fp8kv kernel (fa_decode_paged_fp8.hpp), included inside
// the kernel's braces by fa_decode_fp8kv and, with FA_DEC_WINDOW 1 and `a` a PagedFp8WinDecArgs, by
// fa_decode_fp8kv_window (fa_decode_paged_fp8_window.hpp). A textual include for the reason fa_decode_body.inc
// is one: without FA_DEC_WINDOW the kernel is token for token what it was.
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
#if FA_DEC_WINDOW
    // sliding window (a.window_left >= 0), as fa_decode_body.inc: the tiles start at the tile of row 0's lower
    // bound, the splits share [t_first, n_tiles); scalar arithmetic
    const int t_first = max(diag - a.window_left, 0) / kDecKeys;
    const int lo = pos + diag - a.window_left;         // this lane's first visible key
    const int lo_max = Sq - 1 + diag - a.window_left;  // the last row's: tiles that start below it are masked
    const int tps = (n_tiles - t_first + a.n_split - 1) / a.n_split;
    const int s_lo = min(t_first + split * tps, n_tiles), s_hi = min(s_lo + tps, n_tiles);
#else
    const int tps = (n_tiles + a.n_split - 1) / a.n_split;
    const int s_lo = min(split * tps, n_tiles), s_hi = min(s_lo + tps, n_tiles);
#endif
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
#if FA_DEC_WINDOW
        // (the window's lower bound joins the mask, as in fa_decode_body.inc)
        if (__builtin_amdgcn_ballot_w64(key0 + kDecKeys - 1 > lim) || key0 < lo_max) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = key0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (key > lim || key < lo) s[i] = kNeg;
            }
        }
#else
        if (__builtin_amdgcn_ballot_w64(key0 + kDecKeys - 1 > lim)) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (key0 + (i & 3) + 8 * (i >> 2) + 4 * h > lim) s[i] = kNeg;
        }
#endif
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
