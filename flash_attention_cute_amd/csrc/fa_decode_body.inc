// fa_decode_body.inc -- the body of the fa_decode kernel (fa_decode.hpp), included inside the kernel's
// braces by fa_decode (FA_DEC_PAGED 0) and by fa_decode_paged (fa_decode_paged.hpp, FA_DEC_PAGED 1, `a`
// a PagedDecArgs). A textual include, not a shared function template: with FA_DEC_PAGED 0 the dense
// kernel is token for token what it was, so its instantiations compile to the same code as before the
// paged kernel existed. The paged variant differs only in where a tile's K / V descriptors point
// (PagedKv) and in taking every sequence's key count from seqlens_k.
    using G = Geo<kD>;
    using DG = DecGeo<kD>;
    constexpr int KS = G::kKSteps;
    constexpr int DTL = G::kDTiles;
    constexpr int RB = DG::RB;
    constexpr int NP = DG::kPieces;
    __shared__ __attribute__((aligned(1024))) char lds[DG::kLds];
    __shared__ __attribute__((aligned(1024))) char qlds[kDecRows * RB];
    __shared__ float ml[kDecWaves][kDecRows][2];
    __shared__ uint32_t last_wg;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31;
    const int h = lane >> 5;

    // ---- work: (unit = (b, hkv, rb), split) ----------------------------------------------------
    // fused merge (a.cnt): unit u's splits are the workgroups (u >> 3) * n_split + split of XCD u & 7
    // (the hardware deals workgroups to XCDs by id mod 8), so the last one reads the others' partials
    // through its own L2; the grid pads every XCD to the same count (the extra workgroups leave)
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
    const int Sq = (int)p.seqlen_q, D = (int)p.headdim;  // Sq: positions per q-head (row addressing)
    const float sc = p.softmax_scale;
    const float thr_raw = kRescaleThr / sc;
    // this batch row's keys: positions [k0, k0 + Sk) (a padded batch's key range, DecArgs); else
    // every key
    // (clamped to [0, seqlen_kv]: out-of-range positions never address outside the K / V rows)
    int k0 = 0, Sk = (int)p.seqlen_kv;
#if FA_DEC_PAGED
    Sk = min(max(a.seqlens_k[b], 0), Sk);  // (keys [0, seqlens_k[b]), clamped to the table's capacity)
#else
    if (a.k_lo) {
        const int sk_all = Sk;
        k0 = min(max(a.k_lo[b], 0), sk_all);
        Sk = min(max(a.k_hi[b], k0), sk_all) - k0;
    }
#endif
    const int diag = Sk - Sq;

    // this lane's row
    const int rg = rb * kDecRows + r;
    const bool row_ok = rg < a.rows;
    const int pos = row_ok ? rg % Sq : 0;
    const int lim = (kCausal && row_ok) ? min(Sk - 1, pos + diag) : Sk - 1;  // last visible key

    // ---- this wave's tiles: a contiguous quarter of the split --------------------------------
    const int n_tiles = (Sk + kDecKeys - 1) / kDecKeys;
    // splits of the plan's (maximum) length; with per-sequence key ranges every split takes an equal
    // share of THIS sequence's tiles instead, so a short sequence leaves no split empty and a long
    // one no split overfull
#if FA_DEC_PAGED
    const int tps = (n_tiles + a.n_split - 1) / a.n_split;
#else
    const int tps = a.k_lo ? (n_tiles + a.n_split - 1) / a.n_split : a.tps;
#endif
    const int s_lo = min(split * tps, n_tiles), s_hi = min(s_lo + tps, n_tiles);
    const int per_wave = (s_hi - s_lo + kDecWaves - 1) / kDecWaves;
    const int t_lo = min(s_lo + wave * per_wave, s_hi), t_hi = min(t_lo + per_wave, s_hi);

    const int ks_ = (int)p.k_seqlen_stride, vs_ = (int)p.v_seqlen_stride;
#if FA_DEC_PAGED
    PagedKv pages(p, a, b, hkv, t_lo, t_hi);
#else
    const char *kb = (const char *)p.k_ptr +
                     2 * ((int64_t)b * p.k_batch_stride + (int64_t)hkv * p.k_head_stride + (int64_t)k0 * ks_);
    const char *vb = (const char *)p.v_ptr +
                     2 * ((int64_t)b * p.v_batch_stride + (int64_t)hkv * p.v_head_stride + (int64_t)k0 * vs_);
#endif

    // ---- LDS-DMA source offsets (lane-linear destination, swizzle on the source) ---------------
    constexpr int ROWS_PER_PIECE = 1024 / RB;
    int kvo[NP], vvo[NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        const int row = n * ROWS_PER_PIECE + (16 * lane) / RB;
        const int slot = ((16 * lane) % RB) / 16;
        const int kch = G::k_off(row, slot) % RB / 16;
        const int vch = G::v_off(row, slot) % RB / 16;
        kvo[n] = (kExactD || kch * 8 < D) ? row * ks_ * 2 + 16 * kch : 0x7ffffff0;
        vvo[n] = (kExactD || vch * 8 < D) ? row * vs_ * 2 + 16 * vch : 0x7ffffff0;
    }
    char *ring = lds + wave * DG::kWaveLds;
    const uint32_t ring_u = lds_u32(ring);
    auto issue = [&](const int t) {
        const int key0 = t * kDecKeys;
        const int rows = min(Sk - key0, kDecKeys);
        const uint32_t dst = ring_u + (t & 1) * DG::kSlot;
#if FA_DEC_PAGED
        const char *kt, *vt;
        pages.tile(t, kt, vt);
        const rsrc_t kr = make_rsrc(kt, slab_bytes(rows, ks_, D));
        const rsrc_t vr = make_rsrc(vt, slab_bytes(rows, vs_, D));
#else
        const rsrc_t kr = make_rsrc(kb + 2 * (int64_t)key0 * ks_, slab_bytes(rows, ks_, D));
        const rsrc_t vr = make_rsrc(vb + 2 * (int64_t)key0 * vs_, slab_bytes(rows, vs_, D));
#endif
        if (a.flags & kDecNt) {
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one_nt(kr, dst + n * 1024, kvo[n], n == 0);
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one_nt(vr, dst + DG::kTile + n * 1024, vvo[n], n == 0);
        } else {
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one(kr, dst + n * 1024, kvo[n], n == 0);
#pragma unroll
            for (int n = 0; n < NP; ++n) dma_one(vr, dst + DG::kTile + n * 1024, vvo[n], n == 0);
        }
    };
    // ---- Q: the row block's 32 rows by LDS-DMA into a shared K-swizzled image -----------------
    // (rows are scattered over q-heads / positions; a descriptor over the group's span bounds
    // them, invalid rows and columns past D read 0). Issued before the K/V tiles so that the
    // counted wait below retires it.
    {
        const int64_t qspan = ((int64_t)(a.g - 1) * p.q_head_stride + (int64_t)(Sq - 1) * p.q_seqlen_stride + D) * 2;
        const rsrc_t qr = make_rsrc((const char *)p.q_ptr + 2 * ((int64_t)b * p.q_batch_stride +
                                                                 (int64_t)hkv * a.g * p.q_head_stride),
                                    (uint32_t)qspan);
#pragma unroll
        for (int n = 0; n < DG::kQPiecesPerWave; ++n) {
            const int piece = wave * DG::kQPiecesPerWave + n;
            const int row = piece * ROWS_PER_PIECE + (16 * lane) / RB;
            const int slot = ((16 * lane) % RB) / 16;
            const int ch = G::k_off(row, slot) % RB / 16;
            const int rq = rb * kDecRows + row;
            const int off = (rq < a.rows && (kExactD || ch * 8 < D))
                                ? 2 * ((rq / Sq) * (int)p.q_head_stride + (rq % Sq) * (int)p.q_seqlen_stride) + 16 * ch
                                : 0x7ffffff0;
            dma_one(qr, lds_u32(qlds) + piece * 1024, off, n == 0);
        }
    }
    const bool has0 = t_lo < t_hi, has1 = t_lo + 1 < t_hi;
    if (has0) issue(t_lo);
    if (has1) issue(t_lo + 1);
    if (has1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * NP) : "memory");
    else if (has0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NP) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // every wave's Q pieces landed
    // B operand of S^T = K.Q^T: lane (h, r) holds Q[row r][16 ks + 8 h .. +7]
    u32x4 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const u32x4 *)(qlds + G::k_off(r, 2 * ks + h));

    // ---- per-lane LDS fragment addresses (fa_fwd_w8 layouts) ----------------------------------
    const int g4 = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    int v_addr[DTL];
#pragma unroll
    for (int dt = 0; dt < DTL; ++dt)
        v_addr[dt] = G::v_off(4 * (g4 >> 1) + qq, dt * 4 + 2 * (g4 & 1) + (pp >> 1)) + 8 * (pp & 1);
    int k_addr[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) k_addr[ks] = G::k_off(r, 2 * ks + h);

    f32x16 o[DTL];
#pragma unroll
    for (int dt = 0; dt < DTL; ++dt) o[dt] = (f32x16){};
    float m_use = kNeg, msc = 0.f, l_run = 0.f;

    for (int t = t_lo; t < t_hi; ++t) {
        // tile t landed (the youngest 2*NP pieces, tile t+1, may still be in flight)
        if (t + 1 < t_hi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NP) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const char *K = ring + (t & 1) * DG::kSlot;
        const char *V = K + DG::kTile;
        u32x4 kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *(const u32x4 *)(K + k_addr[ks]);
        u32x4 va[2][DTL];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int dt = 0; dt < DTL; ++dt) {
                const u32x2 lo = tr_read(V + kk * 16 * RB + v_addr[dt]);
                const u32x2 hi = tr_read(V + kk * 16 * RB + 8 * RB + v_addr[dt]);
                va[kk][dt] = (u32x4){lo[0], lo[1], hi[0], hi[1]};
            }
        // the slot is free once its fragments are in registers: refill it with tile t+2
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t + 2 < t_hi) issue(t + 2);

        f32x16 s = {};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = DT::mfma(kf[ks], qf[ks], s);

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
        u32x4 pf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
            pf[kk] = (u32x4){DT::pack(s[8 * kk + 0], s[8 * kk + 1]), DT::pack(s[8 * kk + 2], s[8 * kk + 3]),
                             DT::pack(s[8 * kk + 4], s[8 * kk + 5]), DT::pack(s[8 * kk + 6], s[8 * kk + 7])};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int dt = 0; dt < DTL; ++dt) o[dt] = DT::mfma(va[kk][dt], pf[kk], o[dt]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- merge the 4 wave partials in LDS ------------------------------------------------------
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
    const float inv = L > 0.f ? 1.f / L : 0.f;
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
            // fused merge: every thread's partials are in L2 before the workgroup arrives; the last
            // arrival merges the unit (the others' stores were drained before their arrivals, and
            // its loads bypass its CU's L1)
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
