#pragma once
// fa_decode_paged.hpp -- fa_decode over a paged KV cache (include/fa_gfx950_paged.h), gfx950.
//
// K / V live in a pool of fixed-size pages [num_pages, Hkv, page_size, D] (any stride order, last dim
// contiguous) and sequence b's key n is row n % page_size of page block_table[b][n / page_size]. The
// page size is a multiple of the 32-key tile, so a tile never straddles a page: the only change to
// fa_decode is where a tile's buffer descriptors point and where a sequence's key count comes from -- the
// PagedKv16 policy of decode_body (fa_decode.hpp), over the page walker PagedWalk. The four-wave LDS merge,
// the fp32 partials, the fused merge and fa_decode_combine are shared, and every split takes an equal share
// of its sequence's tiles -- the arithmetic, in its order, of the padded decode (a.k_lo) on the gathered
// dense cache.
//
// The page id is a wave-uniform scalar load. It is fetched when the PREVIOUS tile's DMA is issued (and
// only when that tile was its page's last), so its latency sits behind a tile of MFMA / softmax work
// and never in front of the LDS-DMA issue: the key loop's existing s_waitcnt lgkmcnt(0) before the
// refill has retired it. It must stay a scalar load -- a vector load in the key loop would count
// against the vmcnt that the loop's waits are written for.
#include "fa_decode.hpp"
#include "fa_paged_launch.h"

namespace fa {

// The walk over a sequence's pages, for elements of kElem bytes (2: fp16 / bf16 pools, 1: e4m3 pools)
template <int kElem>
struct PagedWalk {
    typedef const __attribute__((address_space(4))) int32_t *table_t;  // (constant space: a scalar load)
    const char *kh, *vh;  // the pool at this kv-head
    int64_t kps, vps;     // page strides, bytes
    int ks_, vs_;
    table_t row;          // this sequence's block-table row
    int tpp, last_page, t_hi;
    int pi, tip, phys;    // the next tile: its page index in the row, its tile within the page, the page id

    __device__ __forceinline__ PagedWalk(const fa_fwd_params &p, const PagedDecArgs &a, int b, int hkv, int t_lo,
                                         int t_hi_)
        : kps(kElem * p.k_batch_stride), vps(kElem * p.v_batch_stride), ks_((int)p.k_seqlen_stride),
          vs_((int)p.v_seqlen_stride), tpp(a.tiles_per_page), last_page(a.num_pages - 1), t_hi(t_hi_) {
        kh = (const char *)p.k_ptr + kElem * (int64_t)hkv * p.k_head_stride;
        vh = (const char *)p.v_ptr + kElem * (int64_t)hkv * p.v_head_stride;
        row = (table_t)(a.block_table + (int64_t)b * a.block_table_stride);
        pi = t_lo / tpp;
        tip = t_lo - pi * tpp;
        // (a wave without tiles reads no entry: t_lo < t_hi <= the sequence's tiles)
        phys = t_lo < t_hi ? row[pi] : 0;
    }
    // bases of tile t's K and V rows; called once per tile, in increasing t from the wave's first tile
    // (any absolute tile: a window's pages below it are never looked up). The id is clamped into the pool,
    // so a bad entry never addresses outside it; the page term is 64-bit (a pool holds more than 2^31
    // elements); rows past the sequence end are cut off by the caller's descriptor bound, never read from
    // the page.
    __device__ __forceinline__ void tile(int t, const char *&k, const char *&v) {
        const int64_t page = min(max(phys, 0), last_page);
        const int64_t r0 = (int64_t)(tip * kDecKeys) * kElem;
        k = kh + page * kps + r0 * ks_;
        v = vh + page * vps + r0 * vs_;
        if (++tip == tpp) {
            tip = 0;
            ++pi;
            if (t + 1 < t_hi) phys = row[pi];  // the next tile's page, one tile ahead of its use
        }
    }
};

// What the paged policies share: every sequence's key count from seqlens_k (keys [0, seqlens_k[b]), clamped
// to the table's capacity), an equal share of ITS tiles per split, and the walk
template <int kElem, class ArgsT>
struct PagedSeq : PagedWalk<kElem> {
    using Args = ArgsT;
    typedef const __attribute__((address_space(4))) int32_t *len_t;  // (constant space: a scalar load)

    static __device__ __forceinline__ void key_range(const fa_fwd_params &p, const Args &a, const int b, int &k0,
                                                     int &Sk) {
        k0 = 0;
        if constexpr (DecLse<Args>::value) {
            // the LSE variant's length options (fa_paged_lse_launch.h): L_b = clamp(seqlens_k[b] + seqlen_offset),
            // seqlens_k == nullptr: every sequence has clamp(seqlen_offset) keys. |seqlen_offset| <= 2^30 (host)
            const int64_t n = (int64_t)(a.seqlens_k ? ((len_t)a.seqlens_k)[b] : 0) + a.seqlen_offset;
            Sk = (int)(n < 0 ? 0 : n < p.seqlen_kv ? n : p.seqlen_kv);
        } else {
            Sk = min(max(((len_t)a.seqlens_k)[b], 0), (int)p.seqlen_kv);
        }
    }
    static __device__ __forceinline__ int tiles_per_split(const Args &a, const int n_tiles) {
        return (n_tiles + a.n_split - 1) / a.n_split;
    }
    __device__ __forceinline__ PagedSeq(const fa_fwd_params &p, const Args &a, int b, int hkv, int, int t_lo, int t_hi)
        : PagedWalk<kElem>(p, a, b, hkv, t_lo, t_hi) {}
};

// The paged 16-bit pool (ArgsT: PagedDecArgs, or PagedWinDecArgs for the windowed kernel)
template <int kD, class ArgsT = PagedDecArgs>
struct PagedKv16 : Kv16<kD>, PagedSeq<2, ArgsT> {
    using PagedSeq<2, ArgsT>::PagedSeq;
    static __device__ __forceinline__ void scale(const fa_fwd_params &p, const ArgsT &, int, int, float &sc,
                                                 float &vds) {
        sc = p.softmax_scale;
        vds = 1.f;
    }
};

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_paged(const fa_fwd_params p, const PagedDecArgs a) {
    decode_body<PagedKv16<kD>, false, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged(const fa_fwd_params &p, PagedDecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_paged<DT, C, kD, kExact, true>,
                                                 &fa_decode_paged<DT, C, kD, kExact, false>, kPathDecodePaged,
                                                 kPathDecodePagedSplit);
}

}  // namespace fa
