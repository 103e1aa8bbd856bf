#pragma once
// fa_decode_paged.hpp -- fa_decode over a paged KV cache (include/fa_gfx950_paged.h), gfx950.
//
// K / V live in a pool of fixed-size pages [num_pages, Hkv, page_size, D] (any stride order, last dim
// contiguous) and sequence b's key n is row n % page_size of page block_table[b][n / page_size]. The
// page size is a multiple of the 32-key tile, so a tile never straddles a page: the only change to
// fa_decode is where a tile's buffer descriptors point (PagedKv below; the kernel body is fa_decode's own,
// fa_decode_body.inc with FA_DEC_PAGED 1). The four-wave LDS merge, the fp32 partials, the fused merge and fa_decode_combine are shared,
// and every split takes an equal share of its sequence's tiles -- the arithmetic, in its order, of the
// padded decode (a.k_lo) on the gathered dense cache.
//
// The page id is a wave-uniform scalar load. It is fetched when the PREVIOUS tile's DMA is issued (and
// only when that tile was its page's last), so its latency sits behind a tile of MFMA / softmax work
// and never in front of the LDS-DMA issue: the key loop's existing s_waitcnt lgkmcnt(0) before the
// refill has retired it. It must stay a scalar load -- a vector load in the key loop would count
// against the vmcnt that the loop's waits are written for.
#include "fa_decode.hpp"
#include "fa_paged_launch.h"

namespace fa {

struct PagedKv {
    typedef const __attribute__((address_space(4))) int32_t *table_t;  // (constant space: a scalar load)
    const char *kh, *vh;  // the pool at this kv-head
    int64_t kps, vps;     // page strides, bytes
    int ks_, vs_;
    table_t row;          // this sequence's block-table row
    int tpp, last_page, t_hi;
    int pi, tip, phys;    // the next tile: its page index in the row, its tile within the page, the page id

    __device__ __forceinline__ PagedKv(const fa_fwd_params &p, const PagedDecArgs &a, int b, int hkv, int t_lo,
                                       int t_hi_)
        : kps(2 * p.k_batch_stride), vps(2 * p.v_batch_stride), ks_((int)p.k_seqlen_stride),
          vs_((int)p.v_seqlen_stride), tpp(a.tiles_per_page), last_page(a.num_pages - 1), t_hi(t_hi_) {
        kh = (const char *)p.k_ptr + 2 * (int64_t)hkv * p.k_head_stride;
        vh = (const char *)p.v_ptr + 2 * (int64_t)hkv * p.v_head_stride;
        row = (table_t)(a.block_table + (int64_t)b * a.block_table_stride);
        pi = t_lo / tpp;
        tip = t_lo - pi * tpp;
        // (a wave without tiles reads no entry: t_lo < t_hi <= the sequence's tiles)
        phys = t_lo < t_hi ? row[pi] : 0;
    }
    // bases of tile t's K and V rows; called once per tile, in increasing t from the wave's first tile.
    // The id is clamped into the pool, so a bad entry never addresses outside it; the page term is
    // 64-bit (a pool holds more than 2^31 elements); rows past the sequence end are cut off by the
    // caller's descriptor bound, never read from the page.
    __device__ __forceinline__ void tile(int t, const char *&k, const char *&v) {
        const int64_t page = min(max(phys, 0), last_page);
        const int64_t r0 = (int64_t)(tip * kDecKeys) * 2;
        k = kh + page * kps + r0 * ks_;
        v = vh + page * vps + r0 * vs_;
        if (++tip == tpp) {
            tip = 0;
            ++pi;
            if (t + 1 < t_hi) phys = row[pi];  // the next tile's page, one tile ahead of its use
        }
    }
};

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_paged(const fa_fwd_params p, const PagedDecArgs a) {
#define FA_DEC_PAGED 1
#include "fa_decode_body.inc"
#undef FA_DEC_PAGED
}

// as launch_decode: the paged kernel (+ the split combine when a.n_split > 1 and the merge is not fused)
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged(const fa_fwd_params &p, PagedDecArgs a, void *ws, hipStream_t stream) {
    const int64_t units = decode_units(p, a);
    if (a.n_split > 1) {
        const int64_t slots = units * a.n_split * kDecRows;
        a.ws_o = (float *)ws;
        a.ws_lse = (float *)((char *)ws + slots * kD * 4);
    }
    if (a.n_split > 1 && knobs().dec_fuse && same_xcd_placement()) {
        unsigned *err = nullptr;
        a.cnt = split_sync_area(stream, units * 4, &err);
    }
    set_last_dec_fused(a.cnt != nullptr);
    const int64_t grid = a.cnt ? 8 * ((units + 7) / 8) * a.n_split : units * a.n_split;
    if (a.cnt)
        hipLaunchKernelGGL((fa_decode_paged<DT, C, kD, kExact, true>), dim3((uint32_t)grid), dim3(256), 0, stream, p, a);
    else
        hipLaunchKernelGGL((fa_decode_paged<DT, C, kD, kExact>), dim3((uint32_t)grid), dim3(256), 0, stream, p, a);
    if (a.n_split > 1 && !a.cnt)
        hipLaunchKernelGGL((fa_decode_combine<DT, kD, kExact>),
                           dim3((uint32_t)(p.batch_size * p.num_heads_kv * ((a.rows + 3) / 4))), dim3(256), 0, stream,
                           p, static_cast<const DecArgs &>(a));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    set_last_path(a.n_split > 1 ? kPathDecodePagedSplit : kPathDecodePaged);
    return FA_OK;
}

}  // namespace fa
