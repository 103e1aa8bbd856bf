#pragma once
// fa_paged_prefill.hpp -- fa_fwd_w4 over a paged KV cache (include/fa_gfx950_paged_prefill.h), gfx950.
//
// K / V live in a pool of fixed-size pages [num_pages, Hkv, page_size, D] (any stride order, last dim
// contiguous) and sequence b's key n is row n % page_size of page block_table[b][n / page_size]. The page
// size is a multiple of the 64-key tile, so a tile never straddles a page: the only change to fa_fwd_w4 is
// where a tile's buffer descriptors point. The kernel body is fa_fwd_w4's own: fa_fwd_kernels.hpp compiled
// with FA_W4_PAGED 1 names the kernel fa_fwd_w4_paged, takes a sequence's length from seqlens_k (as the
// padded launch takes it from its row arrays) and swaps the K / V tile addressing for PagedTiles -- the tile
// order, masks, softmax, P.V, epilogue and next-block prefetch are the same tokens, so the output is that of
// the padded launch on the gathered dense cache, bit for bit. The dense translation units never define the
// macro: they preprocess to what they were.
//
// Page ids are wave-uniform scalar loads through the constant address space, fetched one page ahead of
// their use (PagedTiles::advance), so their latency sits behind at least one tile of MFMA / softmax work.
// They must stay scalar loads: a vector load in the tile loop would count against the vmcnt values its
// waits are written for (vmcnt_enc(kOStores), dma_wait), and could pull the descriptors into VGPRs, which
// the LDS-DMA asm cannot take.
#define FA_W4_PAGED 1
#include "fa_paged_prefill_launch.h"
#include "fa_fwd_kernels.hpp"

namespace fa {

// Always fa_fwd_w4_paged, whatever g * Sq (the caller picks decode or prefill). Plain 256-row blocks only:
// key-split, zigzag and head-packed blocks are off, as for every launch with per-sequence key ranges.
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged(const fa_fwd_params &p, const PagedPrefillArgs &a, int window_left, hipStream_t stream) {
    PathArgs xa{};
    xa.window_left = window_left;
    const int64_t n_qtiles = (p.seqlen_q + kBlockM - 1) / kBlockM;
    const int64_t nwg = n_qtiles * p.num_heads_q * p.batch_size;
    hipLaunchKernelGGL((fa_fwd_w4_paged<DT, C, kD, kExact>), dim3((uint32_t)w4_grid(nwg)), dim3(256), 0, stream, p,
                       (int)n_qtiles, 0, stamp_buffer(), xa, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    set_last_path(kPathW4);  // (it is that kernel: fa_debug_last_prefill_paged tells the two apart)
    set_last_zigzag(0);
    set_last_prefill_paged(true);
    return FA_OK;
}

}  // namespace fa
