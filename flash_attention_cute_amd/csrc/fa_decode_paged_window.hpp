#pragma once
// fa_decode_paged_window.hpp -- fa_decode_paged and fa_decode_fp8kv with a sliding window
// (include/fa_gfx950_paged_window.h), gfx950: decode_body (fa_decode.hpp) with kWindow = true and the paged
// policies over PagedWinDecArgs / PagedFp8WinDecArgs, in kernels and translation units of their own -- the
// window is a compile-time variant (fa_paged_launch.h has the measurement that rejected a run-time one). What it
// changes is under decode_body's `if constexpr (kWindow)`: the sequence's tiles are [t_first, n_tiles), shared
// equally by the splits, and a per-row lower bound joins the mask. PagedWalk starts at any absolute tile, so pages
// below t_first are never looked up.
#include "fa_decode_paged_fp8.hpp"

namespace fa {

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_paged_window(const fa_fwd_params p, const PagedWinDecArgs a) {
    decode_body<PagedKv16<kD, PagedWinDecArgs>, true, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_fp8kv_window(const fa_fwd_params p, const PagedFp8WinDecArgs a) {
    decode_body<PagedKv8<kD, PagedFp8WinDecArgs>, true, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_window(const fa_fwd_params &p, PagedWinDecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_paged_window<DT, C, kD, kExact, true>,
                                                 &fa_decode_paged_window<DT, C, kD, kExact, false>, kPathDecodePaged,
                                                 kPathDecodePagedSplit);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window(const fa_fwd_params &p, PagedFp8WinDecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_fp8kv_window<DT, C, kD, kExact, true>,
                                                 &fa_decode_fp8kv_window<DT, C, kD, kExact, false>,
                                                 kPathDecodePagedFp8, kPathDecodePagedFp8Split);
}

}  // namespace fa
