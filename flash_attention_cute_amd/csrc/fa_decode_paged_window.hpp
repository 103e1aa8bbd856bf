#pragma once
// fa_decode_paged_window.hpp -- fa_decode_paged and fa_decode_fp8kv with a sliding window
// (include/fa_gfx950_paged_window.h), gfx950: the two kernel bodies expanded once more with FA_DEC_WINDOW 1
// (`a` a PagedWinDecArgs / PagedFp8WinDecArgs), in kernels and translation units of their own, so the
// unwindowed kernels compile to what they were. What the window changes is in the bodies' FA_DEC_WINDOW blocks:
// the sequence's tiles are [t_first, n_tiles), shared equally by the splits, and a per-row lower bound joins
// the mask. PagedKv / PagedKv8 start at any absolute tile, so pages below t_first are never looked up.
#include "fa_decode_paged.hpp"
#include "fa_decode_paged_fp8.hpp"
#include "fa_paged_window_launch.h"

namespace fa {

#define FA_DEC_WINDOW 1
template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_paged_window(const fa_fwd_params p, const PagedWinDecArgs a) {
#define FA_DEC_PAGED 1
#include "fa_decode_body.inc"
#undef FA_DEC_PAGED
}

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_fp8kv_window(const fa_fwd_params p, const PagedFp8WinDecArgs a) {
#include "fa_decode_fp8_body.inc"
}
#undef FA_DEC_WINDOW

// as launch_decode_paged / launch_decode_paged_fp8, for either windowed kernel (`fused` / `plain`: its two
// instantiations): the kernel (+ the split combine when a.n_split > 1 and the merge is not fused)
template <class DT, int kD, bool kExact, class Args, class Kernel>
int launch_window_kernels(const fa_fwd_params &p, Args a, void *ws, hipStream_t stream, Kernel fused, Kernel plain,
                          int path, int path_split) {
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
    hipLaunchKernelGGL(a.cnt ? fused : plain, dim3((uint32_t)grid), dim3(256), 0, stream, p, a);
    if (a.n_split > 1 && !a.cnt)
        hipLaunchKernelGGL((fa_decode_combine<DT, kD, kExact>),
                           dim3((uint32_t)(p.batch_size * p.num_heads_kv * ((a.rows + 3) / 4))), dim3(256), 0, stream,
                           p, static_cast<const DecArgs &>(a));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    set_last_path(a.n_split > 1 ? path_split : path);
    return FA_OK;
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_window(const fa_fwd_params &p, PagedWinDecArgs a, void *ws, hipStream_t stream) {
    return launch_window_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_paged_window<DT, C, kD, kExact, true>,
                                                 &fa_decode_paged_window<DT, C, kD, kExact, false>, kPathDecodePaged,
                                                 kPathDecodePagedSplit);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window(const fa_fwd_params &p, PagedFp8WinDecArgs a, void *ws, hipStream_t stream) {
    return launch_window_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_fp8kv_window<DT, C, kD, kExact, true>,
                                                 &fa_decode_fp8kv_window<DT, C, kD, kExact, false>, kPathDecodePagedFp8,
                                                 kPathDecodePagedFp8Split);
}

}  // namespace fa
