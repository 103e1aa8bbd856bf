// fa_paged_window_launch.h -- internal seam between the sliding-window C-ABI dispatcher
// (fa_paged_window_gfx950.hip, include/fa_gfx950_paged_window.h) and the windowed paged decode instantiations
// (fa_paged_window_inst.hip x 16, fa_paged_fp8_window_inst.hip x 16), beside fa_paged_launch.h and
// fa_paged_fp8_launch.h: the unwindowed dispatchers and their instantiations never see these declarations.
//
// The window is a compile-time variant of the two paged kernels, in translation units of its own. A run-time
// window_left in the unwindowed kernels was built and measured first: the unwindowed decodes then took 1.003
// (16-bit) and 1.008 (FP8) of the parent build's time at B32 / capacity 4096, outside twice that run's A/A
// spread of 0.12-0.13 % (DESIGN.md section 5 "Sliding-window paged decode"). Here the unwindowed kernels keep
// their tokens.
#pragma once

#include "fa_paged_fp8_launch.h"

namespace fa {

// PagedDecArgs / PagedFp8DecArgs plus the window: key n is visible to query row m of sequence b only if
// n >= m + L_b - Sq - window_left. 0 <= window_left <= 2^30 (clamped by the host, so the bound cannot
// overflow 32 bits); "no window" never reaches these kernels, the dispatcher calls the unwindowed entry.
struct PagedWinDecArgs : PagedDecArgs {
    int window_left;
};
struct PagedFp8WinDecArgs : PagedFp8DecArgs {
    int window_left;
};
constexpr int64_t kPagedMaxWindow = int64_t(1) << 30;

inline int clamp_window(int64_t window_left) {
    return (int)(window_left < kPagedMaxWindow ? window_left : kPagedMaxWindow);
}
// Keys the split plan of a windowed launch is made for: a sequence's tiles run from the tile of row 0's lower
// bound to its end, window_left + seqlen_q keys that can start anywhere in a tile -- at most
// ceil((window_left + seqlen_q) / 32) + 1 tiles -- and never more than the table's capacity (p.seqlen_kv).
// A window that covers the capacity: the capacity, i.e. the unwindowed plan.
inline int64_t window_plan_keys(const fa_fwd_params &p, int64_t window_left) {
    const int64_t tiles = (clamp_window(window_left) + p.seqlen_q + kDecKeys - 1) / kDecKeys + 1;
    return tiles * kDecKeys < p.seqlen_kv ? tiles * kDecKeys : p.seqlen_kv;
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_window(const fa_fwd_params &p, PagedWinDecArgs a, void *ws, hipStream_t stream);
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window(const fa_fwd_params &p, PagedFp8WinDecArgs a, void *ws, hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_WINDOW(DT, C, D, E)                                                              \
    extern template int launch_decode_paged_window<DT, C, D, E>(const fa_fwd_params &, PagedWinDecArgs, void *,  \
                                                                hipStream_t);                                    \
    extern template int launch_decode_paged_fp8_window<DT, C, D, E>(const fa_fwd_params &, PagedFp8WinDecArgs,   \
                                                                    void *, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_WINDOW)
#undef FA_DECLARE_EXTERN_PAGED_WINDOW

}  // namespace fa
