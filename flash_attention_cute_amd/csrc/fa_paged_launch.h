// fa_paged_launch.h -- internal seam between the paged-decode C-ABI dispatcher (fa_paged_gfx950.hip: the
// 16-bit, FP8 and sliding-window entries) and the paged decode instantiations (fa_paged_inst.hip,
// fa_paged_fp8_inst.hip, fa_paged_window_inst.hip, fa_paged_fp8_window_inst.hip, x 16 each), beside
// fa_launch.h: the dense dispatcher and its instantiations never see these declarations.
#pragma once

#include "fa_launch.h"

namespace fa {

// fa_debug_last_path values of the FP8 paged decode (after fa_launch.h's Path)
constexpr int kPathDecodePagedFp8 = 11, kPathDecodePagedFp8Split = 12;

// DecArgs plus the page indirection (fa_decode_paged.hpp). In the fa_fwd_params that go with it k_ptr /
// v_ptr are the pool bases, k / v_batch_stride the PAGE stride and seqlen_kv = max_pages * page_size
// (the plan's length); k_lo / k_hi stay nullptr -- a sequence's keys are [0, seqlens_k[b]).
struct PagedDecArgs : DecArgs {
    const int32_t *block_table;  // [B, max_pages] page ids, device
    int64_t block_table_stride;  // elements between rows
    const int32_t *seqlens_k;    // [B], device; clamped to [0, max_pages * page_size] by the kernel
    int num_pages;               // pages of the pool: ids are clamped into [0, num_pages)
    int tiles_per_page;          // page_size / kDecKeys
};
// PagedDecArgs plus the descales (fa_decode_paged_fp8.hpp). In the fa_fwd_params that go with it the k / v
// pointers and strides describe 1-byte e4m3 elements; q / o are the 16-bit DT.
struct PagedFp8DecArgs : PagedDecArgs {
    const float *k_descale, *v_descale;  // [B, Hkv] fp32, device; nullptr: 1.0
    int64_t descale_batch_stride, descale_head_stride;
};
// Either plus the window (fa_decode_paged_window.hpp): key n is visible to query row m of sequence b only if
// n >= m + L_b - Sq - window_left. 0 <= window_left <= 2^30 (clamped by the host, so the bound cannot
// overflow 32 bits); "no window" never reaches these kernels, the dispatcher runs the unwindowed launch.
//
// The window is a compile-time variant of the two paged kernels, in translation units of its own. A run-time
// window_left in the unwindowed kernels was built and measured first: the unwindowed decodes then took 1.003
// (16-bit) and 1.008 (FP8) of the parent build's time at B32 / capacity 4096, outside twice that run's A/A
// spread of 0.12-0.13 % (DESIGN.md section 5 "Sliding-window paged decode").
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

// The split plan of the FP8 launches: decode_plan's rule (every wave at least kDecMinTilesPerWave tiles, at
// most kDecMaxSplit splits) aiming at kFp8DecTargetWgs workgroups instead of kDecTargetWgs. A workgroup
// streams half the bytes per key here, and the measured optimum moves from "fewer, longer splits" to one
// workgroup per CU: B1 Hkv8 131072 keys, same process, 0.0814 / 0.0635 / 0.0555 / 0.0486 / 0.0484 ms at
// 96 / 128 / 160 / 192 / 256 workgroups (profiles/fp8_decode_target_ab.json). A dec_target knob that was
// moved off its default wins.
constexpr int64_t kFp8DecTargetWgs = 256;

inline DecArgs fp8_decode_plan(const fa_fwd_params &p, int max_split) {
    DecArgs a = decode_plan(p, max_split);
    if (knobs().dec_target != kDecTargetWgs) return a;
    const int64_t units = decode_units(p, a);
    const int n_tiles = (int)((p.seqlen_kv + kDecKeys - 1) / kDecKeys);
    int64_t ns = (kFp8DecTargetWgs + units - 1) / units;
    const int64_t by_len = n_tiles / (kDecWaves * kDecMinTilesPerWave);
    ns = ns < by_len ? ns : by_len;
    ns = ns < max_split ? ns : max_split;
    ns = ns < 1 ? 1 : ns;
    a.tps = (int)((n_tiles + ns - 1) / ns);
    a.n_split = (n_tiles + a.tps - 1) / a.tps;
    return a;
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged(const fa_fwd_params &p, PagedDecArgs a, void *ws, hipStream_t stream);
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8(const fa_fwd_params &p, PagedFp8DecArgs a, void *ws, hipStream_t stream);
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_window(const fa_fwd_params &p, PagedWinDecArgs a, void *ws, hipStream_t stream);
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window(const fa_fwd_params &p, PagedFp8WinDecArgs a, void *ws, hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED(DT, C, D, E)                                                                     \
    extern template int launch_decode_paged<DT, C, D, E>(const fa_fwd_params &, PagedDecArgs, void *, hipStream_t); \
    extern template int launch_decode_paged_fp8<DT, C, D, E>(const fa_fwd_params &, PagedFp8DecArgs, void *,     \
                                                             hipStream_t);                                       \
    extern template int launch_decode_paged_window<DT, C, D, E>(const fa_fwd_params &, PagedWinDecArgs, void *,  \
                                                                hipStream_t);                                    \
    extern template int launch_decode_paged_fp8_window<DT, C, D, E>(const fa_fwd_params &, PagedFp8WinDecArgs,   \
                                                                    void *, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED)
#undef FA_DECLARE_EXTERN_PAGED

}  // namespace fa
