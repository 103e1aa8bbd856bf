#pragma once
// fa_decode_paged_sink.hpp -- the four paged decode kernels with attention sinks (include/fa_gfx950_sink.h),
// gfx950: decode_body (fa_decode.hpp) with the paged policies over PagedSinkDecArgs / PagedFp8SinkDecArgs
// (kWindow = false) and PagedWinSinkDecArgs / PagedFp8WinSinkDecArgs (kWindow = true), in kernels and translation
// units of their own. A sink is one learned logit per q-head that joins the softmax denominator and contributes no
// value: softmax over the row's keys plus one key of logit sinks[h] and value 0. The member `sinks` of the argument
// struct turns on, at compile time (DecSink), the three places where a final row is produced: the unsplit epilogue
// (decode_store_o's factor), the fused merge (decode_merge, thread tid < nrow) and fa_decode_combine_sink. Each
// replaces 1 / L by decode_sink_inv's e / (L e + 2^(s2 - max(M, s2))). The partials of a split launch are the
// unsinked ones, so the sink is applied once per row. The key loop is the one of the kernels without sinks; the
// sink's vector load stands behind the loop's last s_waitcnt vmcnt(0), so the ring's counted waits hold.
#include "fa_decode_paged_window.hpp"
#include "fa_paged_sink_launch.h"

namespace fa {

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_paged_sink(const fa_fwd_params p, const PagedSinkDecArgs a) {
    decode_body<PagedKv16<kD, PagedSinkDecArgs>, false, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_fp8kv_sink(const fa_fwd_params p, const PagedFp8SinkDecArgs a) {
    decode_body<PagedKv8<kD, PagedFp8SinkDecArgs>, false, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_paged_window_sink(const fa_fwd_params p,
                                                                      const PagedWinSinkDecArgs a) {
    decode_body<PagedKv16<kD, PagedWinSinkDecArgs>, true, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_fp8kv_window_sink(const fa_fwd_params p,
                                                                      const PagedFp8WinSinkDecArgs a) {
    decode_body<PagedKv8<kD, PagedFp8WinSinkDecArgs>, true, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_sink(const fa_fwd_params &p, PagedSinkDecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_paged_sink<DT, C, kD, kExact, true>,
                                                 &fa_decode_paged_sink<DT, C, kD, kExact, false>, kPathDecodePaged,
                                                 kPathDecodePagedSplit);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_sink(const fa_fwd_params &p, PagedFp8SinkDecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_fp8kv_sink<DT, C, kD, kExact, true>,
                                                 &fa_decode_fp8kv_sink<DT, C, kD, kExact, false>, kPathDecodePagedFp8,
                                                 kPathDecodePagedFp8Split);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_window_sink(const fa_fwd_params &p, PagedWinSinkDecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream,
                                                 &fa_decode_paged_window_sink<DT, C, kD, kExact, true>,
                                                 &fa_decode_paged_window_sink<DT, C, kD, kExact, false>,
                                                 kPathDecodePaged, kPathDecodePagedSplit);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window_sink(const fa_fwd_params &p, PagedFp8WinSinkDecArgs a, void *ws,
                                        hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream,
                                                 &fa_decode_fp8kv_window_sink<DT, C, kD, kExact, true>,
                                                 &fa_decode_fp8kv_window_sink<DT, C, kD, kExact, false>,
                                                 kPathDecodePagedFp8, kPathDecodePagedFp8Split);
}

}  // namespace fa
