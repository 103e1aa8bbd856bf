// fa_paged_sink_launch.h -- internal seam between the attention-sink dispatcher (fa_paged_sink_gfx950.hip) and the
// sink instantiations of the paged decode (fa_paged_sink_inst.hip, fa_paged_fp8_sink_inst.hip,
// fa_paged_window_sink_inst.hip, fa_paged_fp8_window_sink_inst.hip, x 16 each), beside fa_paged_launch.h and
// fa_paged_lse_launch.h: the other dispatchers and instantiations never see these declarations.
#pragma once

#include "fa_paged_launch.h"

namespace fa {

// The four paged argument structs plus the sinks (include/fa_gfx950_sink.h): one fp32 logit per q-head, [Hq],
// device, in final-logit units (no softmax_scale, no k_descale). The member `sinks` is what selects the sink code
// of decode_body, decode_merge and the launcher (fa_decode.hpp DecSink).
//
// A compile-time variant in translation units of its own, as the window and the LSE are (PagedWinDecArgs in
// fa_paged_launch.h has the measurement that rejected a run-time switch in the existing kernels); the window
// stays compile-time inside these kernels as well.
struct PagedSinkDecArgs : PagedDecArgs {
    const float *sinks;
};
struct PagedFp8SinkDecArgs : PagedFp8DecArgs {
    const float *sinks;
};
struct PagedWinSinkDecArgs : PagedWinDecArgs {
    const float *sinks;
};
struct PagedFp8WinSinkDecArgs : PagedFp8WinDecArgs {
    const float *sinks;
};

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_sink(const fa_fwd_params &p, PagedSinkDecArgs a, void *ws, hipStream_t stream);
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_sink(const fa_fwd_params &p, PagedFp8SinkDecArgs a, void *ws, hipStream_t stream);
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_window_sink(const fa_fwd_params &p, PagedWinSinkDecArgs a, void *ws, hipStream_t stream);
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window_sink(const fa_fwd_params &p, PagedFp8WinSinkDecArgs a, void *ws,
                                        hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_SINK(DT, C, D, E)                                                                  \
    extern template int launch_decode_paged_sink<DT, C, D, E>(const fa_fwd_params &, PagedSinkDecArgs, void *,     \
                                                              hipStream_t);                                        \
    extern template int launch_decode_paged_fp8_sink<DT, C, D, E>(const fa_fwd_params &, PagedFp8SinkDecArgs,      \
                                                                  void *, hipStream_t);                            \
    extern template int launch_decode_paged_window_sink<DT, C, D, E>(const fa_fwd_params &, PagedWinSinkDecArgs,   \
                                                                     void *, hipStream_t);                         \
    extern template int launch_decode_paged_fp8_window_sink<DT, C, D, E>(const fa_fwd_params &,                    \
                                                                         PagedFp8WinSinkDecArgs, void *,           \
                                                                         hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_SINK)
#undef FA_DECLARE_EXTERN_PAGED_SINK

}  // namespace fa
