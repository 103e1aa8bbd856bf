// Host-only stand-ins for the 4 x 16 attention-sink paged decode instantiations (csrc/fa_paged_sink_inst.hip,
// csrc/fa_paged_fp8_sink_inst.hip and their two windowed files), beside paged_stub_instances.hip: the sink
// dispatcher (csrc/fa_paged_sink_gfx950.hip) links into its sanitizer test driver without device code, and a
// launch that gets past validation reports FA_ERR_UNSUPPORTED.
#include "fa_paged_sink_launch.h"

namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_sink(const fa_fwd_params &, PagedSinkDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_sink(const fa_fwd_params &, PagedFp8SinkDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_window_sink(const fa_fwd_params &, PagedWinSinkDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window_sink(const fa_fwd_params &, PagedFp8WinSinkDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
#define FA_STUB_SINK_INSTANCE(DT, C, D, E)                                                                          \
    template int launch_decode_paged_sink<DT, C, D, E>(const fa_fwd_params &, PagedSinkDecArgs, void *, hipStream_t); \
    template int launch_decode_paged_fp8_sink<DT, C, D, E>(const fa_fwd_params &, PagedFp8SinkDecArgs, void *,      \
                                                           hipStream_t);                                            \
    template int launch_decode_paged_window_sink<DT, C, D, E>(const fa_fwd_params &, PagedWinSinkDecArgs, void *,   \
                                                              hipStream_t);                                         \
    template int launch_decode_paged_fp8_window_sink<DT, C, D, E>(const fa_fwd_params &, PagedFp8WinSinkDecArgs,    \
                                                                  void *, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_STUB_SINK_INSTANCE)
}  // namespace fa
