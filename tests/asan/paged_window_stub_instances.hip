// Host-only stand-ins for the 32 windowed paged decode instantiations (csrc/fa_paged_window_inst.hip,
// csrc/fa_paged_fp8_window_inst.hip), beside paged_stub_instances.hip and fp8_stub_instances.hip: the window
// dispatcher (csrc/fa_paged_window_gfx950.hip) links into its sanitizer test driver without device code, and a
// launch that gets past validation reports FA_ERR_UNSUPPORTED.
#include "fa_paged_window_launch.h"

namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_window(const fa_fwd_params &, PagedWinDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window(const fa_fwd_params &, PagedFp8WinDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
#define FA_STUB_WINDOW_INSTANCE(DT, C, D, E)                                                                       \
    template int launch_decode_paged_window<DT, C, D, E>(const fa_fwd_params &, PagedWinDecArgs, void *, hipStream_t); \
    template int launch_decode_paged_fp8_window<DT, C, D, E>(const fa_fwd_params &, PagedFp8WinDecArgs, void *,    \
                                                             hipStream_t);
FA_FOR_EACH_INSTANCE(FA_STUB_WINDOW_INSTANCE)
}  // namespace fa
