// Host-only stand-ins for the 64 paged decode instantiations (csrc/fa_paged_inst.hip, csrc/fa_paged_fp8_inst.hip,
// csrc/fa_paged_window_inst.hip, csrc/fa_paged_fp8_window_inst.hip), beside stub_instances.hip: the paged
// dispatcher (csrc/fa_paged_gfx950.hip: the 16-bit, FP8 and sliding-window entries) links into its sanitizer
// test drivers without device code, and a launch that gets past validation reports FA_ERR_UNSUPPORTED.
#include "fa_paged_launch.h"

namespace fa {
#define FA_STUB_PAGED_LAUNCH(NAME, ARGS)                                          \
    template <class DT, bool C, int kD, bool kExact>                              \
    int NAME(const fa_fwd_params &, ARGS, void *, hipStream_t) {                  \
        return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)"); \
    }
FA_STUB_PAGED_LAUNCH(launch_decode_paged, PagedDecArgs)
FA_STUB_PAGED_LAUNCH(launch_decode_paged_fp8, PagedFp8DecArgs)
FA_STUB_PAGED_LAUNCH(launch_decode_paged_window, PagedWinDecArgs)
FA_STUB_PAGED_LAUNCH(launch_decode_paged_fp8_window, PagedFp8WinDecArgs)
#undef FA_STUB_PAGED_LAUNCH

#define FA_STUB_PAGED_INSTANCE(DT, C, D, E)                                                                          \
    template int launch_decode_paged<DT, C, D, E>(const fa_fwd_params &, PagedDecArgs, void *, hipStream_t);         \
    template int launch_decode_paged_fp8<DT, C, D, E>(const fa_fwd_params &, PagedFp8DecArgs, void *, hipStream_t);  \
    template int launch_decode_paged_window<DT, C, D, E>(const fa_fwd_params &, PagedWinDecArgs, void *, hipStream_t); \
    template int launch_decode_paged_fp8_window<DT, C, D, E>(const fa_fwd_params &, PagedFp8WinDecArgs, void *,      \
                                                             hipStream_t);
FA_FOR_EACH_INSTANCE(FA_STUB_PAGED_INSTANCE)
}  // namespace fa
