// Host-only stand-ins for the 2 x 16 LSE paged decode instantiations (csrc/fa_paged_lse_inst.hip,
// csrc/fa_paged_fp8_lse_inst.hip), beside paged_stub_instances.hip: the LSE dispatcher
// (csrc/fa_paged_lse_gfx950.hip) links into its sanitizer test driver without device code, and a launch that
// gets past validation reports FA_ERR_UNSUPPORTED.
#include "fa_paged_lse_launch.h"

namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_lse(const fa_fwd_params &, PagedLseDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_lse(const fa_fwd_params &, PagedFp8LseDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
#define FA_STUB_LSE_INSTANCE(DT, C, D, E)                                                                         \
    template int launch_decode_paged_lse<DT, C, D, E>(const fa_fwd_params &, PagedLseDecArgs, void *, hipStream_t); \
    template int launch_decode_paged_fp8_lse<DT, C, D, E>(const fa_fwd_params &, PagedFp8LseDecArgs, void *,      \
                                                          hipStream_t);
FA_FOR_EACH_INSTANCE(FA_STUB_LSE_INSTANCE)
}  // namespace fa
