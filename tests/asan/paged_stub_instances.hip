// Host-only stand-ins for the 16 paged decode instantiations (csrc/fa_paged_inst.hip), beside
// stub_instances.hip: the paged dispatcher (csrc/fa_paged_gfx950.hip) links into its sanitizer test
// driver without device code, and a launch that gets past validation reports FA_ERR_UNSUPPORTED.
#include "fa_paged_launch.h"

namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged(const fa_fwd_params &, PagedDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
#define FA_STUB_PAGED_INSTANCE(DT, C, D, E) \
    template int launch_decode_paged<DT, C, D, E>(const fa_fwd_params &, PagedDecArgs, void *, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_STUB_PAGED_INSTANCE)
}  // namespace fa
