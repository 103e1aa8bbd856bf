// Host-only stand-ins for the 16 ragged paged fa_fwd_w4 instantiations (csrc/fa_paged_varlen_inst.hip), beside
// paged_prefill_stub_instances.hip: the ragged dispatcher (csrc/fa_paged_varlen_gfx950.hip) links into its
// sanitizer test driver without device code, and a launch that gets past validation reports FA_ERR_UNSUPPORTED.
#include "fa_paged_varlen_launch.h"

namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen(const fa_fwd_params &, const PagedVarlenArgs &, int, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
#define FA_STUB_VARLEN_INSTANCE(DT, C, D, E)                                                                       \
    template int launch_prefill_paged_varlen<DT, C, D, E>(const fa_fwd_params &, const PagedVarlenArgs &, int, \
                                                          hipStream_t);
FA_FOR_EACH_INSTANCE(FA_STUB_VARLEN_INSTANCE)
}  // namespace fa
