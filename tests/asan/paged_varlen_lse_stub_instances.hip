// Host-only stand-ins for the 16 ragged paged fa_fwd_w4 instantiations that write the LSE (csrc/fa_paged_varlen_lse_inst.hip),
// beside paged_varlen_stub_instances.hip: the dispatcher (csrc/fa_paged_varlen_lse_gfx950.hip) links into its
// sanitizer test driver without device code, and a launch that gets past validation reports FA_ERR_UNSUPPORTED.
#include "fa_paged_varlen_lse_launch.h"

namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen_lse(const fa_fwd_params &, const PagedVarlenLseArgs &, int, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
#define FA_STUB_VARLEN_LSE_INSTANCE(DT, C, D, E)                                                                \
    template int launch_prefill_paged_varlen_lse<DT, C, D, E>(const fa_fwd_params &, const PagedVarlenLseArgs &,  \
                                                               int, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_STUB_VARLEN_LSE_INSTANCE)
}  // namespace fa
