// Host-only stand-ins for the 16 FP8 paged decode instantiations (csrc/fa_paged_fp8_inst.hip), beside
// paged_stub_instances.hip: the FP8 dispatcher (csrc/fa_paged_fp8_gfx950.hip) links into its sanitizer
// test driver without device code, and a launch that gets past validation reports FA_ERR_UNSUPPORTED.
#include "fa_paged_fp8_launch.h"

namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8(const fa_fwd_params &, PagedFp8DecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation (sanitizer build)");
}
#define FA_STUB_FP8_INSTANCE(DT, C, D, E) \
    template int launch_decode_paged_fp8<DT, C, D, E>(const fa_fwd_params &, PagedFp8DecArgs, void *, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_STUB_FP8_INSTANCE)
}  // namespace fa
