// fa_paged_varlen_lse_inst.hip -- one ragged paged fa_fwd_w4 instantiation that also writes the LSE per translation
// unit, as fa_paged_varlen_sink_inst.hip: _build.py compiles this file once per combination of FA_INST_DT (F16 |
// BF16), FA_INST_CAUSAL (0 | 1), FA_INST_D (64 | 128) and FA_INST_EXACT (0 | 1), in directories of its own. The
// dense, the uniform paged, the unsinked and the sinked ragged instantiations are untouched by it.
#ifndef FA_INST_STUB
#include "fa_paged_varlen_lse.hpp"
#else
#include "fa_paged_varlen_lse_launch.h"
namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen_lse(const fa_fwd_params &, const PagedVarlenLseArgs &, int, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation");
}
}  // namespace fa
#endif

#if !defined(FA_INST_DT) || !defined(FA_INST_CAUSAL) || !defined(FA_INST_D) || !defined(FA_INST_EXACT)
#error "fa_paged_varlen_lse_inst.hip needs -DFA_INST_DT= -DFA_INST_CAUSAL= -DFA_INST_D= -DFA_INST_EXACT="
#endif

namespace fa {
template int launch_prefill_paged_varlen_lse<FA_INST_DT, (FA_INST_CAUSAL != 0), FA_INST_D, (FA_INST_EXACT != 0)>(
    const fa_fwd_params &, const PagedVarlenLseArgs &, int, hipStream_t);
}  // namespace fa
