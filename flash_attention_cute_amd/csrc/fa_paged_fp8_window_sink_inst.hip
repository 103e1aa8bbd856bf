// fa_paged_fp8_window_sink_inst.hip -- one sink instantiation of the sliding-window FP8 paged decode per translation unit, as fa_paged_lse_inst.hip:
// _build.py compiles this file once per combination of FA_INST_DT (F16 | BF16), FA_INST_CAUSAL (0 | 1),
// FA_INST_D (64 | 128) and FA_INST_EXACT (0 | 1). Each holds the kernel with and without the fused merge and
// fa_decode_combine_sink; the instantiations without sinks are untouched by it.
#ifndef FA_INST_STUB
#include "fa_decode_paged_sink.hpp"
#else
#include "fa_paged_sink_launch.h"
namespace fa {
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_window_sink(const fa_fwd_params &, PagedFp8WinSinkDecArgs, void *, hipStream_t) {
    return set_err(FA_ERR_UNSUPPORTED, "stub instantiation");
}
}  // namespace fa
#endif

#if !defined(FA_INST_DT) || !defined(FA_INST_CAUSAL) || !defined(FA_INST_D) || !defined(FA_INST_EXACT)
#error "fa_paged_fp8_window_sink_inst.hip needs -DFA_INST_DT= -DFA_INST_CAUSAL= -DFA_INST_D= -DFA_INST_EXACT="
#endif

namespace fa {
template int launch_decode_paged_fp8_window_sink<FA_INST_DT, (FA_INST_CAUSAL != 0), FA_INST_D, (FA_INST_EXACT != 0)>(
    const fa_fwd_params &, PagedFp8WinSinkDecArgs, void *, hipStream_t);
}  // namespace fa
