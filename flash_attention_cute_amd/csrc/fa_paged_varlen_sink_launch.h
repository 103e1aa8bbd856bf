// fa_paged_varlen_sink_launch.h -- internal seam between the C-ABI dispatcher of the ragged paged prefill with
// attention sinks (fa_paged_varlen_sink_gfx950.hip, include/fa_gfx950_paged_varlen_sink.h) and its fa_fwd_w4
// instantiations (fa_paged_varlen_sink_inst.hip x 16), beside fa_paged_varlen_launch.h, which it does not change:
// the unsinked ragged dispatcher and instantiations never see these declarations.
#pragma once

#include "fa_paged_varlen_launch.h"

namespace fa {

// fa_fwd_w4_paged with ragged queries and sinks (fa_paged_varlen_sink.hpp): PagedVarlenArgs, and one fp32 logit per
// q-head in final-logit units that joins every row's softmax sum with value 0 (-inf, or at or below -1e30: none).
struct PagedVarlenSinkArgs {
    PagedVarlenArgs varlen;
    const float *sinks;  // [num_heads_q], device
};

// window_left: -1 none, else 0 .. 2^30 (clamped by the host)
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen_sink(const fa_fwd_params &p, const PagedVarlenSinkArgs &a, int window_left,
                                     hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_VARLEN_SINK(DT, C, D, E)                                                            \
    extern template int launch_prefill_paged_varlen_sink<DT, C, D, E>(const fa_fwd_params &,                         \
                                                                      const PagedVarlenSinkArgs &, int, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_VARLEN_SINK)
#undef FA_DECLARE_EXTERN_PAGED_VARLEN_SINK

}  // namespace fa
