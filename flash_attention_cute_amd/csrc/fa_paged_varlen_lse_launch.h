// fa_paged_varlen_lse_launch.h -- internal seam between the C-ABI dispatcher of the ragged paged prefill that also
// writes the LSE (fa_paged_varlen_lse_gfx950.hip, include/fa_gfx950_paged_varlen_lse.h) and its fa_fwd_w4
// instantiations (fa_paged_varlen_lse_inst.hip x 16), beside fa_paged_varlen_sink_launch.h, which it does not change:
// the other ragged dispatchers and instantiations never see these declarations.
#pragma once

#include "fa_paged_varlen_sink_launch.h"

namespace fa {

// fa_fwd_w4_paged with ragged queries, sinks and the LSE (fa_paged_varlen_lse.hpp): PagedVarlenSinkArgs whose sinks
// may be NULL (no head has a sink), and where a row's natural-log LSE goes: element (q-head h, packed row i) at
// lse[h * lse_head_stride + i * lse_row_stride], written for the rows some sequence owns and for no other.
struct PagedVarlenLseArgs {
    PagedVarlenSinkArgs sink;
    float *lse;                                // device, fp32
    int64_t lse_head_stride, lse_row_stride;   // elements; the row stride at most kMaxLseRowStride
};

// (a wave addresses the LSE of its 160-row span through one buffer descriptor with 32-bit byte offsets)
constexpr int64_t kMaxLseRowStride = int64_t(1) << 20;

// window_left: -1 none, else 0 .. 2^30 (clamped by the host)
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen_lse(const fa_fwd_params &p, const PagedVarlenLseArgs &a, int window_left,
                                    hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_VARLEN_LSE(DT, C, D, E)                                                              \
    extern template int launch_prefill_paged_varlen_lse<DT, C, D, E>(const fa_fwd_params &,                          \
                                                                     const PagedVarlenLseArgs &, int, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_VARLEN_LSE)
#undef FA_DECLARE_EXTERN_PAGED_VARLEN_LSE

}  // namespace fa
