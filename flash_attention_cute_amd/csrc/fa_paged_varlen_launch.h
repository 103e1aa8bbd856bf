// fa_paged_varlen_launch.h -- internal seam between the ragged paged-prefill C-ABI dispatcher
// (fa_paged_varlen_gfx950.hip, include/fa_gfx950_paged_varlen.h) and the ragged paged fa_fwd_w4 instantiations
// (fa_paged_varlen_inst.hip x 16), beside fa_paged_prefill_launch.h, which it does not change: the uniform paged
// prefill's dispatcher and instantiations never see these declarations.
#pragma once

#include "fa_paged_prefill_launch.h"

namespace fa {

// fa_fwd_w4_paged with ragged queries (fa_paged_varlen.hpp): the page indirection of PagedPrefillArgs, and q / o
// packed [total_q, Hq, D] (zero batch strides). Sequence b's queries are rows [cu_seqlens_q[b], cu_seqlens_q[b +
// 1]) -- its last positions -- both bounds clamped into [0, total_q] by the kernel; p.seqlen_q only sizes the grid
// (an upper bound of every sequence's rows).
struct PagedVarlenArgs {
    PagedPrefillArgs paged;
    const int32_t *cu_seqlens_q;  // [B + 1], device: the launch's xa.q_rng
    int total_q;                  // rows of q / o
};

// window_left: -1 none, else 0 .. 2^30 (clamped by the host)
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen(const fa_fwd_params &p, const PagedVarlenArgs &a, int window_left, hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_VARLEN(DT, C, D, E)                                                                  \
    extern template int launch_prefill_paged_varlen<DT, C, D, E>(const fa_fwd_params &, const PagedVarlenArgs &, int, \
                                                                 hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_VARLEN)
#undef FA_DECLARE_EXTERN_PAGED_VARLEN

}  // namespace fa
