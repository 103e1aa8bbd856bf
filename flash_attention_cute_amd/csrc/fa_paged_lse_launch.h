// fa_paged_lse_launch.h -- internal seam between the LSE dispatcher (fa_paged_lse_gfx950.hip) and the LSE
// instantiations of the paged decode (fa_paged_lse_inst.hip, fa_paged_fp8_lse_inst.hip, x 16 each), beside
// fa_paged_launch.h: the other dispatchers and instantiations never see these declarations.
#pragma once

#include "fa_paged_launch.h"

namespace fa {

// Where a launch writes its rows' log-sum-exp: element (b, hq, pos) of an fp32 array, by element strides
struct LseOut {
    float *ptr;
    int64_t batch_stride, head_stride, seqlen_stride;
};

// PagedDecArgs / PagedFp8DecArgs plus the LSE output and the length options (include/fa_gfx950_lse.h). The
// member `lse` is what selects the LSE code of decode_body (fa_decode.hpp DecLse); seqlens_k may be nullptr
// here and sequence b has clamp(seqlens_k[b] + seqlen_offset) keys (PagedSeq::key_range).
//
// A compile-time variant in translation units of its own, as the window is (PagedWinDecArgs above has the
// measurement that rejected a run-time switch in the existing kernels).
struct PagedLseDecArgs : PagedDecArgs {
    LseOut lse;
    int seqlen_offset;
};
struct PagedFp8LseDecArgs : PagedFp8DecArgs {
    LseOut lse;
    int seqlen_offset;
};
constexpr int64_t kLseMaxOffset = int64_t(1) << 30;

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_lse(const fa_fwd_params &p, PagedLseDecArgs a, void *ws, hipStream_t stream);
template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_lse(const fa_fwd_params &p, PagedFp8LseDecArgs a, void *ws, hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_LSE(DT, C, D, E)                                                              \
    extern template int launch_decode_paged_lse<DT, C, D, E>(const fa_fwd_params &, PagedLseDecArgs, void *,  \
                                                             hipStream_t);                                    \
    extern template int launch_decode_paged_fp8_lse<DT, C, D, E>(const fa_fwd_params &, PagedFp8LseDecArgs,   \
                                                                 void *, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_LSE)
#undef FA_DECLARE_EXTERN_PAGED_LSE

}  // namespace fa
