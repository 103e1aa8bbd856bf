// fa_paged_fp8_launch.h -- internal seam between the FP8 paged C-ABI dispatcher (fa_paged_fp8_gfx950.hip)
// and the FP8 paged decode instantiations (fa_paged_fp8_inst.hip x 16), beside fa_paged_launch.h: the
// 16-bit dispatchers and their instantiations never see these declarations.
#pragma once

#include "fa_paged_launch.h"

namespace fa {

// fa_debug_last_path values of the FP8 paged decode (after fa_launch.h's Path)
constexpr int kPathDecodePagedFp8 = 11, kPathDecodePagedFp8Split = 12;

// PagedDecArgs plus the descales (fa_decode_paged_fp8.hpp). In the fa_fwd_params that go with it the k / v
// pointers and strides describe 1-byte e4m3 elements; q / o are the 16-bit DT.
struct PagedFp8DecArgs : PagedDecArgs {
    const float *k_descale, *v_descale;  // [B, Hkv] fp32, device; nullptr: 1.0
    int64_t descale_batch_stride, descale_head_stride;
};

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8(const fa_fwd_params &p, PagedFp8DecArgs a, void *ws, hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_FP8(DT, C, D, E)                                                        \
    extern template int launch_decode_paged_fp8<DT, C, D, E>(const fa_fwd_params &, PagedFp8DecArgs, void *, \
                                                             hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_FP8)
#undef FA_DECLARE_EXTERN_PAGED_FP8

}  // namespace fa
