#pragma once
// fa_decode_paged_lse.hpp -- fa_decode_paged and fa_decode_fp8kv that also write every row's softmax
// log-sum-exp (include/fa_gfx950_lse.h), gfx950: decode_body (fa_decode.hpp) with the paged policies over
// PagedLseDecArgs / PagedFp8LseDecArgs, in kernels and translation units of their own. The member `lse` of the
// argument struct turns on, at compile time (DecLse), the three places where a final row is produced: the
// unsplit epilogue beside decode_store_o (thread part == 0 holds the row's M and L), the fused merge
// (decode_merge, thread tid < nrow) and fa_decode_combine_lse (lane 0). Each stores (M + log2 L) ln 2, or -inf
// for a row without a visible key. O is computed by exactly the instructions of the kernels without the LSE.
// The two length options (seqlen_offset, seqlens_k == nullptr) are in PagedSeq::key_range, under the same switch.
#include "fa_decode_paged_fp8.hpp"
#include "fa_paged_lse_launch.h"

namespace fa {

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_paged_lse(const fa_fwd_params p, const PagedLseDecArgs a) {
    decode_body<PagedKv16<kD, PagedLseDecArgs>, false, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool kCausal, int kD, bool kExactD, bool kFuse = false>
__global__ __launch_bounds__(256, 1) void fa_decode_fp8kv_lse(const fa_fwd_params p, const PagedFp8LseDecArgs a) {
    decode_body<PagedKv8<kD, PagedFp8LseDecArgs>, false, DT, kCausal, kD, kExactD, kFuse>(p, a);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_lse(const fa_fwd_params &p, PagedLseDecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_paged_lse<DT, C, kD, kExact, true>,
                                                 &fa_decode_paged_lse<DT, C, kD, kExact, false>, kPathDecodePaged,
                                                 kPathDecodePagedSplit);
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8_lse(const fa_fwd_params &p, PagedFp8LseDecArgs a, void *ws, hipStream_t stream) {
    return launch_decode_kernels<DT, kD, kExact>(p, a, ws, stream, &fa_decode_fp8kv_lse<DT, C, kD, kExact, true>,
                                                 &fa_decode_fp8kv_lse<DT, C, kD, kExact, false>, kPathDecodePagedFp8,
                                                 kPathDecodePagedFp8Split);
}

}  // namespace fa
