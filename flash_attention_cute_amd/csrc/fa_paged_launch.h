// fa_paged_launch.h -- internal seam between the paged C-ABI dispatcher (fa_paged_gfx950.hip) and the
// paged decode instantiations (fa_paged_inst.hip x 16), beside fa_launch.h: the dense dispatcher and
// its instantiations never see these declarations.
#pragma once

#include "fa_launch.h"

namespace fa {

// DecArgs plus the page indirection (fa_decode_paged.hpp). In the fa_fwd_params that go with it k_ptr /
// v_ptr are the pool bases, k / v_batch_stride the PAGE stride and seqlen_kv = max_pages * page_size
// (the plan's length); k_lo / k_hi stay nullptr -- a sequence's keys are [0, seqlens_k[b]).
struct PagedDecArgs : DecArgs {
    const int32_t *block_table;  // [B, max_pages] page ids, device
    int64_t block_table_stride;  // elements between rows
    const int32_t *seqlens_k;    // [B], device; clamped to [0, max_pages * page_size] by the kernel
    int num_pages;               // pages of the pool: ids are clamped into [0, num_pages)
    int tiles_per_page;          // page_size / kDecKeys
};

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged(const fa_fwd_params &p, PagedDecArgs a, void *ws, hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED(DT, C, D, E) \
    extern template int launch_decode_paged<DT, C, D, E>(const fa_fwd_params &, PagedDecArgs, void *, hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED)
#undef FA_DECLARE_EXTERN_PAGED

}  // namespace fa
