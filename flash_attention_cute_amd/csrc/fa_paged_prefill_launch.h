// fa_paged_prefill_launch.h -- internal seam between the paged-prefill C-ABI dispatcher
// (fa_paged_prefill_gfx950.hip, include/fa_gfx950_paged_prefill.h) and the paged fa_fwd_w4 instantiations
// (fa_paged_prefill_inst.hip x 16), beside fa_paged_launch.h: the other dispatchers and their instantiations
// never see these declarations.
#pragma once

#include "fa_launch.h"

namespace fa {

// The page indirection of fa_fwd_w4_paged (fa_paged_prefill.hpp). In the fa_fwd_params that go with it q / o
// are dense, k_ptr / v_ptr are the pool bases, k / v_batch_stride the PAGE stride and seqlen_kv = max_pages *
// page_size (the capacity a length is clamped to). A sequence's keys are [0, seqlens_k[b]); its queries are
// its last seqlen_q positions.
struct PagedPrefillArgs {
    const int32_t *block_table;  // [B, max_pages] page ids, device
    int64_t block_table_stride;  // elements between rows
    const int32_t *seqlens_k;    // [B], device; clamped to [0, max_pages * page_size] by the kernel
    int num_pages;               // pages of the pool: ids are clamped into [0, num_pages)
    int tiles_per_page;          // page_size / kBlockN
};

// window_left: -1 none, else 0 .. 2^30 (clamped by the host)
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged(const fa_fwd_params &p, const PagedPrefillArgs &a, int window_left, hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_PREFILL(DT, C, D, E)                                                           \
    extern template int launch_prefill_paged<DT, C, D, E>(const fa_fwd_params &, const PagedPrefillArgs &, int, \
                                                          hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_PREFILL)
#undef FA_DECLARE_EXTERN_PAGED_PREFILL

}  // namespace fa
