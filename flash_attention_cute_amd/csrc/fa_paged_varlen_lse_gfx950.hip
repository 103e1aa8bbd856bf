// fa_paged_varlen_lse_gfx950.hip -- C-ABI of the ragged paged prefill that also writes the LSE, with or without
// attention sinks (include/fa_gfx950_paged_varlen_lse.h).
//
// Host code only, beside fa_paged_varlen_gfx950.hip and fa_paged_varlen_sink_gfx950.hip, which it does not change
// and which never reference it: the base validation is fa_fwd_gfx950_paged_varlen_check's through its public entry,
// so the entries cannot drift apart, plus the rules that are new here (the LSE array and its strides, an optional
// sinks array); the launch is the fa_fwd_w4 instantiation's of fa_paged_varlen_lse_inst.hip, with the arguments and
// the window clamp of the entries without the LSE. No workspace, as there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_paged_varlen_lse.h"
#include "fa_paged_varlen_lse_launch.h"

namespace {
using fa::set_err;

int check_lse(const fa_paged_varlen_lse_params *v, int dtype, int causal) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    const int rc = fa_fwd_gfx950_paged_varlen_check(&v->varlen, dtype, causal);
    if (rc != FA_OK) return rc;
    if (v->sinks && ((uintptr_t)v->sinks & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "sinks must be NULL or a 4-byte aligned fp32 array");
    if (!v->lse_ptr) return set_err(FA_ERR_INVALID_ARGUMENT, "lse_ptr is NULL");
    if ((uintptr_t)v->lse_ptr & 3) return set_err(FA_ERR_INVALID_ARGUMENT, "lse_ptr must be a 4-byte aligned fp32 array");
    if (v->lse_head_stride < 0 || v->lse_row_stride < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "lse strides must be non-negative (got head %lld, row %lld)",
                       (long long)v->lse_head_stride, (long long)v->lse_row_stride);
    if (v->lse_row_stride > fa::kMaxLseRowStride)
        return set_err(FA_ERR_INVALID_ARGUMENT, "lse_row_stride %lld is larger than the %lld elements served",
                       (long long)v->lse_row_stride, (long long)fa::kMaxLseRowStride);
    return FA_OK;
}

constexpr int64_t kWorkspaceBytes = 0;  // (the kernel reads cu_seqlens_q and sinks itself)
}  // namespace

extern "C" int fa_fwd_gfx950_paged_varlen_lse(const fa_paged_varlen_lse_params *params, int dtype, int causal,
                                              int64_t window_left, void *workspace, int64_t workspace_bytes,
                                              void *stream) {
    fa::set_last_path(fa::kPathNone);
    fa::set_last_prefill_paged(false);
    const int rc = check_lse(params, dtype, causal);
    if (rc != FA_OK) return rc;
    (void)workspace;
    if (workspace_bytes < kWorkspaceBytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)workspace_bytes, (long long)kWorkspaceBytes);
    const fa_paged_varlen_params &v = params->varlen;
    if (v.total_q == 0) return FA_OK;  // (no row to write)
    fa_fwd_params p = v.paged.base;    // the packed layout: a sequence's rows start at cu_seqlens_q[b]
    p.q_batch_stride = p.o_batch_stride = 0;
    fa::PagedVarlenLseArgs a{};
    fa::PagedVarlenArgs &av = a.sink.varlen;
    av.paged.block_table = v.paged.block_table;
    av.paged.block_table_stride = v.paged.block_table_stride;
    av.paged.seqlens_k = v.paged.seqlens_k;
    av.paged.num_pages = (int)v.paged.num_pages;
    av.paged.tiles_per_page = (int)(v.paged.page_size / fa::kBlockN);
    av.cu_seqlens_q = v.cu_seqlens_q;
    av.total_q = (int)v.total_q;
    a.sink.sinks = params->sinks;
    a.lse = params->lse_ptr;
    a.lse_head_stride = params->lse_head_stride;
    a.lse_row_stride = params->lse_row_stride;
    const int64_t max_window = int64_t(1) << 30;  // (hides nothing at any capacity; keeps the bound in 32 bits)
    const int wl = window_left < 0 ? -1 : (int)(window_left < max_window ? window_left : max_window);
    return fa::with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
        return fa::with_headdim(p.headdim, [&](auto d, auto exact) {
            return fa::launch_prefill_paged_varlen_lse<typename decltype(dt)::type, decltype(c)::value,
                                                       decltype(d)::value, decltype(exact)::value>(
                p, a, wl, (hipStream_t)stream);
        });
    });
}

extern "C" int64_t fa_fwd_gfx950_paged_varlen_lse_workspace_size(const fa_paged_varlen_lse_params *params, int dtype,
                                                                 int causal, int64_t window_left) {
    (void)window_left;
    return check_lse(params, dtype, causal) == FA_OK ? kWorkspaceBytes : -1;
}

extern "C" int fa_fwd_gfx950_paged_varlen_lse_check(const fa_paged_varlen_lse_params *params, int dtype, int causal) {
    return check_lse(params, dtype, causal);
}

extern "C" int fa_paged_varlen_lse_version(void) { return FA_GFX950_PAGED_VARLEN_LSE_VERSION; }
