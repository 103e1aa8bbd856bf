// fa_paged_varlen_gfx950.hip -- C-ABI of the ragged paged prefill (include/fa_gfx950_paged_varlen.h).
//
// Host code only, beside fa_paged_prefill_gfx950.hip, which it does not change: validation is
// fa_fwd_gfx950_paged_prefill_check's through its public entry on the packed layout (zero q / o batch strides,
// seqlen_q = max_seqlen_q), plus the rules of the cumulative array; the launch is the ragged paged fa_fwd_w4
// instantiation's (fa_paged_varlen_inst.hip: the paged kernel compiled with per-sequence query ranges, in
// translation units of its own). The kernel reads cu_seqlens_q itself, so the workspace is empty.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_paged_prefill.h"
#include "fa_gfx950_paged_varlen.h"
#include "fa_paged_varlen_launch.h"

namespace {
using fa::set_err;

// the paged params of the packed layout: a sequence's rows start at cu_seqlens_q[b], not at a batch stride
fa_paged_params packed(const fa_paged_varlen_params &v) {
    fa_paged_params pp = v.paged;
    pp.base.q_batch_stride = pp.base.o_batch_stride = 0;
    return pp;
}

int check_varlen(const fa_paged_varlen_params *v, int dtype, int causal) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (!v->cu_seqlens_q) return set_err(FA_ERR_INVALID_ARGUMENT, "cu_seqlens_q must be non-NULL");
    if ((uintptr_t)v->cu_seqlens_q & 3)
        return set_err(FA_ERR_INVALID_ARGUMENT, "cu_seqlens_q must be a 4-byte aligned int32 array");
    if (v->total_q < 0) return set_err(FA_ERR_INVALID_ARGUMENT, "total_q (%lld) must be non-negative",
                                       (long long)v->total_q);
    if (v->total_q > 0x7fffffffLL || v->paged.base.batch_size >= 0x7fffffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "total_q and batch_size + 1 must fit 32 bits");
    const fa_paged_params pp = packed(*v);
    return fa_fwd_gfx950_paged_prefill_check(&pp, dtype, causal);
}

constexpr int64_t kWorkspaceBytes = 0;  // (the kernel reads cu_seqlens_q itself)
}  // namespace

extern "C" int fa_fwd_gfx950_paged_varlen(const fa_paged_varlen_params *params, int dtype, int causal,
                                          int64_t window_left, void *workspace, int64_t workspace_bytes,
                                          void *stream) {
    fa::set_last_path(fa::kPathNone);
    fa::set_last_prefill_paged(false);
    const int rc = check_varlen(params, dtype, causal);
    if (rc != FA_OK) return rc;
    (void)workspace;
    if (workspace_bytes < kWorkspaceBytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)workspace_bytes, (long long)kWorkspaceBytes);
    if (params->total_q == 0) return FA_OK;  // (no row to write)
    const fa_paged_params pp = packed(*params);
    fa::PagedVarlenArgs a{};
    a.paged.block_table = pp.block_table;
    a.paged.block_table_stride = pp.block_table_stride;
    a.paged.seqlens_k = pp.seqlens_k;
    a.paged.num_pages = (int)pp.num_pages;
    a.paged.tiles_per_page = (int)(pp.page_size / fa::kBlockN);
    a.cu_seqlens_q = params->cu_seqlens_q;
    a.total_q = (int)params->total_q;
    const int64_t max_window = int64_t(1) << 30;  // (hides nothing at any capacity; keeps the bound in 32 bits)
    const int wl = window_left < 0 ? -1 : (int)(window_left < max_window ? window_left : max_window);
    const fa_fwd_params &p = pp.base;
    return fa::with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
        return fa::with_headdim(p.headdim, [&](auto d, auto exact) {
            return fa::launch_prefill_paged_varlen<typename decltype(dt)::type, decltype(c)::value, decltype(d)::value,
                                            decltype(exact)::value>(p, a, wl, (hipStream_t)stream);
        });
    });
}

extern "C" int64_t fa_fwd_gfx950_paged_varlen_workspace_size(const fa_paged_varlen_params *params, int dtype,
                                                             int causal, int64_t window_left) {
    (void)window_left;
    return check_varlen(params, dtype, causal) == FA_OK ? kWorkspaceBytes : -1;
}

extern "C" int fa_fwd_gfx950_paged_varlen_check(const fa_paged_varlen_params *params, int dtype, int causal) {
    return check_varlen(params, dtype, causal);
}

extern "C" int fa_paged_varlen_version(void) { return FA_GFX950_PAGED_VARLEN_VERSION; }
