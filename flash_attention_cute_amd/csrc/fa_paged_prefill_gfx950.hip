// fa_paged_prefill_gfx950.hip -- C-ABI of the paged prefill (include/fa_gfx950_paged_prefill.h).
//
// Host code only, beside fa_paged_gfx950.hip (the paged decode entries), which it does not change:
// validation is fa_fwd_gfx950_paged_check's and fa_fwd_gfx950_check's through their public entries, so this
// entry and the decode entries cannot drift apart, plus the one rule that is new here (a page holds whole
// 64-key tiles); the dtype / causal / head-dim dispatch goes to the paged fa_fwd_w4 instantiations
// (fa_paged_prefill_inst.hip). The launch needs no per-sequence arrays -- the kernel clamps seqlens_k itself
// -- so the workspace is empty.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_paged_prefill.h"
#include "fa_paged_prefill_launch.h"

namespace {
using fa::set_err;

int check_prefill(const fa_paged_params *v, int dtype, int causal) {
    if (!v) return fa_fwd_gfx950_paged_check(v, dtype, causal);  // (its message)
    // the pool, the table and the k / v strides: the paged decode's check on a copy that always meets its
    // decode-shape rule (one position, one q-head per kv-head), which is not a rule of this entry
    fa_paged_params one = *v;
    one.base.seqlen_q = 1;
    one.base.num_heads_q = v->base.num_heads_kv;
    one.base.head_q_per_group = 1;
    int rc = fa_fwd_gfx950_paged_check(&one, dtype, causal);
    if (rc != FA_OK) return rc;
    // q / o and the head counts as given
    rc = fa_fwd_gfx950_check(&v->base, dtype, causal);
    if (rc != FA_OK) return rc;
    if (v->page_size % fa::kBlockN != 0)
        return set_err(FA_ERR_UNSUPPORTED,
                       "paged prefill needs page_size (%lld) to be a multiple of %d, the prefill kernel's key tile: "
                       "gather the pages and use fa_fwd_gfx950_padded",
                       (long long)v->page_size, fa::kBlockN);
    // a tile's rows are addressed from its page's base: the offset of a page's last row stays inside 32 bits
    const int64_t row = v->base.k_seqlen_stride > v->base.v_seqlen_stride ? v->base.k_seqlen_stride
                                                                          : v->base.v_seqlen_stride;
    if (v->page_size * row * 2 > 0x7fffffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "a page's rows span more than 2^31 bytes");
    return FA_OK;
}

constexpr int64_t kWorkspaceBytes = 0;  // (no per-sequence arrays: the kernel reads seqlens_k itself)
}  // namespace

extern "C" int fa_fwd_gfx950_paged_prefill(const fa_paged_params *params, int dtype, int causal,
                                           int64_t window_left, void *workspace, int64_t workspace_bytes,
                                           void *stream) {
    fa::set_last_path(fa::kPathNone);
    fa::set_last_prefill_paged(false);
    const int rc = check_prefill(params, dtype, causal);
    if (rc != FA_OK) return rc;
    (void)workspace;
    if (workspace_bytes < kWorkspaceBytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)workspace_bytes, (long long)kWorkspaceBytes);
    fa::PagedPrefillArgs a{};
    a.block_table = params->block_table;
    a.block_table_stride = params->block_table_stride;
    a.seqlens_k = params->seqlens_k;
    a.num_pages = (int)params->num_pages;
    a.tiles_per_page = (int)(params->page_size / fa::kBlockN);
    const int64_t max_window = int64_t(1) << 30;  // (hides nothing at any capacity; keeps the bound in 32 bits)
    const int wl = window_left < 0 ? -1 : (int)(window_left < max_window ? window_left : max_window);
    const fa_fwd_params &p = params->base;
    return fa::with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
        return fa::with_headdim(p.headdim, [&](auto d, auto exact) {
            return fa::launch_prefill_paged<typename decltype(dt)::type, decltype(c)::value, decltype(d)::value,
                                            decltype(exact)::value>(p, a, wl, (hipStream_t)stream);
        });
    });
}

extern "C" int64_t fa_fwd_gfx950_paged_prefill_workspace_size(const fa_paged_params *params, int dtype, int causal,
                                                              int64_t window_left) {
    (void)window_left;
    return check_prefill(params, dtype, causal) == FA_OK ? kWorkspaceBytes : -1;
}

extern "C" int fa_fwd_gfx950_paged_prefill_check(const fa_paged_params *params, int dtype, int causal) {
    return check_prefill(params, dtype, causal);
}

extern "C" int fa_paged_prefill_version(void) { return FA_GFX950_PAGED_PREFILL_VERSION; }
