// fa_paged_window_gfx950.hip -- C-ABI of the sliding-window paged decode, 16-bit and FP8
// (include/fa_gfx950_paged_window.h).
//
// Host code only, beside fa_paged_gfx950.hip and fa_paged_fp8_gfx950.hip, which it does not change: validation
// is theirs, through their public _check entries, so the windowed and unwindowed entries cannot drift apart;
// window_left < 0 IS the unwindowed entry (called, not copied: the same plan and the same bits); otherwise the
// split plan is made for the keys a window can intersect (fa::window_plan_keys) and the dtype / causal /
// head-dim dispatch goes to the windowed instantiations (fa_paged_window_inst.hip, fa_paged_fp8_window_inst.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_paged_window.h"
#include "fa_paged_window_launch.h"

namespace {
using fa::set_err;

// the plan of the unwindowed launch (`plan`: decode_plan, or the FP8 dispatcher's) on a copy of the parameters
// whose seqlen_kv is the window's reach; the kernel still clamps lengths to the real capacity
template <class Plan>
fa::DecArgs window_plan(const fa_fwd_params &p, int64_t window_left, bool split, Plan plan) {
    fa_fwd_params planned = p;
    planned.seqlen_kv = fa::window_plan_keys(p, window_left);
    return plan(planned, split ? fa::kDecMaxSplit : 1);
}

void fill_paged(fa::PagedDecArgs &a, const fa_paged_params &g) {
    a.block_table = g.block_table;
    a.block_table_stride = g.block_table_stride;
    a.seqlens_k = g.seqlens_k;
    a.num_pages = (int)g.num_pages;
    a.tiles_per_page = (int)(g.page_size / fa::kDecKeys);
}

fa::PagedWinDecArgs paged_window_args(const fa_paged_params *v, int64_t window_left, bool split) {
    fa::PagedWinDecArgs a{};
    static_cast<fa::DecArgs &>(a) = window_plan(v->base, window_left, split, fa::decode_plan);
    fill_paged(a, *v);
    a.window_left = fa::clamp_window(window_left);
    return a;
}

fa::PagedFp8WinDecArgs paged_fp8_window_args(const fa_paged_fp8_params *v, int64_t window_left, bool split) {
    fa::PagedFp8WinDecArgs a{};
    static_cast<fa::DecArgs &>(a) = window_plan(v->paged.base, window_left, split, fa::fp8_decode_plan);
    fill_paged(a, v->paged);
    a.k_descale = v->k_descale;
    a.v_descale = v->v_descale;
    a.descale_batch_stride = v->descale_batch_stride;
    a.descale_head_stride = v->descale_head_stride;
    a.window_left = fa::clamp_window(window_left);
    return a;
}

// the workspace checks of the unwindowed entries, then `launch(args)`
template <class Args, class Launch>
int checked_launch(const fa_fwd_params &p, const Args &a, void *workspace, int64_t workspace_bytes, Launch launch) {
    if (workspace && fa::decode_ws_bytes(p, a) > workspace_bytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)workspace_bytes, (long long)fa::decode_ws_bytes(p, a));
    return fa::with_dtype_causal(launch.dtype, launch.causal, [&](auto dt, auto c) {
        return fa::with_headdim(p.headdim, [&](auto d, auto exact) {
            return launch.template run<typename decltype(dt)::type, decltype(c)::value, decltype(d)::value,
                                       decltype(exact)::value>(p, a);
        });
    });
}

struct Launch16 {
    int dtype, causal;
    void *ws;
    hipStream_t stream;
    template <class DT, bool C, int kD, bool kExact>
    int run(const fa_fwd_params &p, const fa::PagedWinDecArgs &a) const {
        return fa::launch_decode_paged_window<DT, C, kD, kExact>(p, a, ws, stream);
    }
};
struct Launch8 {
    int dtype, causal;
    void *ws;
    hipStream_t stream;
    template <class DT, bool C, int kD, bool kExact>
    int run(const fa_fwd_params &p, const fa::PagedFp8WinDecArgs &a) const {
        return fa::launch_decode_paged_fp8_window<DT, C, kD, kExact>(p, a, ws, stream);
    }
};
}  // namespace

extern "C" int fa_fwd_gfx950_paged_window(const fa_paged_params *params, int dtype, int causal, int64_t window_left,
                                          void *workspace, int64_t workspace_bytes, void *stream) {
    if (window_left < 0) return fa_fwd_gfx950_paged(params, dtype, causal, workspace, workspace_bytes, stream);
    fa::set_last_path(fa::kPathNone);
    const int rc = fa_fwd_gfx950_paged_check(params, dtype, causal);
    if (rc != FA_OK) return rc;
    if ((uintptr_t)workspace & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    return checked_launch(params->base, paged_window_args(params, window_left, workspace != nullptr), workspace,
                          workspace_bytes, Launch16{dtype, causal, workspace, (hipStream_t)stream});
}

extern "C" int64_t fa_fwd_gfx950_paged_window_workspace_size(const fa_paged_params *params, int dtype, int causal,
                                                             int64_t window_left) {
    if (window_left < 0) return fa_fwd_gfx950_paged_workspace_size(params, dtype, causal);
    if (fa_fwd_gfx950_paged_check(params, dtype, causal) != FA_OK) return -1;
    return fa::decode_ws_bytes(params->base, paged_window_args(params, window_left, true));
}

extern "C" int fa_fwd_gfx950_paged_window_check(const fa_paged_params *params, int dtype, int causal,
                                                int64_t window_left) {
    (void)window_left;  // every value is valid: negative is "no window", large ones are clamped
    return fa_fwd_gfx950_paged_check(params, dtype, causal);
}

extern "C" int fa_fwd_gfx950_paged_window_fp8(const fa_paged_fp8_params *params, int dtype, int causal,
                                              int64_t window_left, void *workspace, int64_t workspace_bytes,
                                              void *stream) {
    if (window_left < 0) return fa_fwd_gfx950_paged_fp8(params, dtype, causal, workspace, workspace_bytes, stream);
    fa::set_last_path(fa::kPathNone);
    const int rc = fa_fwd_gfx950_paged_fp8_check(params, dtype, causal);
    if (rc != FA_OK) return rc;
    if ((uintptr_t)workspace & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    return checked_launch(params->paged.base, paged_fp8_window_args(params, window_left, workspace != nullptr),
                          workspace, workspace_bytes, Launch8{dtype, causal, workspace, (hipStream_t)stream});
}

extern "C" int64_t fa_fwd_gfx950_paged_window_fp8_workspace_size(const fa_paged_fp8_params *params, int dtype,
                                                                 int causal, int64_t window_left) {
    if (window_left < 0) return fa_fwd_gfx950_paged_fp8_workspace_size(params, dtype, causal);
    if (fa_fwd_gfx950_paged_fp8_check(params, dtype, causal) != FA_OK) return -1;
    return fa::decode_ws_bytes(params->paged.base, paged_fp8_window_args(params, window_left, true));
}

extern "C" int fa_fwd_gfx950_paged_window_fp8_check(const fa_paged_fp8_params *params, int dtype, int causal,
                                                    int64_t window_left) {
    (void)window_left;
    return fa_fwd_gfx950_paged_fp8_check(params, dtype, causal);
}

extern "C" int fa_paged_window_version(void) { return FA_GFX950_PAGED_WINDOW_VERSION; }
