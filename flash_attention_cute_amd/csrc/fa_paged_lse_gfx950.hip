// fa_paged_lse_gfx950.hip -- C-ABI of the paged decode with the LSE output (include/fa_gfx950_lse.h).
//
// Host code only, beside fa_paged_gfx950.hip (the paged decode entries), which it does not change and which
// never references it: the base validation is fa_fwd_gfx950_paged_check's / _paged_fp8_check's through their
// public entries, so these entries and the ones without the LSE cannot drift apart, plus the rules that are
// new here (the LSE array, seqlen_offset, no window); the split plan is the one of the entry without the LSE
// (fa::decode_plan / fa::fp8_decode_plan), so the workspace is the same and O is bit-identical; the dtype /
// causal / head-dim dispatch goes to the LSE instantiations (fa_paged_lse_inst.hip, fa_paged_fp8_lse_inst.hip).
// fa_merge_states_gfx950 lives with its kernel (fa_merge.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_lse.h"
#include "fa_paged_lse_launch.h"

namespace {
using fa::set_err;

// the rules of the LSE entries that the base checks do not know
int check_lse_fields(const float *lse_ptr, int64_t bs, int64_t hs, int64_t ss, int64_t seqlen_offset,
                     int64_t window_left) {
    if (window_left >= 0)
        return set_err(FA_ERR_UNSUPPORTED,
                       "the sliding-window decode kernels have no LSE variant (window_left = %lld): pass "
                       "window_left < 0",
                       (long long)window_left);
    if (!lse_ptr) return set_err(FA_ERR_INVALID_ARGUMENT, "lse_ptr is NULL");
    if ((uintptr_t)lse_ptr & 3) return set_err(FA_ERR_INVALID_ARGUMENT, "lse_ptr must be a 4-byte aligned fp32 array");
    if (bs < 0 || hs < 0 || ss < 0) return set_err(FA_ERR_INVALID_ARGUMENT, "lse strides must be non-negative");
    if (seqlen_offset > fa::kLseMaxOffset || seqlen_offset < -fa::kLseMaxOffset)
        return set_err(FA_ERR_INVALID_ARGUMENT, "seqlen_offset (%lld) must be within +-2^30", (long long)seqlen_offset);
    return FA_OK;
}

// seqlens_k may be NULL here: the base check sees a stand-in that meets its non-NULL, 4-byte-aligned rule (no
// check reads device arrays)
template <class Paged>
void stand_in_seqlens(Paged &g) {
    if (!g.seqlens_k) g.seqlens_k = g.block_table;
}

struct Lse16 {
    using Params = fa_paged_lse_params;
    using Args = fa::PagedLseDecArgs;
    static const fa_paged_params &paged(const Params &v) { return v.paged; }
    static int base_check(const Params &v, int dtype, int causal) {
        fa_paged_params g = v.paged;
        stand_in_seqlens(g);
        return fa_fwd_gfx950_paged_check(&g, dtype, causal);
    }
    static fa::DecArgs plan(const fa_fwd_params &p, int max_split) { return fa::decode_plan(p, max_split); }
    static void fill(Args &, const Params &) {}
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const Args &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_lse<DT, C, kD, kExact>(p, a, ws, stream);
    }
};
struct Lse8 {
    using Params = fa_paged_fp8_lse_params;
    using Args = fa::PagedFp8LseDecArgs;
    static const fa_paged_params &paged(const Params &v) { return v.fp8.paged; }
    static int base_check(const Params &v, int dtype, int causal) {
        fa_paged_fp8_params g = v.fp8;
        stand_in_seqlens(g.paged);
        return fa_fwd_gfx950_paged_fp8_check(&g, dtype, causal);
    }
    static fa::DecArgs plan(const fa_fwd_params &p, int max_split) { return fa::fp8_decode_plan(p, max_split); }
    static void fill(Args &a, const Params &v) {
        a.k_descale = v.fp8.k_descale;
        a.v_descale = v.fp8.v_descale;
        a.descale_batch_stride = v.fp8.descale_batch_stride;
        a.descale_head_stride = v.fp8.descale_head_stride;
    }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const Args &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_fp8_lse<DT, C, kD, kExact>(p, a, ws, stream);
    }
};

template <class Pool>
int lse_check(const typename Pool::Params *v, int dtype, int causal, int64_t window_left) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    const int rc = Pool::base_check(*v, dtype, causal);
    if (rc != FA_OK) return rc;
    return check_lse_fields(v->lse_ptr, v->lse_batch_stride, v->lse_head_stride, v->lse_seqlen_stride,
                            v->seqlen_offset, window_left);
}

template <class Pool>
int lse_entry(const typename Pool::Params *v, int dtype, int causal, int64_t window_left, void *workspace,
              int64_t workspace_bytes, void *stream) {
    fa::set_last_path(fa::kPathNone);
    const int rc = lse_check<Pool>(v, dtype, causal, window_left);
    if (rc != FA_OK) return rc;
    if ((uintptr_t)workspace & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    const fa_paged_params &g = Pool::paged(*v);
    const fa_fwd_params &p = g.base;
    typename Pool::Args a{};
    static_cast<fa::DecArgs &>(a) = Pool::plan(p, workspace ? fa::kDecMaxSplit : 1);
    a.block_table = g.block_table;
    a.block_table_stride = g.block_table_stride;
    a.seqlens_k = g.seqlens_k;
    a.num_pages = (int)g.num_pages;
    a.tiles_per_page = (int)(g.page_size / fa::kDecKeys);
    Pool::fill(a, *v);
    a.lse = fa::LseOut{v->lse_ptr, v->lse_batch_stride, v->lse_head_stride, v->lse_seqlen_stride};
    a.seqlen_offset = (int)v->seqlen_offset;
    if (workspace && fa::decode_ws_bytes(p, a) > workspace_bytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)workspace_bytes, (long long)fa::decode_ws_bytes(p, a));
    return fa::with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
        return fa::with_headdim(p.headdim, [&](auto d, auto exact) {
            return Pool::template launch<typename decltype(dt)::type, decltype(c)::value, decltype(d)::value,
                                         decltype(exact)::value>(p, a, workspace, (hipStream_t)stream);
        });
    });
}

template <class Pool>
int64_t lse_workspace_size(const typename Pool::Params *v, int dtype, int causal, int64_t window_left) {
    if (lse_check<Pool>(v, dtype, causal, window_left) != FA_OK) return -1;
    const fa_fwd_params &p = Pool::paged(*v).base;
    return fa::decode_ws_bytes(p, Pool::plan(p, fa::kDecMaxSplit));
}
}  // namespace

extern "C" int fa_fwd_gfx950_paged_lse(const fa_paged_lse_params *params, int dtype, int causal, int64_t window_left,
                                       void *workspace, int64_t workspace_bytes, void *stream) {
    return lse_entry<Lse16>(params, dtype, causal, window_left, workspace, workspace_bytes, stream);
}
extern "C" int64_t fa_fwd_gfx950_paged_lse_workspace_size(const fa_paged_lse_params *params, int dtype, int causal,
                                                          int64_t window_left) {
    return lse_workspace_size<Lse16>(params, dtype, causal, window_left);
}
extern "C" int fa_fwd_gfx950_paged_lse_check(const fa_paged_lse_params *params, int dtype, int causal,
                                             int64_t window_left) {
    return lse_check<Lse16>(params, dtype, causal, window_left);
}

extern "C" int fa_fwd_gfx950_paged_lse_fp8(const fa_paged_fp8_lse_params *params, int dtype, int causal,
                                           int64_t window_left, void *workspace, int64_t workspace_bytes,
                                           void *stream) {
    return lse_entry<Lse8>(params, dtype, causal, window_left, workspace, workspace_bytes, stream);
}
extern "C" int64_t fa_fwd_gfx950_paged_lse_fp8_workspace_size(const fa_paged_fp8_lse_params *params, int dtype,
                                                              int causal, int64_t window_left) {
    return lse_workspace_size<Lse8>(params, dtype, causal, window_left);
}
extern "C" int fa_fwd_gfx950_paged_lse_fp8_check(const fa_paged_fp8_lse_params *params, int dtype, int causal,
                                                 int64_t window_left) {
    return lse_check<Lse8>(params, dtype, causal, window_left);
}

extern "C" int fa_lse_version(void) { return FA_GFX950_LSE_VERSION; }
