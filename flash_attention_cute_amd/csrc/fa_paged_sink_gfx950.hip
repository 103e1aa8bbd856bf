// fa_paged_sink_gfx950.hip -- C-ABI of the paged decode with attention sinks (include/fa_gfx950_sink.h).
//
// Host code only, beside fa_paged_gfx950.hip (the paged decode entries), which it does not change and which
// never references it: the base validation is fa_fwd_gfx950_paged_check's / _paged_fp8_check's through their
// public entries, so these entries and the ones without sinks cannot drift apart, plus the one rule that is new
// here (the sinks array); the split plan is the one of the entry without sinks (fa::decode_plan /
// fa::fp8_decode_plan, made for fa::window_plan_keys when there is a window), so the workspace is the same and a
// launch whose sinks are all -inf gives the unsinked bits; the dtype / causal / head-dim dispatch goes to the sink
// instantiations (fa_paged_sink_inst.hip, fa_paged_fp8_sink_inst.hip and their two windowed files).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_sink.h"
#include "fa_paged_sink_launch.h"

namespace {
using fa::set_err;

// the rule of the sink entries that the base checks do not know
int check_sinks(const float *sinks) {
    if (!sinks) return set_err(FA_ERR_INVALID_ARGUMENT, "sinks is NULL");
    if ((uintptr_t)sinks & 3) return set_err(FA_ERR_INVALID_ARGUMENT, "sinks must be a 4-byte aligned fp32 array");
    return FA_OK;
}

void fill_paged(fa::PagedDecArgs &a, const fa_paged_params &g) {
    a.block_table = g.block_table;
    a.block_table_stride = g.block_table_stride;
    a.seqlens_k = g.seqlens_k;
    a.num_pages = (int)g.num_pages;
    a.tiles_per_page = (int)(g.page_size / fa::kDecKeys);
}

// What an entry needs to know about its pool (as Pool16 / Pool8 of fa_paged_gfx950.hip)
struct Sink16 {
    using Params = fa_paged_sink_params;
    using Args = fa::PagedSinkDecArgs;
    using WinArgs = fa::PagedWinSinkDecArgs;
    static const fa_paged_params &paged(const Params &v) { return v.paged; }
    static int base_check(const Params &v, int dtype, int causal) {
        return fa_fwd_gfx950_paged_check(&v.paged, dtype, causal);
    }
    static fa::DecArgs plan(const fa_fwd_params &p, int max_split) { return fa::decode_plan(p, max_split); }
    static void fill(fa::PagedDecArgs &a, const Params &v) { fill_paged(a, v.paged); }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const Args &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_sink<DT, C, kD, kExact>(p, a, ws, stream);
    }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const WinArgs &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_window_sink<DT, C, kD, kExact>(p, a, ws, stream);
    }
};
struct Sink8 {
    using Params = fa_paged_fp8_sink_params;
    using Args = fa::PagedFp8SinkDecArgs;
    using WinArgs = fa::PagedFp8WinSinkDecArgs;
    static const fa_paged_params &paged(const Params &v) { return v.fp8.paged; }
    static int base_check(const Params &v, int dtype, int causal) {
        return fa_fwd_gfx950_paged_fp8_check(&v.fp8, dtype, causal);
    }
    static fa::DecArgs plan(const fa_fwd_params &p, int max_split) { return fa::fp8_decode_plan(p, max_split); }
    static void fill(fa::PagedFp8DecArgs &a, const Params &v) {
        fill_paged(a, v.fp8.paged);
        a.k_descale = v.fp8.k_descale;
        a.v_descale = v.fp8.v_descale;
        a.descale_batch_stride = v.fp8.descale_batch_stride;
        a.descale_head_stride = v.fp8.descale_head_stride;
    }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const Args &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_fp8_sink<DT, C, kD, kExact>(p, a, ws, stream);
    }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const WinArgs &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_fp8_window_sink<DT, C, kD, kExact>(p, a, ws, stream);
    }
};

// every window_left is valid (window_left < 0: no window; large values are clamped)
template <class Pool>
int sink_check(const typename Pool::Params *v, int dtype, int causal) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    const int rc = Pool::base_check(*v, dtype, causal);
    if (rc != FA_OK) return rc;
    return check_sinks(v->sinks);
}

// The split plan of the entry without sinks: window_left >= 0, the pool's plan on a copy of the parameters whose
// seqlen_kv is the window's reach (paged_plan of fa_paged_gfx950.hip)
template <class Pool>
fa::DecArgs sink_plan(const typename Pool::Params &v, int64_t window_left, bool split) {
    fa_fwd_params planned = Pool::paged(v).base;
    if (window_left >= 0) planned.seqlen_kv = fa::window_plan_keys(planned, window_left);
    return Pool::plan(planned, split ? fa::kDecMaxSplit : 1);
}

// the workspace check, then the dtype / causal / head-dim dispatch to the launch of `a`'s kernel
template <class Pool, class Args>
int checked_launch(const fa_fwd_params &p, int dtype, int causal, const Args &a, void *workspace,
                   int64_t workspace_bytes, hipStream_t stream) {
    if (workspace && fa::decode_ws_bytes(p, a) > workspace_bytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)workspace_bytes, (long long)fa::decode_ws_bytes(p, a));
    return fa::with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
        return fa::with_headdim(p.headdim, [&](auto d, auto exact) {
            return Pool::template launch<typename decltype(dt)::type, decltype(c)::value, decltype(d)::value,
                                         decltype(exact)::value>(p, a, workspace, stream);
        });
    });
}

template <class Pool>
int sink_entry(const typename Pool::Params *v, int dtype, int causal, int64_t window_left, void *workspace,
               int64_t workspace_bytes, void *stream) {
    fa::set_last_path(fa::kPathNone);
    const int rc = sink_check<Pool>(v, dtype, causal);
    if (rc != FA_OK) return rc;
    if ((uintptr_t)workspace & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    const fa_fwd_params &p = Pool::paged(*v).base;
    const fa::DecArgs plan = sink_plan<Pool>(*v, window_left, workspace != nullptr);
    if (window_left < 0) {
        typename Pool::Args a{};
        static_cast<fa::DecArgs &>(a) = plan;
        Pool::fill(a, *v);
        a.sinks = v->sinks;
        return checked_launch<Pool>(p, dtype, causal, a, workspace, workspace_bytes, (hipStream_t)stream);
    }
    typename Pool::WinArgs a{};
    static_cast<fa::DecArgs &>(a) = plan;
    Pool::fill(a, *v);
    a.window_left = fa::clamp_window(window_left);
    a.sinks = v->sinks;
    return checked_launch<Pool>(p, dtype, causal, a, workspace, workspace_bytes, (hipStream_t)stream);
}

template <class Pool>
int64_t sink_workspace_size(const typename Pool::Params *v, int dtype, int causal, int64_t window_left) {
    if (sink_check<Pool>(v, dtype, causal) != FA_OK) return -1;
    return fa::decode_ws_bytes(Pool::paged(*v).base, sink_plan<Pool>(*v, window_left, true));
}
}  // namespace

extern "C" int fa_fwd_gfx950_paged_sink(const fa_paged_sink_params *params, int dtype, int causal,
                                        int64_t window_left, void *workspace, int64_t workspace_bytes,
                                        void *stream) {
    return sink_entry<Sink16>(params, dtype, causal, window_left, workspace, workspace_bytes, stream);
}
extern "C" int64_t fa_fwd_gfx950_paged_sink_workspace_size(const fa_paged_sink_params *params, int dtype, int causal,
                                                           int64_t window_left) {
    return sink_workspace_size<Sink16>(params, dtype, causal, window_left);
}
extern "C" int fa_fwd_gfx950_paged_sink_check(const fa_paged_sink_params *params, int dtype, int causal, int64_t) {
    return sink_check<Sink16>(params, dtype, causal);
}

extern "C" int fa_fwd_gfx950_paged_sink_fp8(const fa_paged_fp8_sink_params *params, int dtype, int causal,
                                            int64_t window_left, void *workspace, int64_t workspace_bytes,
                                            void *stream) {
    return sink_entry<Sink8>(params, dtype, causal, window_left, workspace, workspace_bytes, stream);
}
extern "C" int64_t fa_fwd_gfx950_paged_sink_fp8_workspace_size(const fa_paged_fp8_sink_params *params, int dtype,
                                                               int causal, int64_t window_left) {
    return sink_workspace_size<Sink8>(params, dtype, causal, window_left);
}
extern "C" int fa_fwd_gfx950_paged_sink_fp8_check(const fa_paged_fp8_sink_params *params, int dtype, int causal,
                                                  int64_t) {
    return sink_check<Sink8>(params, dtype, causal);
}

extern "C" int fa_sink_version(void) { return FA_GFX950_SINK_VERSION; }
