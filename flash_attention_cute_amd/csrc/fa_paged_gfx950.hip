// fa_paged_gfx950.hip -- C-ABI of the paged KV-cache decode: the 16-bit pool (include/fa_gfx950_paged.h), the
// FP8 (e4m3) pool (include/fa_gfx950_fp8.h) and the sliding window over either
// (include/fa_gfx950_paged_window.h).
//
// Host code only, beside fa_fwd_gfx950.hip (whose error channel, knobs and per-stream counter area it
// uses through fa_launch.h): validation of the page pool / block table description, the split plan, and
// the dtype / causal / head-dim dispatch to the paged instantiations (fa_paged_inst.hip,
// fa_paged_fp8_inst.hip, fa_paged_window_inst.hip, fa_paged_fp8_window_inst.hip). The dense dispatcher never
// references these launches. The two pools differ in their checks, their split plan and their launches
// (Pool16 / Pool8 below); every entry is the same template over one of them: window_left < 0 runs the
// unwindowed kernel on the unwindowed plan, otherwise the plan is made for the keys a window can intersect
// (fa::window_plan_keys) and the windowed kernel runs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_paged_window.h"
#include "fa_paged_launch.h"

namespace {
using fa::set_err;

// The decode rule (fa_launch.h decode_rule) is a requirement here: there is no other paged kernel.
int check_decode_rule(const fa_fwd_params &p) {
    switch (fa::decode_rule(p)) {
    case fa::kDecTooManyRows:
        return set_err(FA_ERR_UNSUPPORTED,
                       "paged attention serves decode shapes only (the decode rule: head_q_per_group * seqlen_q "
                       "<= %d, got %lld): gather the pages and use fa_fwd_gfx950_padded",
                       fa::kDecMaxRows, (long long)(p.head_q_per_group * p.seqlen_q));
    case fa::kDecKnobOff:
        return set_err(FA_ERR_UNSUPPORTED, "paged attention needs the split-KV decode kernel (the decode knob is off)");
    case fa::kDecQSpan:
        return set_err(FA_ERR_UNSUPPORTED, "q strides too large for the decode kernel's 32-bit row offsets");
    case fa::kDecOk:
        break;
    }
    return FA_OK;
}

int check_paged(const fa_paged_params *v, int dtype, int causal) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (!v->block_table || !v->seqlens_k)
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table and seqlens_k must be non-NULL");
    if (((uintptr_t)v->block_table & 3) || ((uintptr_t)v->seqlens_k & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table and seqlens_k must be 4-byte aligned int32 arrays");
    if (v->page_size <= 0 || v->page_size % fa::kDecKeys != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "page_size (%lld) must be a positive multiple of %d",
                       (long long)v->page_size, fa::kDecKeys);
    if (v->num_pages < 1 || v->max_pages < 1)
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_pages and max_pages must be at least 1");
    if (v->num_pages > 0x7fffffffLL || v->max_pages > 0x3fffffffLL / v->page_size)
        return set_err(FA_ERR_UNSUPPORTED, "page pool or block table too large");
    if (v->base.seqlen_kv != v->max_pages * v->page_size)
        return set_err(FA_ERR_INVALID_ARGUMENT, "seqlen_kv (%lld) must equal max_pages * page_size (%lld)",
                       (long long)v->base.seqlen_kv, (long long)(v->max_pages * v->page_size));
    if (v->block_table_stride < 0 || (v->base.batch_size > 1 && v->block_table_stride < v->max_pages))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table_stride must be at least max_pages");
    if (v->base.batch_size > 0x7fffffffLL) return set_err(FA_ERR_UNSUPPORTED, "batch too large");
    // the pool strides take the dense checks (multiples of 8 elements, a tile inside 32-bit offsets)
    const int rc = fa_fwd_gfx950_check(&v->base, dtype, causal);
    if (rc != FA_OK) return rc;
    return check_decode_rule(v->base);
}

int check_paged_fp8(const fa_paged_fp8_params *v, int dtype, int causal) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    const fa_fwd_params &p = v->paged.base;
    if (p.headdim > 128) return set_err(FA_ERR_UNSUPPORTED, "only support hidden dimension <= 128");
    if (p.headdim <= 0 || p.headdim % 16 != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "an fp8 KV cache needs a head dim that is a multiple of 16 (got %lld)",
                       (long long)p.headdim);
    // the pool is read in place by 16-byte LDS-DMA chunks of 16 one-byte elements
    if (((uintptr_t)p.k_ptr & 15) || ((uintptr_t)p.v_ptr & 15))
        return set_err(FA_ERR_INVALID_ARGUMENT, "the fp8 K / V pool bases must be 16-byte aligned");
    const int64_t st[6] = {p.k_batch_stride, p.k_head_stride, p.k_seqlen_stride,
                           p.v_batch_stride, p.v_head_stride, p.v_seqlen_stride};
    for (int i = 0; i < 6; ++i)
        if (st[i] % 16 != 0)
            return set_err(FA_ERR_INVALID_ARGUMENT,
                           "the fp8 K / V page, head and row strides must be multiples of 16 elements (16 bytes)");
    if (v->descale_batch_stride < 0 || v->descale_head_stride < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "descale strides must be non-negative");
    if (((uintptr_t)v->k_descale & 3) || ((uintptr_t)v->v_descale & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "k_descale and v_descale must be 4-byte aligned fp32 arrays");
    // everything else (table, lengths, page size, q / o, 32-bit tile offsets, the decode rule) is the
    // 16-bit paged decode's; its stride bounds are in 2-byte elements, so they hold for bytes
    return check_paged(&v->paged, dtype, causal);
}

void fill_paged(fa::PagedDecArgs &a, const fa_paged_params &g) {
    a.block_table = g.block_table;
    a.block_table_stride = g.block_table_stride;
    a.seqlens_k = g.seqlens_k;
    a.num_pages = (int)g.num_pages;
    a.tiles_per_page = (int)(g.page_size / fa::kDecKeys);
}

void fill_descale(fa::PagedFp8DecArgs &a, const fa_paged_fp8_params &v) {
    a.k_descale = v.k_descale;
    a.v_descale = v.v_descale;
    a.descale_batch_stride = v.descale_batch_stride;
    a.descale_head_stride = v.descale_head_stride;
}

// What an entry needs to know about its pool: the parameter struct, the argument structs of the unwindowed
// and the windowed kernel, the check, the split plan and the launches
struct Pool16 {
    using Params = fa_paged_params;
    using Args = fa::PagedDecArgs;
    using WinArgs = fa::PagedWinDecArgs;
    static const fa_paged_params &paged(const Params &v) { return v; }
    static int check(const Params *v, int dtype, int causal) { return check_paged(v, dtype, causal); }
    static fa::DecArgs plan(const fa_fwd_params &p, int max_split) { return fa::decode_plan(p, max_split); }
    static void fill(Args &a, const Params &v) { fill_paged(a, v); }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const Args &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged<DT, C, kD, kExact>(p, a, ws, stream);
    }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const WinArgs &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_window<DT, C, kD, kExact>(p, a, ws, stream);
    }
};
struct Pool8 {
    using Params = fa_paged_fp8_params;
    using Args = fa::PagedFp8DecArgs;
    using WinArgs = fa::PagedFp8WinDecArgs;
    static const fa_paged_params &paged(const Params &v) { return v.paged; }
    static int check(const Params *v, int dtype, int causal) { return check_paged_fp8(v, dtype, causal); }
    static fa::DecArgs plan(const fa_fwd_params &p, int max_split) { return fa::fp8_decode_plan(p, max_split); }
    static void fill(Args &a, const Params &v) {
        fill_paged(a, v.paged);
        fill_descale(a, v);
    }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const Args &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_fp8<DT, C, kD, kExact>(p, a, ws, stream);
    }
    template <class DT, bool C, int kD, bool kExact>
    static int launch(const fa_fwd_params &p, const WinArgs &a, void *ws, hipStream_t stream) {
        return fa::launch_decode_paged_fp8_window<DT, C, kD, kExact>(p, a, ws, stream);
    }
};

// The split plan of a launch. window_left >= 0: the pool's plan on a copy of the parameters whose seqlen_kv is
// the window's reach; the kernel still clamps lengths to the real capacity
template <class Pool>
fa::DecArgs paged_plan(const typename Pool::Params &v, int64_t window_left, bool split) {
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

// The entry / _workspace_size / _check triple of every paged decode (window_left < 0: no window; every other
// value is valid, large ones are clamped)
template <class Pool>
int paged_entry(const typename Pool::Params *params, int dtype, int causal, int64_t window_left, void *workspace,
                int64_t workspace_bytes, void *stream) {
    fa::set_last_path(fa::kPathNone);
    const int rc = Pool::check(params, dtype, causal);
    if (rc != FA_OK) return rc;
    if ((uintptr_t)workspace & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    const fa_fwd_params &p = Pool::paged(*params).base;
    const fa::DecArgs plan = paged_plan<Pool>(*params, window_left, workspace != nullptr);
    if (window_left < 0) {
        typename Pool::Args a{};
        static_cast<fa::DecArgs &>(a) = plan;
        Pool::fill(a, *params);
        return checked_launch<Pool>(p, dtype, causal, a, workspace, workspace_bytes, (hipStream_t)stream);
    }
    typename Pool::WinArgs a{};
    static_cast<fa::DecArgs &>(a) = plan;
    Pool::fill(a, *params);
    a.window_left = fa::clamp_window(window_left);
    return checked_launch<Pool>(p, dtype, causal, a, workspace, workspace_bytes, (hipStream_t)stream);
}

template <class Pool>
int64_t paged_workspace_size(const typename Pool::Params *params, int dtype, int causal, int64_t window_left) {
    if (Pool::check(params, dtype, causal) != FA_OK) return -1;
    return fa::decode_ws_bytes(Pool::paged(*params).base, paged_plan<Pool>(*params, window_left, true));
}
}  // namespace

extern "C" int fa_fwd_gfx950_paged(const fa_paged_params *params, int dtype, int causal, void *workspace,
                                   int64_t workspace_bytes, void *stream) {
    return paged_entry<Pool16>(params, dtype, causal, -1, workspace, workspace_bytes, stream);
}
extern "C" int64_t fa_fwd_gfx950_paged_workspace_size(const fa_paged_params *params, int dtype, int causal) {
    return paged_workspace_size<Pool16>(params, dtype, causal, -1);
}
extern "C" int fa_fwd_gfx950_paged_check(const fa_paged_params *params, int dtype, int causal) {
    return check_paged(params, dtype, causal);
}
extern "C" int fa_paged_version(void) { return FA_GFX950_PAGED_VERSION; }

extern "C" int fa_fwd_gfx950_paged_fp8(const fa_paged_fp8_params *params, int dtype, int causal, void *workspace,
                                       int64_t workspace_bytes, void *stream) {
    return paged_entry<Pool8>(params, dtype, causal, -1, workspace, workspace_bytes, stream);
}
extern "C" int64_t fa_fwd_gfx950_paged_fp8_workspace_size(const fa_paged_fp8_params *params, int dtype, int causal) {
    return paged_workspace_size<Pool8>(params, dtype, causal, -1);
}
extern "C" int fa_fwd_gfx950_paged_fp8_check(const fa_paged_fp8_params *params, int dtype, int causal) {
    return check_paged_fp8(params, dtype, causal);
}
extern "C" int fa_fp8_version(void) { return FA_GFX950_FP8_VERSION; }

extern "C" int fa_fwd_gfx950_paged_window(const fa_paged_params *params, int dtype, int causal, int64_t window_left,
                                          void *workspace, int64_t workspace_bytes, void *stream) {
    return paged_entry<Pool16>(params, dtype, causal, window_left, workspace, workspace_bytes, stream);
}
extern "C" int64_t fa_fwd_gfx950_paged_window_workspace_size(const fa_paged_params *params, int dtype, int causal,
                                                             int64_t window_left) {
    return paged_workspace_size<Pool16>(params, dtype, causal, window_left);
}
extern "C" int fa_fwd_gfx950_paged_window_check(const fa_paged_params *params, int dtype, int causal, int64_t) {
    return check_paged(params, dtype, causal);
}
extern "C" int fa_fwd_gfx950_paged_window_fp8(const fa_paged_fp8_params *params, int dtype, int causal,
                                              int64_t window_left, void *workspace, int64_t workspace_bytes,
                                              void *stream) {
    return paged_entry<Pool8>(params, dtype, causal, window_left, workspace, workspace_bytes, stream);
}
extern "C" int64_t fa_fwd_gfx950_paged_window_fp8_workspace_size(const fa_paged_fp8_params *params, int dtype,
                                                                 int causal, int64_t window_left) {
    return paged_workspace_size<Pool8>(params, dtype, causal, window_left);
}
extern "C" int fa_fwd_gfx950_paged_window_fp8_check(const fa_paged_fp8_params *params, int dtype, int causal,
                                                    int64_t) {
    return check_paged_fp8(params, dtype, causal);
}
extern "C" int fa_paged_window_version(void) { return FA_GFX950_PAGED_WINDOW_VERSION; }
