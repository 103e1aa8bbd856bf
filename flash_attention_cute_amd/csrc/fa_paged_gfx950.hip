// fa_paged_gfx950.hip -- C-ABI of the paged KV-cache decode (include/fa_gfx950_paged.h).
//
// Host code only, beside fa_fwd_gfx950.hip (whose error channel, knobs and per-stream counter area it
// uses through fa_launch.h): validation of the page pool / block table description, the split plan of
// the equivalent dense decode, and the dtype / causal / head-dim dispatch to the paged instantiations
// (fa_paged_inst.hip). The dense dispatcher never references these launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_paged.h"
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

fa::PagedDecArgs paged_plan(const fa_paged_params *v, bool split) {
    fa::PagedDecArgs a{};
    static_cast<fa::DecArgs &>(a) = fa::decode_plan(v->base, split ? fa::kDecMaxSplit : 1);
    a.block_table = v->block_table;
    a.block_table_stride = v->block_table_stride;
    a.seqlens_k = v->seqlens_k;
    a.num_pages = (int)v->num_pages;
    a.tiles_per_page = (int)(v->page_size / fa::kDecKeys);
    return a;
}

int launch_paged(const fa_fwd_params &p, int dtype, int causal, const fa::PagedDecArgs &a, void *ws,
                 hipStream_t stream) {
    return fa::with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
        return fa::with_headdim(p.headdim, [&](auto d, auto exact) {
            return fa::launch_decode_paged<typename decltype(dt)::type, decltype(c)::value, decltype(d)::value,
                                           decltype(exact)::value>(p, a, ws, stream);
        });
    });
}
}  // namespace

extern "C" int fa_fwd_gfx950_paged(const fa_paged_params *params, int dtype, int causal, void *workspace,
                                   int64_t workspace_bytes, void *stream) {
    fa::set_last_path(fa::kPathNone);
    const int rc = check_paged(params, dtype, causal);
    if (rc != FA_OK) return rc;
    if ((uintptr_t)workspace & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    const fa_fwd_params &p = params->base;
    const fa::PagedDecArgs a = paged_plan(params, workspace != nullptr);
    if (workspace && fa::decode_ws_bytes(p, a) > workspace_bytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)workspace_bytes, (long long)fa::decode_ws_bytes(p, a));
    return launch_paged(p, dtype, causal, a, workspace, (hipStream_t)stream);
}

extern "C" int64_t fa_fwd_gfx950_paged_workspace_size(const fa_paged_params *params, int dtype, int causal) {
    if (check_paged(params, dtype, causal) != FA_OK) return -1;
    return fa::decode_ws_bytes(params->base, paged_plan(params, true));
}

extern "C" int fa_fwd_gfx950_paged_check(const fa_paged_params *params, int dtype, int causal) {
    return check_paged(params, dtype, causal);
}

extern "C" int fa_paged_version(void) { return FA_GFX950_PAGED_VERSION; }
