// fa_paged_fp8_gfx950.hip -- C-ABI of the FP8 (e4m3) paged KV-cache decode (include/fa_gfx950_fp8.h).
//
// Host code only, beside fa_paged_gfx950.hip: the page pool / block table description takes the 16-bit
// paged check (through its public entry, so the two cannot drift apart) plus what a byte pool read in
// place needs, the split plan is the 16-bit decode's rule with a workgroup target of its own, and the dtype
// / causal / head-dim dispatch goes to the FP8 instantiations (fa_paged_fp8_inst.hip). Neither 16-bit
// dispatcher references these launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_fp8.h"
#include "fa_paged_fp8_launch.h"

namespace {
using fa::set_err;

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
    return fa_fwd_gfx950_paged_check(&v->paged, dtype, causal);
}

fa::PagedFp8DecArgs paged_fp8_plan(const fa_paged_fp8_params *v, bool split) {
    fa::PagedFp8DecArgs a{};
    const fa_paged_params &g = v->paged;
    static_cast<fa::DecArgs &>(a) = fa::fp8_decode_plan(g.base, split ? fa::kDecMaxSplit : 1);
    a.block_table = g.block_table;
    a.block_table_stride = g.block_table_stride;
    a.seqlens_k = g.seqlens_k;
    a.num_pages = (int)g.num_pages;
    a.tiles_per_page = (int)(g.page_size / fa::kDecKeys);
    a.k_descale = v->k_descale;
    a.v_descale = v->v_descale;
    a.descale_batch_stride = v->descale_batch_stride;
    a.descale_head_stride = v->descale_head_stride;
    return a;
}

int launch_paged_fp8(const fa_fwd_params &p, int dtype, int causal, const fa::PagedFp8DecArgs &a, void *ws,
                     hipStream_t stream) {
    return fa::with_dtype_causal(dtype, causal, [&](auto dt, auto c) {
        return fa::with_headdim(p.headdim, [&](auto d, auto exact) {
            return fa::launch_decode_paged_fp8<typename decltype(dt)::type, decltype(c)::value, decltype(d)::value,
                                               decltype(exact)::value>(p, a, ws, stream);
        });
    });
}
}  // namespace

extern "C" int fa_fwd_gfx950_paged_fp8(const fa_paged_fp8_params *params, int dtype, int causal, void *workspace,
                                       int64_t workspace_bytes, void *stream) {
    fa::set_last_path(fa::kPathNone);
    const int rc = check_paged_fp8(params, dtype, causal);
    if (rc != FA_OK) return rc;
    if ((uintptr_t)workspace & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    const fa_fwd_params &p = params->paged.base;
    const fa::PagedFp8DecArgs a = paged_fp8_plan(params, workspace != nullptr);
    if (workspace && fa::decode_ws_bytes(p, a) > workspace_bytes)
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)workspace_bytes, (long long)fa::decode_ws_bytes(p, a));
    return launch_paged_fp8(p, dtype, causal, a, workspace, (hipStream_t)stream);
}

extern "C" int64_t fa_fwd_gfx950_paged_fp8_workspace_size(const fa_paged_fp8_params *params, int dtype, int causal) {
    if (check_paged_fp8(params, dtype, causal) != FA_OK) return -1;
    return fa::decode_ws_bytes(params->paged.base, paged_fp8_plan(params, true));
}

extern "C" int fa_fwd_gfx950_paged_fp8_check(const fa_paged_fp8_params *params, int dtype, int causal) {
    return check_paged_fp8(params, dtype, causal);
}

extern "C" int fa_fp8_version(void) { return FA_GFX950_FP8_VERSION; }
