// fa_mla_gfx950.hip -- C-ABI of the MLA decode over a paged latent KV cache (include/fa_gfx950_mla.h): the
// checks, the selection of fa_mla_decode (fa_mla_decode.hpp) for both dtypes, and the entries. The plan, the
// workspace, the argument fill and the launch with fa_mla_combine are fa_mla_host.h's, shared with the FP8 and
// sparse entries. A translation unit of its own beside the dispatchers (whose error channel it uses through
// fa_launch.h); no other file references its kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_mla_host.h"

namespace fa {
namespace {

int mla_check(const fa_mla_params *p, int dtype) {
    if (!p) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return set_err(FA_ERR_UNSUPPORTED, "MLA decode supports fp16 / bf16 only (dtype %d)", dtype);
    if (!p->q_ptr || !p->kv_ptr || !p->o_ptr) return set_err(FA_ERR_INVALID_ARGUMENT, "q, kv and o must be non-NULL");
    if (!p->block_table || !p->seqlens_k)
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table and seqlens_k must be non-NULL");
    if (p->headdim_qk != kMlaDqk || p->headdim_v != kMlaDv)
        return set_err(FA_ERR_UNSUPPORTED, "MLA decode is built for head dims (576, 512) only (got (%lld, %lld))",
                       (long long)p->headdim_qk, (long long)p->headdim_v);
    if (p->batch_size < 0 || p->num_heads_q < 1 || p->seqlen_q < 1)
        return set_err(FA_ERR_INVALID_ARGUMENT, "batch_size must be non-negative, num_heads_q and seqlen_q positive");
    if (p->batch_size > 0x7fffffLL || p->num_heads_q * p->seqlen_q > 0xffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "batch or query rows (num_heads_q * seqlen_q) too large");
    if (((uintptr_t)p->block_table & 3) || ((uintptr_t)p->seqlens_k & 3) || ((uintptr_t)p->lse_ptr & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table, seqlens_k and lse must be 4-byte aligned");
    if (p->page_size <= 0 || p->page_size % kDecKeys != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "page_size (%lld) must be a positive multiple of %d",
                       (long long)p->page_size, kDecKeys);
    if (p->num_pages < 1 || p->max_pages < 1)
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_pages and max_pages must be at least 1");
    if (p->num_pages > 0x7fffffffLL || p->max_pages > 0x3fffffffLL / p->page_size)
        return set_err(FA_ERR_UNSUPPORTED, "page pool or block table too large");
    if (p->block_table_stride < 0 || (p->batch_size > 1 && p->block_table_stride < p->max_pages))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table_stride must be at least max_pages");
    if (((uintptr_t)p->q_ptr & 15) || ((uintptr_t)p->kv_ptr & 15) || ((uintptr_t)p->o_ptr & 15))
        return set_err(FA_ERR_INVALID_ARGUMENT, "q, kv and o must be 16-byte aligned");
    if (p->kv_row_stride % 8 != 0 || p->kv_row_stride < kMlaDqk)
        return set_err(FA_ERR_INVALID_ARGUMENT, "the latent row stride (%lld) must be a multiple of 8 and at least %d",
                       (long long)p->kv_row_stride, kMlaDqk);
    if (p->kv_row_stride > (1LL << 24)) return set_err(FA_ERR_UNSUPPORTED, "latent row stride too large");
    const int64_t st[7] = {p->q_batch_stride, p->q_head_stride, p->q_seqlen_stride, p->o_batch_stride,
                           p->o_head_stride,  p->o_seqlen_stride, p->kv_page_stride};
    for (int i = 0; i < 7; ++i)
        if (st[i] < 0 || st[i] % 8 != 0)
            return set_err(FA_ERR_INVALID_ARGUMENT,
                           "the strides of q, o and the page stride must be non-negative multiples of 8 elements");
    if (p->lse_batch_stride < 0 || p->lse_head_stride < 0 || p->lse_seqlen_stride < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "lse strides must be non-negative");
    uint32_t sc_bits;  // (on the bits: the build is -ffinite-math-only, under which a float test may drop NaN and inf)
    __builtin_memcpy(&sc_bits, &p->softmax_scale, sizeof sc_bits);
    if (sc_bits == 0 || sc_bits >= 0x7f800000u)  // +0, any negative value, +inf, NaN
        return set_err(FA_ERR_INVALID_ARGUMENT, "softmax_scale must be finite and > 0");
    if (p->num_splits < 0) return set_err(FA_ERR_INVALID_ARGUMENT, "num_splits must be non-negative");
    return FA_OK;
}

template <class DT>
int mla_launch_kernels(const MlaArgs &a, hipStream_t stream) {
    return mla_run<DT>(a, (int64_t)a.batch * a.n_split, stream, [&](const dim3 grid) {
        if (a.rows <= kDecRows)  // one row block: the kernel without the second block's registers
            hipLaunchKernelGGL((fa_mla_decode<DT, 1>), grid, dim3(256), 0, stream, a);
        else
            hipLaunchKernelGGL((fa_mla_decode<DT, 2>), grid, dim3(256), 0, stream, a);
    });
}

int mla_launch(const fa_mla_params *params, int dtype, void *ws, int64_t ws_bytes, hipStream_t stream) {
    const int rc = mla_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_params &p = *params;
    MlaArgs a = mla_plan(p);
    const int wrc = mla_bind_ws(a, p.batch_size, ws, ws_bytes);
    if (wrc != FA_OK) return wrc;
    if (p.batch_size == 0) return FA_OK;
    mla_fill_args(a, p);  // (kv_rs in 16-bit elements)
    return dtype == FA_DTYPE_F16 ? mla_launch_kernels<F16>(a, stream) : mla_launch_kernels<BF16>(a, stream);
}

}  // namespace
}  // namespace fa

extern "C" int fa_mla_decode_gfx950(const fa_mla_params *params, int dtype, void *workspace, int64_t workspace_bytes,
                                    void *stream) {
    return fa::mla_launch(params, dtype, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int fa_mla_decode_gfx950_check(const fa_mla_params *params, int dtype) {
    return fa::mla_check(params, dtype);
}
extern "C" int64_t fa_mla_decode_gfx950_ws_bytes(const fa_mla_params *params) {
    if (fa::mla_check(params, FA_DTYPE_F16) != FA_OK) return -1;
    const fa::MlaArgs a = fa::mla_plan(*params);
    return fa::mla_ws_bytes(params->batch_size, a.n_split, a.rows);
}
extern "C" int fa_mla_version(void) { return FA_GFX950_MLA_VERSION; }
