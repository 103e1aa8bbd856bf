// fa_mla_fp8_gfx950.hip -- C-ABI of the MLA decode over an FP8 (e4m3) paged latent cache
// (include/fa_gfx950_mla_fp8.h): the checks (the 16-bit entry's, then the byte pool's own), the split plan (the
// 16-bit call's rule, so the workspace is the same), the launches of fa_mla_decode_fp8kv (fa_mla_fp8.hpp) /
// fa_mla_combine (fa_mla_decode.hpp) for both q dtypes, and the entries. A translation unit of its own; no other
// file references its kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_mla_fp8.hpp"

namespace fa {
namespace {

int mla8_check(const fa_mla_fp8_params *v, int dtype) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    const int rc = fa_mla_decode_gfx950_check(&v->base, dtype);  // (strides counted in 1-byte elements)
    if (rc != FA_OK) return rc;
    const fa_mla_params &p = v->base;
    if (p.kv_row_stride % 16 != 0 || p.kv_page_stride % 16 != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT,
                       "the fp8 latent pool's row stride (%lld) and page stride must be multiples of 16 bytes",
                       (long long)p.kv_row_stride);
    if (v->kv_descale_stride < 0) return set_err(FA_ERR_INVALID_ARGUMENT, "kv_descale_stride must be non-negative");
    if ((uintptr_t)v->kv_descale & 3)
        return set_err(FA_ERR_INVALID_ARGUMENT, "kv_descale must be a 4-byte aligned fp32 array");
    return FA_OK;
}

// fa_mla_gfx950.hip's plan: the same splits, so the same workspace
int mla8_splits(const fa_mla_params &p, const int rows) {
    const int n_rg = (rows + kMlaGroupRows - 1) / kMlaGroupRows;
    const int64_t n_tiles = p.max_pages * p.page_size / kDecKeys;
    const int64_t wgs = (p.batch_size > 0 ? p.batch_size : 1) * n_rg;
    int64_t ns = (kMlaTargetWgs + wgs - 1) / wgs;
    const int64_t by_len = n_tiles / kMlaMinTilesPerSplit;
    ns = ns < by_len ? ns : by_len;
    if (p.num_splits > 0) ns = p.num_splits;
    ns = ns < kMlaMaxSplit ? ns : kMlaMaxSplit;
    return (int)(ns < 1 ? 1 : ns);
}

int64_t mla8_ws_bytes(const fa_mla_params &p, const int n_split) {
    return n_split > 1 ? p.batch_size * n_split * p.num_heads_q * p.seqlen_q * (int64_t)(kMlaDv * 4 + 4) : 0;
}

template <class DT>
void mla8_launch_kernels(const MlaArgs &a, const float *descale, const int64_t ds_stride, hipStream_t stream) {
    const int64_t units = (int64_t)a.batch * a.n_split;
    const dim3 grid((uint32_t)(8 * ((units + 7) / 8) * a.n_rg));
    if (a.rows <= kDecRows)  // one row block: the kernel without the second block's registers
        hipLaunchKernelGGL((fa_mla_decode_fp8kv<DT, 1>), grid, dim3(256), 0, stream, a, descale, ds_stride);
    else
        hipLaunchKernelGGL((fa_mla_decode_fp8kv<DT, 2>), grid, dim3(256), 0, stream, a, descale, ds_stride);
    if (a.n_split > 1)
        hipLaunchKernelGGL((fa_mla_combine<DT>), dim3((uint32_t)(4 * a.batch * a.rows)), dim3(256), 0, stream, a);
}

int mla8_launch(const fa_mla_fp8_params *params, int dtype, void *ws, int64_t ws_bytes, hipStream_t stream) {
    const int rc = mla8_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_params &p = params->base;
    MlaArgs a{};
    a.rows = (int)(p.num_heads_q * p.seqlen_q);
    a.n_rg = (a.rows + kMlaGroupRows - 1) / kMlaGroupRows;
    a.n_split = mla8_splits(p, a.rows);
    const int64_t need = mla8_ws_bytes(p, a.n_split);
    if (need > 0 && (!ws || ws_bytes < need))
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)(ws ? ws_bytes : 0), (long long)need);
    if ((uintptr_t)ws & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    if (p.batch_size == 0) return FA_OK;
    a.q = (const char *)p.q_ptr, a.kv = (const char *)p.kv_ptr, a.o = (char *)p.o_ptr, a.lse = p.lse_ptr;
    a.block_table = p.block_table, a.seqlens_k = p.seqlens_k;
    a.q_bs = p.q_batch_stride, a.q_hs = p.q_head_stride, a.q_ss = p.q_seqlen_stride;
    a.o_bs = p.o_batch_stride, a.o_hs = p.o_head_stride, a.o_ss = p.o_seqlen_stride;
    a.lse_bs = p.lse_batch_stride, a.lse_hs = p.lse_head_stride, a.lse_ss = p.lse_seqlen_stride;
    a.kv_ps = p.kv_page_stride, a.kv_rs = (int)p.kv_row_stride;  // bytes
    a.batch = (int)p.batch_size, a.Sq = (int)p.seqlen_q;
    a.num_pages = (int)p.num_pages, a.tiles_per_page = (int)(p.page_size / kDecKeys);
    a.cap_keys = (int)(p.max_pages * p.page_size), a.bt_stride = (int)p.block_table_stride;
    a.causal = p.causal != 0 && p.seqlen_q > 1;
    a.sc = p.softmax_scale;
    if (need > 0) {
        a.ws_o = (float *)ws;
        a.ws_lse = (float *)((char *)ws + p.batch_size * a.n_split * a.rows * (int64_t)(kMlaDv * 4));
    }
    if (dtype == FA_DTYPE_F16) mla8_launch_kernels<F16>(a, params->kv_descale, params->kv_descale_stride, stream);
    else mla8_launch_kernels<BF16>(a, params->kv_descale, params->kv_descale_stride, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

}  // namespace
}  // namespace fa

extern "C" int fa_mla_decode_fp8_gfx950(const fa_mla_fp8_params *params, int q_dtype, void *workspace,
                                        int64_t workspace_bytes, void *stream) {
    return fa::mla8_launch(params, q_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int fa_mla_decode_fp8_gfx950_check(const fa_mla_fp8_params *params, int q_dtype) {
    return fa::mla8_check(params, q_dtype);
}
extern "C" int64_t fa_mla_decode_fp8_gfx950_ws_bytes(const fa_mla_fp8_params *params) {
    if (fa::mla8_check(params, FA_DTYPE_F16) != FA_OK) return -1;
    const fa_mla_params &p = params->base;
    return fa::mla8_ws_bytes(p, fa::mla8_splits(p, (int)(p.num_heads_q * p.seqlen_q)));
}
extern "C" int fa_mla_fp8_version(void) { return FA_GFX950_MLA_FP8_VERSION; }
