// fa_mla_fp8_gfx950.hip -- C-ABI of the MLA decode over an FP8 (e4m3) paged latent cache
// (include/fa_gfx950_mla_fp8.h): the checks (the 16-bit entry's, then the byte pool's own), the selection of
// fa_mla_decode_fp8kv (fa_mla_fp8.hpp) for both q dtypes, and the entries. The plan is the 16-bit entry's
// (mla_plan of fa_mla_host.h: the same splits, so the same workspace), as are the workspace, the argument fill and
// the launch with fa_mla_combine. A translation unit of its own; no other file references its kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_mla_fp8.hpp"
#include "fa_mla_host.h"

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

template <class DT>
int mla8_launch_kernels(const MlaArgs &a, const float *descale, const int64_t ds_stride, hipStream_t stream) {
    return mla_run<DT>(a, (int64_t)a.batch * a.n_split, stream, [&](const dim3 grid) {
        if (a.rows <= kDecRows)  // one row block: the kernel without the second block's registers
            hipLaunchKernelGGL((fa_mla_decode_fp8kv<DT, 1>), grid, dim3(256), 0, stream, a, descale, ds_stride);
        else
            hipLaunchKernelGGL((fa_mla_decode_fp8kv<DT, 2>), grid, dim3(256), 0, stream, a, descale, ds_stride);
    });
}

int mla8_launch(const fa_mla_fp8_params *params, int dtype, void *ws, int64_t ws_bytes, hipStream_t stream) {
    const int rc = mla8_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_params &p = params->base;
    MlaArgs a = mla_plan(p);
    const int wrc = mla_bind_ws(a, p.batch_size, ws, ws_bytes);
    if (wrc != FA_OK) return wrc;
    if (p.batch_size == 0) return FA_OK;
    mla_fill_args(a, p);  // (kv_ps and kv_rs in bytes)
    return dtype == FA_DTYPE_F16 ? mla8_launch_kernels<F16>(a, params->kv_descale, params->kv_descale_stride, stream)
                                 : mla8_launch_kernels<BF16>(a, params->kv_descale, params->kv_descale_stride, stream);
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
    const fa::MlaArgs a = fa::mla_plan(params->base);
    return fa::mla_ws_bytes(params->base.batch_size, a.n_split, a.rows);
}
extern "C" int fa_mla_fp8_version(void) { return FA_GFX950_MLA_FP8_VERSION; }
