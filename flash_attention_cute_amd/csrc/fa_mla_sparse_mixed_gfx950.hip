// fa_mla_sparse_mixed_gfx950.hip -- C-ABI of the sparse MLA decode over the mixed FP8 latent row
// (include/fa_gfx950_mla_mixed.h): the checks (the 16-bit sparse entry's, then the byte row's own), the selection of
// fa_mla_sparse_decode_mixed (fa_mla_sparse_mixed.hpp) and the entries. The plan is the 16-bit sparse entry's
// (mla_splits over B * Sq * head-group workgroups and the list's tiles, kMlaSparseMinTilesPerSplit: the same splits,
// so the same workspace), the workspace, the argument fill and the launch with fa_mla_combine are fa_mla_host.h's. A
// translation unit of its own; no other file references its kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_mla_host.h"
#include "fa_mla_sparse_mixed.hpp"

namespace fa {
namespace {

MlaSparseArgs mlax_plan(const fa_mla_sparse_params &v) {
    const fa_mla_params &p = v.base;
    MlaSparseArgs s{};
    s.Hq = (int)p.num_heads_q;
    s.n_tiles = (int)(v.topk / kDecKeys);
    s.m.rows = (int)(p.num_heads_q * p.seqlen_q);
    s.m.n_rg = (s.Hq + kMlaGroupRows - 1) / kMlaGroupRows;
    s.m.n_split = mla_splits((p.batch_size > 0 ? p.batch_size : 1) * p.seqlen_q * s.m.n_rg, s.n_tiles,
                             kMlaSparseMinTilesPerSplit, p.num_splits);
    return s;
}

int mlax_check(const fa_mla_sparse_params *v, int dtype) {
    const int rc = fa_mla_sparse_decode_gfx950_check(v, dtype);  // (strides counted in 1-byte elements)
    if (rc != FA_OK) return rc;
    if (dtype != FA_DTYPE_BF16)
        return set_err(FA_ERR_UNSUPPORTED, "the mixed-row sparse MLA decode takes bf16 q only (dtype %d)", dtype);
    const fa_mla_params &p = v->base;
    if (p.kv_row_stride < kMixRowBytes || p.kv_row_stride % 16 != 0 || p.kv_page_stride % 16 != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT,
                       "the mixed latent pool's row stride (%lld) must be at least %d and, like the page stride, a "
                       "multiple of 16 bytes", (long long)p.kv_row_stride, kMixRowBytes);
    return FA_OK;
}

int mlax_launch(const fa_mla_sparse_params *params, int dtype, void *ws, int64_t ws_bytes, hipStream_t stream) {
    const int rc = mlax_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_params &p = params->base;
    MlaSparseArgs s = mlax_plan(*params);
    const int wrc = mla_bind_ws(s.m, p.batch_size, ws, ws_bytes);
    if (wrc != FA_OK) return wrc;
    if (p.batch_size == 0) return FA_OK;
    mla_fill_args(s.m, p);  // (kv_ps and kv_rs in bytes)
    s.indices = params->indices;
    s.idx_bs = params->indices_batch_stride, s.idx_ss = params->indices_seqlen_stride;
    s.page_size = (int)p.page_size;
    s.page_shift = (p.page_size & (p.page_size - 1)) == 0 ? __builtin_ctzll((unsigned long long)p.page_size) : -1;
    return mla_run<BF16>(s.m, p.batch_size * p.seqlen_q * s.m.n_split, stream, [&](const dim3 grid) {
        if (s.Hq <= kDecRows)  // one row block: the kernel without the second block's registers
            hipLaunchKernelGGL((fa_mla_sparse_decode_mixed<1>), grid, dim3(256), 0, stream, s);
        else
            hipLaunchKernelGGL((fa_mla_sparse_decode_mixed<2>), grid, dim3(256), 0, stream, s);
    });
}

}  // namespace
}  // namespace fa

extern "C" int fa_mla_sparse_mixed_decode_gfx950(const fa_mla_sparse_params *params, int dtype, void *workspace,
                                                 int64_t workspace_bytes, void *stream) {
    return fa::mlax_launch(params, dtype, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int fa_mla_sparse_mixed_decode_gfx950_check(const fa_mla_sparse_params *params, int dtype) {
    return fa::mlax_check(params, dtype);
}
extern "C" int64_t fa_mla_sparse_mixed_decode_gfx950_ws_bytes(const fa_mla_sparse_params *params) {
    if (fa::mlax_check(params, FA_DTYPE_BF16) != FA_OK) return -1;
    const fa::MlaArgs a = fa::mlax_plan(*params).m;
    return fa::mla_ws_bytes(params->base.batch_size, a.n_split, a.rows);
}
extern "C" int fa_mla_mixed_version(void) { return FA_GFX950_MLA_MIXED_VERSION; }
