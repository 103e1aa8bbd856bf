// fa_mla_sparse_gfx950.hip -- C-ABI of the sparse MLA decode over top-k token indices of the paged latent KV cache
// (include/fa_gfx950_mla_sparse.h): the checks (the dense entry's, then the list's own), the split plan over the
// list's tiles, the selection of fa_mla_sparse_decode (fa_mla_sparse.hpp) for both dtypes, and the entries. The
// split rule, the workspace, the argument fill and the launch with fa_mla_combine are fa_mla_host.h's, shared with
// the dense entries. A translation unit of its own; no other file references its kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_mla_host.h"
#include "fa_mla_sparse.hpp"

namespace fa {
namespace {

// The plan: split s takes tiles s, s + n_split, ... of a list's topk / 32 tiles, a count that is the same for
// every (batch, position); mla_splits' rule over B * Sq * head-group workgroups, a split at least
// kMlaSparseMinTilesPerSplit tiles.
MlaSparseArgs mlas_plan(const fa_mla_sparse_params &v) {
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

// the (b, pos, split) units of the plan
int64_t mlas_units(const fa_mla_params &p, const MlaSparseArgs &s) { return p.batch_size * p.seqlen_q * s.m.n_split; }

int mlas_check(const fa_mla_sparse_params *v, int dtype) {
    if (!v) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    const int rc = fa_mla_decode_gfx950_check(&v->base, dtype);
    if (rc != FA_OK) return rc;
    if (!v->indices) return set_err(FA_ERR_INVALID_ARGUMENT, "indices must be non-NULL");
    if ((uintptr_t)v->indices & 3)  // (all the scalar loads of the list need)
        return set_err(FA_ERR_INVALID_ARGUMENT, "indices must be a 4-byte aligned int32 array");
    if (v->topk <= 0 || v->topk % kDecKeys != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "topk (%lld) must be a positive multiple of %d (pad the list with -1)",
                       (long long)v->topk, kDecKeys);
    if (v->topk > (1LL << 24)) return set_err(FA_ERR_UNSUPPORTED, "topk too large");
    if (v->indices_batch_stride < 0 || v->indices_seqlen_stride < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "the strides of indices must be non-negative");
    const MlaSparseArgs s = mlas_plan(*v);
    if (mla_grid(mlas_units(v->base, s), s.m.n_rg) > 0x7fffffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "batch * seqlen_q * splits * head groups too large for one launch");
    return FA_OK;
}

template <class DT>
int mlas_launch_kernels(const MlaSparseArgs &s, const int64_t units, hipStream_t stream) {
    return mla_run<DT>(s.m, units, stream, [&](const dim3 grid) {
        if (s.Hq <= kDecRows)  // one row block: the kernel without the second block's registers
            hipLaunchKernelGGL((fa_mla_sparse_decode<DT, 1>), grid, dim3(256), 0, stream, s);
        else
            hipLaunchKernelGGL((fa_mla_sparse_decode<DT, 2>), grid, dim3(256), 0, stream, s);
    });
}

int mlas_launch(const fa_mla_sparse_params *params, int dtype, void *ws, int64_t ws_bytes, hipStream_t stream) {
    const int rc = mlas_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_params &p = params->base;
    MlaSparseArgs s = mlas_plan(*params);
    const int wrc = mla_bind_ws(s.m, p.batch_size, ws, ws_bytes);
    if (wrc != FA_OK) return wrc;
    if (p.batch_size == 0) return FA_OK;
    mla_fill_args(s.m, p);  // (kv_rs in 16-bit elements)
    s.indices = params->indices;
    s.idx_bs = params->indices_batch_stride, s.idx_ss = params->indices_seqlen_stride;
    s.page_size = (int)p.page_size;
    s.page_shift = (p.page_size & (p.page_size - 1)) == 0 ? __builtin_ctzll((unsigned long long)p.page_size) : -1;
    const int64_t units = mlas_units(p, s);
    return dtype == FA_DTYPE_F16 ? mlas_launch_kernels<F16>(s, units, stream)
                                 : mlas_launch_kernels<BF16>(s, units, stream);
}

}  // namespace
}  // namespace fa

extern "C" int fa_mla_sparse_decode_gfx950(const fa_mla_sparse_params *params, int dtype, void *workspace,
                                           int64_t workspace_bytes, void *stream) {
    return fa::mlas_launch(params, dtype, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int fa_mla_sparse_decode_gfx950_check(const fa_mla_sparse_params *params, int dtype) {
    return fa::mlas_check(params, dtype);
}
extern "C" int64_t fa_mla_sparse_decode_gfx950_ws_bytes(const fa_mla_sparse_params *params) {
    if (fa::mlas_check(params, FA_DTYPE_F16) != FA_OK) return -1;
    const fa::MlaArgs a = fa::mlas_plan(*params).m;
    return fa::mla_ws_bytes(params->base.batch_size, a.n_split, a.rows);
}
extern "C" int fa_mla_sparse_version(void) { return FA_GFX950_MLA_SPARSE_VERSION; }
