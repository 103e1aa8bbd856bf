// fa_mla_sparse_gfx950.hip -- C-ABI of the sparse MLA decode over top-k token indices of the paged latent KV cache
// (include/fa_gfx950_mla_sparse.h): the checks (the dense entry's, then the list's own), the split plan, the
// launches of fa_mla_sparse_decode (fa_mla_sparse.hpp) / fa_mla_combine (fa_mla_decode.hpp) for both dtypes, and
// the entries. A translation unit of its own; no other file references its kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_mla_sparse.hpp"

namespace fa {
namespace {

// The plan: split s takes tiles s, s + n_split, ... of a list's topk / 32 tiles, a count that is the same for
// every (batch, position): the split count makes the workgroups about kMlaTargetWgs, each split at least
// kMlaSparseMinTilesPerSplit tiles, at most kMlaMaxSplit -- or what num_splits forces.
MlaSparseArgs mlas_plan(const fa_mla_sparse_params &v) {
    const fa_mla_params &p = v.base;
    MlaSparseArgs s{};
    s.Hq = (int)p.num_heads_q;
    s.n_tiles = (int)(v.topk / kDecKeys);
    s.m.rows = (int)(p.num_heads_q * p.seqlen_q);
    s.m.n_rg = (s.Hq + kMlaGroupRows - 1) / kMlaGroupRows;
    const int64_t wgs = (p.batch_size > 0 ? p.batch_size : 1) * p.seqlen_q * s.m.n_rg;
    int64_t ns = (kMlaTargetWgs + wgs - 1) / wgs;
    const int64_t by_len = s.n_tiles / kMlaSparseMinTilesPerSplit;
    ns = ns < by_len ? ns : by_len;
    if (p.num_splits > 0) ns = p.num_splits;
    ns = ns < kMlaMaxSplit ? ns : kMlaMaxSplit;
    s.m.n_split = (int)(ns < 1 ? 1 : ns);
    return s;
}

// workgroups of the plan: the (b, pos, split) units rounded up to whole sets of 8 ids, times the head groups
int64_t mlas_grid(const fa_mla_params &p, const MlaSparseArgs &s) {
    const int64_t units = p.batch_size * p.seqlen_q * s.m.n_split;
    return 8 * ((units + 7) / 8) * s.m.n_rg;
}

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
    if (mlas_grid(v->base, mlas_plan(*v)) > 0x7fffffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "batch * seqlen_q * splits * head groups too large for one launch");
    return FA_OK;
}

int64_t mlas_ws_bytes(const fa_mla_params &p, const MlaSparseArgs &s) {
    return s.m.n_split > 1 ? p.batch_size * s.m.n_split * s.m.rows * (int64_t)(kMlaDv * 4 + 4) : 0;
}

template <class DT>
void mlas_launch_kernels(const MlaSparseArgs &s, const uint32_t grid, hipStream_t stream) {
    if (s.Hq <= kDecRows)  // one row block: the kernel without the second block's registers
        hipLaunchKernelGGL((fa_mla_sparse_decode<DT, 1>), dim3(grid), dim3(256), 0, stream, s);
    else
        hipLaunchKernelGGL((fa_mla_sparse_decode<DT, 2>), dim3(grid), dim3(256), 0, stream, s);
    if (s.m.n_split > 1)
        hipLaunchKernelGGL((fa_mla_combine<DT>), dim3((uint32_t)(4 * s.m.batch * s.m.rows)), dim3(256), 0, stream,
                           s.m);
}

int mlas_launch(const fa_mla_sparse_params *params, int dtype, void *ws, int64_t ws_bytes, hipStream_t stream) {
    const int rc = mlas_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_params &p = params->base;
    MlaSparseArgs s = mlas_plan(*params);
    MlaArgs &a = s.m;
    const int64_t need = mlas_ws_bytes(p, s);
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
    a.kv_ps = p.kv_page_stride, a.kv_rs = (int)p.kv_row_stride;
    a.batch = (int)p.batch_size, a.Sq = (int)p.seqlen_q;
    a.num_pages = (int)p.num_pages, a.tiles_per_page = (int)(p.page_size / kDecKeys);
    a.cap_keys = (int)(p.max_pages * p.page_size), a.bt_stride = (int)p.block_table_stride;
    a.causal = p.causal != 0 && p.seqlen_q > 1;
    a.sc = p.softmax_scale;
    s.indices = params->indices;
    s.idx_bs = params->indices_batch_stride, s.idx_ss = params->indices_seqlen_stride;
    s.page_size = (int)p.page_size;
    s.page_shift = (p.page_size & (p.page_size - 1)) == 0 ? __builtin_ctzll((unsigned long long)p.page_size) : -1;
    if (need > 0) {
        a.ws_o = (float *)ws;
        a.ws_lse = (float *)((char *)ws + p.batch_size * a.n_split * a.rows * (int64_t)(kMlaDv * 4));
    }
    const uint32_t grid = (uint32_t)mlas_grid(p, s);
    if (dtype == FA_DTYPE_F16) mlas_launch_kernels<F16>(s, grid, stream);
    else mlas_launch_kernels<BF16>(s, grid, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
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
    return fa::mlas_ws_bytes(params->base, fa::mlas_plan(*params));
}
extern "C" int fa_mla_sparse_version(void) { return FA_GFX950_MLA_SPARSE_VERSION; }
