#pragma once
// fa_mla_host.h -- the host layer the three MLA decode entries share (fa_mla_gfx950.hip, fa_mla_fp8_gfx950.hip,
// fa_mla_sparse_gfx950.hip): fa_mla_params narrowed into MlaArgs, the split rule, the workspace contract (size,
// check, ws_o / ws_lse) and the launch (grid rule, fa_mla_combine, the launch-error tail). Each file keeps its own
// checks, its kernel selection and its entries; the error channel is fa_launch.h's.
#include "fa_mla_decode.hpp"

namespace fa {

// fa_mla_params narrowed to what the device reads; the plan (rows, n_rg, n_split) and the workspace are the
// caller's. kv_ps / kv_rs are counted in the pool's elements.
inline void mla_fill_args(MlaArgs &a, const fa_mla_params &p) {
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
}

// The split rule: the split count makes the workgroups about kMlaTargetWgs (wgs: the workgroups of one split),
// each split at least min_tiles of the n_tiles, at most kMlaMaxSplit -- or what num_splits forces.
inline int mla_splits(const int64_t wgs, const int64_t n_tiles, const int min_tiles, const int64_t num_splits) {
    int64_t ns = (kMlaTargetWgs + wgs - 1) / wgs;
    const int64_t by_len = n_tiles / min_tiles;
    ns = ns < by_len ? ns : by_len;
    if (num_splits > 0) ns = num_splits;
    ns = ns < kMlaMaxSplit ? ns : kMlaMaxSplit;
    return (int)(ns < 1 ? 1 : ns);
}

// The plan of the dense entries (16-bit and FP8 pool: one plan, so one workspace): a workgroup per (batch, split,
// group of kMlaGroupRows of the Hq * Sq rows), every split an equal share of each sequence's tiles (the kernel's
// t_lo rule), counted over the table's capacity.
inline MlaArgs mla_plan(const fa_mla_params &p) {
    MlaArgs a{};
    a.rows = (int)(p.num_heads_q * p.seqlen_q);
    a.n_rg = (a.rows + kMlaGroupRows - 1) / kMlaGroupRows;
    a.n_split = mla_splits((p.batch_size > 0 ? p.batch_size : 1) * a.n_rg, p.max_pages * p.page_size / kDecKeys,
                           kMlaMinTilesPerSplit, p.num_splits);
    return a;
}

// The workspace: per (batch, split, row) 512 fp32 of O / l and one fp32 lse; none for one split.
inline int64_t mla_ws_bytes(const int64_t batch, const int n_split, const int rows) {
    return n_split > 1 ? batch * n_split * rows * (int64_t)(kMlaDv * 4 + 4) : 0;
}

// checks the caller's workspace against the plan in `a` and points ws_o / ws_lse into it
inline int mla_bind_ws(MlaArgs &a, const int64_t batch, void *ws, const int64_t ws_bytes) {
    const int64_t need = mla_ws_bytes(batch, a.n_split, a.rows);
    if (need > 0 && (!ws || ws_bytes < need))
        return set_err(FA_ERR_INVALID_ARGUMENT, "workspace of %lld bytes is smaller than the %lld required",
                       (long long)(ws ? ws_bytes : 0), (long long)need);
    if ((uintptr_t)ws & 15) return set_err(FA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
    if (need > 0) {
        a.ws_o = (float *)ws;
        a.ws_lse = (float *)((char *)ws + batch * a.n_split * a.rows * (int64_t)(kMlaDv * 4));
    }
    return FA_OK;
}

// workgroups of a decode launch: the units (one per split and whatever shares its tiles) rounded up to whole sets
// of 8 ids, times the n_rg groups that re-read them (ids congruent mod 8: one XCD)
inline int64_t mla_grid(const int64_t units, const int n_rg) { return 8 * ((units + 7) / 8) * n_rg; }

// The launch: `decode(grid)` launches the caller's decode kernel, then the merge of the splits, then the error tail.
template <class DT, class Decode>
int mla_run(const MlaArgs &a, const int64_t units, hipStream_t stream, Decode decode) {
    decode(dim3((uint32_t)mla_grid(units, a.n_rg)));
    if (a.n_split > 1)
        hipLaunchKernelGGL((fa_mla_combine<DT>), dim3((uint32_t)(4 * a.batch * a.rows)), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

}  // namespace fa
