#pragma once
// fa_paged_varlen_lse.hpp -- fa_fwd_w4_paged with ragged queries, attention sinks AND the softmax log-sum-exp of
// every owned row (include/fa_gfx950_paged_varlen_lse.h), gfx950.
//
// The sinked ragged paged prefill kernel of fa_paged_varlen_sink.hpp, compiled once more with FA_W4_LSE 1: it takes
// a PagedVarlenLseArgs, whose sinks may be NULL (the block's sink is then the bits of -inf, the unsinked row), and in
// the epilogue w4_sink_inv_lse hands out, beside O's factor e / L', the bits of (Ms + log2 L') ln 2 from the same Ms
// and L'. Two more stores per wave and block (one fp32 per row, the lower lane half's; a row at or past Sq_b goes out
// of the descriptor's range), which the next block's counted wait includes. The key loop, the page lookup, the masks
// and the O stores are the same tokens: O has the bits of the sinked launch, and with sinks NULL of the unsinked one.
// ONE family: translation units of its own, and every other one preprocesses to what it was.
#define FA_W4_PAGED 1
#define FA_W4_PAGED_VARLEN 1
#define FA_W4_SINK 1
#define FA_W4_LSE 1
#include "fa_paged_varlen_lse_launch.h"
#include "fa_fwd_kernels.hpp"

namespace fa {

// launch_prefill_paged_varlen's launch (fa_paged_varlen.hpp): the same grid, no workspace (so no key-split piece).
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen_lse(const fa_fwd_params &p, const PagedVarlenLseArgs &a, int window_left,
                                    hipStream_t stream) {
    PathArgs xa{};
    xa.window_left = window_left;
    xa.q_rng = a.sink.varlen.cu_seqlens_q;
    xa.rng_hi = 1;
    const int64_t n_qtiles = (p.seqlen_q + kBlockM - 1) / kBlockM;
    const int64_t nwg = n_qtiles * p.num_heads_q * p.batch_size;
    hipLaunchKernelGGL((fa_fwd_w4_paged<DT, C, kD, kExact>), dim3((uint32_t)w4_grid(nwg)), dim3(256), 0, stream, p,
                       (int)n_qtiles, 0, stamp_buffer(), xa, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    set_last_path(kPathW4);
    set_last_zigzag(0);
    set_last_prefill_paged(true);
    return FA_OK;
}

}  // namespace fa
