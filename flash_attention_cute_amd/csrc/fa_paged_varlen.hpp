#pragma once
// fa_paged_varlen.hpp -- fa_fwd_w4_paged with RAGGED queries (include/fa_gfx950_paged_varlen.h), gfx950.
//
// The paged prefill kernel of fa_paged_prefill.hpp, compiled once more with FA_W4_PAGED_VARLEN 1: it takes a
// PagedVarlenArgs, and every Q block takes its rows from cu_seqlens_q (xa.q_rng, rng_hi = 1; both bounds clamped
// against total_q) where the uniform kernel takes the batch row's last seqlen_q positions. Everything else -- the
// page lookup, the tile order, the masks per sequence, the epilogue -- is the same tokens, so the output is that of
// the dense packed varlen launch on the gathered keys, bit for bit. Translation units of its own (as the window
// and LSE decode variants): the uniform paged kernel never sees the macro and compiles to what it was.
#define FA_W4_PAGED 1
#define FA_W4_PAGED_VARLEN 1
#include "fa_paged_varlen_launch.h"
#include "fa_fwd_kernels.hpp"

namespace fa {

// n_qtiles from p.seqlen_q = max_seqlen_q: q-tiles past a sequence's own rows end through the kernel's n_end = 0
// rule. Plain 256-row blocks only, as every paged launch.
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen(const fa_fwd_params &p, const PagedVarlenArgs &a, int window_left,
                                hipStream_t stream) {
    PathArgs xa{};
    xa.window_left = window_left;
    xa.q_rng = a.cu_seqlens_q;
    xa.rng_hi = 1;
    const int64_t n_qtiles = (p.seqlen_q + kBlockM - 1) / kBlockM;
    const int64_t nwg = n_qtiles * p.num_heads_q * p.batch_size;
    hipLaunchKernelGGL((fa_fwd_w4_paged<DT, C, kD, kExact>), dim3((uint32_t)w4_grid(nwg)), dim3(256), 0, stream, p,
                       (int)n_qtiles, 0, stamp_buffer(), xa, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    set_last_path(kPathW4);  // (it is that kernel: fa_debug_last_prefill_paged tells the two apart)
    set_last_zigzag(0);
    set_last_prefill_paged(true);
    return FA_OK;
}

}  // namespace fa
