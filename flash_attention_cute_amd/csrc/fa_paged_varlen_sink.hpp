#pragma once
// fa_paged_varlen_sink.hpp -- fa_fwd_w4_paged with ragged queries AND attention sinks
// (include/fa_gfx950_paged_varlen_sink.h), gfx950.
//
// The ragged paged prefill kernel of fa_paged_varlen.hpp, compiled once more with FA_W4_SINK 1: it takes a
// PagedVarlenSinkArgs, loads sinks[q-head] where a block's q-head is decoded (a scalar load, kept in an SGPR) and,
// in the epilogue, replaces a row's 1 / L by w4_sink_inv's e / (L e + 2^(s2 - max(M, s2))) -- decode_sink_inv's
// arithmetic on this kernel's state. The key loop, the page lookup, the masks and the stores are the same tokens,
// so a head whose sink is -inf has the bits of the unsinked launch. Translation units of its own (as the window,
// LSE and sink variants of the decode): the unsinked ragged kernel never sees the macro and compiles to what it was.
#define FA_W4_PAGED 1
#define FA_W4_PAGED_VARLEN 1
#define FA_W4_SINK 1
#include "fa_paged_varlen_sink_launch.h"
#include "fa_fwd_kernels.hpp"

namespace fa {

// launch_prefill_paged_varlen's launch (fa_paged_varlen.hpp): the same grid, no workspace.
template <class DT, bool C, int kD, bool kExact>
int launch_prefill_paged_varlen_sink(const fa_fwd_params &p, const PagedVarlenSinkArgs &a, int window_left,
                                     hipStream_t stream) {
    PathArgs xa{};
    xa.window_left = window_left;
    xa.q_rng = a.varlen.cu_seqlens_q;
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
