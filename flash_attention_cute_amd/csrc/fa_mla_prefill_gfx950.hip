// fa_mla_prefill_gfx950.hip -- C-ABI of the MLA prefill attention over packed sequences
// (include/fa_gfx950_mla_prefill.h): the checks, the plan (which row-block variant of fa_mla_prefill,
// fa_mla_prefill.hpp, and its grid), the launch and the entries, both dtypes. A translation unit of its own beside
// the dispatchers (whose error channel it uses through fa_launch.h); no other file references its kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_mla_prefill.hpp"

namespace fa {
namespace {

// The plan: 256-row workgroups (two row blocks per wave: every K / V fragment read from LDS feeds two MFMAs)
// unless no sequence has more than 128 query rows, where the second row block would be empty registers.
constexpr int kMpSmallRows = 4 * kDecRows;

int mp_check(const fa_mla_prefill_params *p, int dtype) {
    if (!p) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return set_err(FA_ERR_UNSUPPORTED, "MLA prefill supports fp16 / bf16 only (dtype %d)", dtype);
    if (p->headdim_qk != kMpDqk || p->headdim_v != kMpDv)
        return set_err(FA_ERR_UNSUPPORTED,
                       "MLA prefill is built for head dims (headdim_qk, headdim_v) = (192, 128) only (got (%lld, %lld))",
                       (long long)p->headdim_qk, (long long)p->headdim_v);
    if (!p->q_ptr || !p->k_nope_ptr || !p->k_rope_ptr || !p->v_ptr || !p->o_ptr)
        return set_err(FA_ERR_INVALID_ARGUMENT, "q_ptr, k_nope_ptr, k_rope_ptr, v_ptr and o_ptr must be non-NULL");
    if (!p->cu_seqlens_q || !p->cu_seqlens_k)
        return set_err(FA_ERR_INVALID_ARGUMENT, "cu_seqlens_q and cu_seqlens_k must be non-NULL");
    if (((uintptr_t)p->cu_seqlens_q & 3) || ((uintptr_t)p->cu_seqlens_k & 3) || ((uintptr_t)p->lse_ptr & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "cu_seqlens_q, cu_seqlens_k and lse_ptr must be 4-byte aligned");
    if (p->batch_size < 0 || p->total_q < 0 || p->total_k < 0 || p->max_seqlen_q < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "batch_size, total_q, total_k and max_seqlen_q must be non-negative");
    if (p->num_heads_q < 1 || p->num_heads_kv < 1 || p->num_heads_q % p->num_heads_kv != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_heads_q (%lld) must be a positive multiple of num_heads_kv (%lld)",
                       (long long)p->num_heads_q, (long long)p->num_heads_kv);
    if (p->batch_size > 0xffffLL || p->num_heads_q > 0xffffLL || p->total_q > 0x3fffffffLL ||
        p->total_k > 0x3fffffffLL || p->max_seqlen_q > 0x3fffffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "batch_size, num_heads_q, total_q, total_k or max_seqlen_q too large");
    if (p->batch_size * p->num_heads_q * ((p->max_seqlen_q + kMpSmallRows - 1) / kMpSmallRows) > 0x0fffffffLL)
        return set_err(FA_ERR_UNSUPPORTED,
                       "too many row blocks (batch_size * num_heads_q * ceil(max_seqlen_q / 128) above 2^28)");
    if (((uintptr_t)p->q_ptr & 15) || ((uintptr_t)p->k_nope_ptr & 15) || ((uintptr_t)p->k_rope_ptr & 15) ||
        ((uintptr_t)p->v_ptr & 15) || ((uintptr_t)p->o_ptr & 15))
        return set_err(FA_ERR_INVALID_ARGUMENT, "q_ptr, k_nope_ptr, k_rope_ptr, v_ptr and o_ptr must be 16-byte aligned");
    const int64_t st[10] = {p->q_row_stride,      p->q_head_stride,      p->k_nope_row_stride, p->k_nope_head_stride,
                            p->k_rope_row_stride, p->k_rope_head_stride, p->v_row_stride,      p->v_head_stride,
                            p->o_row_stride,      p->o_head_stride};
    const char *const st_name[10] = {"q_row_stride",      "q_head_stride",      "k_nope_row_stride", "k_nope_head_stride",
                                     "k_rope_row_stride", "k_rope_head_stride", "v_row_stride",      "v_head_stride",
                                     "o_row_stride",      "o_head_stride"};
    for (int i = 0; i < 10; ++i)
        if (st[i] < 0 || st[i] % 8 != 0)
            return set_err(FA_ERR_INVALID_ARGUMENT, "%s (%lld) must be a non-negative multiple of 8 elements", st_name[i],
                           (long long)st[i]);
    // a tile's descriptor ends (rows - 1) * stride + width elements in: a narrower row stride would let the rows
    // past a sequence's end alias the rows inside it
    if (p->k_nope_row_stride < kMpNope || p->k_rope_row_stride < kMpRope || p->v_row_stride < kMpDv)
        return set_err(FA_ERR_INVALID_ARGUMENT,
                       "k_nope_row_stride, k_rope_row_stride and v_row_stride must be at least 128, 64 and 128");
    if (p->k_nope_row_stride > (1LL << 23) || p->k_rope_row_stride > (1LL << 23) || p->v_row_stride > (1LL << 23))
        return set_err(FA_ERR_UNSUPPORTED, "k_nope_row_stride, k_rope_row_stride or v_row_stride too large");
    if (p->lse_head_stride < 0 || p->lse_row_stride < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "lse_head_stride and lse_row_stride must be non-negative");
    uint32_t sc_bits;  // (on the bits: the build is -ffinite-math-only, under which a float test may drop NaN and inf)
    __builtin_memcpy(&sc_bits, &p->softmax_scale, sizeof sc_bits);
    if (sc_bits == 0 || sc_bits >= 0x7f800000u)  // +0, any negative value, +inf, NaN
        return set_err(FA_ERR_INVALID_ARGUMENT, "softmax_scale must be finite and > 0");
    return FA_OK;
}

template <class DT>
int mp_launch_kernel(const MlaPrefillArgs &a, const int rows, hipStream_t stream) {
    const dim3 grid((uint32_t)(8 * a.per));
    if (rows == kMpSmallRows)
        hipLaunchKernelGGL((fa_mla_prefill<DT, 1>), grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((fa_mla_prefill<DT, 2>), grid, dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

int mp_launch(const fa_mla_prefill_params *params, int dtype, hipStream_t stream) {
    const int rc = mp_check(params, dtype);
    if (rc != FA_OK) return rc;
    const fa_mla_prefill_params &p = *params;
    if (p.batch_size == 0 || p.total_q == 0 || p.max_seqlen_q == 0) return FA_OK;
    MlaPrefillArgs a{};
    a.q = (const char *)p.q_ptr, a.kn = (const char *)p.k_nope_ptr, a.kr = (const char *)p.k_rope_ptr;
    a.v = (const char *)p.v_ptr, a.o = (char *)p.o_ptr, a.lse = p.lse_ptr;
    a.cu_q = p.cu_seqlens_q, a.cu_k = p.cu_seqlens_k;
    a.q_rs = p.q_row_stride, a.q_hs = p.q_head_stride, a.o_rs = p.o_row_stride, a.o_hs = p.o_head_stride;
    a.kn_rs = (int)p.k_nope_row_stride, a.kn_hs = p.k_nope_head_stride;
    a.kr_rs = (int)p.k_rope_row_stride, a.kr_hs = p.k_rope_head_stride;
    a.v_rs = (int)p.v_row_stride, a.v_hs = p.v_head_stride;
    a.lse_hs = p.lse_head_stride, a.lse_rs = p.lse_row_stride;
    a.total_q = (int)p.total_q, a.total_k = (int)p.total_k;
    a.g = (int)(p.num_heads_q / p.num_heads_kv), a.causal = p.causal != 0;
    a.sc = p.softmax_scale;
    // the plan: one item per (sequence, q-head, row block), dealt to the 8 XCDs as contiguous ranges of a.per items
    const int rows = p.max_seqlen_q <= kMpSmallRows ? kMpSmallRows : 2 * kMpSmallRows;
    a.hq = (int)p.num_heads_q;
    a.n_blk = (int)((p.max_seqlen_q + rows - 1) / rows);
    a.n_items = (int)(p.batch_size * p.num_heads_q * a.n_blk);
    a.per = (a.n_items + 7) / 8;
    return dtype == FA_DTYPE_F16 ? mp_launch_kernel<F16>(a, rows, stream) : mp_launch_kernel<BF16>(a, rows, stream);
}

}  // namespace
}  // namespace fa

extern "C" int fa_mla_prefill_gfx950(const fa_mla_prefill_params *params, int dtype, void *stream) {
    return fa::mp_launch(params, dtype, (hipStream_t)stream);
}
extern "C" int fa_mla_prefill_gfx950_check(const fa_mla_prefill_params *params, int dtype) {
    return fa::mp_check(params, dtype);
}
extern "C" int fa_mla_prefill_version(void) { return FA_GFX950_MLA_PREFILL_VERSION; }
