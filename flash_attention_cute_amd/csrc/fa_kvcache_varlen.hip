// fa_kvcache_varlen.hip -- ragged in-place KV-cache append with fused rotate-half RoPE for gfx950 (C-ABI
// fa_kvcache_append_varlen_gfx950, include/fa_gfx950_kvcache_varlen.h): the write side of one step of a
// continuous batch, beside fa_kvcache.hip (one seqlen_new per batch), which it does not change.
//
// The same HBM-bound mapping as fa_kvcache.hip -- one thread owns a chunk pair of one row (fa_kvcache_move.h:
// the same movers, so the rotation is fa_rope.hip's bit for bit) -- over the PACKED rows: the host knows
// total_new and total_q, so the grid has no empty workgroups, and a row finds its sequence by a binary search
// of the cumulative array (B + 1 int32, L2-resident). Both cumulative arrays are clamped on the device
// (n0 = clamp(cu[b], 0, total), n1 = clamp(cu[b + 1], n0, total)); a row that no sequence owns is left alone.
// A write is DROPPED when its position is past the table's capacity or its page id is outside the pool --
// never clamped. Every page term of an address is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_kvcache_varlen.h"
#include "fa_kvcache_move.h"
#include "fa_launch.h"

namespace fa {
namespace {

using namespace kvmove;

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the sequence that owns packed row `row`: the last b in [0, B) whose clamped start is <= row (the last, so
// that empty sequences in front of it are passed over); n0 / n1: its clamped bounds. false: no sequence owns
// the row (it lies before cu[0], at or past cu[B], or the array is not monotone there).
__device__ __forceinline__ bool find_seq(const int32_t *cu, const int batch, const int total, const int row, int &b,
                                         int &n0, int &n1) {
    int lo = 0, hi = batch - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (clampi(cu[mid], 0, total) <= row) lo = mid;
        else hi = mid - 1;
    }
    b = lo;
    n0 = clampi(cu[b], 0, total);
    n1 = clampi(cu[b + 1], n0, total);
    return row >= n0 && row < n1;
}

// items: [0, n_kv) K rows, [n_kv, 2 n_kv) V rows, [2 n_kv, 2 n_kv + n_q) q rows, each (packed row, h, chunk)
// row-major. Threads [0, B) of the launch also write seqlens_out (the host launches at least B threads).
template <bool kF16, int kMode>
__global__ __launch_bounds__(256) void fa_kvcache_append_varlen_kernel(const fa_kvcache_varlen_params p,
                                                                       const int64_t n_kv, const int64_t n_items,
                                                                       const int per_row) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t cap = p.max_pages * p.page_size;
    const int batch = (int)p.batch_size, total_new = (int)p.total_new, total_q = (int)p.total_q;
    if (p.seqlens_out && i < p.batch_size) {
        int64_t len = p.seqlens_k[i];
        len = len < 0 ? 0 : len > cap ? cap : len;
        int64_t n = 0;
        if (p.cu_seqlens_new) {
            const int n0 = clampi(p.cu_seqlens_new[i], 0, total_new);
            n = clampi(p.cu_seqlens_new[i + 1], n0, total_new) - n0;
        }
        const int64_t out = len + n;
        p.seqlens_out[i] = (int32_t)(out > cap ? cap : out);
    }
    if (i >= n_items) return;
    const int kind = i < n_kv ? 0 : i < 2 * n_kv ? 1 : 2;  // K, V, q
    const int64_t j = i - (kind == 0 ? 0 : kind == 1 ? n_kv : 2 * n_kv);
    const int c = (int)(j % per_row);
    const int64_t rh = j / per_row;  // (packed row, h) row-major
    const int64_t heads = kind == 2 ? p.num_heads_q : p.num_heads_kv;
    const int64_t h = rh % heads;
    const int row = (int)(rh / heads);

    int b, r0, r1;
    if (!find_seq(kind == 2 ? p.cu_seqlens_q : p.cu_seqlens_new, batch, kind == 2 ? total_q : total_new, row, b, r0,
                  r1))
        return;  // a row of no sequence: left alone
    const int64_t s = row - r0;
    int64_t len = p.seqlens_k[b];
    len = len < 0 ? 0 : len > cap ? cap : len;

    const uint16_t *x;
    uint16_t *o;
    int64_t pos;
    if (kind == 2) {
        int64_t n_new = 0;
        if (p.cu_seqlens_new) {
            const int n0 = clampi(p.cu_seqlens_new[b], 0, total_new);
            n_new = clampi(p.cu_seqlens_new[b + 1], n0, total_new) - n0;
        }
        const int64_t end = len + n_new > cap ? cap : len + n_new;  // seqlens_out[b], recomputed
        pos = end - (r1 - r0) + s;
        pos = pos < 0 ? 0 : pos;
        x = (const uint16_t *)p.q + (int64_t)row * p.q_row_stride + h * p.q_head_stride;
        o = (uint16_t *)p.q_out + (int64_t)row * p.qo_row_stride + h * p.qo_head_stride;
    } else {
        pos = len + s;
        if (pos >= cap) return;  // past the table's capacity: dropped
        const int64_t page = p.block_table[(int64_t)b * p.block_table_stride + pos / p.page_size];
        if (page < 0 || page >= p.num_pages) return;  // outside the pool: dropped, never clamped
        const int64_t r = pos % p.page_size;
        if (kind == 0) {
            x = (const uint16_t *)p.k_new + (int64_t)row * p.kn_row_stride + h * p.kn_head_stride;
            o = (uint16_t *)p.k_cache + page * p.k_page_stride + h * p.k_head_stride + r * p.k_row_stride;
        } else {
            x = (const uint16_t *)p.v_new + (int64_t)row * p.vn_row_stride + h * p.vn_head_stride;
            o = (uint16_t *)p.v_cache + page * p.v_page_stride + h * p.v_head_stride + r * p.v_row_stride;
        }
    }
    const uint16_t *cs = nullptr, *sn = nullptr;
    if (kind != 1 && p.cos) {
        pos = pos > p.max_pos - 1 ? p.max_pos - 1 : pos;  // a table shorter than the position: its last row
        cs = (const uint16_t *)p.cos + pos * p.cs_row_stride;
        sn = (const uint16_t *)p.sin + pos * p.cs_row_stride;
    }
    if constexpr (kMode == kVec) {
        const int d0 = c * 8;
        move_vec<kF16>(x, o, cs, sn, d0, d0 + (int)p.headdim / 2);
    } else if constexpr (kMode == kPair) {
        move_pair<kF16>(x, o, cs, sn, c, c + (int)p.headdim / 2);
    } else {
        o[c] = x[c];
    }
}

// the 16-B path needs every chunk of every tensor the launch touches 16-B aligned
int pick_mode(const fa_kvcache_varlen_params &p) {
    bool vec = p.headdim % 16 == 0;
    if (p.total_new > 0)
        vec = vec && vec_ok({p.kn_row_stride, p.kn_head_stride, p.vn_row_stride, p.vn_head_stride, p.k_page_stride,
                             p.k_head_stride, p.k_row_stride, p.v_page_stride, p.v_head_stride, p.v_row_stride},
                            {p.k_new, p.v_new, p.k_cache, p.v_cache});
    if (p.total_q > 0)
        vec = vec && vec_ok({p.q_row_stride, p.q_head_stride, p.qo_row_stride, p.qo_head_stride}, {p.q, p.q_out});
    if (p.cos) vec = vec && vec_ok({p.cs_row_stride}, {p.cos, p.sin});
    return mode_of(vec, p.headdim);
}

int check(const fa_kvcache_varlen_params *p, int dtype) {
    if (!p) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return set_err(FA_ERR_UNSUPPORTED, "the ragged KV-cache append supports fp16 / bf16 only (dtype %d)", dtype);
    if (!p->seqlens_k) return set_err(FA_ERR_INVALID_ARGUMENT, "seqlens_k must be non-NULL");
    if (!p->block_table)
        return set_err(FA_ERR_UNSUPPORTED, "the ragged append writes paged caches only: block_table must be non-NULL "
                                           "(a dense cache: fa_kvcache_append_gfx950 per chunk length)");
    if (((uintptr_t)p->block_table & 3) || ((uintptr_t)p->seqlens_k & 3) || ((uintptr_t)p->seqlens_out & 3) ||
        ((uintptr_t)p->cu_seqlens_new & 3) || ((uintptr_t)p->cu_seqlens_q & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table, seqlens_k, seqlens_out, cu_seqlens_new and cu_seqlens_q "
                                                "must be 4-byte aligned int32 arrays");
    if (p->batch_size < 0 || p->total_new < 0 || p->total_q < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "batch_size, total_new and total_q must be non-negative");
    if (p->num_heads_kv < 1 || p->headdim < 1)
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_heads_kv and headdim must be at least 1");
    if (p->page_size <= 0 || p->page_size % kDecKeys != 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "page_size (%lld) must be a positive multiple of %d",
                       (long long)p->page_size, kDecKeys);
    if (p->max_pages < 1 || p->num_pages < 1)
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_pages and max_pages must be at least 1");
    if (p->num_pages > 0x7fffffffLL || p->max_pages > 0x3fffffffLL / p->page_size || p->batch_size >= 0x7fffffffLL ||
        p->total_new > 0x7fffffffLL || p->total_q > 0x7fffffffLL || p->headdim > 0x7fffffffLL ||
        p->num_heads_kv > 0x7fffffffLL || p->num_heads_q > 0x7fffffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "page pool, block table or problem too large");
    if (p->block_table_stride < 0 || (p->batch_size > 1 && p->block_table_stride < p->max_pages))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table_stride must be at least max_pages");
    if ((p->total_new > 0) != (p->k_new != nullptr) || (p->total_new > 0) != (p->v_new != nullptr))
        return set_err(FA_ERR_INVALID_ARGUMENT, "k_new and v_new must both be given, or total_new must be 0");
    if (p->total_new > 0 && !p->cu_seqlens_new)
        return set_err(FA_ERR_INVALID_ARGUMENT, "cu_seqlens_new must be non-NULL when total_new > 0");
    if (p->total_new > 0 && (!p->k_cache || !p->v_cache))
        return set_err(FA_ERR_INVALID_ARGUMENT, "k_cache and v_cache must be non-NULL");
    if ((p->cos != nullptr) != (p->sin != nullptr))
        return set_err(FA_ERR_INVALID_ARGUMENT, "cos and sin must be given together");
    if ((p->total_q > 0) != (p->q != nullptr) || (p->total_q > 0) != (p->q_out != nullptr))
        return set_err(FA_ERR_INVALID_ARGUMENT, "q and q_out must both be given, or total_q must be 0");
    if (p->total_q > 0) {
        if (!p->cu_seqlens_q) return set_err(FA_ERR_INVALID_ARGUMENT, "cu_seqlens_q must be non-NULL when total_q > 0");
        if (!p->cos) return set_err(FA_ERR_INVALID_ARGUMENT, "q is rotated only: it needs the cos / sin tables");
        if (p->num_heads_q < 1 || p->num_heads_q % p->num_heads_kv != 0)
            return set_err(FA_ERR_INVALID_ARGUMENT,
                           "num_heads_q (%lld) must be a positive multiple of num_heads_kv (%lld)",
                           (long long)p->num_heads_q, (long long)p->num_heads_kv);
    }
    if (const int rc = kvmove::check_tables_and_lengths(p->cos, p->headdim, p->max_pos, p->seqlens_k,
                                                        p->seqlens_out, p->batch_size))
        return rc;
    // one thread per item (at most headdim per row), 256 per workgroup, a 1-D grid
    if ((2.0 * p->num_heads_kv * p->total_new + (double)p->num_heads_q * p->total_q) * (double)p->headdim >
        0x7fffffffLL * 256.0)
        return set_err(FA_ERR_UNSUPPORTED, "too many rows for one launch");
    return set_err(FA_OK, "%s", "");
}

int launch(const fa_kvcache_varlen_params *p, int dtype, hipStream_t stream) {
    const int rc = check(p, dtype);
    if (rc != FA_OK) return rc;
    if (p->batch_size == 0) return FA_OK;
    const int mode = pick_mode(*p);
    const int per_row = per_row_of(p->headdim, mode);
    const int64_t n_kv = p->num_heads_kv * p->total_new * per_row;
    const int64_t items = 2 * n_kv + p->num_heads_q * p->total_q * per_row;
    const int64_t threads = items > p->batch_size ? items : p->batch_size;  // (seqlens_out: one thread per b)
    const dim3 grid((uint32_t)((threads + 255) / 256));
#define FA_KV_LAUNCH(F16, MODE)                                                                                  \
    hipLaunchKernelGGL((fa_kvcache_append_varlen_kernel<F16, MODE>), grid, dim3(256), 0, stream, *p, n_kv, items, \
                       per_row)
    if (dtype == FA_DTYPE_F16) {
        if (mode == kVec) FA_KV_LAUNCH(true, kVec);
        else if (mode == kPair) FA_KV_LAUNCH(true, kPair);
        else FA_KV_LAUNCH(true, kElem);
    } else {
        if (mode == kVec) FA_KV_LAUNCH(false, kVec);
        else if (mode == kPair) FA_KV_LAUNCH(false, kPair);
        else FA_KV_LAUNCH(false, kElem);
    }
#undef FA_KV_LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_LAUNCH, "HIP launch failed: %s", hipGetErrorString(e));
    return FA_OK;
}

}  // namespace
}  // namespace fa

extern "C" int fa_kvcache_append_varlen_gfx950(const fa_kvcache_varlen_params *params, int dtype, void *stream) {
    return fa::launch(params, dtype, (hipStream_t)stream);
}

extern "C" int fa_kvcache_append_varlen_gfx950_check(const fa_kvcache_varlen_params *params, int dtype) {
    return fa::check(params, dtype);
}

extern "C" int fa_kvcache_varlen_version(void) { return FA_GFX950_KVCACHE_VARLEN_VERSION; }
