// fa_kvcache.hip -- in-place KV-cache append with fused rotate-half RoPE for gfx950 (C-ABI
// fa_kvcache_append_gfx950, include/fa_gfx950_kvcache.h): the write side of the paged / dense cache.
//
// One launch writes the new K rows (rotated at their positions) and V rows into the pages the block
// table names, rotates q at the sequence's last positions and advances the lengths -- what a caller
// otherwise composes from a cos / sin gather, two fa_rope launches, the (page, row) arithmetic, two
// index_put_ and an add. No reference counterpart (the reference has no KV cache).
//
// HBM-bound with no reuse: like fa_rope_kernel one thread owns an 8-element chunk of the first half of
// a row and its partner in the second half (16-B loads and plain 16-B stores), consecutive lanes take
// consecutive chunks, then consecutive rows. The rotation is fa_rope.hip's arithmetic, bit for bit:
// fma(x, cos, rot * sin) in fp32 behind the same pin, one RNE rounding. A write is DROPPED when its
// position is past the table's capacity or its page id is outside the pool -- never clamped (the
// header says why). Every page term of an address is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_gfx950_kvcache.h"
#include "fa_kvcache_move.h"
#include "fa_launch.h"

namespace fa {
namespace {

// ld / st / pack2, Mode, move_vec, move_pair: fa_kvcache_move.h, shared with fa_kvcache_varlen.hip. The movers
// keep fa_rope.hip's fp32 pin there, the line
//     asm volatile("" : "+v"(a), "+v"(bb));
// between the fma and the one rounding (without it hipcc folds the step into a mixed-precision fma).
// KEEP THE QUOTED LINE: tests/test_kvcache_abi.py (test_kvcache_source_is_a_translation_unit_of_its_own) looks for
// it in THIS file, as it did when the movers were defined here. Since they moved, that assertion checks this
// comment and no longer code; the code is checked by tests/test_kvcache_varlen_abi.py
// (test_both_append_kernels_share_one_definition_of_the_movers) and, bit for bit, by the GPU append tests.
using namespace kvmove;

// items: [0, n_kv) K rows, [n_kv, 2 n_kv) V rows, [2 n_kv, 2 n_kv + n_q) q rows, each (b, h, s, chunk)
// row-major. Threads [0, B) of the launch also write seqlens_out (the launch has at least B items).
template <bool kF16, int kMode>
__global__ __launch_bounds__(256) void fa_kvcache_append_kernel(const fa_kvcache_params p, const int64_t n_kv,
                                                                const int64_t n_items, const int per_row) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int64_t cap = p.max_pages * p.page_size;
    if (p.seqlens_out && i < p.batch_size) {
        int64_t len = p.seqlens_k[i];
        len = len < 0 ? 0 : len > cap ? cap : len;
        const int64_t out = len + p.seqlen_new;
        p.seqlens_out[i] = (int32_t)(out > cap ? cap : out);
    }
    const int kind = i < n_kv ? 0 : i < 2 * n_kv ? 1 : 2;  // K, V, q
    const int64_t j = i - (kind == 0 ? 0 : kind == 1 ? n_kv : 2 * n_kv);
    const int c = (int)(j % per_row);
    const int64_t row = j / per_row;  // (b, h, s) row-major
    const int64_t rows_s = kind == 2 ? p.seqlen_q : p.seqlen_new;
    const int64_t heads = kind == 2 ? p.num_heads_q : p.num_heads_kv;
    const int64_t s = row % rows_s, bh = row / rows_s;
    const int64_t h = bh % heads, b = bh / heads;
    int64_t len = p.seqlens_k[b];
    len = len < 0 ? 0 : len > cap ? cap : len;

    const uint16_t *x;
    uint16_t *o;
    int64_t pos;
    if (kind == 2) {
        const int64_t end = len + p.seqlen_new > cap ? cap : len + p.seqlen_new;  // seqlens_out[b], recomputed
        pos = end - p.seqlen_q + s;
        pos = pos < 0 ? 0 : pos;
        x = (const uint16_t *)p.q + b * p.q_batch_stride + h * p.q_head_stride + s * p.q_seqlen_stride;
        o = (uint16_t *)p.q_out + b * p.qo_batch_stride + h * p.qo_head_stride + s * p.qo_seqlen_stride;
    } else {
        pos = len + s;
        if (pos >= cap) return;  // past the table's capacity: dropped
        int64_t page = b;
        if (p.block_table) {
            page = p.block_table[b * p.block_table_stride + pos / p.page_size];
            if (page < 0 || page >= p.num_pages) return;  // outside the pool: dropped, never clamped
        }
        const int64_t r = pos % p.page_size;
        if (kind == 0) {
            x = (const uint16_t *)p.k_new + b * p.kn_batch_stride + h * p.kn_head_stride + s * p.kn_seqlen_stride;
            o = (uint16_t *)p.k_cache + page * p.k_page_stride + h * p.k_head_stride + r * p.k_row_stride;
        } else {
            x = (const uint16_t *)p.v_new + b * p.vn_batch_stride + h * p.vn_head_stride + s * p.vn_seqlen_stride;
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
int pick_mode(const fa_kvcache_params &p) {
    bool vec = p.headdim % 16 == 0;
    if (p.seqlen_new > 0)
        vec = vec && vec_ok({p.kn_batch_stride, p.kn_head_stride, p.kn_seqlen_stride, p.vn_batch_stride,
                             p.vn_head_stride, p.vn_seqlen_stride, p.k_page_stride, p.k_head_stride, p.k_row_stride,
                             p.v_page_stride, p.v_head_stride, p.v_row_stride},
                            {p.k_new, p.v_new, p.k_cache, p.v_cache});
    if (p.seqlen_q > 0)
        vec = vec && vec_ok({p.q_batch_stride, p.q_head_stride, p.q_seqlen_stride, p.qo_batch_stride,
                             p.qo_head_stride, p.qo_seqlen_stride},
                            {p.q, p.q_out});
    if (p.cos) vec = vec && vec_ok({p.cs_row_stride}, {p.cos, p.sin});
    return mode_of(vec, p.headdim);
}

}  // namespace

int kvcache_check(const fa_kvcache_params *p, int dtype) {
    if (!p) return set_err(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    if (dtype != FA_DTYPE_F16 && dtype != FA_DTYPE_BF16)
        return set_err(FA_ERR_UNSUPPORTED, "the KV-cache append supports fp16 / bf16 only (dtype %d)", dtype);
    if (!p->seqlens_k) return set_err(FA_ERR_INVALID_ARGUMENT, "seqlens_k must be non-NULL");
    if (((uintptr_t)p->block_table & 3) || ((uintptr_t)p->seqlens_k & 3) || ((uintptr_t)p->seqlens_out & 3))
        return set_err(FA_ERR_INVALID_ARGUMENT,
                       "block_table, seqlens_k and seqlens_out must be 4-byte aligned int32 arrays");
    if (p->batch_size < 0 || p->seqlen_new < 0 || p->seqlen_q < 0)
        return set_err(FA_ERR_INVALID_ARGUMENT, "batch_size, seqlen_new and seqlen_q must be non-negative");
    if (p->num_heads_kv < 1 || p->headdim < 1)
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_heads_kv and headdim must be at least 1");
    if (p->page_size <= 0 || (p->block_table && p->page_size % kDecKeys != 0))
        return set_err(FA_ERR_INVALID_ARGUMENT, "page_size (%lld) must be a positive multiple of %d%s",
                       (long long)p->page_size, kDecKeys, p->block_table ? "" : " (dense cache: positive)");
    if (p->max_pages < 1 || (p->block_table && p->num_pages < 1))
        return set_err(FA_ERR_INVALID_ARGUMENT, "num_pages and max_pages must be at least 1");
    if (!p->block_table && p->max_pages != 1)
        return set_err(FA_ERR_INVALID_ARGUMENT, "a dense cache (block_table NULL) has max_pages 1");
    if ((p->block_table && p->num_pages > 0x7fffffffLL) || p->max_pages > 0x3fffffffLL / p->page_size || p->batch_size > 0x7fffffffLL ||
        p->seqlen_new > 0x3fffffffLL || p->seqlen_q > 0x3fffffffLL || p->headdim > 0x7fffffffLL ||
        p->num_heads_kv > 0x7fffffffLL || p->num_heads_q > 0x7fffffffLL)
        return set_err(FA_ERR_UNSUPPORTED, "page pool, block table or problem too large");
    if (p->block_table && (p->block_table_stride < 0 || (p->batch_size > 1 && p->block_table_stride < p->max_pages)))
        return set_err(FA_ERR_INVALID_ARGUMENT, "block_table_stride must be at least max_pages");
    if ((p->seqlen_new > 0) != (p->k_new != nullptr) || (p->seqlen_new > 0) != (p->v_new != nullptr))
        return set_err(FA_ERR_INVALID_ARGUMENT, "k_new and v_new must both be given, or seqlen_new must be 0");
    if (p->seqlen_new > 0 && (!p->k_cache || !p->v_cache))
        return set_err(FA_ERR_INVALID_ARGUMENT, "k_cache and v_cache must be non-NULL");
    if ((p->cos != nullptr) != (p->sin != nullptr))
        return set_err(FA_ERR_INVALID_ARGUMENT, "cos and sin must be given together");
    if ((p->seqlen_q > 0) != (p->q != nullptr) || (p->seqlen_q > 0) != (p->q_out != nullptr))
        return set_err(FA_ERR_INVALID_ARGUMENT, "q and q_out must both be given, or seqlen_q must be 0");
    if (p->seqlen_q > 0) {
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
    if ((double)p->batch_size * (2.0 * p->num_heads_kv * p->seqlen_new + (double)p->num_heads_q * p->seqlen_q) *
            (double)p->headdim > 0x7fffffffLL * 256.0)
        return set_err(FA_ERR_UNSUPPORTED, "too many rows for one launch");
    return set_err(FA_OK, "%s", "");
}

int kvcache_launch(const fa_kvcache_params *p, int dtype, hipStream_t stream) {
    const int rc = kvcache_check(p, dtype);
    if (rc != FA_OK) return rc;
    if (p->batch_size == 0 || (p->seqlen_new == 0 && p->seqlen_q == 0)) return FA_OK;
    const int mode = pick_mode(*p);
    const int per_row = per_row_of(p->headdim, mode);
    const int64_t n_kv = p->batch_size * p->num_heads_kv * p->seqlen_new * per_row;
    const int64_t items = 2 * n_kv + p->batch_size * p->num_heads_q * p->seqlen_q * per_row;
    const dim3 grid((uint32_t)((items + 255) / 256));
#define FA_KV_LAUNCH(F16, MODE) \
    hipLaunchKernelGGL((fa_kvcache_append_kernel<F16, MODE>), grid, dim3(256), 0, stream, *p, n_kv, items, per_row)
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

}  // namespace fa

extern "C" int fa_kvcache_append_gfx950(const fa_kvcache_params *params, int dtype, void *stream) {
    return fa::kvcache_launch(params, dtype, (hipStream_t)stream);
}

extern "C" int fa_kvcache_append_gfx950_check(const fa_kvcache_params *params, int dtype) {
    return fa::kvcache_check(params, dtype);
}

extern "C" int fa_kvcache_version(void) { return FA_GFX950_KVCACHE_VERSION; }
