// flash_attention_api.cpp -- torch host API of the gfx950 FlashAttention-2 forward.
//
// Host-side mirror of reference csrc/flash_attention_api.cpp:14-141 (same function name, same
// argument meaning, same TORCH_CHECK messages, same decode q-head packing and stride-preserving
// output allocation). Differences, all MI355X-side:
//   * the compute-capability check (reference :17-19) becomes a gfx950 architecture check that is
//     cached per device instead of two device-attribute queries per call;
//   * the kernel is reached through the C-ABI of include/fa_gfx950.h (fa_fwd_gfx950), not a C++
//     template dispatch (reference csrc/kernel_dispatcher.h); runtime errors come back as a
//     RuntimeError instead of exit() (reference csrc/utils.h:9-18);
//   * inputs whose base pointer or strides are not 16-byte aligned (the reference silently assumes
//     alignment, csrc/flash_attention_template.cuh:135-137) are copied to a contiguous buffer.
//
// Every entry point reads: its checks, its layout decisions, one fill_params call (fill_packed_params for packed
// rows; fill_paged behind either for a paged cache), the fields where its layout deviates, its call
// (launch_with_workspace where the launch takes scratch). The steps they share are named once, below.
#include <torch/extension.h>

#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "fa_gfx950.h"
#include "fa_gfx950_fp8.h"
#include "fa_gfx950_kvcache.h"
#include "fa_gfx950_kvcache_varlen.h"
#include "fa_gfx950_lse.h"
#include "fa_gfx950_paged.h"
#include "fa_gfx950_paged_prefill.h"
#include "fa_gfx950_paged_varlen.h"
#include "fa_gfx950_paged_varlen_lse.h"
#include "fa_gfx950_paged_varlen_sink.h"
#include "fa_gfx950_paged_window.h"
#include "fa_gfx950_sink.h"

namespace flash_attention {

namespace {

bool device_is_gfx950(int device) {
    static std::mutex mu;
    static std::vector<int> cache;  // -1 unknown, 0 no, 1 yes
    std::lock_guard<std::mutex> lock(mu);
    if ((int)cache.size() <= device) cache.resize(device + 1, -1);
    if (cache[device] < 0) {
        hipDeviceProp_t prop;
        const hipError_t e = hipGetDeviceProperties(&prop, device);
        TORCH_CHECK(e == hipSuccess, "hipGetDeviceProperties failed: ", hipGetErrorString(e));
        cache[device] = std::string(prop.gcnArchName).rfind("gfx950", 0) == 0 ? 1 : 0;
    }
    return cache[device] == 1;
}

void require_gfx950(const torch::Device &device) {
    TORCH_CHECK(device_is_gfx950(device.index()),
                "flash attention (gfx950 build) is only supported on MI355X / gfx950 devices");
}

int fa_dtype(const torch::Tensor &t) { return t.scalar_type() == torch::kHalf ? FA_DTYPE_F16 : FA_DTYPE_BF16; }

void *current_stream(const torch::Tensor &t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

void check_rc(int rc, const char *fn) {
    TORCH_CHECK(rc == FA_OK, fn, " failed (code ", rc, "): ", fa_last_error());
}

bool aligned16(const torch::Tensor &t) {
    if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 != 0) return false;
    for (int i = 0; i < 3; ++i)
        if (t.stride(i) % 8 != 0 && t.size(i) > 1) return false;
    return true;
}

torch::Tensor aligned_or_contiguous(const torch::Tensor &t) { return aligned16(t) ? t : t.contiguous(); }

// stride-preserving output (reference :85): o inherits q's physical layout, so the
// transpose(1, 2).reshape(...) of the HF attention caller stays copy-free
torch::Tensor alloc_out_like(const torch::Tensor &qx) {
    auto o = torch::empty_like(qx);
    return aligned16(o) ? o : torch::empty(qx.sizes(), qx.options());
}

// the kernels' fp32 scratch: taken from torch's caching allocator on the current stream, so it is
// graph-capture safe and reused; undefined (data: nullptr) when the launch needs none
torch::Tensor workspace_for(int64_t bytes, const torch::TensorOptions &options) {
    return bytes > 0 ? torch::empty({bytes}, options.dtype(torch::kUInt8)) : torch::Tensor();
}
void *data_or_null(const torch::Tensor &ws) { return ws.defined() ? ws.data_ptr() : nullptr; }

// o (of the packed or copied q) in the caller's shape
torch::Tensor shaped_like(const torch::Tensor &o, const torch::Tensor &q) {
    return o.sizes() != q.sizes() ? o.reshape(q.sizes()) : o;
}

int64_t stride_or_zero(const torch::Tensor &t, int dim) {
    // a size-1 dimension may carry any stride; the kernel never steps along it
    return t.size(dim) == 1 ? 0 : t.stride(dim);
}

// The checks every dense entry words the same way (reference :21-27, :39-43, :53-59), in three pieces
// because the entries put checks of their own between them.
void check_4d(const torch::Tensor &q, const torch::Tensor &k, const torch::Tensor &v) {
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "q, k, v must be 4-D [batch, heads, seqlen, dim]");
}
void check_qkv_4d(const torch::Tensor &q, const torch::Tensor &k, const torch::Tensor &v) {
    check_4d(q, k, v);
    TORCH_CHECK(q.size(0) == k.size(0) && q.size(0) == v.size(0), "q, k, v must have the same batch size");
    TORCH_CHECK(k.size(1) == v.size(1), "k, v must have the same number of heads");
    TORCH_CHECK(k.size(2) == v.size(2), "k, v must have the same sequence length");
    TORCH_CHECK(q.size(3) == k.size(3) && q.size(3) == v.size(3), "q, k, v must have the same hidden dimension");
}
void check_dtype(const torch::Tensor &q, const torch::Tensor &k, const torch::Tensor &v) {
    TORCH_CHECK(q.dtype() == k.dtype() && q.dtype() == v.dtype(), "q, k, v must have the same data type");
    TORCH_CHECK(q.dtype() == torch::kHalf || q.dtype() == torch::kBFloat16,
                "q, k, v only support fp16 or bf16 data type");
}
// kernel constraints on the head dim (q's last dimension) and the device; the last check an entry
// can fail on CPU tensors
void check_headdim_device(const torch::Tensor &q, const torch::Tensor &k, const torch::Tensor &v) {
    TORCH_CHECK(q.size(-1) % 8 == 0, "hidden dimension must be multiple of 8");
    TORCH_CHECK(q.size(-1) <= 128, "only support hidden dimension <= 128");
    TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda(), "q, k, v must be on CUDA device");
    TORCH_CHECK(q.device() == k.device() && q.device() == v.device(), "q, k, v must be on the same CUDA device");
}

// Decode q-head packing (reference :64-83): with one query row per head, the q-heads of one
// kv group become the rows of a single (batch, kv-head) problem so one workgroup serves the
// whole group from one K/V stream: q [B, Hq, 1, D] as [B, Hkv, g, D], which fill_params describes as
// MHA over the packed rows (reference :100). The caller drops causal masking, as the reference (:81).
torch::Tensor pack_head_q(const torch::Tensor &qx, int64_t head_kv) {
    torch::Tensor p = qx.reshape({qx.size(0), head_kv, qx.size(1) / head_kv, qx.size(3)});
    return aligned16(p) ? p : p.contiguous();
}

// The dense 4-D problem of q [B, Hq, Sq, D], k / v [B, Hkv, Sk, D] and o (q's shape): pointers, sizes,
// the three stride groups and the scale. An entry whose layout differs overwrites those fields after
// the call.
void fill_params(fa_fwd_params &params, const torch::Tensor &qx, const torch::Tensor &kx, const torch::Tensor &vx,
                 const torch::Tensor &o, float softmax_scale) {
    params.q_ptr = qx.data_ptr();
    params.k_ptr = kx.data_ptr();
    params.v_ptr = vx.data_ptr();
    params.o_ptr = o.data_ptr();
    params.batch_size = qx.size(0);
    params.num_heads_q = qx.size(1);
    params.num_heads_kv = kx.size(1);
    params.seqlen_q = qx.size(2);
    params.seqlen_kv = kx.size(2);
    params.headdim = qx.size(3);
    params.head_q_per_group = qx.size(1) / kx.size(1);
    params.q_batch_stride = stride_or_zero(qx, 0);
    params.k_batch_stride = stride_or_zero(kx, 0);
    params.v_batch_stride = stride_or_zero(vx, 0);
    params.o_batch_stride = stride_or_zero(o, 0);
    params.q_head_stride = stride_or_zero(qx, 1);
    params.k_head_stride = stride_or_zero(kx, 1);
    params.v_head_stride = stride_or_zero(vx, 1);
    params.o_head_stride = stride_or_zero(o, 1);
    params.q_seqlen_stride = stride_or_zero(qx, 2);
    params.k_seqlen_stride = stride_or_zero(kx, 2);
    params.v_seqlen_stride = stride_or_zero(vx, 2);
    params.o_seqlen_stride = stride_or_zero(o, 2);
    // log2(e) folded into the scale on the host (reference :87)
    // (float * double -> float, exactly as `softmax_scale *= M_LOG2E` there)
    softmax_scale *= M_LOG2E;
    params.softmax_scale = softmax_scale;
}

// cos / sin tables of RoPE: [B, S, D], [1, S, D] or [S, D] of x's dtype on x's device; returns the
// table as [B', S, D] with 16-B aligned rows (B' = 1: shared by every batch row, batch stride 0)
torch::Tensor rope_table(const torch::Tensor &t, const torch::Tensor &x, int64_t batch, int64_t seqlen, int64_t dim,
                         const char *name) {
    TORCH_CHECK(t.dim() == 2 || t.dim() == 3, name, " must be [B, S, D] or [S, D]");
    torch::Tensor u = t.dim() == 2 ? t.unsqueeze(0) : t;
    TORCH_CHECK(u.size(0) == batch || u.size(0) == 1, name, " batch must be 1 or ", batch);
    TORCH_CHECK(u.size(1) == seqlen && u.size(2) == dim, name, " must cover ", seqlen, " positions x ", dim);
    TORCH_CHECK(u.dtype() == x.dtype(), name, " must have the dtype of q / k");
    TORCH_CHECK(u.device() == x.device(), name, " must be on the device of q / k");
    const bool ok = reinterpret_cast<uintptr_t>(u.data_ptr()) % 16 == 0 && u.stride(2) == 1 &&
                    (u.stride(1) % 8 == 0 || u.size(1) == 1) && (u.stride(0) % 8 == 0 || u.size(0) == 1);
    return ok ? u : u.contiguous();
}

fa_rope_params rope_params(const torch::Tensor &x, const torch::Tensor &out, const torch::Tensor &cs,
                           const torch::Tensor &sn) {
    fa_rope_params r;
    r.x = x.data_ptr();
    r.out = out.data_ptr();
    r.cos = cs.data_ptr();
    r.sin = sn.data_ptr();
    r.batch_size = x.size(0);
    r.num_heads = x.size(1);
    r.seqlen = x.size(2);
    r.headdim = x.size(3);
    r.x_batch_stride = x.stride(0);
    r.x_head_stride = x.stride(1);
    r.x_seqlen_stride = x.stride(2);
    r.out_batch_stride = out.stride(0);
    r.out_head_stride = out.stride(1);
    r.out_seqlen_stride = out.stride(2);
    r.cs_batch_stride = stride_or_zero(cs, 0);
    r.cs_seqlen_stride = cs.stride(1);
    return r;
}

// The packed 3-D problem of q / o [total_q, Hq, D] and k / v [total_k, Hkv, D] over `batch` sequences, not
// fill_params' dense one: rows are dimension 0, the strides are taken as they are, and the four batch strides stay
// as the caller zeroed them (a sequence starts at row cu_seqlens[b]).
bool aligned_rows(const torch::Tensor &t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && (t.stride(0) % 8 == 0 || t.size(0) <= 1) &&
           (t.stride(1) % 8 == 0 || t.size(1) <= 1);
}
void fill_packed_params(fa_fwd_params &params, const torch::Tensor &qx, const torch::Tensor &kx, const torch::Tensor &vx,
                        const torch::Tensor &o, int64_t batch, int64_t max_seqlen_q, int64_t max_seqlen_k,
                        float softmax_scale) {
    params.q_ptr = qx.data_ptr();
    params.k_ptr = kx.data_ptr();
    params.v_ptr = vx.data_ptr();
    params.o_ptr = o.data_ptr();
    params.batch_size = batch;
    params.num_heads_q = qx.size(1);
    params.num_heads_kv = kx.size(1);
    params.seqlen_q = max_seqlen_q;
    params.seqlen_kv = max_seqlen_k;
    params.headdim = qx.size(2);
    params.head_q_per_group = qx.size(1) / kx.size(1);
    params.q_head_stride = qx.stride(1);
    params.k_head_stride = kx.stride(1);
    params.v_head_stride = vx.stride(1);
    params.o_head_stride = o.stride(1);
    params.q_seqlen_stride = qx.stride(0);
    params.k_seqlen_stride = kx.stride(0);
    params.v_seqlen_stride = vx.stride(0);
    params.o_seqlen_stride = o.stride(0);
    softmax_scale *= M_LOG2E;  // (as fill_params)
    params.softmax_scale = softmax_scale;
}

// The steps of every entry whose launch takes fp32 scratch: the size query (negative: the library's own
// message), the scratch, the launch. `name` is the C entry (its size query: <name>_workspace_size).
template <class SizeFn, class LaunchFn>
void launch_with_workspace(const char *name, SizeFn size_fn, LaunchFn launch_fn, const torch::TensorOptions &options,
                           const char *launch_name = nullptr) {
    const int64_t ws_bytes = size_fn();
    TORCH_CHECK(ws_bytes >= 0, name, "_workspace_size failed: ", fa_last_error());
    torch::Tensor ws = workspace_for(ws_bytes, options);
    check_rc(launch_fn(data_or_null(ws), ws_bytes), launch_name ? launch_name : name);
}

// A paged KV cache as an attention entry sees it: the pools [num_pages, Hkv, page_size, D], block_table int32
// [batch, max_pages] and cache_seqlens int32 [batch]. The entries differ in three ways, each on purpose:
struct PagedCacheOptions {
    int page_multiple;        // 32: the decode kernels' key tile; 64: the paged fa_fwd_w4's
    bool copy_table;          // a table whose column stride is not 1: copied, or refused (read in place, to the letter)
    bool lengths_required;    // false: without cache_seqlens every sequence has seqlen_offset keys
    bool one_device_message;  // the wording only: "block_table and cache_seqlens must be on the device of q" in one
                              // check behind both shape checks, or one message each
};
// (page_multiple, copy_table, lengths_required, one_device_message)
constexpr PagedCacheOptions kPagedDecode = {32, true, true, true};    // the entries of paged_fwd_impl
constexpr PagedCacheOptions kPagedLse = {32, false, false, false};    // flash_attention_paged_lse_fwd
constexpr PagedCacheOptions kPagedRagged = {64, false, true, false};  // flash_attention_paged_varlen_fwd

// The tensors behind the raw pointers of a fa_paged_params: they stay alive as long as this struct.
struct PagedCache {
    torch::Tensor k, v, table, seqlens;  // (seqlens undefined: none given)
};

// The pools' own shape rules, in two pieces like the dense checks: these are reachable with CPU tensors (every
// paged entry calls check_headdim_device behind them), paged_cache's are not.
void check_pools(const torch::Tensor &k_cache, const torch::Tensor &v_cache, const PagedCacheOptions &opts) {
    TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4, "the caches must be 4-D [pages, heads, page_size, dim]");
    TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), "k_cache, v_cache must have the same shape");
    TORCH_CHECK(k_cache.size(0) > 0 && k_cache.size(1) > 0, "the caches must have at least one page and one head");
    TORCH_CHECK(k_cache.size(2) > 0 && k_cache.size(2) % opts.page_multiple == 0,
                "page_size must be a positive multiple of ", opts.page_multiple);
}

void check_table(const torch::Tensor &block_table, int64_t batch) {
    TORCH_CHECK(block_table.dtype() == torch::kInt32 && block_table.dim() == 2 && block_table.size(0) == batch &&
                    block_table.size(1) > 0,
                "block_table must be int32 [batch, max_pages]");
}
// (the appends and the unwindowed decode copy; a [batch, 1] table is copied too, as it always was)
torch::Tensor table_with_contiguous_rows(const torch::Tensor &t) { return t.stride(1) == 1 ? t : t.contiguous(); }

// The table and the lengths of `batch` sequences on q's device, checked; the table copied where the entry allows it.
PagedCache paged_cache(const torch::Tensor &k_cache, const torch::Tensor &v_cache, const torch::Tensor &block_table,
                       const c10::optional<torch::Tensor> &cache_seqlens, int64_t batch, const torch::Device &device,
                       const PagedCacheOptions &opts) {
    TORCH_INTERNAL_ASSERT(cache_seqlens.has_value() || !opts.lengths_required);
    const bool each = !opts.one_device_message;
    check_table(block_table, batch);
    TORCH_CHECK(!each || block_table.device() == device, "block_table must be on the device of q");
    TORCH_CHECK(opts.copy_table || block_table.stride(1) == 1 || block_table.size(1) == 1,
                "block_table rows must be contiguous (the table is read in place)");
    if (cache_seqlens.has_value()) {
        TORCH_CHECK(cache_seqlens->dtype() == torch::kInt32 && cache_seqlens->dim() == 1 && cache_seqlens->size(0) == batch,
                    "cache_seqlens must be int32 [batch]");
        TORCH_CHECK(!each || cache_seqlens->device() == device, "cache_seqlens must be on the device of q");
    }
    TORCH_CHECK(each || (block_table.device() == device && (!cache_seqlens.has_value() || cache_seqlens->device() == device)),
                "block_table and cache_seqlens must be on the device of q");
    return PagedCache{k_cache, v_cache, opts.copy_table ? table_with_contiguous_rows(block_table) : block_table,
                      cache_seqlens.has_value() ? *cache_seqlens : torch::Tensor()};
}

// Every field of `pp` that depends on the cache, over a base that fill_params / fill_packed_params filled for the
// pools as given. The pool is read where it is; only a 16-bit pool whose strides are not 16-byte multiples is copied
// (an fp8 pool never: the library rejects one that is not 16-byte aligned). The copies, the lengths' included, are
// made here and not in paged_cache: an entry that returns early with nothing to launch has copied nothing.
void fill_paged(fa_paged_params &pp, PagedCache &c) {
    if (c.k.dtype() != at::kFloat8_e4m3fn) {
        c.k = aligned_or_contiguous(c.k);
        c.v = aligned_or_contiguous(c.v);
    }
    if (c.seqlens.defined()) c.seqlens = c.seqlens.contiguous();
    fa_fwd_params &params = pp.base;
    params.k_ptr = c.k.data_ptr();
    params.v_ptr = c.v.data_ptr();
    params.seqlen_kv = c.table.size(1) * c.k.size(2);
    params.k_batch_stride = stride_or_zero(c.k, 0);  // (the page stride)
    params.v_batch_stride = stride_or_zero(c.v, 0);
    params.k_head_stride = stride_or_zero(c.k, 1);
    params.v_head_stride = stride_or_zero(c.v, 1);
    params.k_seqlen_stride = c.k.stride(2);
    params.v_seqlen_stride = c.v.stride(2);
    pp.block_table = c.table.data_ptr<int32_t>();
    pp.block_table_stride = c.table.stride(0);
    pp.max_pages = c.table.size(1);
    pp.num_pages = c.k.size(0);
    pp.page_size = c.k.size(2);
    pp.seqlens_k = c.seqlens.defined() ? c.seqlens.data_ptr<int32_t>() : nullptr;
}

// q [B, Hq, Sq, D] against the pools: the checks the 4-D paged entries share, up to their data types
void check_q_and_pools(const torch::Tensor &q, const torch::Tensor &k_cache, const torch::Tensor &v_cache,
                       const PagedCacheOptions &opts) {
    TORCH_CHECK(q.dim() == 4 && k_cache.dim() == 4 && v_cache.dim() == 4,
                "q must be 4-D [batch, heads, seqlen, dim], the caches 4-D [pages, heads, page_size, dim]");
    check_pools(k_cache, v_cache, opts);
    TORCH_CHECK(q.size(3) == k_cache.size(3), "q and the caches must have the same hidden dimension");
    TORCH_CHECK(q.size(0) > 0 && q.size(1) > 0 && q.size(2) > 0 && q.size(3) > 0, "q must have at least one element");
    TORCH_CHECK(q.size(1) % k_cache.size(1) == 0,
                "number of heads in q must be multiple of number of heads in k and v");
}

// The [B, Hkv] fp32 descales of an fp8 entry (nullptr / undefined tensor: 1.0)
struct Fp8Descales {
    const torch::Tensor *k, *v;
};
Fp8Descales descales_of(const c10::optional<torch::Tensor> &k, const c10::optional<torch::Tensor> &v) {
    return Fp8Descales{k.has_value() ? &*k : nullptr, v.has_value() ? &*v : nullptr};
}

// their pointers and the strides both share, into either fp8 struct; returns the tensors behind the pointers
template <class Fp8Params>
std::pair<torch::Tensor, torch::Tensor> fill_descales(Fp8Params &fp, const Fp8Descales &ds, const torch::Tensor &like,
                                                      int64_t bs, int64_t hkv) {
    auto prep = [&](const torch::Tensor *t, const char *name) {
        if (!t || !t->defined()) return torch::Tensor();
        TORCH_CHECK(t->dtype() == torch::kFloat32 && t->dim() == 2 && t->size(0) == bs && t->size(1) == hkv, name,
                    " must be fp32 [batch, kv heads]");
        TORCH_CHECK(t->device() == like.device(), name, " must be on the device of q / the caches");
        return *t;
    };
    torch::Tensor keep_k = prep(ds.k, "k_descale"), keep_v = prep(ds.v, "v_descale");
    // one stride pair serves both arrays: a tensor laid out differently from the other is made contiguous
    if (keep_k.defined() && keep_v.defined() &&
        (stride_or_zero(keep_k, 0) != stride_or_zero(keep_v, 0) || stride_or_zero(keep_k, 1) != stride_or_zero(keep_v, 1) ||
         keep_k.stride(0) < 0 || keep_k.stride(1) < 0)) {
        keep_k = keep_k.contiguous();
        keep_v = keep_v.contiguous();
    }
    const torch::Tensor &any = keep_k.defined() ? keep_k : keep_v;
    fp.k_descale = keep_k.defined() ? keep_k.data_ptr<float>() : nullptr;
    fp.v_descale = keep_v.defined() ? keep_v.data_ptr<float>() : nullptr;
    fp.descale_batch_stride = any.defined() ? stride_or_zero(any, 0) : 0;
    fp.descale_head_stride = any.defined() ? stride_or_zero(any, 1) : 0;
    return {keep_k, keep_v};
}

// the LSE destination of either LSE struct
template <class LseParams>
void fill_lse(LseParams &lp, const torch::Tensor &lse, int64_t seqlen_offset) {
    lp.lse_ptr = lse.data_ptr<float>();
    lp.lse_batch_stride = lse.stride(0);
    lp.lse_head_stride = lse.stride(1);
    lp.lse_seqlen_stride = lse.stride(2);
    lp.seqlen_offset = seqlen_offset;
}

// The [max_pos, D] cos / sin tables of an append, of `dtype` on the caches' device (`dtype_words`: how the entry
// names that dtype), with contiguous rows and one row stride; both undefined when none are given.
std::pair<torch::Tensor, torch::Tensor> append_rope_tables(const c10::optional<torch::Tensor> &cos,
                                                           const c10::optional<torch::Tensor> &sin, int64_t d,
                                                           caffe2::TypeMeta dtype, const torch::Device &device,
                                                           const char *dtype_words) {
    if (!cos.has_value()) return {};
    TORCH_CHECK(d % 2 == 0, "RoPE needs an even head dimension");
    auto table = [&](const torch::Tensor &t, const char *name) {
        TORCH_CHECK(t.dim() == 2 && t.size(0) > 0 && t.size(1) == d, name, " must be [max_pos, ", d, "]");
        TORCH_CHECK(t.dtype() == dtype, name, dtype_words);
        TORCH_CHECK(t.device() == device, name, " must be on the device of the caches");
        return t.stride(1) == 1 ? t : t.contiguous();
    };
    torch::Tensor cs = table(*cos, "rotary_cos"), sn = table(*sin, "rotary_sin");
    TORCH_CHECK(cs.size(0) == sn.size(0), "rotary_cos and rotary_sin must have the same number of rows");
    if (cs.size(0) > 1 && cs.stride(0) != sn.stride(0)) {
        cs = cs.contiguous();
        sn = sn.contiguous();
    }
    return {cs, sn};
}

// The fields either append struct names alike: the tables, the cache the rows go to (`bt` undefined: a dense
// [B, Hkv, Smax, D] cache, one "page" per batch row) and the lengths in and out.
template <class AppendParams>
void fill_append_cache(AppendParams &p, const torch::Tensor &k_cache, const torch::Tensor &v_cache,
                       const torch::Tensor &bt, const torch::Tensor &sl, const torch::Tensor &new_seqlens,
                       const torch::Tensor &cs, const torch::Tensor &sn) {
    if (cs.defined()) {
        p.cos = cs.data_ptr();
        p.sin = sn.data_ptr();
        p.cs_row_stride = stride_or_zero(cs, 0);
        p.max_pos = cs.size(0);
    }
    p.k_cache = k_cache.data_ptr();
    p.v_cache = v_cache.data_ptr();
    p.k_page_stride = stride_or_zero(k_cache, 0);
    p.k_head_stride = stride_or_zero(k_cache, 1);
    p.k_row_stride = stride_or_zero(k_cache, 2);
    p.v_page_stride = stride_or_zero(v_cache, 0);
    p.v_head_stride = stride_or_zero(v_cache, 1);
    p.v_row_stride = stride_or_zero(v_cache, 2);
    p.block_table = bt.defined() ? bt.data_ptr<int32_t>() : nullptr;
    p.block_table_stride = bt.defined() ? bt.stride(0) : 0;
    p.max_pages = bt.defined() ? bt.size(1) : 1;
    p.num_pages = k_cache.size(0);
    p.page_size = k_cache.size(2);
    p.seqlens_k = sl.data_ptr<int32_t>();
    p.seqlens_out = new_seqlens.data_ptr<int32_t>();
    p.batch_size = sl.size(0);
    p.num_heads_kv = k_cache.size(1);
    p.headdim = k_cache.size(3);
}

}  // namespace

// out = x * cos + rotate_half(x) * sin for x [B, H, S, D] (fp16 / bf16, last dim contiguous); out keeps
// x's strides (HF's [B, S, H, D] projection views stay copy-free). One HIP pass (csrc/fa_rope.hip).
torch::Tensor rope_apply(torch::Tensor &x, torch::Tensor &cos, torch::Tensor &sin) {
    TORCH_CHECK(x.dim() == 4, "x must be 4-D [batch, heads, seqlen, dim]");
    TORCH_CHECK(x.dtype() == torch::kHalf || x.dtype() == torch::kBFloat16, "RoPE supports fp16 or bf16");
    TORCH_CHECK(x.is_cuda(), "x must be on CUDA device");
    TORCH_CHECK(x.stride(3) == 1, "x must be contiguous in the last dimension");
    TORCH_CHECK(x.size(3) % 2 == 0, "RoPE needs an even head dimension");
    c10::DeviceGuard device_guard(x.device());
    torch::Tensor cs = rope_table(cos, x, x.size(0), x.size(2), x.size(3), "cos");
    torch::Tensor sn = rope_table(sin, x, x.size(0), x.size(2), x.size(3), "sin");
    TORCH_CHECK(cs.size(0) == sn.size(0) && cs.strides() == sn.strides(), "cos and sin must have the same layout");
    auto out = torch::empty_like(x);
    if (x.numel() == 0) return out;
    const fa_rope_params r = rope_params(x, out, cs, sn);
    check_rc(fa_rope_gfx950(&r, fa_dtype(x), current_stream(x)), "fa_rope_gfx950");
    return out;
}

// window_left >= 0 (flash_attention_window_fwd, after its cut): the local-window entry, no pack
torch::Tensor fwd_impl(torch::Tensor &q, torch::Tensor &k, torch::Tensor &v, float softmax_scale, bool causal,
                       int64_t window_left) {
    // Check input shape (reference :21-37)
    check_qkv_4d(q, k, v);
    TORCH_CHECK(q.size(0) > 0 && q.size(1) > 0 && q.size(2) > 0 && q.size(3) > 0,
                "q, k, v must have at least one element");
    TORCH_CHECK(k.size(2) > 0, "q, k, v must have at least one element");
    TORCH_CHECK(q.size(1) >= k.size(1),
                "number of heads in q must be greater or equal to number of heads in k and v");
    TORCH_CHECK(q.size(1) % k.size(1) == 0, "number of heads in q must be multiple of number of heads in k and v");

    // Check input data type (reference :39-43)
    check_dtype(q, k, v);

    // Check input memory contiguity (reference :45-51)
    TORCH_CHECK(q.stride(3) == 1, "q must be contiguous in the last dimension");
    TORCH_CHECK(k.stride(3) == 1, "k must be contiguous in the last dimension");
    TORCH_CHECK(v.stride(3) == 1, "v must be contiguous in the last dimension");

    // Check kernel constraints (reference :53-59)
    check_headdim_device(q, k, v);

    c10::DeviceGuard device_guard(q.device());
    require_gfx950(q.device());

    torch::Tensor qx = aligned_or_contiguous(q);
    torch::Tensor kx = aligned_or_contiguous(k);
    torch::Tensor vx = aligned_or_contiguous(v);
    if (qx.size(2) == 1 && window_left < 0) {  // (the window entry never packs)
        qx = pack_head_q(qx, kx.size(1));
        causal = false;
    }
    auto o = alloc_out_like(qx);

    fa_fwd_params params;
    fill_params(params, qx, kx, vx, o, softmax_scale);

    const int dtype = fa_dtype(qx), c = causal ? 1 : 0;
    void *stream = current_stream(qx);
    if (window_left >= 0) {
        check_rc(fa_fwd_gfx950_window(&params, dtype, c, window_left, stream), "fa_fwd_gfx950_window");
        return shaped_like(o, q);
    }
    // split-KV decode (few rows per kv-head) and key-split causal blocks want fp32 scratch for their partials
    launch_with_workspace(
        "fa_fwd_gfx950", [&] { return fa_fwd_gfx950_workspace_size(&params, dtype, c); },
        [&](void *ws, int64_t ws_bytes) { return fa_fwd_gfx950_ws(&params, dtype, c, ws, ws_bytes, stream); },
        qx.options(), "fa_fwd_gfx950_ws");
    return shaped_like(o, q);
}

torch::Tensor flash_attention_fwd(torch::Tensor &q, torch::Tensor &k, torch::Tensor &v, float softmax_scale,
                                  bool causal) {
    return fwd_impl(q, k, v, softmax_scale, causal, -1);
}

// Local (sliding-window) attention, include/fa_gfx950.h fa_fwd_gfx950_window: key n visible to query
// m iff n >= m + Sk - Sq - window_left (and, causal, n <= m + Sk - Sq). The keys left of every row's
// window are cut off here as views of k / v; when the window masks nothing more (decode: Sq == 1)
// the plain forward runs on the rest (q-head pack and split-KV decode included).
torch::Tensor flash_attention_window_fwd(torch::Tensor &q, torch::Tensor &k, torch::Tensor &v, int64_t window_left,
                                         float softmax_scale, bool causal) {
    TORCH_CHECK(window_left >= 0, "window_left must be >= 0");
    check_4d(q, k, v);
    TORCH_CHECK(k.size(2) == v.size(2), "k, v must have the same sequence length");
    const int64_t sq = q.size(2), sk = k.size(2);
    const int64_t cut = sk - sq - window_left;
    torch::Tensor kc = cut > 0 ? k.narrow(2, cut, sk - cut) : k;
    torch::Tensor vc = cut > 0 ? v.narrow(2, cut, sk - cut) : v;
    if (kc.size(2) - 1 <= window_left) return fwd_impl(q, kc, vc, softmax_scale, causal, -1);
    return fwd_impl(q, kc, vc, softmax_scale, causal, window_left);
}

// Attention with RoPE applied to q inside the kernel's Q load (fa_fwd_gfx950_rope); k is already
// rotated. Query blocks the split-KV decode kernel serves (Sq == 1 pack, g * Sq <= 64) and other head
// dims rotate q with rope_apply first and take the plain path.
torch::Tensor flash_attention_rope_fwd(torch::Tensor &q, torch::Tensor &k, torch::Tensor &v, torch::Tensor &cos,
                                       torch::Tensor &sin, float softmax_scale, bool causal) {
    check_4d(q, k, v);
    TORCH_CHECK(k.size(1) > 0 && q.size(1) % k.size(1) == 0,
                "number of heads in q must be multiple of number of heads in k and v");
    const int64_t g = q.size(1) / k.size(1), sq = q.size(2), d = q.size(3);
    const bool fused = (d == 64 || d == 128) && sq > 1 && g * sq > 64 && q.is_cuda() && q.stride(3) == 1 &&
                       (q.dtype() == torch::kHalf || q.dtype() == torch::kBFloat16);
    if (!fused) {
        torch::Tensor qr = rope_apply(q, cos, sin);
        return flash_attention_fwd(qr, k, v, softmax_scale, causal);
    }
    // the checks of flash_attention_fwd on a dry run of the same tensors (no Sq == 1 pack here)
    check_qkv_4d(q, k, v);
    TORCH_CHECK(k.size(2) > 0 && q.size(0) > 0, "q, k, v must have at least one element");
    TORCH_CHECK(q.dtype() == k.dtype() && q.dtype() == v.dtype(), "q, k, v must have the same data type");
    TORCH_CHECK(k.stride(3) == 1 && v.stride(3) == 1, "k, v must be contiguous in the last dimension");
    TORCH_CHECK(k.is_cuda() && v.is_cuda() && q.device() == k.device() && q.device() == v.device(),
                "q, k, v must be on the same CUDA device");
    c10::DeviceGuard device_guard(q.device());
    require_gfx950(q.device());
    torch::Tensor cs = rope_table(cos, q, q.size(0), sq, d, "cos");
    torch::Tensor sn = rope_table(sin, q, q.size(0), sq, d, "sin");
    TORCH_CHECK(cs.size(0) == sn.size(0) && cs.strides() == sn.strides(), "cos and sin must have the same layout");
    torch::Tensor qx = aligned_or_contiguous(q);
    torch::Tensor kx = aligned_or_contiguous(k);
    torch::Tensor vx = aligned_or_contiguous(v);
    auto o = alloc_out_like(qx);

    fa_rope_fwd_params rp;
    fill_params(rp.base, qx, kx, vx, o, softmax_scale);
    const fa_rope_params tables = rope_params(qx, o, cs, sn);  // the tables as rope_apply describes them
    rp.rope_cos = tables.cos;
    rp.rope_sin = tables.sin;
    rp.rope_batch_stride = tables.cs_batch_stride;
    rp.rope_seqlen_stride = tables.cs_seqlen_stride;
    check_rc(fa_fwd_gfx950_rope(&rp, fa_dtype(qx), causal ? 1 : 0, current_stream(qx)), "fa_fwd_gfx950_rope");
    return shaped_like(o, q);
}

// Variable-length (packed) batches: q [total_q, Hq, D], k / v [total_k, Hkv, D], cu_seqlens_* int32
// [B + 1] on the device (include/fa_gfx950.h fa_fwd_gfx950_varlen). No reference counterpart
// (varlen is a TODO at reference README.md:18); the checks follow flash_attention_fwd's.
torch::Tensor flash_attention_varlen_fwd(torch::Tensor &q, torch::Tensor &k, torch::Tensor &v,
                                         torch::Tensor &cu_seqlens_q, torch::Tensor &cu_seqlens_k,
                                         int64_t max_seqlen_q, int64_t max_seqlen_k, float softmax_scale,
                                         bool causal, int64_t window_left) {
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3, "varlen q, k, v must be 3-D [total, heads, dim]");
    TORCH_CHECK(k.size(0) == v.size(0), "k, v must have the same number of rows");
    TORCH_CHECK(k.size(1) == v.size(1), "k, v must have the same number of heads");
    TORCH_CHECK(q.size(2) == k.size(2) && q.size(2) == v.size(2), "q, k, v must have the same hidden dimension");
    TORCH_CHECK(q.size(1) > 0 && k.size(1) > 0 && q.size(2) > 0, "q, k, v must have at least one head");
    TORCH_CHECK(q.size(1) % k.size(1) == 0, "number of heads in q must be multiple of number of heads in k and v");
    check_dtype(q, k, v);
    TORCH_CHECK(q.stride(2) == 1 && k.stride(2) == 1 && v.stride(2) == 1,
                "q, k, v must be contiguous in the last dimension");
    check_headdim_device(q, k, v);
    TORCH_CHECK(cu_seqlens_q.dtype() == torch::kInt32 && cu_seqlens_k.dtype() == torch::kInt32,
                "cu_seqlens must be int32");
    TORCH_CHECK(cu_seqlens_q.dim() == 1 && cu_seqlens_k.dim() == 1 && cu_seqlens_q.size(0) == cu_seqlens_k.size(0) &&
                    cu_seqlens_q.size(0) >= 2,
                "cu_seqlens_q and cu_seqlens_k must be 1-D with batch_size + 1 entries");
    TORCH_CHECK(cu_seqlens_q.device() == q.device() && cu_seqlens_k.device() == q.device(),
                "cu_seqlens must be on the same device as q");
    TORCH_CHECK(max_seqlen_q >= 0 && max_seqlen_k >= 0, "max_seqlen must be non-negative");

    c10::DeviceGuard device_guard(q.device());
    require_gfx950(q.device());
    auto o = torch::empty_like(q);
    if (q.size(0) == 0 || max_seqlen_q == 0) return o;
    if (max_seqlen_k == 0) return o.zero_();  // no sequence has a key: every row is 0

    torch::Tensor qx = aligned_rows(q) ? q : q.contiguous();
    torch::Tensor kx = aligned_rows(k) ? k : k.contiguous();
    torch::Tensor vx = aligned_rows(v) ? v : v.contiguous();
    if (!aligned_rows(o)) o = torch::empty(q.sizes(), q.options());
    torch::Tensor cq = cu_seqlens_q.contiguous(), ck = cu_seqlens_k.contiguous();

    fa_varlen_params vp = {};
    fill_packed_params(vp.base, qx, kx, vx, o, cq.size(0) - 1, max_seqlen_q, max_seqlen_k, softmax_scale);
    vp.cu_seqlens_q = cq.data_ptr<int32_t>();
    vp.cu_seqlens_k = ck.data_ptr<int32_t>();

    const int dtype = fa_dtype(qx);
    void *stream = current_stream(qx);
    const int rc = window_left >= 0 ? fa_fwd_gfx950_varlen_window(&vp, dtype, causal ? 1 : 0, window_left, stream)
                                    : fa_fwd_gfx950_varlen(&vp, dtype, causal ? 1 : 0, stream);
    check_rc(rc, "fa_fwd_gfx950_varlen");
    return o;
}

// Padded batches (include/fa_gfx950.h fa_fwd_gfx950_padded): dense q [B, Hq, Sq, D], k / v
// [B, Hkv, Sk, D] (any strides, last dim contiguous) with the real tokens of batch row b at key
// positions [k_start[b], k_end[b]) and, optionally, query positions [q_start[b], q_end[b]) -- int32
// [B] on the device. Read in place: no packing copy, no host synchronisation (graph-capturable).
// Output rows outside the query ranges are 0. Sq == 1 without query ranges takes the q-head pack
// and the split-KV decode kernel over each sequence's key range (a window there narrows the key
// range on the device instead). No reference counterpart (the reference drops attention_mask).
torch::Tensor flash_attention_padded_fwd(torch::Tensor &q, torch::Tensor &k, torch::Tensor &v,
                                         c10::optional<torch::Tensor> q_start, c10::optional<torch::Tensor> q_end,
                                         torch::Tensor &k_start, torch::Tensor &k_end, float softmax_scale,
                                         bool causal, int64_t window_left) {
    check_qkv_4d(q, k, v);
    TORCH_CHECK(q.size(0) > 0 && q.size(1) > 0 && q.size(2) > 0 && q.size(3) > 0 && k.size(2) > 0,
                "q, k, v must have at least one element");
    TORCH_CHECK(q.size(1) % k.size(1) == 0, "number of heads in q must be multiple of number of heads in k and v");
    check_dtype(q, k, v);
    TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1 && v.stride(3) == 1,
                "q, k, v must be contiguous in the last dimension");
    check_headdim_device(q, k, v);
    TORCH_CHECK(q_start.has_value() == q_end.has_value(), "q_start and q_end must be given together");
    const int64_t bs = q.size(0);
    auto check_range = [&](const torch::Tensor &t, const char *name) {
        TORCH_CHECK(t.dtype() == torch::kInt32 && t.dim() == 1 && t.size(0) == bs, name, " must be int32 [batch]");
        TORCH_CHECK(t.device() == q.device(), name, " must be on the device of q");
    };
    check_range(k_start, "k_start");
    check_range(k_end, "k_end");
    const bool q_ranges = q_start.has_value();
    if (q_ranges) {
        check_range(*q_start, "q_start");
        check_range(*q_end, "q_end");
    }
    c10::DeviceGuard device_guard(q.device());
    require_gfx950(q.device());

    // the prefill kernel addresses a ranged sequence by absolute rows (row r at base + r * seqlen
    // stride): the batch stride must be a multiple of the seqlen stride, the same multiple for k and v
    // (q and o) -- other layouts are copied to a contiguous buffer
    auto rows_per_batch = [](const torch::Tensor &t) -> int64_t {
        if (t.size(0) == 1) return 0;
        if (t.stride(2) <= 0 || t.stride(0) % t.stride(2) != 0) return -1;
        return t.stride(0) / t.stride(2);
    };
    torch::Tensor qx = aligned_or_contiguous(q);
    torch::Tensor kx = aligned_or_contiguous(k);
    torch::Tensor vx = aligned_or_contiguous(v);
    if (rows_per_batch(kx) < 0 || rows_per_batch(kx) != rows_per_batch(vx) || kx.stride(2) != vx.stride(2)) {
        kx = kx.contiguous();
        vx = vx.contiguous();
    }
    torch::Tensor ks = k_start.contiguous(), ke = k_end.contiguous(), qs, qe;
    if (q_ranges) {
        qs = q_start->contiguous();
        qe = q_end->contiguous();
    }
    // decode: one query row that sees the last window_left + 1 keys of its range -> narrow the range
    if (window_left >= 0 && qx.size(2) == 1 && !q_ranges) {
        ks = torch::maximum(ks, ke - (int32_t)std::min<int64_t>(window_left + 1, 0x7fffffff));
        window_left = -1;
    }
    // Sq == 1: the q-head pack of flash_attention_fwd (reference :64-83)
    const bool pack = qx.size(2) == 1 && !q_ranges && window_left < 0;
    if (pack) {
        qx = pack_head_q(qx, kx.size(1));
        causal = false;
    }
    if (rows_per_batch(qx) < 0) qx = qx.contiguous();  // (the prefill path may run, also after a pack)
    auto o = torch::empty_like(qx);
    if (!aligned16(o) || o.strides() != qx.strides()) o = torch::empty(qx.sizes(), qx.options());
    // the prefill kernel addresses q and o rows with ONE rows-per-batch multiple: a q that is not
    // dense (a seqlen slice of a longer buffer, a view cut from a wider tensor) leaves empty_like with
    // a contiguous o, so q is made contiguous too
    if (rows_per_batch(o) != rows_per_batch(qx)) {
        qx = qx.contiguous();
        o = torch::empty(qx.sizes(), qx.options());
    }
    if (q_ranges) o.zero_();  // rows outside the query ranges are not written by the kernel

    fa_padded_params pp;
    fa_fwd_params &params = pp.base;
    fill_params(params, qx, kx, vx, o, softmax_scale);
    // the seqlen strides convert rows into addresses on the prefill path, even at size 1
    if (!pack) {
        params.q_seqlen_stride = qx.stride(2);
        params.o_seqlen_stride = o.stride(2);
    }
    params.k_seqlen_stride = kx.stride(2);
    params.v_seqlen_stride = vx.stride(2);
    pp.q_start = q_ranges ? qs.data_ptr<int32_t>() : nullptr;
    pp.q_end = q_ranges ? qe.data_ptr<int32_t>() : nullptr;
    pp.k_start = ks.data_ptr<int32_t>();
    pp.k_end = ke.data_ptr<int32_t>();

    const int dtype = fa_dtype(qx), c = causal ? 1 : 0;
    launch_with_workspace(
        "fa_fwd_gfx950_padded", [&] { return fa_fwd_gfx950_padded_workspace_size(&pp, dtype, c, window_left); },
        [&](void *ws, int64_t ws_bytes) {
            return fa_fwd_gfx950_padded(&pp, dtype, c, window_left, ws, ws_bytes, current_stream(qx));
        },
        qx.options());
    return shaped_like(o, q);
}

// Paged KV-cache decode (include/fa_gfx950_paged.h fa_fwd_gfx950_paged): q [B, Hq, Sq, D] dense, the
// caches page pools [num_pages, Hkv, page_size, D] (any strides, last dim contiguous; page_size a
// multiple of 32), block_table int32 [B, max_pages], cache_seqlens int32 [B], both on the device. The
// pool is read in place: no gather, no host synchronisation (graph-capturable). Decode shapes only
// (g * Sq <= 64; larger query blocks: flash_attention_paged_prefill_fwd below, or the Python op's
// copying path); Sq == 1 takes the q-head pack of
// flash_attention_fwd. No reference counterpart.
//
// fp8 (flash_attention_paged_fp8_fwd, include/fa_gfx950_fp8.h fa_fwd_gfx950_paged_fp8): the caches are
// torch.float8_e4m3fn pools read in place (never copied: 16-byte aligned, strides multiples of 16), q / o
// stay fp16 / bf16, k_descale / v_descale are fp32 [B, Hkv] device tensors of any strides (undefined: 1.0).
//
// window (flash_attention_paged_window_fwd / _fp8_fwd, include/fa_gfx950_paged_window.h): window_left >= 0
// goes to the windowed entries WITHOUT the q-head pack -- the window is relative to the real Sq, so a decode
// step is passed as Sq 1 with g q-heads per kv-head (the same kernel rows and arithmetic as the pack, causal
// dropped as the pack drops it); window_left < 0 is the unwindowed call, to the letter.
//
// sinks (flash_attention_paged_sink_fwd / _fp8_fwd, include/fa_gfx950_sink.h): fp32 [Hq] on q's device, one extra
// softmax column per q-head of that logit and value 0; the sink entries, with or without a window, never with the
// q-head pack (the pack loses the q-head a row belongs to).
torch::Tensor paged_fwd_impl(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                             torch::Tensor &block_table, torch::Tensor &cache_seqlens, float softmax_scale,
                             bool causal, const Fp8Descales *fp8, int64_t window_left = -1, bool prefill = false,
                             const torch::Tensor *sinks = nullptr) {
    check_q_and_pools(q, k_cache, v_cache, kPagedDecode);
    torch::Tensor sinks_c;
    if (sinks) {
        TORCH_CHECK(!prefill, "the paged prefill kernel has no sinks");
        TORCH_CHECK(sinks->dim() == 1 && sinks->size(0) == q.size(1) && sinks->dtype() == torch::kFloat32,
                    "sinks must be fp32 [heads of q]");
        TORCH_CHECK(sinks->device() == q.device(), "sinks must be on the device of q");
        sinks_c = sinks->contiguous();
    }
    if (fp8) {
        TORCH_CHECK(k_cache.dtype() == at::kFloat8_e4m3fn && v_cache.dtype() == at::kFloat8_e4m3fn,
                    "the fp8 caches must be torch.float8_e4m3fn");
        check_dtype(q, q, q);
    } else {
        check_dtype(q, k_cache, v_cache);
    }
    TORCH_CHECK(q.stride(3) == 1 && k_cache.stride(3) == 1 && v_cache.stride(3) == 1,
                "q, k, v must be contiguous in the last dimension");
    check_headdim_device(q, k_cache, v_cache);
    PagedCache cache = paged_cache(k_cache, v_cache, block_table, cache_seqlens, q.size(0), q.device(), kPagedDecode);
    c10::DeviceGuard device_guard(q.device());
    require_gfx950(q.device());

    torch::Tensor qx = aligned_or_contiguous(q);
    const bool window = window_left >= 0;
    if (qx.size(2) == 1 && !prefill) {  // Sq == 1: the q-head pack of flash_attention_fwd (reference :64-83)
        if (!window && !sinks) qx = pack_head_q(qx, k_cache.size(1));
        causal = false;
    }
    auto o = alloc_out_like(qx);

    fa_paged_fp8_sink_params sp8;  // (the FP8 struct of the sink entries holds every other one)
    memset(&sp8, 0, sizeof(sp8));
    fa_paged_fp8_params &fp = sp8.fp8;
    fa_paged_params &pp = fp.paged;
    fill_params(pp.base, qx, k_cache, v_cache, o, softmax_scale);
    fill_paged(pp, cache);
    // (prefill: 16-bit pools only, the Python op keeps FP8 pools on its copying path)
    TORCH_CHECK(!prefill || !fp8, "the paged prefill kernel reads 16-bit pools only");
    std::pair<torch::Tensor, torch::Tensor> descales;
    if (fp8) descales = fill_descales(fp, *fp8, q, q.size(0), k_cache.size(1));

    // one of seven C entries, each with the size query of its name
    enum Entry { kPrefill, kWindowFp8, kFp8, kWindow, kPlain, kSinkFp8, kSink };
    static const char *const names[] = {"fa_fwd_gfx950_paged_prefill", "fa_fwd_gfx950_paged_window_fp8",
                                        "fa_fwd_gfx950_paged_fp8", "fa_fwd_gfx950_paged_window", "fa_fwd_gfx950_paged",
                                        "fa_fwd_gfx950_paged_sink_fp8", "fa_fwd_gfx950_paged_sink"};
    const Entry entry = sinks     ? (fp8 ? kSinkFp8 : kSink)
                        : prefill ? kPrefill
                        : fp8     ? (window ? kWindowFp8 : kFp8)
                        : window  ? kWindow
                                  : kPlain;
    const int dtype = fa_dtype(qx), c = causal ? 1 : 0;
    void *stream = current_stream(qx);
    fa_paged_sink_params sp;
    memset(&sp, 0, sizeof(sp));
    if (sinks) {
        sp8.sinks = sinks_c.data_ptr<float>();
        sp.paged = pp;
        sp.sinks = sp8.sinks;
    }
    launch_with_workspace(
        names[entry],
        [&]() -> int64_t {
            switch (entry) {
                case kPrefill: return fa_fwd_gfx950_paged_prefill_workspace_size(&pp, dtype, c, window_left);
                case kWindowFp8: return fa_fwd_gfx950_paged_window_fp8_workspace_size(&fp, dtype, c, window_left);
                case kFp8: return fa_fwd_gfx950_paged_fp8_workspace_size(&fp, dtype, c);
                case kWindow: return fa_fwd_gfx950_paged_window_workspace_size(&pp, dtype, c, window_left);
                case kSinkFp8: return fa_fwd_gfx950_paged_sink_fp8_workspace_size(&sp8, dtype, c, window_left);
                case kSink: return fa_fwd_gfx950_paged_sink_workspace_size(&sp, dtype, c, window_left);
                default: return fa_fwd_gfx950_paged_workspace_size(&pp, dtype, c);
            }
        },
        [&](void *ws, int64_t ws_bytes) -> int {
            switch (entry) {
                case kPrefill: return fa_fwd_gfx950_paged_prefill(&pp, dtype, c, window_left, ws, ws_bytes, stream);
                case kWindowFp8: return fa_fwd_gfx950_paged_window_fp8(&fp, dtype, c, window_left, ws, ws_bytes, stream);
                case kFp8: return fa_fwd_gfx950_paged_fp8(&fp, dtype, c, ws, ws_bytes, stream);
                case kWindow: return fa_fwd_gfx950_paged_window(&pp, dtype, c, window_left, ws, ws_bytes, stream);
                case kSinkFp8: return fa_fwd_gfx950_paged_sink_fp8(&sp8, dtype, c, window_left, ws, ws_bytes, stream);
                case kSink: return fa_fwd_gfx950_paged_sink(&sp, dtype, c, window_left, ws, ws_bytes, stream);
                default: return fa_fwd_gfx950_paged(&pp, dtype, c, ws, ws_bytes, stream);
            }
        },
        qx.options());
    return shaped_like(o, q);
}

torch::Tensor flash_attention_paged_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                        torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                        float softmax_scale, bool causal) {
    return paged_fwd_impl(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, nullptr);
}

torch::Tensor flash_attention_paged_fp8_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                            torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                            c10::optional<torch::Tensor> k_descale,
                                            c10::optional<torch::Tensor> v_descale, float softmax_scale, bool causal) {
    const Fp8Descales ds = descales_of(k_descale, v_descale);
    return paged_fwd_impl(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, &ds);
}

torch::Tensor flash_attention_paged_window_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                               torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                               int64_t window_left, float softmax_scale, bool causal) {
    return paged_fwd_impl(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, nullptr, window_left);
}

// Prefill-sized query blocks over a 16-bit paged cache (include/fa_gfx950_paged_prefill.h
// fa_fwd_gfx950_paged_prefill): the pool read in place by the paged fa_fwd_w4, page_size a multiple of 64, any
// g * Sq (no q-head pack), window_left < 0 for no window. The Python op routes g * Sq > 64 here.
torch::Tensor flash_attention_paged_prefill_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                                torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                                int64_t window_left, float softmax_scale, bool causal) {
    return paged_fwd_impl(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, nullptr, window_left,
                          true);
}

torch::Tensor flash_attention_paged_window_fp8_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                                   torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                                   int64_t window_left, c10::optional<torch::Tensor> k_descale,
                                                   c10::optional<torch::Tensor> v_descale, float softmax_scale,
                                                   bool causal) {
    const Fp8Descales ds = descales_of(k_descale, v_descale);
    return paged_fwd_impl(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, &ds, window_left);
}

// Paged decode with attention sinks (include/fa_gfx950_sink.h fa_fwd_gfx950_paged_sink / _sink_fp8): sinks fp32
// [Hq] on q's device, window_left < 0 for no window. Decode shapes only (the library refuses g * Sq > 64).
torch::Tensor flash_attention_paged_sink_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                             torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                             torch::Tensor &sinks, int64_t window_left, float softmax_scale,
                                             bool causal) {
    return paged_fwd_impl(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, nullptr, window_left,
                          false, &sinks);
}

torch::Tensor flash_attention_paged_sink_fp8_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                                 torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                                 torch::Tensor &sinks, int64_t window_left,
                                                 c10::optional<torch::Tensor> k_descale,
                                                 c10::optional<torch::Tensor> v_descale, float softmax_scale,
                                                 bool causal) {
    const Fp8Descales ds = descales_of(k_descale, v_descale);
    return paged_fwd_impl(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, &ds, window_left,
                          false, &sinks);
}

// Paged decode that also returns the softmax log-sum-exp (include/fa_gfx950_lse.h fa_fwd_gfx950_paged_lse /
// _lse_fp8; the pool's dtype selects the entry): (o, lse) with lse fp32 [B, Hq, Sq] in natural log units, -inf
// for rows without a visible key; o is bit-identical to flash_attention_paged_fwd / _fp8_fwd. Decode shapes only,
// no window. Sequence b has clamp(cache_seqlens[b] + seqlen_offset) keys, or clamp(seqlen_offset) without
// cache_seqlens. No q-head pack: a decode step runs as Sq 1 with g q-heads per kv-head (the same kernel rows and
// arithmetic as the pack, causal dropped as the pack drops it), so q may be any 16-byte aligned strided view --
// the shared-prefix decode passes a group of sequences as the positions of one batch row. `out` / `lse_out`:
// caller-owned destinations (any strides, out 16-byte aligned), written in place; q is then never copied.
std::tuple<torch::Tensor, torch::Tensor> flash_attention_paged_lse_fwd(
    torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache, torch::Tensor &block_table,
    c10::optional<torch::Tensor> cache_seqlens, int64_t seqlen_offset, c10::optional<torch::Tensor> k_descale,
    c10::optional<torch::Tensor> v_descale, float softmax_scale, bool causal, c10::optional<torch::Tensor> out,
    c10::optional<torch::Tensor> lse_out) {
    check_q_and_pools(q, k_cache, v_cache, kPagedLse);
    const bool fp8 = k_cache.dtype() == at::kFloat8_e4m3fn;
    if (fp8) {
        TORCH_CHECK(v_cache.dtype() == at::kFloat8_e4m3fn, "the fp8 caches must be torch.float8_e4m3fn");
        check_dtype(q, q, q);
    } else {
        TORCH_CHECK(!k_descale.has_value() && !v_descale.has_value(), "k_descale / v_descale go with an fp8 cache");
        check_dtype(q, k_cache, v_cache);
    }
    TORCH_CHECK(q.stride(3) == 1 && k_cache.stride(3) == 1 && v_cache.stride(3) == 1,
                "q, k, v must be contiguous in the last dimension");
    check_headdim_device(q, k_cache, v_cache);
    const int64_t bs = q.size(0);
    PagedCache cache = paged_cache(k_cache, v_cache, block_table, cache_seqlens, bs, q.device(), kPagedLse);
    c10::DeviceGuard device_guard(q.device());
    require_gfx950(q.device());

    torch::Tensor qx = aligned_or_contiguous(q);
    if (qx.size(2) == 1) causal = false;
    torch::Tensor o;
    if (out.has_value()) {
        TORCH_CHECK(out->sizes() == q.sizes() && out->dtype() == q.dtype() && out->device() == q.device(),
                    "out must have q's shape, data type and device");
        TORCH_CHECK(out->stride(3) == 1 && aligned16(*out), "out must be 16-byte aligned, last dimension contiguous");
        o = *out;
    } else {
        o = alloc_out_like(qx);
    }
    torch::Tensor lse;
    if (lse_out.has_value()) {
        TORCH_CHECK(lse_out->dim() == 3 && lse_out->size(0) == bs && lse_out->size(1) == q.size(1) &&
                        lse_out->size(2) == q.size(2) && lse_out->dtype() == torch::kFloat32 &&
                        lse_out->device() == q.device(),
                    "lse_out must be fp32 [batch, heads, seqlen] on q's device");
        lse = *lse_out;
    } else {
        lse = torch::empty({bs, q.size(1), q.size(2)}, q.options().dtype(torch::kFloat32));
    }
    TORCH_CHECK(lse.stride(0) >= 0 && lse.stride(1) >= 0 && lse.stride(2) >= 0, "lse strides must be non-negative");

    fa_paged_fp8_lse_params lp8;
    memset(&lp8, 0, sizeof(lp8));
    fa_paged_params &pp = lp8.fp8.paged;
    fill_params(pp.base, qx, k_cache, v_cache, o, softmax_scale);
    fill_paged(pp, cache);
    const int dtype = fa_dtype(qx), c = causal ? 1 : 0;
    void *stream = current_stream(qx);
    if (fp8) {
        const auto descales = fill_descales(lp8.fp8, descales_of(k_descale, v_descale), q, bs, k_cache.size(1));
        fill_lse(lp8, lse, seqlen_offset);
        launch_with_workspace(
            "fa_fwd_gfx950_paged_lse_fp8", [&] { return fa_fwd_gfx950_paged_lse_fp8_workspace_size(&lp8, dtype, c, -1); },
            [&](void *ws, int64_t ws_bytes) { return fa_fwd_gfx950_paged_lse_fp8(&lp8, dtype, c, -1, ws, ws_bytes, stream); },
            qx.options());
    } else {
        fa_paged_lse_params lp;
        memset(&lp, 0, sizeof(lp));
        lp.paged = pp;
        fill_lse(lp, lse, seqlen_offset);
        launch_with_workspace(
            "fa_fwd_gfx950_paged_lse", [&] { return fa_fwd_gfx950_paged_lse_workspace_size(&lp, dtype, c, -1); },
            [&](void *ws, int64_t ws_bytes) { return fa_fwd_gfx950_paged_lse(&lp, dtype, c, -1, ws, ws_bytes, stream); },
            qx.options());
    }
    return {o, lse};
}

// Merge of partial attention states (include/fa_gfx950_lse.h fa_merge_states_gfx950): outs [N, B, H, S, D]
// fp16 / bf16 and lses [N, B, H, S] fp32 (any strides; outs copied only if not 16-byte aligned) -> (out
// [B, H, S, D], lse [B, H, S] or an empty tensor). One HIP pass.
// merge_states_into: the checks and the launch, into `o` [B, H, S, D] and `lse` [B, H, S] (undefined: none) as the
// caller laid them out -- views of any strides the library takes (the packed merge passes transposed ones).
void merge_states_into(const torch::Tensor &outs, const torch::Tensor &lses, torch::Tensor &o, torch::Tensor &lse) {
    const bool return_lse = lse.defined();
    TORCH_CHECK(outs.dim() == 5 && lses.dim() == 4, "outs must be [parts, batch, heads, seqlen, dim], lses "
                "[parts, batch, heads, seqlen]");
    TORCH_CHECK(outs.sizes().slice(0, 4) == lses.sizes(), "outs and lses must agree in their first four dimensions");
    TORCH_CHECK(outs.dtype() == torch::kHalf || outs.dtype() == torch::kBFloat16, "outs only support fp16 or bf16");
    TORCH_CHECK(lses.dtype() == torch::kFloat32, "lses must be fp32");
    TORCH_CHECK(outs.size(0) >= 1, "at least one partial state is needed");
    TORCH_CHECK(outs.size(4) > 0 && outs.size(4) % 8 == 0, "hidden dimension must be multiple of 8");
    TORCH_CHECK(outs.is_cuda() && lses.is_cuda() && outs.device() == lses.device(),
                "outs and lses must be on the same CUDA device");
    c10::DeviceGuard device_guard(outs.device());
    require_gfx950(outs.device());
    bool ok = outs.stride(4) == 1 && reinterpret_cast<uintptr_t>(outs.data_ptr()) % 16 == 0;
    for (int i = 0; i < 4; ++i) ok = ok && (outs.size(i) == 1 || (outs.stride(i) >= 0 && outs.stride(i) % 8 == 0));
    torch::Tensor ox = ok ? outs : outs.contiguous();
    bool lok = true;
    for (int i = 0; i < 4; ++i) lok = lok && (lses.size(i) == 1 || lses.stride(i) >= 0);
    torch::Tensor lx = lok ? lses : lses.contiguous();
    fa_merge_params mp;
    memset(&mp, 0, sizeof(mp));
    mp.outs = ox.data_ptr();
    mp.lses = lx.data_ptr<float>();
    mp.out = o.data_ptr();
    mp.lse = return_lse ? lse.data_ptr<float>() : nullptr;
    mp.num_parts = ox.size(0);
    mp.batch_size = ox.size(1);
    mp.num_heads = ox.size(2);
    mp.seqlen = ox.size(3);
    mp.headdim = ox.size(4);
    mp.outs_part_stride = stride_or_zero(ox, 0);
    mp.outs_batch_stride = stride_or_zero(ox, 1);
    mp.outs_head_stride = stride_or_zero(ox, 2);
    mp.outs_seqlen_stride = stride_or_zero(ox, 3);
    mp.lses_part_stride = stride_or_zero(lx, 0);
    mp.lses_batch_stride = stride_or_zero(lx, 1);
    mp.lses_head_stride = stride_or_zero(lx, 2);
    mp.lses_seqlen_stride = stride_or_zero(lx, 3);
    mp.out_batch_stride = stride_or_zero(o, 0);
    mp.out_head_stride = stride_or_zero(o, 1);
    mp.out_seqlen_stride = stride_or_zero(o, 2);
    if (return_lse) {
        mp.lse_batch_stride = stride_or_zero(lse, 0);
        mp.lse_head_stride = stride_or_zero(lse, 1);
        mp.lse_seqlen_stride = stride_or_zero(lse, 2);
    }
    check_rc(fa_merge_states_gfx950(&mp, ox.dtype() == torch::kHalf ? FA_DTYPE_F16 : FA_DTYPE_BF16, current_stream(ox)),
             "fa_merge_states_gfx950");
}

std::tuple<torch::Tensor, torch::Tensor> flash_attention_merge_states(torch::Tensor &outs, torch::Tensor &lses,
                                                                      bool return_lse) {
    TORCH_CHECK(outs.dim() == 5 && lses.dim() == 4, "outs must be [parts, batch, heads, seqlen, dim], lses "
                "[parts, batch, heads, seqlen]");
    auto o = torch::empty({outs.size(1), outs.size(2), outs.size(3), outs.size(4)}, outs.options());
    torch::Tensor lse = return_lse ? torch::empty({outs.size(1), outs.size(2), outs.size(3)}, lses.options()) : torch::Tensor();
    merge_states_into(outs, lses, o, lse);
    return {o, return_lse ? lse : torch::empty({0}, lses.options())};
}

// In-place KV-cache append with fused RoPE (include/fa_gfx950_kvcache.h fa_kvcache_append_gfx950): the new
// k / v [B, Hkv, Sn, D] are written at positions cache_seqlens[b] + i of the paged ([num_pages, Hkv,
// page_size, D] + block_table int32 [B, max_pages]) or dense ([B, Hkv, Smax, D], no table) cache, k rotated
// at those positions when the [max_pos, D] tables are given; q [B, Hq, Sq, D] is rotated at the sequence's
// last Sq positions after the append. Returns (new_seqlens int32 [B], q_rot or an empty tensor). The caches
// are written where they are -- never copied, whatever their alignment -- in one launch with no host
// synchronisation (graph-capturable). No reference counterpart.
//
// fp8 (flash_attention_kvcache_append_fp8, include/fa_gfx950_fp8.h fa_kvcache_append_fp8_gfx950): the caches
// are torch.float8_e4m3fn, k / v / q / the tables fp16 or bf16; k (rotated, rounded to its dtype) and v are
// quantized with the [B, Hkv] descales on the way in, q_rot stays 16-bit.
std::tuple<torch::Tensor, torch::Tensor> kvcache_append_impl(
    torch::Tensor &k_cache, torch::Tensor &v_cache, c10::optional<torch::Tensor> k, c10::optional<torch::Tensor> v,
    torch::Tensor &cache_seqlens, c10::optional<torch::Tensor> block_table, c10::optional<torch::Tensor> q,
    c10::optional<torch::Tensor> rotary_cos, c10::optional<torch::Tensor> rotary_sin, const Fp8Descales *fp8) {
    TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4,
                "the caches must be 4-D [pages, heads, page_size, dim] or [batch, heads, seqlen, dim]");
    TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), "k_cache, v_cache must have the same shape");
    TORCH_CHECK(k_cache.dtype() == v_cache.dtype(), "k_cache, v_cache must have the same data type");
    // the 16-bit dtype of k / v / q / the tables: the caches' own, or with an fp8 cache the inputs'
    auto io_dtype = k_cache.dtype();
    if (fp8) {
        TORCH_CHECK(k_cache.dtype() == at::kFloat8_e4m3fn, "the fp8 caches must be torch.float8_e4m3fn");
        io_dtype = k.has_value() ? k->dtype() : q.has_value() ? q->dtype() : caffe2::TypeMeta::Make<at::Half>();
        TORCH_CHECK(io_dtype == torch::kHalf || io_dtype == torch::kBFloat16,
                    "k, v and q only support fp16 or bf16 data type");
    } else {
        TORCH_CHECK(k_cache.dtype() == torch::kHalf || k_cache.dtype() == torch::kBFloat16,
                    "the caches only support fp16 or bf16 data type");
    }
    TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && k_cache.device() == v_cache.device(),
                "the caches must be on the same CUDA device");
    TORCH_CHECK(k_cache.stride(3) == 1 && v_cache.stride(3) == 1,
                "the caches must be contiguous in the last dimension (they are written in place, never copied)");
    TORCH_CHECK(k_cache.size(1) > 0 && k_cache.size(2) > 0 && k_cache.size(3) > 0,
                "the caches must have at least one head, one row and one element per row");
    TORCH_CHECK(k.has_value() == v.has_value(), "k and v must be given together");
    TORCH_CHECK(rotary_cos.has_value() == rotary_sin.has_value(), "rotary_cos and rotary_sin must be given together");
    TORCH_CHECK(!q.has_value() || rotary_cos.has_value(), "q is rotated only: it needs rotary_cos / rotary_sin");
    const int64_t bs = cache_seqlens.dim() == 1 ? cache_seqlens.size(0) : -1;
    const int64_t hkv = k_cache.size(1), d = k_cache.size(3);
    TORCH_CHECK(cache_seqlens.dtype() == torch::kInt32 && bs >= 0, "cache_seqlens must be int32 [batch]");
    TORCH_CHECK(cache_seqlens.device() == k_cache.device(), "cache_seqlens must be on the device of the caches");
    const bool paged = block_table.has_value();
    if (paged) {
        check_table(*block_table, bs);
        TORCH_CHECK(block_table->device() == k_cache.device(), "block_table must be on the device of the caches");
        TORCH_CHECK(k_cache.size(0) > 0 && k_cache.size(2) % 32 == 0, "page_size must be a positive multiple of 32");
    } else {
        TORCH_CHECK(k_cache.size(0) == bs, "a dense cache must have cache_seqlens' batch size");
    }
    auto check_new = [&](const torch::Tensor &t, const char *name, int64_t heads_multiple_of) {
        TORCH_CHECK(t.dim() == 4 && t.size(0) == bs && t.size(3) == d, name, " must be [batch, heads, seqlen, dim] "
                    "with the batch of cache_seqlens and the caches' hidden dimension");
        TORCH_CHECK(t.size(1) > 0 && t.size(1) % heads_multiple_of == 0, name, ": wrong number of heads");
        TORCH_CHECK(t.dtype() == io_dtype, name, fp8 ? " must have the data type of k" : " must have the caches' data type");
        TORCH_CHECK(t.device() == k_cache.device(), name, " must be on the device of the caches");
        TORCH_CHECK(t.stride(3) == 1, name, " must be contiguous in the last dimension");
    };
    int64_t sn = 0, sq = 0, hq = 0;
    if (k.has_value()) {
        check_new(*k, "k", hkv);
        check_new(*v, "v", hkv);
        TORCH_CHECK(k->size(1) == hkv && k->sizes() == v->sizes(), "k, v must have the caches' number of heads");
        sn = k->size(2);
    }
    if (q.has_value()) {
        check_new(*q, "q", hkv);
        hq = q->size(1);
        sq = q->size(2);
    }
    torch::Tensor cs, sn_t;
    std::tie(cs, sn_t) = append_rope_tables(rotary_cos, rotary_sin, d, io_dtype, k_cache.device(),
                                            fp8 ? " must have the data type of k" : " must have the caches' data type");
    c10::DeviceGuard device_guard(k_cache.device());
    require_gfx950(k_cache.device());

    const int64_t page_size = k_cache.size(2), max_pages = paged ? block_table->size(1) : 1;
    torch::Tensor q_rot = q.has_value() ? torch::empty(q->sizes(), q->options())
                                        : torch::empty({0}, k_cache.options().dtype(io_dtype));
    if (bs == 0 || (sn == 0 && sq == 0))  // nothing to launch: the lengths, clamped as the kernel clamps them
        return {cache_seqlens.clamp(0, max_pages * page_size), q_rot};
    torch::Tensor sl = cache_seqlens.contiguous();
    torch::Tensor new_seqlens = torch::empty({bs}, sl.options());
    torch::Tensor bt;  // (undefined: the dense cache)
    if (paged) bt = table_with_contiguous_rows(*block_table);

    if (fp8) {  // the quantizing kernel moves 16 bytes per load: inputs that are not so aligned are copied
        if (k.has_value()) {
            k = aligned_or_contiguous(*k);
            v = aligned_or_contiguous(*v);
        }
        if (q.has_value()) q = aligned_or_contiguous(*q);
        if (cs.defined() && (cs.stride(0) % 8 != 0 || reinterpret_cast<uintptr_t>(cs.data_ptr()) % 16 != 0 ||
                             reinterpret_cast<uintptr_t>(sn_t.data_ptr()) % 16 != 0)) {
            cs = cs.clone(at::MemoryFormat::Contiguous);
            sn_t = sn_t.clone(at::MemoryFormat::Contiguous);
        }
    }
    fa_kvcache_fp8_params fp;
    memset(&fp, 0, sizeof(fp));
    fa_kvcache_params &p = fp.base;
    if (sn > 0) {
        p.k_new = k->data_ptr();
        p.v_new = v->data_ptr();
        p.kn_batch_stride = stride_or_zero(*k, 0);
        p.kn_head_stride = stride_or_zero(*k, 1);
        p.kn_seqlen_stride = stride_or_zero(*k, 2);
        p.vn_batch_stride = stride_or_zero(*v, 0);
        p.vn_head_stride = stride_or_zero(*v, 1);
        p.vn_seqlen_stride = stride_or_zero(*v, 2);
    }
    if (sq > 0) {
        p.q = q->data_ptr();
        p.q_out = q_rot.data_ptr();
        p.q_batch_stride = stride_or_zero(*q, 0);
        p.q_head_stride = stride_or_zero(*q, 1);
        p.q_seqlen_stride = stride_or_zero(*q, 2);
        p.qo_batch_stride = stride_or_zero(q_rot, 0);
        p.qo_head_stride = stride_or_zero(q_rot, 1);
        p.qo_seqlen_stride = stride_or_zero(q_rot, 2);
    }
    fill_append_cache(p, k_cache, v_cache, bt, sl, new_seqlens, cs, sn_t);
    p.num_heads_q = hq;
    p.seqlen_new = sn;
    p.seqlen_q = sq;
    if (fp8) {
        const auto descales = fill_descales(fp, *fp8, k_cache, bs, hkv);
        const int dtype = io_dtype == torch::kHalf ? FA_DTYPE_F16 : FA_DTYPE_BF16;
        check_rc(fa_kvcache_append_fp8_gfx950(&fp, dtype, current_stream(k_cache)), "fa_kvcache_append_fp8_gfx950");
        return {new_seqlens, q_rot};
    }
    check_rc(fa_kvcache_append_gfx950(&p, fa_dtype(k_cache), current_stream(k_cache)), "fa_kvcache_append_gfx950");
    return {new_seqlens, q_rot};
}

std::tuple<torch::Tensor, torch::Tensor> flash_attention_kvcache_append(
    torch::Tensor &k_cache, torch::Tensor &v_cache, c10::optional<torch::Tensor> k, c10::optional<torch::Tensor> v,
    torch::Tensor &cache_seqlens, c10::optional<torch::Tensor> block_table, c10::optional<torch::Tensor> q,
    c10::optional<torch::Tensor> rotary_cos, c10::optional<torch::Tensor> rotary_sin) {
    return kvcache_append_impl(k_cache, v_cache, k, v, cache_seqlens, block_table, q, rotary_cos, rotary_sin, nullptr);
}

std::tuple<torch::Tensor, torch::Tensor> flash_attention_kvcache_append_fp8(
    torch::Tensor &k_cache, torch::Tensor &v_cache, c10::optional<torch::Tensor> k, c10::optional<torch::Tensor> v,
    torch::Tensor &cache_seqlens, c10::optional<torch::Tensor> block_table, c10::optional<torch::Tensor> q,
    c10::optional<torch::Tensor> rotary_cos, c10::optional<torch::Tensor> rotary_sin,
    c10::optional<torch::Tensor> k_descale, c10::optional<torch::Tensor> v_descale) {
    const Fp8Descales ds = descales_of(k_descale, v_descale);
    return kvcache_append_impl(k_cache, v_cache, k, v, cache_seqlens, block_table, q, rotary_cos, rotary_sin, &ds);
}

// Ragged queries over a 16-bit paged cache (include/fa_gfx950_paged_varlen.h fa_fwd_gfx950_paged_varlen): q packed
// [total_q, Hq, D] with cu_seqlens_q int32 [B + 1] on the device, sequence b's rows its last positions over
// cache_seqlens[b] keys; the pool read in place by the paged fa_fwd_w4 (page_size a multiple of 64). q is read in
// place when its row and head strides are multiples of 8 and its base is 16-byte aligned (a slice of a fused QKV
// projection), else made contiguous, as flash_attention_varlen_fwd does. No host synchronisation.
//
// sinks (flash_attention_paged_varlen_sink_fwd, include/fa_gfx950_paged_varlen_sink.h): fp32 [Hq] on q's device, one
// extra softmax column per q-head of that logit and value 0; the same steps, the sink entry.
//
// with_lse (flash_attention_paged_varlen_lse_fwd, include/fa_gfx950_paged_varlen_lse.h): the launch also writes the
// natural-log LSE of every owned row, fp32 [Hq, total_q]; sinks may then be absent. `out` and `lse` of the struct are
// the destinations where the caller brought them (the two states of a shared-prefix step are written side by side
// into one stacked tensor, so their merge needs no copy), else allocated here; both hold the results afterwards.
struct RaggedLse {
    torch::Tensor out, lse;
};
torch::Tensor paged_varlen_impl(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                torch::Tensor &cu_seqlens_q, int64_t max_seqlen_q, torch::Tensor &block_table,
                                torch::Tensor &cache_seqlens, int64_t window_left, float softmax_scale, bool causal,
                                const torch::Tensor *sinks = nullptr, RaggedLse *with_lse = nullptr) {
    TORCH_CHECK(q.dim() == 3, "ragged q must be 3-D [total_q, heads, dim]");
    if (with_lse && with_lse->out.defined()) {
        const torch::Tensor &d = with_lse->out;
        TORCH_CHECK(d.sizes() == q.sizes() && d.dtype() == q.dtype() && d.device() == q.device(),
                    "out must have the shape, dtype and device of q");
        TORCH_CHECK(d.stride(2) == 1 && aligned_rows(d),
                    "out must have contiguous rows, strides that are multiples of 8 and a 16-byte aligned base");
    }
    if (with_lse && with_lse->lse.defined()) {
        const torch::Tensor &d = with_lse->lse;
        TORCH_CHECK(d.dim() == 2 && d.size(0) == q.size(1) && d.size(1) == q.size(0) && d.dtype() == torch::kFloat32 &&
                        d.device() == q.device(),
                    "lse must be fp32 [heads of q, total_q] on the device of q");
        TORCH_CHECK(d.stride(0) >= 0 && d.stride(1) >= 0, "lse must have non-negative strides");
    }
    torch::Tensor sinks_c;
    if (sinks) {
        TORCH_CHECK(sinks->dim() == 1 && sinks->size(0) == q.size(1) && sinks->dtype() == torch::kFloat32,
                    "sinks must be fp32 [heads of q]");
        TORCH_CHECK(sinks->device() == q.device(), "sinks must be on the device of q");
        sinks_c = sinks->contiguous();
    }
    check_pools(k_cache, v_cache, kPagedRagged);
    TORCH_CHECK(q.size(2) == k_cache.size(3), "q and the caches must have the same hidden dimension");
    TORCH_CHECK(q.size(1) > 0 && q.size(2) > 0, "q must have at least one head and one element per row");
    TORCH_CHECK(q.size(1) % k_cache.size(1) == 0,
                "number of heads in q must be multiple of number of heads in k and v");
    check_dtype(q, k_cache, v_cache);
    TORCH_CHECK(q.stride(2) == 1 && k_cache.stride(3) == 1 && v_cache.stride(3) == 1,
                "q, k, v must be contiguous in the last dimension");
    check_headdim_device(q, k_cache, v_cache);
    TORCH_CHECK(cu_seqlens_q.dtype() == torch::kInt32 && cu_seqlens_q.dim() == 1 && cu_seqlens_q.size(0) >= 1,
                "cu_seqlens_q must be int32 with batch_size + 1 entries");
    const int64_t bs = cu_seqlens_q.size(0) - 1;
    TORCH_CHECK(cu_seqlens_q.device() == q.device(), "cu_seqlens_q must be on the device of q");
    PagedCache cache = paged_cache(k_cache, v_cache, block_table, cache_seqlens, bs, q.device(), kPagedRagged);
    TORCH_CHECK(max_seqlen_q >= 0, "max_seqlen_q must be non-negative");
    c10::DeviceGuard device_guard(q.device());
    require_gfx950(q.device());

    auto o = with_lse && with_lse->out.defined() ? with_lse->out : torch::empty_like(q);
    if (with_lse) {
        if (!with_lse->lse.defined())
            with_lse->lse = torch::empty({q.size(1), q.size(0)}, q.options().dtype(torch::kFloat32));
        with_lse->out = o;
    }
    // nothing to launch: no row, no q-tile, or an empty step (batch 0, as the append and the C ABI take it)
    if (q.size(0) == 0 || max_seqlen_q == 0 || bs == 0) return o;
    torch::Tensor qx = aligned_rows(q) ? q : q.contiguous();
    if (!aligned_rows(o) || o.stride(2) != 1) o = torch::empty(q.sizes(), q.options());
    if (with_lse) with_lse->out = o;
    torch::Tensor cq = cu_seqlens_q.contiguous();

    fa_paged_varlen_params vp;
    memset(&vp, 0, sizeof(vp));
    fa_paged_params &pp = vp.paged;
    fa_fwd_params &params = pp.base;
    // (of the pools, fill_packed_params keeps the head count; fill_paged writes every other k / v field)
    fill_packed_params(params, qx, k_cache, v_cache, o, bs, max_seqlen_q, 0, softmax_scale);
    fill_paged(pp, cache);
    // The library checks q / o with the dense entry's rules -- every stride a multiple of 8, max_seqlen_q rows one
    // row stride apart -- also along a dimension of size 1, which in torch may carry any stride: a single head gets
    // 0 and a single row the dense row size. (flash_attention_varlen_fwd passes such strides as they are.)
    params.q_head_stride = stride_or_zero(qx, 1);
    params.o_head_stride = stride_or_zero(o, 1);
    params.q_seqlen_stride = qx.size(0) == 1 ? qx.size(1) * qx.size(2) : qx.stride(0);
    params.o_seqlen_stride = o.size(0) == 1 ? o.size(1) * o.size(2) : o.stride(0);
    vp.cu_seqlens_q = cq.data_ptr<int32_t>();
    vp.total_q = qx.size(0);
    const int dtype = fa_dtype(qx), c = causal ? 1 : 0;
    if (with_lse) {
        fa_paged_varlen_lse_params lp;
        memset(&lp, 0, sizeof(lp));
        lp.varlen = vp;
        lp.sinks = sinks ? sinks_c.data_ptr<float>() : nullptr;
        // (fill_lse on the [1, Hq, total_q] view: its head and row strides are this entry's two)
        struct {
            float *lse_ptr;
            int64_t lse_batch_stride, lse_head_stride, lse_seqlen_stride, seqlen_offset;
        } dst;
        fill_lse(dst, with_lse->lse.unsqueeze(0), 0);
        lp.lse_ptr = dst.lse_ptr;
        lp.lse_head_stride = dst.lse_head_stride;
        lp.lse_row_stride = dst.lse_seqlen_stride;
        launch_with_workspace(
            "fa_fwd_gfx950_paged_varlen_lse",
            [&] { return fa_fwd_gfx950_paged_varlen_lse_workspace_size(&lp, dtype, c, window_left); },
            [&](void *ws, int64_t ws_bytes) {
                return fa_fwd_gfx950_paged_varlen_lse(&lp, dtype, c, window_left, ws, ws_bytes, current_stream(qx));
            },
            qx.options());
        return o;
    }
    if (sinks) {
        fa_paged_varlen_sink_params sp;
        memset(&sp, 0, sizeof(sp));
        sp.varlen = vp;
        sp.sinks = sinks_c.data_ptr<float>();
        launch_with_workspace(
            "fa_fwd_gfx950_paged_varlen_sink",
            [&] { return fa_fwd_gfx950_paged_varlen_sink_workspace_size(&sp, dtype, c, window_left); },
            [&](void *ws, int64_t ws_bytes) {
                return fa_fwd_gfx950_paged_varlen_sink(&sp, dtype, c, window_left, ws, ws_bytes, current_stream(qx));
            },
            qx.options());
        return o;
    }
    launch_with_workspace(
        "fa_fwd_gfx950_paged_varlen",
        [&] { return fa_fwd_gfx950_paged_varlen_workspace_size(&vp, dtype, c, window_left); },
        [&](void *ws, int64_t ws_bytes) {
            return fa_fwd_gfx950_paged_varlen(&vp, dtype, c, window_left, ws, ws_bytes, current_stream(qx));
        },
        qx.options());
    return o;
}

torch::Tensor flash_attention_paged_varlen_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                               torch::Tensor &cu_seqlens_q, int64_t max_seqlen_q,
                                               torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                               int64_t window_left, float softmax_scale, bool causal) {
    return paged_varlen_impl(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table, cache_seqlens, window_left,
                             softmax_scale, causal);
}

// The same with attention sinks (include/fa_gfx950_paged_varlen_sink.h fa_fwd_gfx950_paged_varlen_sink): sinks fp32
// [Hq] on q's device, any Sq_b, window_left < 0 for no window.
torch::Tensor flash_attention_paged_varlen_sink_fwd(torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache,
                                                    torch::Tensor &cu_seqlens_q, int64_t max_seqlen_q,
                                                    torch::Tensor &block_table, torch::Tensor &cache_seqlens,
                                                    torch::Tensor &sinks, int64_t window_left, float softmax_scale,
                                                    bool causal) {
    return paged_varlen_impl(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table, cache_seqlens, window_left,
                             softmax_scale, causal, &sinks);
}

// The same that also returns the LSE (include/fa_gfx950_paged_varlen_lse.h fa_fwd_gfx950_paged_varlen_lse): sinks
// optional; (out [total_q, Hq, D], lse fp32 [Hq, total_q], natural log). out_dst / lse_dst: written in place and
// returned when given (views into a stacked pair of states), else allocated.
std::tuple<torch::Tensor, torch::Tensor> flash_attention_paged_varlen_lse_fwd(
    torch::Tensor &q, torch::Tensor &k_cache, torch::Tensor &v_cache, torch::Tensor &cu_seqlens_q,
    int64_t max_seqlen_q, torch::Tensor &block_table, torch::Tensor &cache_seqlens,
    c10::optional<torch::Tensor> sinks, int64_t window_left, float softmax_scale, bool causal,
    c10::optional<torch::Tensor> out_dst, c10::optional<torch::Tensor> lse_dst) {
    RaggedLse r{out_dst.has_value() ? *out_dst : torch::Tensor(), lse_dst.has_value() ? *lse_dst : torch::Tensor()};
    paged_varlen_impl(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table, cache_seqlens, window_left,
                      softmax_scale, causal, sinks.has_value() ? &*sinks : nullptr, &r);
    return {r.out, r.lse};
}

// Merge of PACKED partial states, the layout of the ragged step (fa_merge_states_gfx950 with B = 1, Sq = total_q: it
// takes every stride this needs): outs [N, total_q, H, D], lses [N, H, total_q] -> (out [total_q, H, D] contiguous,
// lse [H, total_q] or an empty tensor). One HIP pass, as flash_attention_merge_states.
std::tuple<torch::Tensor, torch::Tensor> flash_attention_merge_states_packed(torch::Tensor &outs, torch::Tensor &lses,
                                                                             bool return_lse) {
    TORCH_CHECK(outs.dim() == 4 && lses.dim() == 3, "packed outs must be [parts, total_q, heads, dim], lses "
                "[parts, heads, total_q]");
    TORCH_CHECK(outs.size(0) == lses.size(0) && outs.size(1) == lses.size(2) && outs.size(2) == lses.size(1),
                "packed outs [parts, total_q, heads, dim] and lses [parts, heads, total_q] must agree");
    torch::Tensor o = torch::empty({outs.size(1), outs.size(2), outs.size(3)}, outs.options());
    torch::Tensor lse = return_lse ? torch::empty({lses.size(1), lses.size(2)}, lses.options()) : torch::Tensor();
    torch::Tensor outs5 = outs.unsqueeze(1).transpose(2, 3), lses4 = lses.unsqueeze(1);
    torch::Tensor o4 = o.unsqueeze(0).transpose(1, 2), lse3 = return_lse ? lse.unsqueeze(0) : torch::Tensor();
    merge_states_into(outs5, lses4, o4, lse3);
    return {o, return_lse ? lse : torch::empty({0}, lses.options())};
}

// Ragged in-place KV-cache append with fused RoPE (include/fa_gfx950_kvcache_varlen.h
// fa_kvcache_append_varlen_gfx950): k / v packed [total_new, Hkv, D] with cu_seqlens_new int32 [B + 1], token i of
// sequence b written at position cache_seqlens[b] + i of the paged 16-bit cache; q packed [total_q, Hq, D] with
// its own cu_seqlens_q rotated at the sequence's last positions after the append. Returns (new_seqlens int32 [B],
// q_rot or an empty tensor). One launch, nothing copied, no host synchronisation (graph-capturable).
std::tuple<torch::Tensor, torch::Tensor> flash_attention_kvcache_append_varlen(
    torch::Tensor &k_cache, torch::Tensor &v_cache, torch::Tensor &k, torch::Tensor &v, torch::Tensor &cu_seqlens_new,
    torch::Tensor &cache_seqlens, torch::Tensor &block_table, c10::optional<torch::Tensor> rotary_cos,
    c10::optional<torch::Tensor> rotary_sin, c10::optional<torch::Tensor> q,
    c10::optional<torch::Tensor> cu_seqlens_q) {
    TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4, "the caches must be 4-D [pages, heads, page_size, dim]");
    TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), "k_cache, v_cache must have the same shape");
    TORCH_CHECK(k_cache.dtype() == v_cache.dtype(), "k_cache, v_cache must have the same data type");
    TORCH_CHECK(k_cache.dtype() == torch::kHalf || k_cache.dtype() == torch::kBFloat16,
                "the caches only support fp16 or bf16 data type");
    TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && k_cache.device() == v_cache.device(),
                "the caches must be on the same CUDA device");
    TORCH_CHECK(k_cache.stride(3) == 1 && v_cache.stride(3) == 1,
                "the caches must be contiguous in the last dimension (they are written in place, never copied)");
    TORCH_CHECK(k_cache.size(0) > 0 && k_cache.size(1) > 0 && k_cache.size(3) > 0 && k_cache.size(2) > 0 &&
                    k_cache.size(2) % 32 == 0,
                "the caches need at least one page and one head, and page_size a positive multiple of 32");
    TORCH_CHECK(rotary_cos.has_value() == rotary_sin.has_value(), "rotary_cos and rotary_sin must be given together");
    TORCH_CHECK(!q.has_value() || rotary_cos.has_value(), "q is rotated only: it needs rotary_cos / rotary_sin");
    TORCH_CHECK(q.has_value() == cu_seqlens_q.has_value(), "q and cu_seqlens_q must be given together");
    const auto dev = k_cache.device();
    const int64_t bs = cache_seqlens.dim() == 1 ? cache_seqlens.size(0) : -1;
    const int64_t hkv = k_cache.size(1), d = k_cache.size(3);
    TORCH_CHECK(cache_seqlens.dtype() == torch::kInt32 && bs >= 0, "cache_seqlens must be int32 [batch]");
    TORCH_CHECK(cache_seqlens.device() == dev, "cache_seqlens must be on the device of the caches");
    check_table(block_table, bs);
    TORCH_CHECK(block_table.device() == dev, "block_table must be on the device of the caches");
    auto check_cu = [&](const torch::Tensor &t, const char *name) {
        TORCH_CHECK(t.dtype() == torch::kInt32 && t.dim() == 1 && t.size(0) == bs + 1, name,
                    " must be int32 with batch + 1 entries");
        TORCH_CHECK(t.device() == dev, name, " must be on the device of the caches");
    };
    auto check_rows = [&](const torch::Tensor &t, const char *name, int64_t heads_multiple_of) {
        TORCH_CHECK(t.dim() == 3 && t.size(2) == d, name, " must be [total, heads, dim] with the caches' hidden dimension");
        TORCH_CHECK(t.size(1) > 0 && t.size(1) % heads_multiple_of == 0, name, ": wrong number of heads");
        TORCH_CHECK(t.dtype() == k_cache.dtype(), name, " must have the caches' data type");
        TORCH_CHECK(t.device() == dev, name, " must be on the device of the caches");
        TORCH_CHECK(t.stride(2) == 1, name, " must be contiguous in the last dimension");
    };
    check_cu(cu_seqlens_new, "cu_seqlens_new");
    check_rows(k, "k", hkv);
    check_rows(v, "v", hkv);
    TORCH_CHECK(k.size(1) == hkv && k.sizes() == v.sizes(), "k, v must have the caches' number of heads");
    if (q.has_value()) {
        check_cu(*cu_seqlens_q, "cu_seqlens_q");
        check_rows(*q, "q", hkv);
    }
    torch::Tensor cs, sn_t;
    std::tie(cs, sn_t) = append_rope_tables(rotary_cos, rotary_sin, d, k_cache.dtype(), dev,
                                            " must have the caches' data type");
    c10::DeviceGuard device_guard(dev);
    require_gfx950(dev);

    const int64_t tn = k.size(0), tq = q.has_value() ? q->size(0) : 0;
    torch::Tensor q_rot = q.has_value() ? torch::empty(q->sizes(), q->options()) : torch::empty({0}, k_cache.options());
    torch::Tensor sl = cache_seqlens.contiguous();
    torch::Tensor new_seqlens = torch::empty({bs}, sl.options());
    if (bs == 0) return {new_seqlens, q_rot};
    torch::Tensor bt = table_with_contiguous_rows(block_table);
    torch::Tensor cn = cu_seqlens_new.contiguous(), cq;

    fa_kvcache_varlen_params p;
    memset(&p, 0, sizeof(p));
    p.cu_seqlens_new = cn.data_ptr<int32_t>();
    p.total_new = tn;
    if (tn > 0) {
        p.k_new = k.data_ptr();
        p.v_new = v.data_ptr();
        p.kn_row_stride = stride_or_zero(k, 0);
        p.kn_head_stride = stride_or_zero(k, 1);
        p.vn_row_stride = stride_or_zero(v, 0);
        p.vn_head_stride = stride_or_zero(v, 1);
    }
    if (tq > 0) {
        cq = cu_seqlens_q->contiguous();
        p.cu_seqlens_q = cq.data_ptr<int32_t>();
        p.total_q = tq;
        p.q = q->data_ptr();
        p.q_out = q_rot.data_ptr();
        p.q_row_stride = stride_or_zero(*q, 0);
        p.q_head_stride = stride_or_zero(*q, 1);
        p.qo_row_stride = stride_or_zero(q_rot, 0);
        p.qo_head_stride = stride_or_zero(q_rot, 1);
        p.num_heads_q = q->size(1);
    }
    fill_append_cache(p, k_cache, v_cache, bt, sl, new_seqlens, cs, sn_t);
    check_rc(fa_kvcache_append_varlen_gfx950(&p, fa_dtype(k_cache), current_stream(k_cache)),
             "fa_kvcache_append_varlen_gfx950");
    return {new_seqlens, q_rot};
}

}  // namespace flash_attention

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("flash_attention_fwd", &flash_attention::flash_attention_fwd,
          "FlashAttention-2 forward, hand-written HIP kernel for MI355X / gfx950");
    m.def("flash_attention_varlen_fwd", &flash_attention::flash_attention_varlen_fwd,
          "FlashAttention-2 forward over packed variable-length sequences (cu_seqlens), gfx950");
    m.def("flash_attention_rope_fwd", &flash_attention::flash_attention_rope_fwd,
          "FlashAttention-2 forward with rotate-half RoPE applied to q in the kernel's Q load, gfx950");
    m.def("flash_attention_window_fwd", &flash_attention::flash_attention_window_fwd,
          "FlashAttention-2 forward with a local (sliding) window of window_left + 1 keys, gfx950");
    m.def("flash_attention_padded_fwd", &flash_attention::flash_attention_padded_fwd,
          "FlashAttention-2 forward over padded batches (per-sequence query / key ranges in dense tensors), gfx950");
    m.def("flash_attention_paged_fwd", &flash_attention::flash_attention_paged_fwd,
          "FlashAttention-2 decode over a paged KV cache (block table, per-sequence lengths), gfx950");
    m.def("rope_apply", &flash_attention::rope_apply, "rotate-half RoPE, one HIP pass (gfx950)");
    m.def("abi_version", []() { return fa_abi_version(); });
    m.def("paged_version", []() { return fa_paged_version(); });
    m.def("flash_attention_kvcache_append", &flash_attention::flash_attention_kvcache_append,
          "In-place KV-cache append (paged or dense) with fused rotate-half RoPE of k and q, one HIP launch (gfx950)");
    m.def("kvcache_version", []() { return fa_kvcache_version(); });
    m.def("flash_attention_paged_fp8_fwd", &flash_attention::flash_attention_paged_fp8_fwd,
          "FlashAttention-2 decode over a paged FP8 (e4m3) KV cache read in place, fp16 / bf16 q and o, gfx950");
    m.def("flash_attention_kvcache_append_fp8", &flash_attention::flash_attention_kvcache_append_fp8,
          "Quantizing in-place append to an FP8 (e4m3) KV cache with fused rotate-half RoPE, one HIP launch (gfx950)");
    m.def("fp8_version", []() { return fa_fp8_version(); });
    m.def("flash_attention_paged_window_fwd", &flash_attention::flash_attention_paged_window_fwd,
          "Sliding-window decode over a paged KV cache: pages below the window are never read, gfx950");
    m.def("flash_attention_paged_window_fp8_fwd", &flash_attention::flash_attention_paged_window_fp8_fwd,
          "Sliding-window decode over a paged FP8 (e4m3) KV cache read in place, gfx950");
    m.def("paged_window_version", []() { return fa_paged_window_version(); });
    m.def("flash_attention_paged_prefill_fwd", &flash_attention::flash_attention_paged_prefill_fwd,
          "Prefill-sized query blocks over a 16-bit paged KV cache read in place (page_size % 64 == 0), gfx950");
    m.def("paged_prefill_version", []() { return fa_paged_prefill_version(); });
    m.def("flash_attention_paged_lse_fwd", &flash_attention::flash_attention_paged_lse_fwd,
          "Paged decode (16-bit or FP8 pool) that also returns the softmax log-sum-exp, gfx950");
    m.def("flash_attention_merge_states", &flash_attention::flash_attention_merge_states,
          "Merge partial attention states (outputs and log-sum-exps over disjoint key sets), one HIP pass (gfx950)");
    m.def("lse_version", []() { return fa_lse_version(); });
    m.def("flash_attention_paged_sink_fwd", &flash_attention::flash_attention_paged_sink_fwd,
          "Paged KV-cache decode with attention sinks (one extra softmax column per q-head), windowed or not, gfx950");
    m.def("flash_attention_paged_sink_fp8_fwd", &flash_attention::flash_attention_paged_sink_fp8_fwd,
          "Paged FP8 (e4m3) KV-cache decode with attention sinks, windowed or not, gfx950");
    m.def("sink_version", []() { return fa_sink_version(); });
    m.def("flash_attention_paged_varlen_fwd", &flash_attention::flash_attention_paged_varlen_fwd,
          "Ragged (packed, cu_seqlens_q) query blocks over a 16-bit paged KV cache read in place, gfx950");
    m.def("paged_varlen_version", []() { return fa_paged_varlen_version(); });
    m.def("flash_attention_kvcache_append_varlen", &flash_attention::flash_attention_kvcache_append_varlen,
          "Ragged in-place append to a paged KV cache with fused rotate-half RoPE of k and q, one HIP launch (gfx950)");
    m.def("kvcache_varlen_version", []() { return fa_kvcache_varlen_version(); });
    m.def("flash_attention_paged_varlen_sink_fwd", &flash_attention::flash_attention_paged_varlen_sink_fwd,
          "Ragged query blocks over a 16-bit paged KV cache with attention sinks, windowed or not, gfx950");
    m.def("paged_varlen_sink_version", []() { return fa_paged_varlen_sink_version(); });
    m.def("flash_attention_paged_varlen_lse_fwd", &flash_attention::flash_attention_paged_varlen_lse_fwd,
          "Ragged query blocks over a 16-bit paged KV cache, returning (out, lse); sinks and window optional, gfx950");
    m.def("paged_varlen_lse_version", []() { return fa_paged_varlen_lse_version(); });
    m.def("flash_attention_merge_states_packed", &flash_attention::flash_attention_merge_states_packed,
          "Merge packed partial attention states ([N, total_q, H, D], lse [N, H, total_q]), one HIP pass (gfx950)");
}
