"""``flash_attention::forward`` custom op and ``flash_attn_func`` for MI355X.

Host-side mirror of reference flash_attention/flash_attention.py:1-53 -- same op name, schema,
registrations, default-scale rule and wrapper behaviour:

* ``torch.library.custom_op("flash_attention::forward", mutates_args=())`` whose default (CPU)
  implementation is ``F.scaled_dot_product_attention`` (reference :6-15);
* ``register_kernel(..., "cuda")`` -- ROCm devices report device type "cuda" -- which zero-pads
  the head dim to a multiple of 8, makes the last dim contiguous, calls the gfx950 extension
  (``flash_attention_fwd``) and slices the padding off again (reference :17-38);
* ``register_fake`` returning ``empty_like(q)`` (reference :40-43);
* ``flash_attn_func(q, k, v, softmax_scale=None, causal=False)`` with ``scale = D ** -0.5``
  computed on the UNPADDED head dim (reference :46-53).

GPU tensors always go through the hand-written HIP kernel: if the extension failed to load, the
"cuda" kernel raises instead of falling back to a PyTorch implementation.

Beyond the reference (its README.md:18 lists varlen as a TODO): ``flash_attention::varlen_forward``
/ ``flash_attn_varlen_func`` over packed variable-length sequences described by int32 ``cu_seqlens``
prefix sums (the layout a padding mask is lowered to; ``hf_attention`` does that lowering), with the
same registrations (CPU default, "cuda" kernel, fake) and the same pad / contiguity wrapper.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import Optional

import torch

from .load_cpp_extention import load_extension

try:
    flash_attention_cuda = load_extension()
    _load_error = None
except Exception as e:  # noqa: BLE001 -- surfaced when a GPU tensor reaches the op
    flash_attention_cuda = None
    _load_error = e


def _require_ext() -> None:
    """A GPU tensor reached an op but the extension did not load: an error, never another implementation."""
    if flash_attention_cuda is None:
        raise RuntimeError(f"gfx950 flash attention extension is not available: {_load_error!r}")


def _default_scale(q: torch.Tensor, softmax_scale):
    """``D ** -0.5`` on the UNPADDED head dim unless the caller gave a scale (reference :49-50). A given scale must
    be finite and > 0 -- the kernels track the running max of the unscaled scores -- and is refused here as the
    C-ABI refuses it (include/fa_gfx950.h), so the CPU defaults and the GPU kernels agree."""
    if softmax_scale is None:
        return q.size(-1) ** -0.5
    if not (math.isfinite(softmax_scale) and softmax_scale > 0):
        raise RuntimeError(f"softmax_scale must be finite and > 0 (got {softmax_scale})")
    return softmax_scale


def _padded_call(fn, tensors, *args):
    """``fn(*tensors, *args)`` as every "cuda" kernel calls the extension (reference :19-38): the tensors'
    head dim (their last) zero-padded to a multiple of 8 and made contiguous, the padding sliced off the
    result again."""
    head_dim = tensors[0].size(-1)
    pad = -head_dim % 8
    if pad:
        tensors = [torch.nn.functional.pad(t, [0, pad]) for t in tensors]
    attn = fn(*[t if t.stride(-1) == 1 else t.contiguous() for t in tensors], *args)
    return attn[..., :head_dim] if pad else attn


def _masked_sdpa(q, k, v, mask, softmax_scale):
    """torch SDPA with the kernel's semantics, for the CPU defaults: GQA, ``mask`` [Sq, Sk] bool (True =
    visible, or None), rows that see no key 0 as on the GPU."""
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=softmax_scale,
                                                         enable_gqa=True)
    if mask is not None:
        o = o.masked_fill(~mask.any(dim=1)[None, None, :, None], 0)
    return o


@torch.library.custom_op("flash_attention::forward", mutates_args=())
def flash_attention_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, softmax_scale: float = None,
                            causal: bool = False) -> torch.Tensor:
    # q: [batch_size, n_heads, q_seq_len, d]; k, v: [batch_size, n_heads_kv, kv_seq_len, d]
    # Non-GPU default, as in the reference: torch SDPA (top-left causal, no GQA expansion).
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.",
                  stacklevel=2)
    return torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=softmax_scale, is_causal=causal)


@torch.library.register_kernel("flash_attention::forward", "cuda")
def flash_attention_forward_cuda(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, softmax_scale: float = None,
                                 causal: bool = False) -> torch.Tensor:
    _require_ext()
    return _padded_call(flash_attention_cuda.flash_attention_fwd, (q, k, v), softmax_scale, causal)


@torch.library.register_fake("flash_attention::forward")
def flash_attention_forward_fake(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, softmax_scale: float = None,
                                 causal: bool = False) -> torch.Tensor:
    return torch.empty_like(q)


def flash_attn_func(q, k, v, softmax_scale=None, causal=False):
    # q: [batch_size, n_heads, q_seq_len, d]; k, v: [batch_size, n_heads_kv, kv_seq_len, d]
    softmax_scale = _default_scale(q, softmax_scale)
    return torch.ops.flash_attention.forward(q, k, v, softmax_scale, causal)


# ---------------------------------------------------------------------------------------------
# variable-length (packed) sequences -- no reference counterpart (reference README.md:18 TODO)
# ---------------------------------------------------------------------------------------------
def split_errors(reset: bool = False) -> int:
    """Key-split hand-offs on the current device that timed out since the last reset (include/fa_gfx950.h
    ``fa_split_errors``): a causal block split over two workgroups whose second piece did not see its
    partner's partial result within ~1 s, so its rows are wrong. 0 in a healthy run; one host
    synchronisation."""
    from . import _debug

    return int(_debug.lib().fa_split_errors(1 if reset else 0))


def _bottom_right_causal(sq: int, sk: int, device) -> torch.Tensor:
    """[sq, sk] bool, True = visible: key n is visible to query m iff n <= m + sk - sq
    (the kernel's causal convention, reference csrc/mask.cuh:37-39)."""
    m = torch.arange(sq, device=device)[:, None]
    n = torch.arange(sk, device=device)[None, :]
    return n <= m + (sk - sq)


@torch.library.custom_op("flash_attention::varlen_forward", mutates_args=())
def flash_attention_varlen_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor,
                                   cu_seqlens_k: torch.Tensor, max_seqlen_q: int, max_seqlen_k: int,
                                   softmax_scale: float = None, causal: bool = False,
                                   window_left: int = -1) -> torch.Tensor:
    # q: [total_q, n_heads, d]; k, v: [total_k, n_heads_kv, d]; cu_seqlens_*: int32 [batch_size + 1].
    # Non-GPU default: per-sequence torch SDPA with the kernel's semantics (bottom-right causal,
    # GQA, rows that see no key are 0; window_left >= 0: the local window per sequence).
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    out = torch.zeros_like(q)
    cq, ck = cu_seqlens_q.tolist(), cu_seqlens_k.tolist()
    for b in range(len(cq) - 1):
        q0, q1, k0, k1 = cq[b], cq[b + 1], ck[b], ck[b + 1]
        if q1 == q0 or k1 == k0:
            continue
        qs, ks, vs = (t.transpose(0, 1).unsqueeze(0) for t in (q[q0:q1], k[k0:k1], v[k0:k1]))
        if window_left >= 0:
            mask = _window_mask(q1 - q0, k1 - k0, window_left, causal, q.device)
        else:
            mask = _bottom_right_causal(q1 - q0, k1 - k0, q.device) if causal else None
        out[q0:q1] = _masked_sdpa(qs, ks, vs, mask, softmax_scale)[0].transpose(0, 1)
    return out


@torch.library.register_kernel("flash_attention::varlen_forward", "cuda")
def flash_attention_varlen_forward_cuda(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                        cu_seqlens_q: torch.Tensor, cu_seqlens_k: torch.Tensor, max_seqlen_q: int,
                                        max_seqlen_k: int, softmax_scale: float = None,
                                        causal: bool = False, window_left: int = -1) -> torch.Tensor:
    _require_ext()
    return _padded_call(flash_attention_cuda.flash_attention_varlen_fwd, (q, k, v), cu_seqlens_q, cu_seqlens_k,
                        max_seqlen_q, max_seqlen_k, softmax_scale, causal, int(window_left))


@torch.library.register_fake("flash_attention::varlen_forward")
def flash_attention_varlen_forward_fake(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                                        softmax_scale=None, causal=False, window_left=-1):
    return torch.empty_like(q)


def _check_varlen_enabled() -> bool:
    """FA_CHECK_VARLEN, read at every call (setting it after import takes effect)."""
    return os.environ.get("FA_CHECK_VARLEN", "0") not in ("", "0")


def _check_varlen_maxima(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
    """Raise if a sequence is longer than the max_seqlen the caller passed (FA_CHECK_VARLEN=1)."""
    for name, cu, mx in (("q", cu_seqlens_q, max_seqlen_q), ("k", cu_seqlens_k, max_seqlen_k)):
        longest = int((cu[1:] - cu[:-1]).max()) if cu.numel() > 1 else 0
        if longest > mx:
            raise ValueError(f"max_seqlen_{name}={mx} is smaller than the longest sequence ({longest}) "
                             f"in cu_seqlens_{name}")


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale=None,
                           causal=False, window_left=-1):
    """Attention over packed sequences: q [total_q, Hq, D], k/v [total_k, Hkv, D]; sequence b owns rows
    [cu_seqlens_q[b], cu_seqlens_q[b+1]) of q and [cu_seqlens_k[b], cu_seqlens_k[b+1]) of k/v
    (int32, on q's device). ``max_seqlen_q`` / ``max_seqlen_k`` must be the true maxima: the GPU grid
    is sized by ``max_seqlen_q``, so a smaller value leaves the rows of longer sequences uncomputed.
    With ``FA_CHECK_VARLEN=1`` in the environment (read at every call) both are verified against
    ``cu_seqlens_*`` (one host sync per call; off by default, as in the reference's varlen API).
    ``window_left >= 0``: the local window of ``flash_attn_window_func`` within each sequence."""
    softmax_scale = _default_scale(q, softmax_scale)
    if _check_varlen_enabled():
        _check_varlen_maxima(cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k))
    return torch.ops.flash_attention.varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q),
                                                    int(max_seqlen_k), softmax_scale, causal, int(window_left))


# ---------------------------------------------------------------------------------------------
# padded batches -- per-sequence ranges inside dense tensors (include/fa_gfx950.h
# fa_fwd_gfx950_padded); no reference counterpart (the reference drops attention_mask,
# models/rope_attn_fwd.py:40-64). An HF left / right padding mask is lowered to this: the KV cache
# and the projections are read in place, decode steps keep the q-head pack and split-KV kernel.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("flash_attention::padded_forward", mutates_args=())
def flash_attention_padded_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_start: torch.Tensor,
                                   k_end: torch.Tensor, q_start: Optional[torch.Tensor] = None,
                                   q_end: Optional[torch.Tensor] = None, softmax_scale: float = None,
                                   causal: bool = False, window_left: int = -1) -> torch.Tensor:
    # q: [B, Hq, Sq, D]; k, v: [B, Hkv, Sk, D]; batch row b's keys are positions [k_start[b], k_end[b])
    # and (optional) its queries [q_start[b], q_end[b]). Non-GPU default: per-sequence torch SDPA with
    # the kernel's semantics (bottom-right causal per sequence, GQA, rows outside / with no key 0).
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    out = torch.zeros_like(q)
    sq = q.size(2)
    ks, ke = k_start.tolist(), k_end.tolist()
    qs = q_start.tolist() if q_start is not None else [0] * q.size(0)
    qe = q_end.tolist() if q_end is not None else [sq] * q.size(0)
    for b in range(q.size(0)):
        q0, q1, k0, k1 = qs[b], qe[b], ks[b], ke[b]
        if q1 <= q0 or k1 <= k0:
            continue
        if window_left >= 0:
            mask = _window_mask(q1 - q0, k1 - k0, window_left, causal, q.device)
        else:
            # bottom-right per sequence (one query row sees every key, as the Sq == 1 pack's non-causal)
            mask = _bottom_right_causal(q1 - q0, k1 - k0, q.device) if causal else None
        out[b:b + 1, :, q0:q1] = _masked_sdpa(q[b:b + 1, :, q0:q1], k[b:b + 1, :, k0:k1], v[b:b + 1, :, k0:k1], mask,
                                              softmax_scale)
    return out


@torch.library.register_kernel("flash_attention::padded_forward", "cuda")
def flash_attention_padded_forward_cuda(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_start: torch.Tensor,
                                        k_end: torch.Tensor, q_start: Optional[torch.Tensor] = None,
                                        q_end: Optional[torch.Tensor] = None, softmax_scale: float = None,
                                        causal: bool = False, window_left: int = -1) -> torch.Tensor:
    _require_ext()
    return _padded_call(flash_attention_cuda.flash_attention_padded_fwd, (q, k, v), q_start, q_end, k_start, k_end,
                        softmax_scale, causal, int(window_left))


@torch.library.register_fake("flash_attention::padded_forward")
def flash_attention_padded_forward_fake(q, k, v, k_start, k_end, q_start=None, q_end=None, softmax_scale=None,
                                        causal=False, window_left=-1):
    return torch.empty_like(q)


def flash_attn_padded_func(q, k, v, k_start, k_end, q_start=None, q_end=None, softmax_scale=None, causal=False,
                           window_left=-1):
    """Attention over a padded batch read in place: q [B, Hq, Sq, D], k / v [B, Hkv, Sk, D] (any strides,
    e.g. HF projection views and the KV cache), batch row b's real keys at positions
    ``[k_start[b], k_end[b])`` and, optionally, its real queries at ``[q_start[b], q_end[b])`` (int32 [B]
    on q's device; default: every query row). Causal / window masks are bottom-right aligned per
    sequence; output rows outside the query ranges are 0. No host synchronisation (graph-capturable);
    Sq == 1 takes the q-head pack and the split-KV decode kernel."""
    softmax_scale = _default_scale(q, softmax_scale)
    return torch.ops.flash_attention.padded_forward(q, k, v, k_start, k_end, q_start, q_end, softmax_scale, causal,
                                                    int(window_left))


# ---------------------------------------------------------------------------------------------
# RoPE: the reference rotates q and k with elementwise torch ops before the
# call (reference models/rope_attn_fwd.py:8-38, :88). Here k is rotated in one HIP pass
# (``apply_rope``; the KV cache stores rotated keys) and q inside the attention kernel's Q load
# (``flash_attn_rope_func``).
# ---------------------------------------------------------------------------------------------
def _rope_reference(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x [B, H, S, D] * cos + rotate_half(x) * sin with cos / sin [B|1, S, D] or [S, D], in fp32,
    rounded once to x's dtype (the kernels' arithmetic up to the fma)."""
    cos = cos if cos.dim() == 3 else cos[None]
    sin = sin if sin.dim() == 3 else sin[None]
    xf = x.float()
    half = x.shape[-1] // 2
    rot = torch.cat((-xf[..., half:], xf[..., :half]), dim=-1)
    return (xf * cos.float()[:, None] + rot * sin.float()[:, None]).to(x.dtype)


@torch.library.custom_op("flash_attention::rope_apply", mutates_args=())
def flash_attention_rope_apply(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    return _rope_reference(x, cos, sin)


@torch.library.register_kernel("flash_attention::rope_apply", "cuda")
def flash_attention_rope_apply_cuda(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    _require_ext()
    x = x.contiguous() if x.stride(3) != 1 else x
    return flash_attention_cuda.rope_apply(x, cos.to(x.dtype), sin.to(x.dtype))


@torch.library.register_fake("flash_attention::rope_apply")
def flash_attention_rope_apply_fake(x, cos, sin):
    return torch.empty_like(x)


@torch.library.custom_op("flash_attention::rope_forward", mutates_args=())
def flash_attention_rope_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor,
                                 sin: torch.Tensor, softmax_scale: float = None, causal: bool = False) -> torch.Tensor:
    # q unrotated [B, Hq, Sq, D]; k (already rotated), v [B, Hkv, Sk, D]; cos / sin of q's positions.
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    return torch.nn.functional.scaled_dot_product_attention(_rope_reference(q, cos, sin), k, v, scale=softmax_scale,
                                                            is_causal=causal)


@torch.library.register_kernel("flash_attention::rope_forward", "cuda")
def flash_attention_rope_forward_cuda(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor,
                                      sin: torch.Tensor, softmax_scale: float = None,
                                      causal: bool = False) -> torch.Tensor:
    _require_ext()
    cos, sin = cos.to(q.dtype), sin.to(q.dtype)
    if q.size(3) % 8 != 0:  # padded head dims: rotate first (the halves are those of the real D)
        return flash_attention_forward_cuda(flash_attention_rope_apply_cuda(q, cos, sin), k, v, softmax_scale, causal)
    return _padded_call(flash_attention_cuda.flash_attention_rope_fwd, (q, k, v), cos, sin, softmax_scale, causal)


@torch.library.register_fake("flash_attention::rope_forward")
def flash_attention_rope_forward_fake(q, k, v, cos, sin, softmax_scale=None, causal=False):
    return torch.empty_like(q)


def apply_rope(x, cos, sin):
    """Rotate-half RoPE of x [B, H, S, D] with cos / sin [B|1, S, D] or [S, D] (one HIP pass on GPU)."""
    return torch.ops.flash_attention.rope_apply(x, cos, sin)


def flash_attn_rope_func(q, k, v, cos, sin, softmax_scale=None, causal=False):
    """``flash_attn_func(apply_rope(q, cos, sin), k, v, ...)`` with the rotation of q fused into the
    attention kernel's Q load; k must already be rotated (``apply_rope``)."""
    softmax_scale = _default_scale(q, softmax_scale)
    return torch.ops.flash_attention.rope_forward(q, k, v, cos, sin, softmax_scale, causal)


# ---------------------------------------------------------------------------------------------
# Local (sliding-window) attention -- the reference computes the Qwen2 sliding window and then
# ignores it (reference models/rope_attn_fwd.py:95-101); include/fa_gfx950.h fa_fwd_gfx950_window.
# ---------------------------------------------------------------------------------------------
def _window_mask(sq: int, sk: int, window_left: int, causal: bool, device) -> torch.Tensor:
    """[sq, sk] bool, True = visible: key n is visible to query m iff n >= m + sk - sq - window_left
    and, with causal, n <= m + sk - sq (transformers' sliding_window_causal_mask_function with
    sliding_window = window_left + 1, bottom-right aligned as the kernel's causal mask)."""
    m = torch.arange(sq, device=device)[:, None]
    n = torch.arange(sk, device=device)[None, :]
    vis = n >= m + (sk - sq) - window_left
    if causal:
        vis = vis & (n <= m + (sk - sq))
    return vis


@torch.library.custom_op("flash_attention::window_forward", mutates_args=())
def flash_attention_window_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, window_left: int,
                                   softmax_scale: float = None, causal: bool = False) -> torch.Tensor:
    # q: [B, Hq, Sq, D]; k, v: [B, Hkv, Sk, D]. Non-GPU default: torch SDPA under the window mask
    # (GQA expanded; rows that see no key are 0, as on the GPU).
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    return _masked_sdpa(q, k, v, _window_mask(q.size(2), k.size(2), window_left, causal, q.device), softmax_scale)


@torch.library.register_kernel("flash_attention::window_forward", "cuda")
def flash_attention_window_forward_cuda(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, window_left: int,
                                        softmax_scale: float = None, causal: bool = False) -> torch.Tensor:
    _require_ext()
    if window_left < 0:
        raise ValueError(f"window_left must be >= 0 (got {window_left})")
    return _padded_call(flash_attention_cuda.flash_attention_window_fwd, (q, k, v), int(window_left), softmax_scale,
                        causal)


@torch.library.register_fake("flash_attention::window_forward")
def flash_attention_window_forward_fake(q, k, v, window_left, softmax_scale=None, causal=False):
    return torch.empty_like(q)


def flash_attn_window_func(q, k, v, window_left, softmax_scale=None, causal=False):
    """``flash_attn_func`` where query m sees only keys n >= m + Sk - Sq - window_left: a sliding
    window of ``window_left + 1`` keys ending at the (bottom-right) diagonal with ``causal``.
    transformers' ``sliding_window`` W is ``window_left = W - 1`` (flash-attn ``window_size=(W - 1,
    -1)``)."""
    softmax_scale = _default_scale(q, softmax_scale)
    return torch.ops.flash_attention.window_forward(q, k, v, int(window_left), softmax_scale, causal)


# ---------------------------------------------------------------------------------------------
# Paged KV cache -- block-table attention on the split-KV decode kernel (include/fa_gfx950_paged.h
# fa_fwd_gfx950_paged); no reference counterpart (the reference has no KV cache). The layout of
# vLLM-style engines and flash-attn's flash_attn_with_kvcache(..., block_table=...): the caches are
# page pools [num_pages, Hkv, page_size, D], sequence b's key n is row n % page_size of page
# block_table[b][n / page_size], and it has cache_seqlens[b] keys.
# ---------------------------------------------------------------------------------------------
_PAGED_DECODE_MAX_ROWS = 64  # csrc/fa_launch.h kDecMaxRows: (q-head, position) rows per kv-head
_PAGED_PREFILL_TILE = 64  # csrc/fa_launch.h kBlockN: the paged prefill kernel's pages hold whole key tiles


def _gather_pages(cache: torch.Tensor, block_table: torch.Tensor) -> torch.Tensor:
    """The table's pages as a dense [B, Hkv, max_pages * page_size, D] (a copy; ids clamped into the pool
    as the kernel clamps them, so unused entries may hold anything)."""
    b, max_pages = block_table.shape
    num_pages, hkv, page_size, d = cache.shape
    ids = block_table.reshape(-1).clamp(0, num_pages - 1).to(torch.int64)
    pages = cache.index_select(0, ids).reshape(b, max_pages, hkv, page_size, d)
    return pages.transpose(1, 2).reshape(b, hkv, max_pages * page_size, d)


@torch.library.custom_op("flash_attention::paged_forward", mutates_args=())
def flash_attention_paged_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                  block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                  softmax_scale: float = None, causal: bool = False) -> torch.Tensor:
    # q: [B, Hq, Sq, D] (each sequence's last Sq positions); caches: [num_pages, Hkv, page_size, D];
    # block_table: int32 [B, max_pages]; cache_seqlens: int32 [B]. Non-GPU default: per-sequence gather
    # of the sequence's pages + torch SDPA with the kernel's semantics (bottom-right causal per sequence,
    # GQA, rows with no visible key 0, lengths clamped to the table's capacity).
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    return _paged_reference(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, -1)


def _sdpa_with_sink(q, k, v, mask, softmax_scale, sinks):
    """``_masked_sdpa`` with one extra softmax column per q-head, of logit ``sinks[h]`` (fp32 [Hq], final-logit
    units: not scaled) and value 0, in fp32: the column is concatenated to the scaled, masked scores. Rows that see
    no key are 0."""
    g = q.size(1) // k.size(1)
    scale = q.size(-1) ** -0.5 if softmax_scale is None else softmax_scale
    s = torch.matmul(q.float(), k.float().repeat_interleave(g, dim=1).transpose(2, 3)) * scale  # [1, Hq, Sq, n]
    if mask is not None:
        s = s.masked_fill(~mask[None, None], float("-inf"))
    col = sinks.float()[None, :, None, None].expand(s.size(0), -1, s.size(2), 1)
    p = torch.softmax(torch.cat([s, col], dim=-1), dim=-1)[..., :-1]
    p = torch.nan_to_num(p, nan=0.0)  # (a row whose every column is -inf)
    o = torch.matmul(p, v.float().repeat_interleave(g, dim=1))
    if mask is not None:
        o = o.masked_fill(~mask.any(dim=1)[None, None, :, None], 0)
    return o.to(q.dtype)


def _paged_reference(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, window_left, sinks=None):
    """The non-GPU default of the paged ops. With a window (``window_left >= 0``, ``_window_mask`` per
    sequence) the pages wholly below the sequence's first visible key are not gathered, as the kernel never
    reads them or their table entries. ``sinks`` (the sink ops): one extra softmax column per q-head."""
    out = torch.zeros_like(q)
    sq = q.size(2)
    num_pages, _, page_size, _ = k_cache.shape
    cap = block_table.size(1) * page_size
    for b, n in enumerate(cache_seqlens.tolist()):
        n = min(max(n, 0), cap)
        if n == 0:
            continue
        first = max(0, n - sq - window_left) // page_size if window_left >= 0 else 0  # the first page read
        k0 = first * page_size
        ids = block_table[b, first:(n + page_size - 1) // page_size].clamp(0, num_pages - 1).to(torch.int64)
        kb = k_cache.index_select(0, ids).transpose(0, 1).flatten(1, 2)[None, :, :n - k0]
        vb = v_cache.index_select(0, ids).transpose(0, 1).flatten(1, 2)[None, :, :n - k0]
        if window_left >= 0:
            mask = _window_mask(sq, n, window_left, causal, q.device)[:, k0:]
        else:
            mask = _bottom_right_causal(sq, n, q.device) if causal else None
        if sinks is not None:
            out[b:b + 1] = _sdpa_with_sink(q[b:b + 1], kb, vb, mask, softmax_scale, sinks)
        else:
            out[b:b + 1] = _masked_sdpa(q[b:b + 1], kb, vb, mask, softmax_scale)
    return out


@torch.library.register_kernel("flash_attention::paged_forward", "cuda")
def flash_attention_paged_forward_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                       block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                       softmax_scale: float = None, causal: bool = False) -> torch.Tensor:
    return _paged_cuda(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, -1)


def _paged_cuda(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal, window_left):
    _require_ext()
    g, sq = q.size(1) // k_cache.size(1), q.size(2)
    if g * sq > _PAGED_DECODE_MAX_ROWS:
        # larger query blocks (a chunked prefill on a paged cache): the paged prefill kernel reads a 16-bit
        # pool in place when a page holds whole 64-key tiles and the head dim needs no padding copy
        if k_cache.size(2) % _PAGED_PREFILL_TILE == 0 and q.size(3) % 8 == 0:
            return _padded_call(flash_attention_cuda.flash_attention_paged_prefill_fwd, (q, k_cache, v_cache),
                                block_table, cache_seqlens, int(window_left), softmax_scale, causal)
        # the copying path, for the other page sizes (32, 96, ...) and a padded head dim: the table's pages
        # are gathered into a dense cache for the padded entry (with the window, if any). No host
        # synchronisation either, so it stays graph-capturable.
        k = _gather_pages(k_cache, block_table)
        v = _gather_pages(v_cache, block_table)
        return flash_attention_padded_forward_cuda(q, k, v, torch.zeros_like(cache_seqlens), cache_seqlens, None,
                                                   None, softmax_scale, causal, window_left)
    # (a head dim that is no multiple of 8 pads the pool: a copy of it)
    if window_left >= 0:
        return _padded_call(flash_attention_cuda.flash_attention_paged_window_fwd, (q, k_cache, v_cache), block_table,
                            cache_seqlens, int(window_left), softmax_scale, causal)
    return _padded_call(flash_attention_cuda.flash_attention_paged_fwd, (q, k_cache, v_cache), block_table,
                        cache_seqlens, softmax_scale, causal)


@torch.library.register_fake("flash_attention::paged_forward")
def flash_attention_paged_forward_fake(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale=None,
                                       causal=False):
    return torch.empty_like(q)


# Sliding window over the paged cache (include/fa_gfx950_paged_window.h fa_fwd_gfx950_paged_window): ops of
# their own beside paged_forward / paged_forward_fp8, whose schemas stay as they are.
_MAX_WINDOW = 2 ** 30  # (the library clamps a larger window to this; it covers any capacity)


@torch.library.custom_op("flash_attention::paged_window_forward", mutates_args=())
def flash_attention_paged_window_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                         block_table: torch.Tensor, cache_seqlens: torch.Tensor, window_left: int,
                                         softmax_scale: float = None, causal: bool = False) -> torch.Tensor:
    # paged_forward where query m of sequence b sees only keys n >= m + L_b - Sq - window_left
    # (window_left < 0: no window). Non-GPU default: paged_forward's, under _window_mask per sequence.
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    return _paged_reference(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal,
                            min(int(window_left), _MAX_WINDOW))


@torch.library.register_kernel("flash_attention::paged_window_forward", "cuda")
def flash_attention_paged_window_forward_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                              block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                              window_left: int, softmax_scale: float = None,
                                              causal: bool = False) -> torch.Tensor:
    return _paged_cuda(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal,
                       min(int(window_left), _MAX_WINDOW))


@torch.library.register_fake("flash_attention::paged_window_forward")
def flash_attention_paged_window_forward_fake(q, k_cache, v_cache, block_table, cache_seqlens, window_left,
                                              softmax_scale=None, causal=False):
    return torch.empty_like(q)


def flash_attn_paged_func(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale=None, causal=False,
                          k_descale=None, v_descale=None, window_left=-1, return_lse=False, sinks=None):
    """Attention of q [B, Hq, Sq, D] -- each sequence's LAST Sq positions -- over a paged KV cache:
    ``k_cache`` / ``v_cache`` [num_pages, Hkv, page_size, D] with any strides (flash-attn's
    [num_pages, page_size, Hkv, D] is ``cache.transpose(1, 2)``), ``page_size`` a multiple of 32;
    ``block_table`` int32 [B, max_pages] and ``cache_seqlens`` int32 [B] on q's device. Sequence b's key n
    is row ``n % page_size`` of page ``block_table[b, n // page_size]``. Lengths are clamped to
    ``[0, max_pages * page_size]`` and page ids into the pool on the device; entries of pages a sequence
    does not reach, and the rows of its last page past its end, are never read. Causal masks are
    bottom-right aligned per sequence; a sequence without keys gives 0 rows.

    Decode shapes (``Hq / Hkv * Sq <= 64``) read the pool in place with the paged split-KV kernel. Larger
    query blocks (a prompt chunk over a cached prefix) read a 16-bit pool in place with the paged prefill
    kernel when ``page_size`` is a multiple of 64 and D a multiple of 8, bit-identical to
    ``flash_attn_padded_func`` on the gathered cache. They take the COPYING path -- the table's pages
    gathered into a dense cache (``index_select``) for ``flash_attn_padded_func`` -- for FP8 pools, other
    page sizes (32, 96, ...) and a padded head dim. No path synchronises with the host, so all can be
    captured in a graph.

    An FP8 cache (``torch.float8_e4m3fn`` pools, 16-byte aligned, D a multiple of 16; q and the output stay
    fp16 / bf16) is read in place by the FP8 paged kernel with the descales ``k_descale`` / ``v_descale``
    (fp32 [B, Hkv] on q's device, any strides; a Python float is expanded; None is 1.0): ``out = v_descale *
    softmax(softmax_scale * k_descale * q . K8^T) . V8`` with the bytes widened exactly. Its copying path
    multiplies the widened K by ``k_descale`` in q's dtype, which rounds K once more.

    ``window_left >= 0`` is a sliding window, per sequence, on either cache format: with ``L_b`` the clamped
    length, query m sees only keys ``n >= m + L_b - Sq - window_left`` (and ``n <= m + L_b - Sq`` with
    ``causal``): ``window_left + 1`` keys ending at the diagonal, flash-attn's ``window_size=(window_left,
    ...)``, transformers' ``sliding_window - 1``. The decode kernel then reads only the 32-key tiles from
    ``max(0, L_b - Sq - window_left) // 32`` on: PAGES WHOLLY BELOW THAT TILE, AND THEIR TABLE ENTRIES, ARE
    NEVER READ, so an engine may free them and leave anything in the entries; its splits are planned for the
    window, not the cache. The paged prefill kernel gives the same guarantee per 64-key tile (pages wholly
    below ``max(0, L_b - Sq - window_left) // 64 * 64`` and their entries are never read). The copying path
    passes the window to ``flash_attn_padded_func`` (it gathers every page of the table, so there the entries
    of freed pages must still be valid to clamp). ``window_left < 0``
    (the default) is no window: the call above, bit for bit.

    ``return_lse=True`` returns ``(out, lse)``: ``lse`` fp32 [B, Hq, Sq], the natural-log
    ``ln sum_n exp(softmax_scale * q . k_n)`` over each row's visible keys (flash-attn's ``softmax_lse``; with an
    FP8 cache the scale includes ``k_descale``, ``v_descale`` does not enter), ``-inf`` for a row without a
    visible key. ``out`` is bit-identical to the call without it. Decode shapes only and no window
    (``NotImplementedError`` otherwise), D a multiple of 8. Two such results over disjoint key sets combine
    with ``flash_attn_merge_states``. The default runs the unchanged call.

    ``sinks`` ([Hq] on q's device; fp32, or fp16 / bf16 converted once; ``ValueError`` for any other shape) are
    attention sinks, flash-attn's ``s_aux`` / vLLM's ``sinks``, as the gpt-oss models have them: one learned logit
    per q-head that joins the softmax denominator and contributes no value, ``out = (v_descale) sum_n exp(s_n - mu)
    v_n / (sum_n exp(s_n - mu) + exp(sinks[h] - mu))`` with ``mu = max(max_n s_n, sinks[h])`` over the row's
    visible keys. ``sinks`` is in final-logit units: NOT multiplied by ``softmax_scale`` or ``k_descale`` (HF's
    eager gpt-oss semantics, the column concatenated to the scaled, masked scores). Both cache formats, with or
    without ``window_left``; kernels of their own apply the sink once per row where the final row is produced
    (in a split launch: in the merge). ``-inf`` (anything at or below -1e30) on a head means no sink there: that
    head's rows have the bits of the call without ``sinks``. A row without a visible key stays 0. Decode shapes
    only (``Hq / Hkv * Sq <= 64``), D a multiple of 8, and not with ``return_lse=True``
    (``NotImplementedError`` each): a longer chunk with sinks, a uniform one too, goes through
    ``flash_attn_paged_varlen_func(..., sinks=)`` with a uniform ``cu_seqlens_q`` (q packed [B * Sq, Hq, D]).
    ``sinks=None`` is the call above, bit for bit."""
    softmax_scale = _default_scale(q, softmax_scale)
    window_left = int(window_left)
    if sinks is not None:
        return _paged_sink(q, k_cache, v_cache, block_table, cache_seqlens, sinks, window_left, softmax_scale, causal,
                           k_descale, v_descale, return_lse)
    if return_lse:
        return _paged_lse(q, k_cache, v_cache, block_table, cache_seqlens, 0, softmax_scale, causal, k_descale,
                          v_descale, window_left)
    if _is_fp8_cache(k_cache, v_cache, k_descale, v_descale):
        b, hkv = q.size(0), k_cache.size(1)
        kd = _descale_arg(k_descale, "k_descale", b, hkv, q.device)
        vd = _descale_arg(v_descale, "v_descale", b, hkv, q.device)
        if window_left >= 0:
            return torch.ops.flash_attention.paged_window_forward_fp8(q, k_cache, v_cache, block_table, cache_seqlens,
                                                                      window_left, kd, vd, softmax_scale, causal)
        return torch.ops.flash_attention.paged_forward_fp8(q, k_cache, v_cache, block_table, cache_seqlens, kd, vd,
                                                           softmax_scale, causal)
    if window_left >= 0:
        return torch.ops.flash_attention.paged_window_forward(q, k_cache, v_cache, block_table, cache_seqlens,
                                                              window_left, softmax_scale, causal)
    return torch.ops.flash_attention.paged_forward(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale,
                                                   causal)


# ---------------------------------------------------------------------------------------------
# KV-cache append -- the write side of the paged / dense cache, with RoPE fused in
# (include/fa_gfx950_kvcache.h fa_kvcache_append_gfx950); no reference counterpart. The append half of
# flash-attn's flash_attn_with_kvcache: new token i of sequence b goes to position n = cache_seqlens[b]
# + i, i.e. row n % page_size of page block_table[b][n / page_size] (dense cache: row n of batch row b).
# A write is dropped, never redirected: positions past the capacity and page ids outside the pool.
# ---------------------------------------------------------------------------------------------
@torch.library.custom_op("flash_attention::kvcache_append", mutates_args=("k_cache", "v_cache"))
def flash_attention_kvcache_append(k_cache: torch.Tensor, v_cache: torch.Tensor, k: Optional[torch.Tensor],
                                   v: Optional[torch.Tensor], cache_seqlens: torch.Tensor,
                                   block_table: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None,
                                   rotary_cos: Optional[torch.Tensor] = None,
                                   rotary_sin: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    # caches: [num_pages, Hkv, page_size, D] with block_table int32 [B, max_pages], or dense [B, Hkv, Smax,
    # D] without; k, v: [B, Hkv, Sn, D] (or None); q: [B, Hq, Sq, D] (or None); rotary_*: [max_pos, D].
    # Non-GPU default: the kernel's semantics token by token, with the same drop rules.
    if q is not None and rotary_cos is None:
        raise ValueError("q is rotated only: it needs rotary_cos / rotary_sin")
    num_pages, _, page_size, _ = k_cache.shape
    max_pages = block_table.size(1) if block_table is not None else 1
    cap = max_pages * page_size
    sn = k.size(2) if k is not None else 0
    lens = [min(max(n, 0), cap) for n in cache_seqlens.tolist()]
    new_lens = [min(n + sn, cap) for n in lens]
    table = block_table.tolist() if block_table is not None else None
    rope = rotary_cos is not None
    if rope:
        cos, sin = rotary_cos.to(k_cache.dtype), rotary_sin.to(k_cache.dtype)
        max_pos = cos.size(0)
    for b, n0 in enumerate(lens):
        for i in range(sn):
            n = n0 + i
            if n >= cap:
                continue  # past the table's capacity: dropped
            page = table[b][n // page_size] if table is not None else b
            if page < 0 or page >= num_pages:
                continue  # outside the pool: dropped, never clamped
            kr = k[b:b + 1, :, i:i + 1]
            if rope:
                pos = min(n, max_pos - 1)
                kr = _rope_reference(kr, cos[pos:pos + 1], sin[pos:pos + 1])
            k_cache[page, :, n % page_size] = kr[0, :, 0]
            v_cache[page, :, n % page_size] = v[b, :, i]
    if q is None:
        q_rot = k_cache.new_empty(0)
    else:
        sq = q.size(2)
        pos = torch.tensor([[min(max(e - sq + i, 0), max_pos - 1) for i in range(sq)] for e in new_lens],
                           dtype=torch.int64, device=q.device).reshape(-1, sq)
        q_rot = _rope_reference(q, cos[pos], sin[pos])
    return torch.tensor(new_lens, dtype=torch.int32, device=cache_seqlens.device), q_rot


@torch.library.register_kernel("flash_attention::kvcache_append", "cuda")
def flash_attention_kvcache_append_cuda(k_cache: torch.Tensor, v_cache: torch.Tensor, k: Optional[torch.Tensor],
                                        v: Optional[torch.Tensor], cache_seqlens: torch.Tensor,
                                        block_table: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None,
                                        rotary_cos: Optional[torch.Tensor] = None,
                                        rotary_sin: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    _require_ext()
    # the inputs may be copied to make their last dimension contiguous; the caches never are (a copy would
    # swallow the write): the binding rejects a cache whose last dimension is not contiguous
    k, v, q = (t.contiguous() if t is not None and t.stride(3) != 1 else t for t in (k, v, q))
    if rotary_cos is not None:
        rotary_cos, rotary_sin = rotary_cos.to(k_cache.dtype), rotary_sin.to(k_cache.dtype)
    new_seqlens, q_rot = flash_attention_cuda.flash_attention_kvcache_append(
        k_cache, v_cache, k, v, cache_seqlens, block_table, q, rotary_cos, rotary_sin)
    return new_seqlens, q_rot


@torch.library.register_fake("flash_attention::kvcache_append")
def flash_attention_kvcache_append_fake(k_cache, v_cache, k, v, cache_seqlens, block_table=None, q=None,
                                        rotary_cos=None, rotary_sin=None):
    q_rot = k_cache.new_empty(0) if q is None else torch.empty(q.shape, dtype=q.dtype, device=q.device)
    return torch.empty_like(cache_seqlens, memory_format=torch.contiguous_format), q_rot


def flash_attn_kvcache_append(k_cache, v_cache, k, v, cache_seqlens, block_table=None, rotary_cos=None,
                              rotary_sin=None, k_descale=None, v_descale=None):
    """Append the new keys / values ``k`` / ``v`` [B, Hkv, Sn, D] to a KV cache IN PLACE, one HIP launch:
    token i of sequence b is written at position ``n = cache_seqlens[b] + i`` -- row ``n % page_size`` of
    page ``block_table[b, n // page_size]`` of the pools ``k_cache`` / ``v_cache`` [num_pages, Hkv,
    page_size, D] (the layout ``flash_attn_paged_func`` reads), or, without a table, row n of batch row b of
    a dense cache [B, Hkv, Smax, D] (the layout ``flash_attn_padded_func`` reads). With ``rotary_cos`` /
    ``rotary_sin`` [max_pos, D] (``apply_rope``'s full-width rotate-half tables) k is rotated at position n
    on the way, bit for bit as ``apply_rope`` would; v is stored as it is. Returns ``new_seqlens``
    (int32 [B], a new tensor: ``min(cache_seqlens + Sn, capacity)``; ``cache_seqlens`` is not modified).

    A write is DROPPED, never redirected: tokens past the capacity ``max_pages * page_size`` (``Smax``)
    and tokens whose page id lies outside ``[0, num_pages)`` are not written -- unlike the read path,
    which clamps ids, because a clamped write would corrupt another sequence's page. Negative lengths
    count as 0; positions past the tables use their last row. Two sequences that write the same physical
    row are the caller's error. The caches are never copied (any strides with a contiguous last dimension,
    any alignment); no host synchronisation, so the call can be captured in a graph.

    An FP8 cache (``torch.float8_e4m3fn``; k / v fp16 or bf16) is QUANTIZED on the way in with the descales
    ``k_descale`` / ``v_descale`` (fp32 [B, Hkv], a Python float, or None = 1.0): ``byte = e4m3_rne(clamp(x /
    descale, -448, 448))``, x the rotated key already rounded to k's dtype (V: the input). It needs a 16-byte
    aligned cache with strides that are multiples of 16 and D a multiple of 16."""
    if _is_fp8_cache(k_cache, v_cache, k_descale, v_descale):
        b, hkv = cache_seqlens.size(0), k_cache.size(1)
        return torch.ops.flash_attention.kvcache_append_fp8(
            k_cache, v_cache, k, v, cache_seqlens, block_table, None, rotary_cos, rotary_sin,
            _descale_arg(k_descale, "k_descale", b, hkv, k_cache.device),
            _descale_arg(v_descale, "v_descale", b, hkv, k_cache.device))[0]
    return torch.ops.flash_attention.kvcache_append(k_cache, v_cache, k, v, cache_seqlens, block_table, None,
                                                    rotary_cos, rotary_sin)[0]


def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, rotary_cos=None, rotary_sin=None,
                            cache_seqlens=None, block_table=None, softmax_scale=None, causal=False,
                            return_seqlens=False, k_descale=None, v_descale=None, window_left=-1,
                            shared_prefix_len=0, sinks=None):
    """flash-attn's ``flash_attn_with_kvcache`` in this project's [B, H, S, D] layout: one serving step on
    a paged (``block_table`` given) or dense KV cache. When ``k`` / ``v`` [B, Hkv, Sn, D] are given they are
    appended in place at ``cache_seqlens`` (``flash_attn_kvcache_append``: the same drop rules); when the
    rotary tables [max_pos, D] are given, k is rotated at its new positions and q [B, Hq, Sq, D] at the
    sequence's last Sq positions after the append -- K, V and q in ONE launch. Then q attends over the
    cache up to the advanced lengths: ``flash_attn_paged_func`` with a table, ``flash_attn_padded_func``
    over ``[0, new_seqlens)`` without. Returns the attention output, or ``(out, new_seqlens)`` with
    ``return_seqlens=True``; ``cache_seqlens`` (required, int32 [B]) is not modified -- the caller copies
    ``new_seqlens`` into it (``cache_seqlens.copy_(new_seqlens)``) or takes them from
    ``flash_attn_kvcache_append``. No host synchronisation (graph-capturable).

    With FP8 caches (``torch.float8_e4m3fn``) and the descales ``k_descale`` / ``v_descale`` (fp32 [B, Hkv], a
    Python float, or None = 1.0) the append quantizes and the FP8 paged kernel reads the bytes in place. A
    dense FP8 cache [B, Hkv, Smax, D] is read by the same kernel through an identity table (batch row b is
    page b, ``page_size = Smax``), so ``Smax`` must be a multiple of 32 (``ValueError`` otherwise): there
    is no FP8 variant of the padded prefill kernel.

    ``window_left >= 0`` (flash-attn's ``window_size=(window_left, ...)``) windows the attention half as
    ``flash_attn_paged_func(window_left=...)`` does; the append is unchanged. On a paged cache, and on a dense
    FP8 cache through its identity table, the windowed paged kernel never reads the pages below the window. On
    a dense 16-bit cache a decode step (``Sq == 1``) folds the window into its key range on the device,
    ``[max(new_seqlens - 1 - window_left, 0), new_seqlens)``, and runs the split-KV decode kernel; ``Sq > 1``
    passes the window to ``flash_attn_padded_func``. Still no host synchronisation.

    ``shared_prefix_len > 0`` runs the attention half as ``flash_attn_paged_shared_prefix_func(...,
    prefix_len=shared_prefix_len)`` over the advanced lengths (its contract applies): paged caches only, decode
    steps (``Sq == 1``) only, no window (``ValueError`` otherwise); the append is unchanged. The default 0 is the
    call above, bit for bit.

    ``sinks`` ([Hq], see ``flash_attn_paged_func``) runs the attention half as ``flash_attn_paged_func(...,
    sinks=sinks)`` over the advanced lengths; the append is unchanged. Only the paged decode kernels have sinks, so
    a DENSE 16-bit cache [B, Hkv, Smax, D] is then read through an identity table as the dense FP8 cache is
    (batch row b is page b, ``page_size = Smax``): ``Smax`` must be a multiple of 32, ``ValueError`` otherwise --
    the padded kernels have no sinks and nothing is copied. Not with ``shared_prefix_len`` (``ValueError``).
    ``sinks=None`` is the call above, bit for bit."""
    window_left = int(window_left)
    shared_prefix_len = int(shared_prefix_len)
    if sinks is not None:
        if shared_prefix_len:
            raise ValueError("shared_prefix_len and sinks cannot be combined")
        sinks = _sinks_arg(sinks, q)  # (the errors of the attention half, before anything is appended)
        _check_sink_shape(q, k_cache)
        if block_table is None and k_cache.size(2) % 32 != 0:
            raise ValueError(f"with sinks a dense cache is read through the paged kernel: its length "
                             f"({k_cache.size(2)}) must be a multiple of 32")
    if shared_prefix_len:
        if block_table is None:
            raise ValueError("shared_prefix_len applies to a paged cache (block_table) only")
        if q.size(2) != 1:
            raise ValueError(f"shared_prefix_len applies to decode steps (Sq == 1) only (got Sq = {q.size(2)})")
        if window_left >= 0:
            raise ValueError("shared_prefix_len and window_left cannot be combined")
    if cache_seqlens is None:
        raise ValueError("flash_attn_with_kvcache needs cache_seqlens (int32 [batch])")
    if (k is None) != (v is None):
        raise ValueError("k and v must be given together")
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError("rotary_cos and rotary_sin must be given together")
    softmax_scale = _default_scale(q, softmax_scale)
    new_seqlens, q_rot = cache_seqlens, q
    if _is_fp8_cache(k_cache, v_cache, k_descale, v_descale):
        b, hkv = q.size(0), k_cache.size(1)
        if block_table is None and k_cache.size(2) % 32 != 0:
            raise ValueError(f"a dense fp8 cache is read through the paged kernel: its length ({k_cache.size(2)}) "
                             "must be a multiple of 32")
        kd = _descale_arg(k_descale, "k_descale", b, hkv, q.device)
        vd = _descale_arg(v_descale, "v_descale", b, hkv, q.device)
        if rotary_cos is not None:
            new_seqlens, q_rot = torch.ops.flash_attention.kvcache_append_fp8(
                k_cache, v_cache, k, v, cache_seqlens, block_table, q, rotary_cos.to(q.dtype), rotary_sin.to(q.dtype),
                kd, vd)
        elif k is not None:
            new_seqlens, _ = torch.ops.flash_attention.kvcache_append_fp8(
                k_cache, v_cache, k, v, cache_seqlens, block_table, None, None, None, kd, vd)
        table = block_table
        if table is None:  # a dense cache: batch row b is page b
            table = torch.arange(b, dtype=torch.int32, device=q.device)[:, None]
        if sinks is not None:
            out = _paged_sink(q_rot, k_cache, v_cache, table, new_seqlens, sinks, window_left, softmax_scale, causal,
                              kd, vd)
        elif shared_prefix_len:
            out = flash_attn_paged_shared_prefix_func(q_rot, k_cache, v_cache, table, new_seqlens, shared_prefix_len,
                                                      softmax_scale, causal, kd, vd)
        elif window_left >= 0:
            out = torch.ops.flash_attention.paged_window_forward_fp8(q_rot, k_cache, v_cache, table, new_seqlens,
                                                                     window_left, kd, vd, softmax_scale, causal)
        else:
            out = torch.ops.flash_attention.paged_forward_fp8(q_rot, k_cache, v_cache, table, new_seqlens, kd, vd,
                                                              softmax_scale, causal)
        return (out, new_seqlens) if return_seqlens else out
    if rotary_cos is not None:  # (cast as apply_rope casts its tables)
        new_seqlens, q_rot = torch.ops.flash_attention.kvcache_append(
            k_cache, v_cache, k, v, cache_seqlens, block_table, q, rotary_cos.to(q.dtype), rotary_sin.to(q.dtype))
    elif k is not None:
        new_seqlens, _ = torch.ops.flash_attention.kvcache_append(k_cache, v_cache, k, v, cache_seqlens, block_table)
    if sinks is not None:
        table = block_table
        if table is None:  # a dense cache: batch row b is page b
            table = torch.arange(q.size(0), dtype=torch.int32, device=q.device)[:, None]
        out = _paged_sink(q_rot, k_cache, v_cache, table, new_seqlens, sinks, window_left, softmax_scale, causal,
                          None, None)
    elif shared_prefix_len:
        out = flash_attn_paged_shared_prefix_func(q_rot, k_cache, v_cache, block_table, new_seqlens, shared_prefix_len,
                                                  softmax_scale, causal)
    elif block_table is not None:
        out = flash_attn_paged_func(q_rot, k_cache, v_cache, block_table, new_seqlens, softmax_scale, causal,
                                    window_left=window_left)
    elif window_left >= 0 and q.size(2) == 1:
        # one query row: its window IS a key range (no row-dependent bound), so the padded decode kernel serves it
        k_start = (new_seqlens - 1 - min(window_left, _MAX_WINDOW)).clamp(min=0)
        out = flash_attn_padded_func(q_rot, k_cache, v_cache, k_start, new_seqlens, softmax_scale=softmax_scale,
                                     causal=causal)
    else:
        out = flash_attn_padded_func(q_rot, k_cache, v_cache, torch.zeros_like(new_seqlens), new_seqlens,
                                     softmax_scale=softmax_scale, causal=causal, window_left=window_left)
    return (out, new_seqlens) if return_seqlens else out


# ---------------------------------------------------------------------------------------------
# FP8 (OCP e4m3, torch.float8_e4m3fn) KV cache -- a quantizing append and an in-place paged decode
# (include/fa_gfx950_fp8.h); no reference counterpart (its README lists quantized types as a TODO). The
# cache format of vLLM-style engines and of flash-attn's k_descale / v_descale. Scales are DESCALES: fp32,
# positive, one per (batch row, kv-head); q and the output stay fp16 / bf16.
#   read:   out = v_descale[b,h] * softmax((softmax_scale * k_descale[b,h]) * q . T(K8)^T) . T(V8)
#   write:  byte = e4m3_rne(clamp(fp32(x) / descale[b,h], -448, 448))
# ---------------------------------------------------------------------------------------------
FP8_DTYPE = torch.float8_e4m3fn
FP8_MAX = 448.0
_FP8_UNSUPPORTED = tuple(getattr(torch, n) for n in ("float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz")
                         if hasattr(torch, n))


def _is_fp8_cache(k_cache, v_cache, k_descale, v_descale) -> bool:
    """Whether the caches are the FP8 format the kernels serve; the wrappers' dtype errors."""
    if k_cache.dtype != v_cache.dtype:
        raise ValueError(f"k_cache and v_cache must have the same data type (got {k_cache.dtype} and {v_cache.dtype})")
    if k_cache.dtype in _FP8_UNSUPPORTED:
        raise ValueError(f"an 8-bit KV cache must be torch.float8_e4m3fn (OCP e4m3), not {k_cache.dtype}")
    fp8 = k_cache.dtype == FP8_DTYPE
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise ValueError(f"k_descale / v_descale go with a torch.float8_e4m3fn cache, not {k_cache.dtype}")
    return fp8


def _descale_arg(x, name, batch, heads_kv, device):
    """None, a Python number (expanded, stride 0) or an fp32 tensor broadcastable to [B, Hkv] on ``device``."""
    if x is None:
        return None
    if isinstance(x, (int, float)):
        return torch.full((1, 1), float(x), dtype=torch.float32, device=device).expand(batch, heads_kv)
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise ValueError(f"{name} must be an fp32 tensor [batch, kv heads], a Python float or None")
    if x.device != torch.device(device):
        raise ValueError(f"{name} must be on {device} (got {x.device})")
    try:
        return x.expand(batch, heads_kv)
    except RuntimeError as e:
        raise ValueError(f"{name} must be [batch, kv heads] = [{batch}, {heads_kv}] (got {tuple(x.shape)})") from e


def quantize_e4m3(x: torch.Tensor, descale) -> torch.Tensor:
    """``e4m3_rne(clamp(fp32(x) / descale, -448, 448))``: the write formula (descale broadcasts against x)."""
    return (x.float() / descale).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)


def _descale_or_ones(x, batch, heads_kv, device):
    return torch.ones(batch, heads_kv, dtype=torch.float32, device=device) if x is None else x.to(torch.float32)


@torch.library.custom_op("flash_attention::paged_forward_fp8", mutates_args=())
def flash_attention_paged_forward_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                      block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                      k_descale: Optional[torch.Tensor] = None,
                                      v_descale: Optional[torch.Tensor] = None, softmax_scale: float = None,
                                      causal: bool = False) -> torch.Tensor:
    # Non-GPU default: dequantize and reuse paged_forward's default, in fp32 so that folding the per-(b, h)
    # descales into q and the output rounds nothing
    return _paged_fp8_reference(q, k_cache, v_cache, block_table, cache_seqlens, k_descale, v_descale, softmax_scale,
                                causal, -1)


def _paged_fp8_reference(q, k_cache, v_cache, block_table, cache_seqlens, k_descale, v_descale, softmax_scale, causal,
                         window_left, sinks=None):
    b, hkv = q.size(0), k_cache.size(1)
    g = q.size(1) // hkv
    kd = _descale_or_ones(k_descale, b, hkv, q.device).repeat_interleave(g, dim=1)[:, :, None, None]
    vd = _descale_or_ones(v_descale, b, hkv, q.device).repeat_interleave(g, dim=1)[:, :, None, None]
    scale = q.size(-1) ** -0.5 if softmax_scale is None else softmax_scale
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=3)
    out = _paged_reference(q.float() * kd, k_cache.float(), v_cache.float(), block_table, cache_seqlens, scale, causal,
                           window_left, sinks)
    return (out * vd).to(q.dtype)


@torch.library.register_kernel("flash_attention::paged_forward_fp8", "cuda")
def flash_attention_paged_forward_fp8_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                           block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                           k_descale: Optional[torch.Tensor] = None,
                                           v_descale: Optional[torch.Tensor] = None, softmax_scale: float = None,
                                           causal: bool = False) -> torch.Tensor:
    return _paged_fp8_cuda(q, k_cache, v_cache, block_table, cache_seqlens, k_descale, v_descale, softmax_scale, causal,
                           -1)


def _paged_fp8_cuda(q, k_cache, v_cache, block_table, cache_seqlens, k_descale, v_descale, softmax_scale, causal,
                    window_left):
    _require_ext()
    hkv = k_cache.size(1)
    g, sq = q.size(1) // hkv, q.size(2)
    if g * sq > _PAGED_DECODE_MAX_ROWS:
        # the copying path of paged_forward: gather the bytes, widen them to q's dtype (exact), fold k_descale
        # into the widened K (one more rounding of K, in q's dtype) and v_descale into the output
        k = _gather_pages(k_cache.view(torch.uint8), block_table).view(FP8_DTYPE).to(q.dtype)
        v = _gather_pages(v_cache.view(torch.uint8), block_table).view(FP8_DTYPE).to(q.dtype)
        if k_descale is not None:
            k = k * k_descale[:, :, None, None].to(q.dtype)
        out = flash_attention_padded_forward_cuda(q, k, v, torch.zeros_like(cache_seqlens), cache_seqlens, None, None,
                                                  softmax_scale, causal, window_left)
        if v_descale is not None:
            out = (out.float() * v_descale.repeat_interleave(g, dim=1)[:, :, None, None]).to(q.dtype)
        return out
    # the pool is read in place, never padded or copied: the library rejects D % 16 != 0 and misaligned pools
    if window_left >= 0:
        return flash_attention_cuda.flash_attention_paged_window_fp8_fwd(
            q if q.stride(-1) == 1 else q.contiguous(), k_cache, v_cache, block_table, cache_seqlens, int(window_left),
            k_descale, v_descale, softmax_scale, causal)
    return flash_attention_cuda.flash_attention_paged_fp8_fwd(
        q if q.stride(-1) == 1 else q.contiguous(), k_cache, v_cache, block_table, cache_seqlens, k_descale,
        v_descale, softmax_scale, causal)


@torch.library.register_fake("flash_attention::paged_forward_fp8")
def flash_attention_paged_forward_fp8_fake(q, k_cache, v_cache, block_table, cache_seqlens, k_descale=None,
                                           v_descale=None, softmax_scale=None, causal=False):
    return torch.empty_like(q)


@torch.library.custom_op("flash_attention::paged_window_forward_fp8", mutates_args=())
def flash_attention_paged_window_forward_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                             block_table: torch.Tensor, cache_seqlens: torch.Tensor, window_left: int,
                                             k_descale: Optional[torch.Tensor] = None,
                                             v_descale: Optional[torch.Tensor] = None, softmax_scale: float = None,
                                             causal: bool = False) -> torch.Tensor:
    # paged_forward_fp8 under the sliding window of paged_window_forward (window_left < 0: no window)
    return _paged_fp8_reference(q, k_cache, v_cache, block_table, cache_seqlens, k_descale, v_descale, softmax_scale,
                                causal, min(int(window_left), _MAX_WINDOW))


@torch.library.register_kernel("flash_attention::paged_window_forward_fp8", "cuda")
def flash_attention_paged_window_forward_fp8_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                                  block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                                  window_left: int, k_descale: Optional[torch.Tensor] = None,
                                                  v_descale: Optional[torch.Tensor] = None,
                                                  softmax_scale: float = None, causal: bool = False) -> torch.Tensor:
    return _paged_fp8_cuda(q, k_cache, v_cache, block_table, cache_seqlens, k_descale, v_descale, softmax_scale, causal,
                           min(int(window_left), _MAX_WINDOW))


@torch.library.register_fake("flash_attention::paged_window_forward_fp8")
def flash_attention_paged_window_forward_fp8_fake(q, k_cache, v_cache, block_table, cache_seqlens, window_left,
                                                  k_descale=None, v_descale=None, softmax_scale=None, causal=False):
    return torch.empty_like(q)


# Attention sinks on the paged decode (include/fa_gfx950_sink.h fa_fwd_gfx950_paged_sink / _sink_fp8): ops of their
# own beside the paged ops, whose schemas stay as they are. A sink is one learned logit per q-head (flash-attn's
# ``s_aux``, vLLM's ``sinks``, the gpt-oss models') that joins the softmax denominator and contributes no value:
#   out = (v_descale) sum_n exp(s_n - mu) v_n / (sum_n exp(s_n - mu) + exp(sinks[h] - mu)),  mu = max(max_n s_n, sinks[h])
# with s_n the scaled, masked scores; ``sinks`` is in final-logit units (no softmax_scale, no k_descale).
def _check_sink_shape(q, k_cache, return_lse=False):
    """The wrapper errors of every call with sinks: the sink kernels serve decode shapes and return no LSE."""
    if return_lse:
        raise NotImplementedError("sinks with return_lse=True: no kernel writes the LSE of a sinked row")
    g, sq = q.size(1) // k_cache.size(1), q.size(2)
    if g * sq > _PAGED_DECODE_MAX_ROWS:
        raise NotImplementedError(f"sinks are served for decode shapes only (Hq / Hkv * Sq <= "
                                  f"{_PAGED_DECODE_MAX_ROWS}, got {g * sq}): the uniform prefill kernels and the "
                                  "copying path have no sinks; a longer chunk goes through "
                                  "flash_attn_paged_varlen_func(..., sinks=) with a uniform cu_seqlens_q")
    if q.size(3) % 8 != 0:
        raise NotImplementedError(f"the calls with sinks need a head dim that is a multiple of 8 (got {q.size(3)})")


def _sinks_arg(sinks, q):
    """``sinks`` as the ops take it: fp32 [Hq] on q's device (fp16 / bf16 converted once)."""
    if not isinstance(sinks, torch.Tensor) or sinks.dim() != 1 or sinks.size(0) != q.size(1):
        got = tuple(sinks.shape) if isinstance(sinks, torch.Tensor) else type(sinks).__name__
        raise ValueError(f"sinks must be a tensor [Hq] = [{q.size(1)}] (got {got})")
    if sinks.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"sinks must be fp32, fp16 or bf16 (got {sinks.dtype})")
    if sinks.device != q.device:
        raise ValueError(f"sinks must be on {q.device} (got {sinks.device})")
    return sinks.float()


def _paged_sink_cuda(q, k_cache, v_cache, block_table, cache_seqlens, sinks, window_left, k_descale, v_descale,
                     softmax_scale, causal, fp8):
    _require_ext()
    _check_sink_shape(q, k_cache)  # (no quiet other path: the library would refuse these shapes as well)
    qc = q if q.stride(-1) == 1 else q.contiguous()
    window_left = min(int(window_left), _MAX_WINDOW)
    if fp8:
        return flash_attention_cuda.flash_attention_paged_sink_fp8_fwd(
            qc, k_cache, v_cache, block_table, cache_seqlens, sinks, window_left, k_descale, v_descale, softmax_scale,
            causal)
    return flash_attention_cuda.flash_attention_paged_sink_fwd(qc, k_cache, v_cache, block_table, cache_seqlens, sinks,
                                                               window_left, softmax_scale, causal)


@torch.library.custom_op("flash_attention::paged_forward_sink", mutates_args=())
def flash_attention_paged_forward_sink(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                       block_table: torch.Tensor, cache_seqlens: torch.Tensor, sinks: torch.Tensor,
                                       window_left: int = -1, softmax_scale: float = None,
                                       causal: bool = False) -> torch.Tensor:
    # paged_forward / paged_window_forward (window_left < 0: no window) with one extra softmax column per q-head of
    # logit sinks[h] (fp32 [Hq]) and value 0. Non-GPU default: _paged_reference with that column.
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    return _paged_reference(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal,
                            min(int(window_left), _MAX_WINDOW), sinks)


@torch.library.register_kernel("flash_attention::paged_forward_sink", "cuda")
def flash_attention_paged_forward_sink_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                            block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                            sinks: torch.Tensor, window_left: int = -1, softmax_scale: float = None,
                                            causal: bool = False) -> torch.Tensor:
    return _paged_sink_cuda(q, k_cache, v_cache, block_table, cache_seqlens, sinks, window_left, None, None,
                            softmax_scale, causal, False)


@torch.library.register_fake("flash_attention::paged_forward_sink")
def flash_attention_paged_forward_sink_fake(q, k_cache, v_cache, block_table, cache_seqlens, sinks, window_left=-1,
                                            softmax_scale=None, causal=False):
    return torch.empty_like(q)


@torch.library.custom_op("flash_attention::paged_forward_sink_fp8", mutates_args=())
def flash_attention_paged_forward_sink_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                           block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                           sinks: torch.Tensor, window_left: int = -1,
                                           k_descale: Optional[torch.Tensor] = None,
                                           v_descale: Optional[torch.Tensor] = None, softmax_scale: float = None,
                                           causal: bool = False) -> torch.Tensor:
    # paged_forward_fp8 / paged_window_forward_fp8 with the sink column; the sink is not multiplied by k_descale
    return _paged_fp8_reference(q, k_cache, v_cache, block_table, cache_seqlens, k_descale, v_descale, softmax_scale,
                                causal, min(int(window_left), _MAX_WINDOW), sinks)


@torch.library.register_kernel("flash_attention::paged_forward_sink_fp8", "cuda")
def flash_attention_paged_forward_sink_fp8_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                                block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                                sinks: torch.Tensor, window_left: int = -1,
                                                k_descale: Optional[torch.Tensor] = None,
                                                v_descale: Optional[torch.Tensor] = None,
                                                softmax_scale: float = None, causal: bool = False) -> torch.Tensor:
    return _paged_sink_cuda(q, k_cache, v_cache, block_table, cache_seqlens, sinks, window_left, k_descale, v_descale,
                            softmax_scale, causal, True)


@torch.library.register_fake("flash_attention::paged_forward_sink_fp8")
def flash_attention_paged_forward_sink_fp8_fake(q, k_cache, v_cache, block_table, cache_seqlens, sinks,
                                                window_left=-1, k_descale=None, v_descale=None, softmax_scale=None,
                                                causal=False):
    return torch.empty_like(q)


def _paged_sink(q, k_cache, v_cache, block_table, cache_seqlens, sinks, window_left, softmax_scale, causal, k_descale,
                v_descale, return_lse=False):
    """The call of every wrapper with ``sinks``: its errors, then the sink op of the cache's format."""
    sinks = _sinks_arg(sinks, q)
    _check_sink_shape(q, k_cache, return_lse)
    if _is_fp8_cache(k_cache, v_cache, k_descale, v_descale):
        b, hkv = q.size(0), k_cache.size(1)
        kd = _descale_arg(k_descale, "k_descale", b, hkv, q.device)
        vd = _descale_arg(v_descale, "v_descale", b, hkv, q.device)
        return torch.ops.flash_attention.paged_forward_sink_fp8(q, k_cache, v_cache, block_table, cache_seqlens, sinks,
                                                                window_left, kd, vd, softmax_scale, causal)
    return torch.ops.flash_attention.paged_forward_sink(q, k_cache, v_cache, block_table, cache_seqlens, sinks,
                                                        window_left, softmax_scale, causal)


def _io_dtype(k, q):
    """The 16-bit dtype of an fp8 append's inputs (q_rot's dtype; fp16 when there is neither k nor q)."""
    return k.dtype if k is not None else q.dtype if q is not None else torch.float16


@torch.library.custom_op("flash_attention::kvcache_append_fp8", mutates_args=("k_cache", "v_cache"))
def flash_attention_kvcache_append_fp8(k_cache: torch.Tensor, v_cache: torch.Tensor, k: Optional[torch.Tensor],
                                       v: Optional[torch.Tensor], cache_seqlens: torch.Tensor,
                                       block_table: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None,
                                       rotary_cos: Optional[torch.Tensor] = None,
                                       rotary_sin: Optional[torch.Tensor] = None,
                                       k_descale: Optional[torch.Tensor] = None,
                                       v_descale: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    # Non-GPU default: kvcache_append's default on 16-bit scratch caches (placement, drop rules, rotation
    # and rounding to the input dtype are its own), then the rows it wrote are quantized into the fp8 caches.
    # A second run with each sequence's number as the "key" tells which sequence wrote which row.
    dt = _io_dtype(k, q)
    k16 = torch.zeros(k_cache.shape, dtype=dt, device=k_cache.device)
    v16 = torch.zeros(v_cache.shape, dtype=dt, device=v_cache.device)
    new_seqlens, q_rot = flash_attention_kvcache_append(k16, v16, k, v, cache_seqlens, block_table, q, rotary_cos,
                                                        rotary_sin)
    if k is not None and k.size(2) > 0:
        b, hkv = k.size(0), k.size(1)
        mark = torch.zeros(*k_cache.shape[:3], 1, dtype=torch.float32, device=k_cache.device)
        ids = torch.arange(1, b + 1, dtype=torch.float32, device=k.device)[:, None, None, None].expand(
            b, hkv, k.size(2), 1)
        flash_attention_kvcache_append(mark, torch.zeros_like(mark), ids, ids, cache_seqlens, block_table)
        owner = mark[..., 0].to(torch.int64) - 1  # [pages, Hkv, rows]: the sequence that wrote the row, or -1
        written = owner >= 0
        head = torch.arange(hkv, device=k_cache.device)[None, :, None].expand_as(owner)
        for cache, x16, ds in ((k_cache, k16, k_descale), (v_cache, v16, v_descale)):
            d = _descale_or_ones(ds, b, hkv, k_cache.device)[owner.clamp(min=0), head]  # [pages, Hkv, rows]
            # (through byte views: index_put_ is not implemented for float8 tensors)
            cache.view(torch.uint8)[written] = quantize_e4m3(x16[written], d[written][:, None]).view(torch.uint8)
    return new_seqlens, q_rot


@torch.library.register_kernel("flash_attention::kvcache_append_fp8", "cuda")
def flash_attention_kvcache_append_fp8_cuda(k_cache: torch.Tensor, v_cache: torch.Tensor, k: Optional[torch.Tensor],
                                            v: Optional[torch.Tensor], cache_seqlens: torch.Tensor,
                                            block_table: Optional[torch.Tensor] = None,
                                            q: Optional[torch.Tensor] = None,
                                            rotary_cos: Optional[torch.Tensor] = None,
                                            rotary_sin: Optional[torch.Tensor] = None,
                                            k_descale: Optional[torch.Tensor] = None,
                                            v_descale: Optional[torch.Tensor] = None
                                            ) -> tuple[torch.Tensor, torch.Tensor]:
    _require_ext()
    # as kvcache_append: inputs may be copied, the caches never (the binding rejects a cache whose last
    # dimension is not contiguous, the library one that is not 16-byte aligned)
    k, v, q = (t.contiguous() if t is not None and t.stride(3) != 1 else t for t in (k, v, q))
    if rotary_cos is not None:
        dt = _io_dtype(k, q)
        rotary_cos, rotary_sin = rotary_cos.to(dt), rotary_sin.to(dt)
    new_seqlens, q_rot = flash_attention_cuda.flash_attention_kvcache_append_fp8(
        k_cache, v_cache, k, v, cache_seqlens, block_table, q, rotary_cos, rotary_sin, k_descale, v_descale)
    return new_seqlens, q_rot


@torch.library.register_fake("flash_attention::kvcache_append_fp8")
def flash_attention_kvcache_append_fp8_fake(k_cache, v_cache, k, v, cache_seqlens, block_table=None, q=None,
                                            rotary_cos=None, rotary_sin=None, k_descale=None, v_descale=None):
    q_rot = (torch.empty(0, dtype=_io_dtype(k, q), device=k_cache.device) if q is None
             else torch.empty(q.shape, dtype=q.dtype, device=q.device))
    return torch.empty_like(cache_seqlens, memory_format=torch.contiguous_format), q_rot


# ---------------------------------------------------------------------------------------------
# LSE output, state merge and shared-prefix decode on the paged cache (include/fa_gfx950_lse.h); no
# reference counterpart. The LSE is flash-attn's ``softmax_lse`` (natural log), the merge vLLM's
# ``merge_attn_states`` / flashinfer's ``merge_state``: attention results over DISJOINT key sets combine
# exactly, which is what shared-prefix (cascade) decode and sequence-sharded decode are built from.
# ---------------------------------------------------------------------------------------------
_SHARED_PREFIX_GROUP_ROWS = 32  # (q-head, sequence) rows of one prefix-phase group: g * c (one 32-row block)


def _paged_lse_reference(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset, k_descale, v_descale,
                         softmax_scale, causal):
    """The non-GPU default of the LSE ops, a float restatement: (o, lse) with the kernel's semantics (lengths
    ``clamp(cache_seqlens[b] + seqlen_offset)`` or ``clamp(seqlen_offset)``, bottom-right causal per sequence, GQA,
    rows without a visible key o = 0 and lse = -inf; FP8: k_descale in the scale, v_descale on o)."""
    b_, hq, sq, d = q.shape
    num_pages, hkv, page_size, _ = k_cache.shape
    g = hq // hkv
    cap = block_table.size(1) * page_size
    scale = d ** -0.5 if softmax_scale is None else softmax_scale
    lens = cache_seqlens.tolist() if cache_seqlens is not None else [0] * b_
    out = torch.zeros(q.shape, dtype=torch.float32, device=q.device)
    lse = torch.full((b_, hq, sq), float("-inf"), dtype=torch.float32, device=q.device)
    for b, n in enumerate(lens):
        n = min(max(n + seqlen_offset, 0), cap)
        if n == 0:
            continue
        ids = block_table[b, :(n + page_size - 1) // page_size].clamp(0, num_pages - 1).to(torch.int64)
        kb = k_cache.index_select(0, ids).float().transpose(0, 1).flatten(1, 2)[:, :n].repeat_interleave(g, dim=0)
        vb = v_cache.index_select(0, ids).float().transpose(0, 1).flatten(1, 2)[:, :n].repeat_interleave(g, dim=0)
        s = torch.matmul(q[b].float(), kb.transpose(1, 2)) * scale  # [Hq, Sq, n]
        if k_descale is not None:
            s = s * k_descale[b].float().repeat_interleave(g)[:, None, None]
        if causal:
            s = s.masked_fill(~_bottom_right_causal(sq, n, q.device)[None], float("-inf"))
        l = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - l.masked_fill(l == float("-inf"), 0)[..., None])
        o = torch.matmul(p, vb)
        if v_descale is not None:
            o = o * v_descale[b].float().repeat_interleave(g)[:, None, None]
        out[b], lse[b] = o, l
    return out.to(q.dtype), lse


def _paged_lse_cuda(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset, k_descale, v_descale,
                    softmax_scale, causal, out=None, lse=None):
    _require_ext()
    if block_table.stride(1) != 1 and block_table.size(1) > 1:  # (rows are read in place: a row is contiguous)
        block_table = block_table.contiguous()
    return flash_attention_cuda.flash_attention_paged_lse_fwd(
        q if q.stride(-1) == 1 else q.contiguous(), k_cache, v_cache, block_table, cache_seqlens, int(seqlen_offset),
        k_descale, v_descale, softmax_scale, causal, out, lse)


@torch.library.custom_op("flash_attention::paged_forward_lse", mutates_args=())
def flash_attention_paged_forward_lse(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                      block_table: torch.Tensor, cache_seqlens: Optional[torch.Tensor],
                                      seqlen_offset: int = 0, softmax_scale: float = None,
                                      causal: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    # paged_forward that also returns lse fp32 [B, Hq, Sq] (natural log; -inf for rows without a visible key);
    # sequence b has clamp(cache_seqlens[b] + seqlen_offset) keys, clamp(seqlen_offset) without cache_seqlens.
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    return _paged_lse_reference(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset, None, None,
                                softmax_scale, causal)


@torch.library.register_kernel("flash_attention::paged_forward_lse", "cuda")
def flash_attention_paged_forward_lse_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                           block_table: torch.Tensor, cache_seqlens: Optional[torch.Tensor],
                                           seqlen_offset: int = 0, softmax_scale: float = None,
                                           causal: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    o, lse = _paged_lse_cuda(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset, None, None,
                             softmax_scale, causal)
    return o, lse


@torch.library.register_fake("flash_attention::paged_forward_lse")
def flash_attention_paged_forward_lse_fake(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset=0,
                                           softmax_scale=None, causal=False):
    return torch.empty_like(q), q.new_empty(q.shape[:3], dtype=torch.float32)


@torch.library.custom_op("flash_attention::paged_forward_lse_fp8", mutates_args=())
def flash_attention_paged_forward_lse_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                          block_table: torch.Tensor, cache_seqlens: Optional[torch.Tensor],
                                          k_descale: Optional[torch.Tensor] = None,
                                          v_descale: Optional[torch.Tensor] = None, seqlen_offset: int = 0,
                                          softmax_scale: float = None,
                                          causal: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    return _paged_lse_reference(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset, k_descale, v_descale,
                                softmax_scale, causal)


@torch.library.register_kernel("flash_attention::paged_forward_lse_fp8", "cuda")
def flash_attention_paged_forward_lse_fp8_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                               block_table: torch.Tensor, cache_seqlens: Optional[torch.Tensor],
                                               k_descale: Optional[torch.Tensor] = None,
                                               v_descale: Optional[torch.Tensor] = None, seqlen_offset: int = 0,
                                               softmax_scale: float = None,
                                               causal: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    o, lse = _paged_lse_cuda(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset, k_descale, v_descale,
                             softmax_scale, causal)
    return o, lse


@torch.library.register_fake("flash_attention::paged_forward_lse_fp8")
def flash_attention_paged_forward_lse_fp8_fake(q, k_cache, v_cache, block_table, cache_seqlens, k_descale=None,
                                               v_descale=None, seqlen_offset=0, softmax_scale=None, causal=False):
    return torch.empty_like(q), q.new_empty(q.shape[:3], dtype=torch.float32)


def _check_lse_shape(q, k_cache, window_left):
    """The wrapper errors of every LSE call: the LSE kernels serve decode shapes without a window."""
    if window_left >= 0:
        raise NotImplementedError("the sliding-window decode kernels have no LSE variant (window_left >= 0)")
    g, sq = q.size(1) // k_cache.size(1), q.size(2)
    if g * sq > _PAGED_DECODE_MAX_ROWS:
        raise NotImplementedError(f"the LSE is returned for decode shapes only (Hq / Hkv * Sq <= "
                                  f"{_PAGED_DECODE_MAX_ROWS}, got {g * sq}): the prefill kernels have no LSE variant")
    if q.size(3) % 8 != 0:
        raise NotImplementedError(f"the LSE calls need a head dim that is a multiple of 8 (got {q.size(3)})")


def _paged_lse(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset, softmax_scale, causal, k_descale,
               v_descale, window_left):
    _check_lse_shape(q, k_cache, window_left)
    if _is_fp8_cache(k_cache, v_cache, k_descale, v_descale):
        b, hkv = q.size(0), k_cache.size(1)
        kd = _descale_arg(k_descale, "k_descale", b, hkv, q.device)
        vd = _descale_arg(v_descale, "v_descale", b, hkv, q.device)
        return torch.ops.flash_attention.paged_forward_lse_fp8(q, k_cache, v_cache, block_table, cache_seqlens, kd, vd,
                                                               seqlen_offset, softmax_scale, causal)
    return torch.ops.flash_attention.paged_forward_lse(q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset,
                                                       softmax_scale, causal)


def _merge_reference(outs, lses, return_lse):
    """The non-GPU default of merge_states, a float restatement of the kernel's rule."""
    mx = lses.max(dim=0).values
    w = torch.exp(lses - mx.masked_fill(mx == float("-inf"), 0))  # (a -inf part weighs 0)
    sw = w.sum(dim=0)
    o = (w[..., None] * outs.float()).sum(dim=0) / sw.masked_fill(sw == 0, 1)[..., None]
    o = o.masked_fill((sw == 0)[..., None], 0).to(outs.dtype)
    lse = mx + torch.log(sw)  # (all -inf: -inf + log 0 = -inf)
    return o, (lse.masked_fill(sw == 0, float("-inf")) if return_lse else lses.new_empty(0))


@torch.library.custom_op("flash_attention::merge_states", mutates_args=())
def flash_attention_merge_states(outs: torch.Tensor, lses: torch.Tensor,
                                 return_lse: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    # outs [N, B, H, S, D] fp16 / bf16, lses [N, B, H, S] fp32 -> (out [B, H, S, D], lse [B, H, S] or empty)
    return _merge_reference(outs, lses, return_lse)


@torch.library.register_kernel("flash_attention::merge_states", "cuda")
def flash_attention_merge_states_cuda(outs: torch.Tensor, lses: torch.Tensor,
                                      return_lse: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    _require_ext()
    o, lse = flash_attention_cuda.flash_attention_merge_states(outs, lses, return_lse)
    return o, lse


@torch.library.register_fake("flash_attention::merge_states")
def flash_attention_merge_states_fake(outs, lses, return_lse=False):
    return (outs.new_empty(outs.shape[1:]),
            lses.new_empty(lses.shape[1:]) if return_lse else lses.new_empty(0))


# The merge of PACKED states (outs [N, total_q, H, D], lses [N, H, total_q] -> out [total_q, H, D], lse [H, total_q]):
# an op beside merge_states, which allocates [B, H, S, D] and keeps its schema; the same kernel and C entry.
@torch.library.custom_op("flash_attention::merge_states_packed", mutates_args=())
def flash_attention_merge_states_packed(outs: torch.Tensor, lses: torch.Tensor,
                                        return_lse: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    o, lse = _merge_reference(outs.transpose(1, 2), lses, return_lse)  # ([N, H, T, D] against [N, H, T])
    return o.transpose(0, 1).contiguous(), lse


@torch.library.register_kernel("flash_attention::merge_states_packed", "cuda")
def flash_attention_merge_states_packed_cuda(outs: torch.Tensor, lses: torch.Tensor,
                                             return_lse: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    _require_ext()
    o, lse = flash_attention_cuda.flash_attention_merge_states_packed(outs, lses, return_lse)
    return o, lse


@torch.library.register_fake("flash_attention::merge_states_packed")
def flash_attention_merge_states_packed_fake(outs, lses, return_lse=False):
    return (outs.new_empty(outs.shape[1:]),
            lses.new_empty(lses.shape[1:]) if return_lse else lses.new_empty(0))


def flash_attn_merge_states(outs, lses, return_lse=False):
    """Merge N partial attention states over DISJOINT key sets: ``outs`` [N, B, Hq, Sq, D] (fp16 / bf16, D a
    multiple of 8) and ``lses`` [N, B, Hq, Sq] (fp32, natural log, as ``flash_attn_paged_func(return_lse=True)``
    returns them), as tensors of any strides or as sequences of N tensors (stacked: a copy). Per row,
    ``w_i = exp(lse_i - max_i lse_i)``, ``out = sum_i w_i o_i / sum_i w_i`` in fp32 rounded once, ``lse = max_i lse_i
    + ln sum_i w_i``; a part with ``lse = -inf`` weighs 0 and a row whose parts all are gives 0 and ``-inf``.
    1 <= N <= 16. One memory-bound HIP pass, no host synchronisation (graph-capturable). Returns ``out`` or
    ``(out, lse)``.

    PACKED states, the layout of the ragged step (``flash_attn_paged_varlen_func(return_lse=True)``): ``outs``
    [N, total_q, Hq, D] with ``lses`` [N, Hq, total_q], or sequences of N such tensors; returns ``out``
    [total_q, Hq, D] contiguous and ``lse`` [Hq, total_q]. The same kernel and rule (one batch row of ``total_q``
    positions, read through the packed strides)."""
    if not isinstance(outs, torch.Tensor):
        outs = torch.stack(list(outs))
    if not isinstance(lses, torch.Tensor):
        lses = torch.stack(list(lses))
    packed = outs.dim() == 4 and lses.dim() == 3
    if packed:
        if outs.size(0) != lses.size(0) or outs.size(1) != lses.size(2) or outs.size(2) != lses.size(1):
            raise ValueError(f"packed outs must be [N, total_q, Hq, D] and lses [N, Hq, total_q] (got "
                             f"{tuple(outs.shape)} and {tuple(lses.shape)})")
    elif outs.dim() != 5 or lses.dim() != 4 or outs.shape[:4] != lses.shape:
        raise ValueError(f"outs must be [N, B, Hq, Sq, D] and lses [N, B, Hq, Sq] (got {tuple(outs.shape)} and "
                         f"{tuple(lses.shape)})")
    if not 1 <= outs.size(0) <= 16:
        raise ValueError(f"1 to 16 partial states can be merged (got {outs.size(0)})")
    if outs.size(-1) % 8 != 0:
        raise ValueError(f"the head dim must be a multiple of 8 (got {outs.size(-1)})")
    if lses.dtype != torch.float32:
        raise ValueError(f"lses must be fp32 (got {lses.dtype})")
    if packed:
        o, lse = torch.ops.flash_attention.merge_states_packed(outs, lses, return_lse)
        return (o, lse) if return_lse else o
    o, lse = torch.ops.flash_attention.merge_states(outs, lses, return_lse)
    return (o, lse) if return_lse else o


def _check_shared_prefix_enabled() -> bool:
    """FA_CHECK_SHARED_PREFIX, read at every call (as FA_CHECK_VARLEN is)."""
    return os.environ.get("FA_CHECK_SHARED_PREFIX", "0") not in ("", "0")


def _check_shared_prefix_table(block_table, n_pre, groups):
    """Raise if the rows of a group differ in their prefix entries (FA_CHECK_SHARED_PREFIX=1; one host read)."""
    bad = []
    for lo, hi in groups:
        rows = block_table[lo:hi, :n_pre]
        bad.append((rows != rows[:1]).any())
    if bool(torch.stack(bad).any()):
        raise ValueError("flash_attn_paged_shared_prefix_func: the sequences of a group must carry the same page ids "
                         "in their first prefix_len / page_size block-table entries")


def _lse_into(q, k_cache, v_cache, table, seqlens, offset, kd, vd, scale, causal, out, lse):
    """One LSE decode launch that writes o / lse through the given (strided) views."""
    if q.is_cuda:
        _paged_lse_cuda(q, k_cache, v_cache, table, seqlens, offset, kd, vd, scale, causal, out, lse)
    else:
        o, l = _paged_lse_reference(q, k_cache, v_cache, table, seqlens, offset, kd, vd, scale, causal)
        out.copy_(o)
        lse.copy_(l)


def flash_attn_paged_shared_prefix_func(q, k_cache, v_cache, block_table, cache_seqlens, prefix_len,
                                        softmax_scale=None, causal=False, k_descale=None, v_descale=None,
                                        return_lse=False, _group_rows=None):
    """A decode step (q [B, Hq, 1, D]) of ``flash_attn_paged_func`` for a batch whose sequences SHARE their first
    ``prefix_len`` keys (a system prompt, few-shot examples, a prefix-cache hit, beam or parallel sampling): the
    shared pages are streamed once per GROUP of sequences instead of once per sequence. 16-bit and FP8 pools.

    The caller's contract:

    * ``prefix_len`` is a Python int and a multiple of ``page_size`` (``ValueError`` otherwise), at most the
      table's capacity;
    * every sequence holds at least ``prefix_len`` keys; a shorter ``cache_seqlens[b]`` is treated as exactly
      ``prefix_len`` (its suffix clamps to 0 keys);
    * sequences are grouped ``c = max(1, 32 // (Hq / Hkv))`` at a time in batch order (rows ``[i c, (i + 1) c)``,
      the last group may be shorter); the rows of one group carry the same page ids in their first
      ``prefix_len / page_size`` table entries and, with an FP8 cache, the same descales. So a batch in which
      EVERY sequence shares the prefix qualifies, as does one sorted so that each group does;
    * ``FA_CHECK_SHARED_PREFIX=1`` (read per call, eager only, off by default) verifies the table condition
      with one host read and raises ``ValueError``.

    Three launches, four when ``B % c != 0``; no copies, no helper kernels, no host synchronisation
    (graph-capturable). Prefix phase: each group is ONE batch row of the LSE decode kernel -- q viewed in place
    as [B / c, Hq, c, D], the table ``block_table[::c, :prefix_len / page_size]``, every row ``prefix_len`` keys,
    non-causal. Suffix phase: the LSE decode kernel over ``block_table[:, prefix_len / page_size:]`` with
    ``cache_seqlens - prefix_len`` keys (the offset is applied in the kernel). Then ``flash_attn_merge_states``.

    What is never read: the prefix table entries of every row but a group's first; in the prefix phase, entries
    at or past ``prefix_len / page_size``.

    The result differs from ``flash_attn_paged_func`` on the same table by rounding only (the two partial
    outputs are rounded to q's dtype before the merge). ``prefix_len == 0`` IS ``flash_attn_paged_func``, bit for
    bit. ``return_lse=True`` also returns the merged lse. It is an explicit call: nothing dispatches to it; it
    pays off for long prefixes and many sequences (DESIGN.md section 5 has the measured crossover).
    ``Sq > 1`` raises ``ValueError`` (the (sequence, position) rows of a group are not one strided view)."""
    prefix_len = int(prefix_len)
    page_size = k_cache.size(2)
    if prefix_len < 0 or prefix_len % page_size != 0:
        raise ValueError(f"prefix_len ({prefix_len}) must be a non-negative multiple of page_size ({page_size})")
    if q.dim() != 4 or q.size(2) != 1:
        raise ValueError(f"shared-prefix decode serves decode steps (q [B, Hq, 1, D]) only (got {tuple(q.shape)})")
    if prefix_len == 0:
        return flash_attn_paged_func(q, k_cache, v_cache, block_table, cache_seqlens, softmax_scale, causal,
                                     k_descale, v_descale, return_lse=return_lse)
    n_pre = prefix_len // page_size
    if n_pre > block_table.size(1):
        raise ValueError(f"prefix_len ({prefix_len}) exceeds the block table's capacity "
                         f"({block_table.size(1) * page_size})")
    softmax_scale = _default_scale(q, softmax_scale)
    _check_lse_shape(q, k_cache, -1)
    b, hq, _, d = q.shape
    hkv = k_cache.size(1)
    g = hq // hkv
    kd = vd = None
    if _is_fp8_cache(k_cache, v_cache, k_descale, v_descale):
        kd = _descale_arg(k_descale, "k_descale", b, hkv, q.device)
        vd = _descale_arg(v_descale, "v_descale", b, hkv, q.device)
    rows = _SHARED_PREFIX_GROUP_ROWS if _group_rows is None else int(_group_rows)
    c = max(1, min(rows, _PAGED_DECODE_MAX_ROWS) // g)
    n_full = b // c
    groups = [(i * c, (i + 1) * c) for i in range(n_full)] + ([(n_full * c, b)] if b % c else [])
    if _check_shared_prefix_enabled() and not torch.compiler.is_compiling() and not (
            q.is_cuda and torch.cuda.is_current_stream_capturing()):
        _check_shared_prefix_table(block_table, n_pre, groups)
    if q.stride(-1) != 1:
        q = q.contiguous()
    if block_table.stride(1) != 1:
        block_table = block_table.contiguous()

    # the two states: [0] the prefix phase, [1] the suffix phase
    outs = torch.empty((2, b, hq, 1, d), dtype=q.dtype, device=q.device)
    lses = torch.empty((2, b, hq, 1), dtype=torch.float32, device=q.device)
    # prefix phase: rows [lo, lo + n * cc) as n batch rows of cc positions, each group's first table row
    for lo, n, cc in ((0, n_full, c), (n_full * c, 1, b % c)):
        if n == 0 or cc == 0:
            continue
        qv = q.as_strided((n, hq, cc, d), (cc * q.stride(0), q.stride(1), q.stride(0), 1),
                          q.storage_offset() + lo * q.stride(0))
        ov = outs.as_strided((n, hq, cc, d), (cc * hq * d, d, hq * d, 1), lo * hq * d)
        lv = lses.as_strided((n, hq, cc), (cc * hq, 1, hq), lo * hq)
        hi = lo + n * cc
        _lse_into(qv, k_cache, v_cache, block_table[lo:hi:cc, :n_pre], None, prefix_len,
                  None if kd is None else kd[lo:hi:cc], None if vd is None else vd[lo:hi:cc], softmax_scale, False,
                  ov, lv)
    # suffix phase: every sequence's own keys (a table without suffix columns: 0 keys, no entry is read)
    if n_pre < block_table.size(1):
        table, lens, off = block_table[:, n_pre:], cache_seqlens, -prefix_len
    else:
        table, lens, off = block_table[:, :1], None, 0
    _lse_into(q, k_cache, v_cache, table, lens, off, kd, vd, softmax_scale, causal, outs[1], lses[1])
    return flash_attn_merge_states(outs, lses, return_lse)


# ---------------------------------------------------------------------------------------------
# Ragged queries and a ragged append on the paged cache -- one step of a continuous batch
# (include/fa_gfx950_paged_varlen.h fa_fwd_gfx950_paged_varlen, include/fa_gfx950_kvcache_varlen.h
# fa_kvcache_append_varlen_gfx950); no reference counterpart. flash-attn's packed layout: q [total_q, Hq, D]
# with cu_seqlens_q, sequence b's rows its LAST Sq_b positions over cache_seqlens[b] keys of the page pool
# -- what flash_attn_varlen_func(..., block_table=...) gives an engine. New ops beside the uniform ones,
# whose schemas stay as they are.
# ---------------------------------------------------------------------------------------------
def _clamped_ranges(cu: torch.Tensor, total: int):
    """[(r0, r1)] per sequence, clamped as the kernels clamp a cumulative array: r0 into [0, total], r1 into
    [r0, total]."""
    c = cu.tolist()
    out = []
    for b in range(len(c) - 1):
        r0 = min(max(c[b], 0), total)
        out.append((r0, min(max(c[b + 1], r0), total)))
    return out


def _paged_varlen_unsupported(q, k_cache, v_cache):
    """The layouts the ragged paged kernel does not read, with the alternative to use instead."""
    alt = ("call flash_attn_paged_func once per chunk length, or gather the pages into packed keys for "
           "flash_attn_varlen_func")
    if k_cache.dtype == FP8_DTYPE or v_cache.dtype == FP8_DTYPE:
        raise NotImplementedError(f"flash_attn_paged_varlen_func does not read FP8 pools: {alt}")
    if k_cache.size(2) % _PAGED_PREFILL_TILE != 0:
        raise NotImplementedError(f"flash_attn_paged_varlen_func needs page_size ({k_cache.size(2)}) to be a multiple "
                                  f"of {_PAGED_PREFILL_TILE}: {alt}")
    if q.size(-1) % 8 != 0:
        raise NotImplementedError(f"flash_attn_paged_varlen_func needs a head dim ({q.size(-1)}) that is a multiple "
                                  f"of 8: {alt}")


def _paged_varlen_reference(q, k_cache, v_cache, cu_seqlens_q, block_table, cache_seqlens, softmax_scale, causal,
                            window_left, sinks=None, return_lse=False):
    """The non-GPU default of the ragged paged ops: a per-sequence loop in the style of ``_paged_reference`` (the
    sequence's pages gathered, torch SDPA under the kernel's masks, rows with no visible key 0, both arrays clamped
    as the kernel clamps them). ``sinks`` (the sink op): one extra softmax column per q-head. ``return_lse`` (the
    LSE op): also the float LSE [Hq, total_q], ``ln(sum_n exp(s_n) + exp(sinks[h]))`` over the row's visible keys --
    a sink at or below -1e30 adds nothing, an owned row with no visible key has its sink (``-inf`` without one), a
    row that no sequence owns ``-inf``."""
    window_left = min(int(window_left), _MAX_WINDOW)
    out = torch.zeros_like(q)
    if return_lse:
        lse = torch.full((q.size(1), q.size(0)), float("-inf"), dtype=torch.float32, device=q.device)
        sink_col = None
        if sinks is not None:
            sink_col = sinks.float().masked_fill(sinks.float() <= -1e30, float("-inf")).clamp(max=1e30)[:, None]
        scale = q.size(-1) ** -0.5 if softmax_scale is None else softmax_scale
        g = q.size(1) // k_cache.size(1)
    num_pages, _, page_size, _ = k_cache.shape
    cap = block_table.size(1) * page_size
    lens = cache_seqlens.tolist()
    for b, (q0, q1) in enumerate(_clamped_ranges(cu_seqlens_q, q.size(0))):
        n, sq = min(max(lens[b], 0), cap), q1 - q0
        if return_lse and sink_col is not None:
            lse[:, q0:q1] = sink_col
        if n == 0 or sq == 0:
            continue
        first = max(0, n - sq - window_left) // page_size if window_left >= 0 else 0  # the first page read
        k0 = first * page_size
        ids = block_table[b, first:(n + page_size - 1) // page_size].clamp(0, num_pages - 1).to(torch.int64)
        kb = k_cache.index_select(0, ids).transpose(0, 1).flatten(1, 2)[None, :, :n - k0]
        vb = v_cache.index_select(0, ids).transpose(0, 1).flatten(1, 2)[None, :, :n - k0]
        if window_left >= 0:
            mask = _window_mask(sq, n, window_left, causal, q.device)[:, k0:]
        else:
            mask = _bottom_right_causal(sq, n, q.device) if causal else None
        qb = q[q0:q1].transpose(0, 1)[None]
        if sinks is not None:
            out[q0:q1] = _sdpa_with_sink(qb, kb, vb, mask, softmax_scale, sinks)[0].transpose(0, 1)
        else:
            out[q0:q1] = _masked_sdpa(qb, kb, vb, mask, softmax_scale)[0].transpose(0, 1)
        if return_lse:
            sc = torch.matmul(qb[0].float(), kb[0].float().repeat_interleave(g, dim=0).transpose(1, 2)) * scale
            if mask is not None:
                sc = sc.masked_fill(~mask[None], float("-inf"))
            l = torch.logsumexp(sc, dim=-1)  # [Hq, sq]
            lse[:, q0:q1] = l if sink_col is None else torch.logaddexp(l, sink_col.expand_as(l))
    return (out, lse) if return_lse else out


@torch.library.custom_op("flash_attention::paged_varlen_forward", mutates_args=())
def flash_attention_paged_varlen_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                         cu_seqlens_q: torch.Tensor, max_seqlen_q: int, block_table: torch.Tensor,
                                         cache_seqlens: torch.Tensor, softmax_scale: float = None,
                                         causal: bool = False, window_left: int = -1) -> torch.Tensor:
    # q: [total_q, Hq, D] packed; caches: [num_pages, Hkv, page_size, D]; cu_seqlens_q: int32 [B + 1];
    # block_table: int32 [B, max_pages]; cache_seqlens: int32 [B]. Non-GPU default: _paged_varlen_reference.
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    _paged_varlen_unsupported(q, k_cache, v_cache)
    return _paged_varlen_reference(q, k_cache, v_cache, cu_seqlens_q, block_table, cache_seqlens, softmax_scale,
                                   causal, window_left)


@torch.library.register_kernel("flash_attention::paged_varlen_forward", "cuda")
def flash_attention_paged_varlen_forward_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                              cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                                              block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                              softmax_scale: float = None, causal: bool = False,
                                              window_left: int = -1) -> torch.Tensor:
    _require_ext()
    _paged_varlen_unsupported(q, k_cache, v_cache)
    if q.stride(-1) != 1:
        q = q.contiguous()
    return flash_attention_cuda.flash_attention_paged_varlen_fwd(
        q, k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), block_table, cache_seqlens,
        min(int(window_left), _MAX_WINDOW), softmax_scale, causal)


@torch.library.register_fake("flash_attention::paged_varlen_forward")
def flash_attention_paged_varlen_forward_fake(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table,
                                              cache_seqlens, softmax_scale=None, causal=False, window_left=-1):
    return torch.empty_like(q)


# The same with attention sinks (include/fa_gfx950_paged_varlen_sink.h fa_fwd_gfx950_paged_varlen_sink): an op of its
# own, so that paged_varlen_forward keeps its schema. ``sinks``: fp32 [Hq] on q's device, in final-logit units.
@torch.library.custom_op("flash_attention::paged_varlen_forward_sink", mutates_args=())
def flash_attention_paged_varlen_forward_sink(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                              cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                                              block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                              sinks: torch.Tensor, softmax_scale: float = None,
                                              causal: bool = False, window_left: int = -1) -> torch.Tensor:
    # Non-GPU default: _paged_varlen_reference with one extra softmax column per q-head (_sdpa_with_sink).
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    _paged_varlen_unsupported(q, k_cache, v_cache)
    return _paged_varlen_reference(q, k_cache, v_cache, cu_seqlens_q, block_table, cache_seqlens, softmax_scale,
                                   causal, window_left, sinks)


@torch.library.register_kernel("flash_attention::paged_varlen_forward_sink", "cuda")
def flash_attention_paged_varlen_forward_sink_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                                   cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                                                   block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                                   sinks: torch.Tensor, softmax_scale: float = None,
                                                   causal: bool = False, window_left: int = -1) -> torch.Tensor:
    _require_ext()
    _paged_varlen_unsupported(q, k_cache, v_cache)
    if q.stride(-1) != 1:
        q = q.contiguous()
    return flash_attention_cuda.flash_attention_paged_varlen_sink_fwd(
        q, k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), block_table, cache_seqlens, sinks,
        min(int(window_left), _MAX_WINDOW), softmax_scale, causal)


@torch.library.register_fake("flash_attention::paged_varlen_forward_sink")
def flash_attention_paged_varlen_forward_sink_fake(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table,
                                                   cache_seqlens, sinks, softmax_scale=None, causal=False,
                                                   window_left=-1):
    return torch.empty_like(q)


# The same that also returns the softmax log-sum-exp (include/fa_gfx950_paged_varlen_lse.h
# fa_fwd_gfx950_paged_varlen_lse): an op of its own once more, so that the two above keep their schemas. ``sinks``
# is optional here (ONE kernel family: without it every head's sink is -inf); lse fp32 [Hq, total_q], natural log.
@torch.library.custom_op("flash_attention::paged_varlen_forward_lse", mutates_args=())
def flash_attention_paged_varlen_forward_lse(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                             cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                                             block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                             sinks: Optional[torch.Tensor] = None, softmax_scale: float = None,
                                             causal: bool = False,
                                             window_left: int = -1) -> tuple[torch.Tensor, torch.Tensor]:
    # Non-GPU default: _paged_varlen_reference with the float LSE.
    warnings.warn("Flash Attention only support cuda now, fallback to pytorch implementation.", stacklevel=2)
    _paged_varlen_unsupported(q, k_cache, v_cache)
    return _paged_varlen_reference(q, k_cache, v_cache, cu_seqlens_q, block_table, cache_seqlens, softmax_scale,
                                   causal, window_left, sinks, return_lse=True)


def _paged_varlen_lse_cuda(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table, cache_seqlens, sinks,
                           softmax_scale, causal, window_left, out=None, lse=None):
    _require_ext()
    _paged_varlen_unsupported(q, k_cache, v_cache)
    if q.stride(-1) != 1:
        q = q.contiguous()
    return flash_attention_cuda.flash_attention_paged_varlen_lse_fwd(
        q, k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), block_table, cache_seqlens, sinks,
        min(int(window_left), _MAX_WINDOW), softmax_scale, causal, out, lse)


@torch.library.register_kernel("flash_attention::paged_varlen_forward_lse", "cuda")
def flash_attention_paged_varlen_forward_lse_cuda(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                                                  cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                                                  block_table: torch.Tensor, cache_seqlens: torch.Tensor,
                                                  sinks: Optional[torch.Tensor] = None, softmax_scale: float = None,
                                                  causal: bool = False,
                                                  window_left: int = -1) -> tuple[torch.Tensor, torch.Tensor]:
    o, lse = _paged_varlen_lse_cuda(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table, cache_seqlens,
                                    sinks, softmax_scale, causal, window_left)
    return o, lse


@torch.library.register_fake("flash_attention::paged_varlen_forward_lse")
def flash_attention_paged_varlen_forward_lse_fake(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table,
                                                  cache_seqlens, sinks=None, softmax_scale=None, causal=False,
                                                  window_left=-1):
    return torch.empty_like(q), q.new_empty((q.shape[1], q.shape[0]), dtype=torch.float32)


def flash_attn_paged_varlen_func(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table, cache_seqlens,
                                 softmax_scale=None, causal=False, window_left=-1, sinks=None, return_lse=False):
    """Attention of RAGGED query blocks over a paged KV cache, in one launch: ``q`` [total_q, Hq, D] packed
    (flash-attn's varlen layout), sequence b owning rows ``[cu_seqlens_q[b], cu_seqlens_q[b + 1])`` (int32
    [B + 1] on q's device) -- its LAST ``Sq_b`` positions over ``L_b = clamp(cache_seqlens[b], 0, max_pages *
    page_size)`` keys of the pools ``k_cache`` / ``v_cache`` [num_pages, Hkv, page_size, D] (any strides) named by
    ``block_table`` int32 [B, max_pages], as in ``flash_attn_paged_func``. Returns ``out`` [total_q, Hq, D].

    Masks are per sequence: key n is visible to query m iff ``window_left < 0 or n >= m + L_b - Sq_b -
    window_left`` and, with ``causal``, ``n <= m + L_b - Sq_b``. Rows that see no key are 0; ``Sq_b == 0`` and
    ``L_b == 0`` are valid. Rows of ``out`` outside ``[cu_seqlens_q[0], cu_seqlens_q[B])`` are unspecified.

    ``q`` is read in place when its row and head strides are multiples of 8 and its base is 16-byte aligned (a
    slice of a fused QKV projection); other layouts are made contiguous. ``max_seqlen_q`` (a host int) sizes
    the grid and must be at least the true maximum ``Sq_b``; a larger value only launches empty q-tiles, a
    smaller one leaves rows uncomputed. ``FA_CHECK_VARLEN=1`` in the environment verifies it (one host sync).

    On the device both bounds of a sequence are clamped into ``[0, total_q]`` (the second to at least the first),
    so a bad ``cu_seqlens_q`` never reads or writes outside ``q`` / ``out``; page ids are clamped into the pool
    and lengths to the table's capacity. Per sequence, with its own ``Sq_b``: table entries at or past
    ``ceil(L_b / page_size)`` are never read, and with a window the PAGES WHOLLY BELOW ``max(0, L_b - Sq_b -
    window_left) // 64 * 64``, AND THEIR TABLE ENTRIES, ARE NEVER READ. The result is bit-identical to
    ``flash_attn_varlen_func`` on the gathered keys packed densely. No host synchronisation (graph-capturable).

    This is the paged PREFILL kernel: every sequence costs at least one 256-row block per q-head, so A
    ONE-TOKEN SEQUENCE COSTS A WHOLE 256-ROW BLOCK. An engine should send its pure decode sequences to
    ``flash_attn_paged_func`` and only the sequences with prompt chunks here. 16-bit pools with ``page_size`` a
    multiple of 64 and D a multiple of 8 only (``NotImplementedError`` otherwise: call ``flash_attn_paged_func``
    once per chunk length, or gather the pages for ``flash_attn_varlen_func``).

    ``sinks`` (fp32 [Hq] on q's device; fp16 / bf16 are converted once; ``ValueError`` otherwise): attention
    sinks, as in ``flash_attn_paged_func`` -- one learned logit per q-head, in final-logit units (not multiplied by
    ``softmax_scale``), that joins every row's softmax denominator with value 0; ``-inf`` is no sink on that head
    (the bits of the call without sinks), and a row without a visible key stays 0. Any ``Sq_b``: this is where a
    prompt chunk of a model with sinks goes -- a UNIFORM chunk too, with a uniform ``cu_seqlens_q``, since
    ``flash_attn_paged_func`` serves sinks for decode shapes only. ``None`` is the call without the argument, bit
    for bit. The same layouts only: with FP8 pools, other page sizes or head dims it is ``NotImplementedError``
    as above, and those alternatives have no sinks beyond decode shapes.

    ``return_lse=True`` returns ``(out, lse)``: ``lse`` fp32 [Hq, total_q] contiguous (flash-attn's varlen layout),
    ``ln(sum_n exp(s_n) + exp(sinks[h]))`` over the row's visible keys in natural-log units, with or without
    ``sinks`` and ``window_left`` -- the partial state ``flash_attn_merge_states`` combines with the states of other
    key sets (keys sharded over devices or pools, a shared prefix:
    ``flash_attn_paged_varlen_shared_prefix_func``). A row without a visible key has ``lse = sinks[h]`` (the sink's
    weight over its zero value), or ``-inf`` without a sink; pass ``sinks`` to exactly ONE of the states that are
    merged. ``out`` has the bits of the call without ``return_lse``; rows that no sequence owns are unspecified in
    both. ``False`` is the call without the argument, bit for bit, through the ops without the LSE."""
    softmax_scale = _default_scale(q, softmax_scale)
    if sinks is not None:
        sinks = _sinks_arg(sinks, q)
    if _check_varlen_enabled():
        longest = int((cu_seqlens_q[1:] - cu_seqlens_q[:-1]).max()) if cu_seqlens_q.numel() > 1 else 0
        if longest > int(max_seqlen_q):
            raise ValueError(f"max_seqlen_q={int(max_seqlen_q)} is smaller than the longest sequence ({longest}) "
                             "in cu_seqlens_q")
    if return_lse:
        out, lse = torch.ops.flash_attention.paged_varlen_forward_lse(q, k_cache, v_cache, cu_seqlens_q,
                                                                      int(max_seqlen_q), block_table, cache_seqlens,
                                                                      sinks, softmax_scale, causal, int(window_left))
        return out, lse
    if sinks is not None:
        return torch.ops.flash_attention.paged_varlen_forward_sink(q, k_cache, v_cache, cu_seqlens_q,
                                                                   int(max_seqlen_q), block_table, cache_seqlens,
                                                                   sinks, softmax_scale, causal, int(window_left))
    return torch.ops.flash_attention.paged_varlen_forward(q, k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q),
                                                          block_table, cache_seqlens, softmax_scale, causal,
                                                          int(window_left))


@torch.library.custom_op("flash_attention::kvcache_append_varlen", mutates_args=("k_cache", "v_cache"))
def flash_attention_kvcache_append_varlen(k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor,
                                          v: torch.Tensor, cu_seqlens_new: torch.Tensor, cache_seqlens: torch.Tensor,
                                          block_table: torch.Tensor, rotary_cos: Optional[torch.Tensor] = None,
                                          rotary_sin: Optional[torch.Tensor] = None,
                                          q: Optional[torch.Tensor] = None,
                                          cu_seqlens_q: Optional[torch.Tensor] = None
                                          ) -> tuple[torch.Tensor, torch.Tensor]:
    # caches: [num_pages, Hkv, page_size, D] with block_table int32 [B, max_pages]; k, v: [total_new, Hkv, D]
    # packed with cu_seqlens_new int32 [B + 1]; q: [total_q, Hq, D] with cu_seqlens_q (or None); rotary_*:
    # [max_pos, D]. Non-GPU default: the kernel's semantics token by token, with the same drop rules.
    if q is not None and rotary_cos is None:
        raise ValueError("q is rotated only: it needs rotary_cos / rotary_sin")
    if (q is None) != (cu_seqlens_q is None):
        raise ValueError("q and cu_seqlens_q must be given together")
    if k_cache.dtype == FP8_DTYPE:
        raise NotImplementedError("flash_attn_kvcache_append_varlen writes 16-bit paged caches only: use "
                                  "flash_attn_kvcache_append per chunk length for an FP8 cache")
    num_pages, _, page_size, _ = k_cache.shape
    cap = block_table.size(1) * page_size
    lens = [min(max(n, 0), cap) for n in cache_seqlens.tolist()]
    new_rng = _clamped_ranges(cu_seqlens_new, k.size(0))
    new_lens = [min(n + r1 - r0, cap) for n, (r0, r1) in zip(lens, new_rng)]
    table = block_table.tolist()
    rope = rotary_cos is not None
    if rope:
        cos, sin = rotary_cos.to(k_cache.dtype), rotary_sin.to(k_cache.dtype)
        max_pos = cos.size(0)
    for b, (r0, r1) in enumerate(new_rng):
        for i in range(r1 - r0):
            n = lens[b] + i
            if n >= cap:
                continue  # past the table's capacity: dropped
            page = table[b][n // page_size]
            if page < 0 or page >= num_pages:
                continue  # outside the pool: dropped, never clamped
            kr = k[r0 + i][None, :, None]
            if rope:
                pos = min(n, max_pos - 1)
                kr = _rope_reference(kr, cos[pos:pos + 1], sin[pos:pos + 1])
            k_cache[page, :, n % page_size] = kr[0, :, 0]
            v_cache[page, :, n % page_size] = v[r0 + i]
    if q is None:
        q_rot = k_cache.new_empty(0)
    else:
        q_rot = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        for b, (r0, r1) in enumerate(_clamped_ranges(cu_seqlens_q, q.size(0))):
            if r1 == r0:
                continue
            pos = torch.tensor([min(max(new_lens[b] - (r1 - r0) + i, 0), max_pos - 1) for i in range(r1 - r0)],
                               dtype=torch.int64, device=q.device)
            q_rot[r0:r1] = _rope_reference(q[r0:r1].transpose(0, 1)[None], cos[pos], sin[pos])[0].transpose(0, 1)
    return torch.tensor(new_lens, dtype=torch.int32, device=cache_seqlens.device), q_rot


@torch.library.register_kernel("flash_attention::kvcache_append_varlen", "cuda")
def flash_attention_kvcache_append_varlen_cuda(k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor,
                                               v: torch.Tensor, cu_seqlens_new: torch.Tensor,
                                               cache_seqlens: torch.Tensor, block_table: torch.Tensor,
                                               rotary_cos: Optional[torch.Tensor] = None,
                                               rotary_sin: Optional[torch.Tensor] = None,
                                               q: Optional[torch.Tensor] = None,
                                               cu_seqlens_q: Optional[torch.Tensor] = None
                                               ) -> tuple[torch.Tensor, torch.Tensor]:
    _require_ext()
    if k_cache.dtype == FP8_DTYPE:
        raise NotImplementedError("flash_attn_kvcache_append_varlen writes 16-bit paged caches only: use "
                                  "flash_attn_kvcache_append per chunk length for an FP8 cache")
    # the inputs may be copied to make their last dimension contiguous; the caches never are
    k, v, q = (t.contiguous() if t is not None and t.stride(-1) != 1 else t for t in (k, v, q))
    if rotary_cos is not None:
        rotary_cos, rotary_sin = rotary_cos.to(k_cache.dtype), rotary_sin.to(k_cache.dtype)
    new_seqlens, q_rot = flash_attention_cuda.flash_attention_kvcache_append_varlen(
        k_cache, v_cache, k, v, cu_seqlens_new, cache_seqlens, block_table, rotary_cos, rotary_sin, q, cu_seqlens_q)
    return new_seqlens, q_rot


@torch.library.register_fake("flash_attention::kvcache_append_varlen")
def flash_attention_kvcache_append_varlen_fake(k_cache, v_cache, k, v, cu_seqlens_new, cache_seqlens, block_table,
                                               rotary_cos=None, rotary_sin=None, q=None, cu_seqlens_q=None):
    q_rot = k_cache.new_empty(0) if q is None else torch.empty(q.shape, dtype=q.dtype, device=q.device)
    return torch.empty_like(cache_seqlens, memory_format=torch.contiguous_format), q_rot


def flash_attn_kvcache_append_varlen(k_cache, v_cache, k, v, cu_seqlens_new, cache_seqlens, block_table,
                                     rotary_cos=None, rotary_sin=None, q=None, cu_seqlens_q=None):
    """Append RAGGED new keys / values to a paged KV cache IN PLACE, one HIP launch: ``k`` / ``v`` [total_new,
    Hkv, D] packed, sequence b owning rows ``[cu_seqlens_new[b], cu_seqlens_new[b + 1])`` (int32 [B + 1]). Token
    i of sequence b is written at position ``n = cache_seqlens[b] + i`` -- row ``n % page_size`` of page
    ``block_table[b, n // page_size]`` -- under ``flash_attn_kvcache_append``'s rules to the letter: with the
    rotary tables [max_pos, D] k is rotated at ``min(n, max_pos - 1)``, bit for bit as ``apply_rope`` would; a
    write is DROPPED, never redirected, past the capacity ``max_pages * page_size`` or on a page id outside
    ``[0, num_pages)``; only the written cache rows are touched. Returns ``new_seqlens`` (int32 [B]:
    ``min(len_b + n_b, capacity)``; ``cache_seqlens`` is not modified), or ``(new_seqlens, q_rotated)`` when ``q``
    [total_q, Hq, D] is given with its own ``cu_seqlens_q``: row i of sequence b's ``Sq_b`` rows rotated at
    ``max(new_seqlens[b] - Sq_b + i, 0)`` -- the sequence's last ``Sq_b`` positions after the append, the
    convention of ``flash_attn_paged_varlen_func``.

    Both cumulative arrays are clamped on the device (a start into ``[0, total]``, an end into ``[start,
    total]``), so a bad array never reads outside the inputs. 16-bit paged caches only (dense caches and the FP8
    quantizing append: ``flash_attn_kvcache_append`` per chunk length). No host synchronisation."""
    new_seqlens, q_rot = torch.ops.flash_attention.kvcache_append_varlen(
        k_cache, v_cache, k, v, cu_seqlens_new, cache_seqlens, block_table, rotary_cos, rotary_sin, q, cu_seqlens_q)
    return new_seqlens if q is None else (new_seqlens, q_rot)


def flash_attn_varlen_with_kvcache(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, k=None, v=None,
                                   cu_seqlens_new=None, rotary_cos=None, rotary_sin=None, cache_seqlens=None,
                                   block_table=None, softmax_scale=None, causal=False, window_left=-1,
                                   return_seqlens=False, sinks=None, return_lse=False):
    """One step of a continuous batch on the paged cache, ``flash_attn_with_kvcache`` in the packed layout: the
    new ``k`` / ``v`` [total_new, Hkv, D] are appended in place at ``cache_seqlens``
    (``flash_attn_kvcache_append_varlen``; ``cu_seqlens_new`` defaults to ``cu_seqlens_q``, a step's new tokens
    being its queries), with the rotary tables k is rotated at its new positions and ``q`` [total_q, Hq, D] at
    each sequence's last ``Sq_b`` positions after the append, then q attends over the advanced lengths
    (``flash_attn_paged_varlen_func``, whose contract applies). Returns ``out`` [total_q, Hq, D], or ``(out,
    new_seqlens)`` with ``return_seqlens=True``; ``cache_seqlens`` is not modified. Two launches and no host
    synchronisation, so the step can be captured in a graph.

    ``sinks`` (fp32 [Hq], or ``None``): attention sinks in the attention half, as in
    ``flash_attn_paged_varlen_func``; a bad ``sinks``, or a layout the sinked kernel does not read, is refused
    before anything is appended.

    ``return_lse=True``: the attention half also returns its LSE (fp32 [Hq, total_q], as
    ``flash_attn_paged_varlen_func(return_lse=True)``): ``(out, lse)``, or ``(out, lse, new_seqlens)`` with
    ``return_seqlens=True``. ``False`` is the call without the argument, bit for bit."""
    if cache_seqlens is None or block_table is None:
        raise ValueError("flash_attn_varlen_with_kvcache needs cache_seqlens (int32 [batch]) and block_table")
    if sinks is not None:
        sinks = _sinks_arg(sinks, q)  # (the errors of the attention half, before anything is appended)
    if sinks is not None or return_lse:
        _paged_varlen_unsupported(q, k_cache, v_cache)
    if (k is None) != (v is None):
        raise ValueError("k and v must be given together")
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError("rotary_cos and rotary_sin must be given together")
    softmax_scale = _default_scale(q, softmax_scale)
    new_seqlens, q_rot = cache_seqlens, q
    if k is not None or rotary_cos is not None:
        if k is None:  # (q rotated at the current lengths: an append of no token)
            k = v = q.new_empty((0, k_cache.size(1), q.size(-1)))
            cu_seqlens_new = torch.zeros_like(cu_seqlens_q)
        elif cu_seqlens_new is None:
            cu_seqlens_new = cu_seqlens_q
        if rotary_cos is not None:  # (cast as apply_rope casts its tables)
            new_seqlens, q_rot = torch.ops.flash_attention.kvcache_append_varlen(
                k_cache, v_cache, k, v, cu_seqlens_new, cache_seqlens, block_table, rotary_cos.to(q.dtype),
                rotary_sin.to(q.dtype), q, cu_seqlens_q)
        else:
            new_seqlens, _ = torch.ops.flash_attention.kvcache_append_varlen(
                k_cache, v_cache, k, v, cu_seqlens_new, cache_seqlens, block_table)
    if return_lse:
        out, lse = flash_attn_paged_varlen_func(q_rot, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table,
                                                new_seqlens, softmax_scale, causal, window_left, sinks, True)
        return (out, lse, new_seqlens) if return_seqlens else (out, lse)
    out = flash_attn_paged_varlen_func(q_rot, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table, new_seqlens,
                                       softmax_scale, causal, window_left, sinks)
    return (out, new_seqlens) if return_seqlens else out


def _varlen_lse_into(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, table, seqlens, sinks, scale, causal, out, lse):
    """One ragged LSE launch that writes o / lse into the given tensors (as ``_lse_into`` for the decode)."""
    if q.is_cuda:
        _paged_varlen_lse_cuda(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, table, seqlens, sinks, scale, causal,
                               -1, out, lse)
    else:
        o, l = _paged_varlen_reference(q, k_cache, v_cache, cu_seqlens_q, table, seqlens, scale, causal, -1, sinks,
                                       return_lse=True)
        out.copy_(o)
        lse.copy_(l)


def flash_attn_paged_varlen_shared_prefix_func(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table,
                                               cache_seqlens, prefix_len, group_size=None, softmax_scale=None,
                                               causal=False, sinks=None, return_lse=False):
    """One step of ``flash_attn_paged_varlen_func`` for a ragged batch whose sequences SHARE their first
    ``prefix_len`` keys, ``group_size`` consecutive sequences at a time (``None``: the whole batch; the last group
    may be shorter): speculative-token blocks, short chunks or parallel samples behind one system prompt. The shared
    pages are streamed once per GROUP and q-head instead of once per sequence and q-head, and the group's rows fill
    the kernel's 256-row blocks that a short sequence alone leaves almost empty.

    The caller's contract:

    * ``prefix_len`` is a Python int and a multiple of ``page_size`` (``ValueError`` otherwise), at most the
      table's capacity;
    * every sequence holds at least ``prefix_len + Sq_b`` keys, so its chunk lies wholly behind the prefix (a
      sequence that does not is computed as if it did: its prefix rows are not masked);
    * the rows of one group carry the same page ids in their first ``prefix_len / page_size`` table entries;
      ``FA_CHECK_SHARED_PREFIX=1`` (read per call, eager only, off by default) verifies that with one host read
      and raises ``ValueError``;
    * no ``window_left``: a row's window would cut into the prefix per sequence (not built).

    How it runs: the packed layout makes a group of sequences ONE ragged sequence whose ``cu_seqlens_q`` entries
    are the group's boundaries. Prefix phase, one launch of the LSE kernel: ``cu_seqlens_q[0:B:c]`` and the last
    entry, the table ``block_table[::c, :prefix_len / page_size]`` (a strided view), every group ``prefix_len``
    keys (the lengths are the first entries of ``cache_seqlens``, which the table's capacity clamps to exactly
    ``prefix_len``), NON-causal, ``max_seqlen_q`` times ``c``, no sinks. Suffix phase, one launch: the table
    ``block_table[:, prefix_len / page_size:]`` with ``cache_seqlens - prefix_len`` keys, ``causal`` and ``sinks``
    as given -- the sink is in exactly one state, which makes the merge exact. Then the packed
    ``flash_attn_merge_states``. Three launches and two small device ops (the group boundaries, the suffix
    lengths); no host synchronisation, so the step can be captured in a graph.

    What is never read: the prefix table entries of every row but a group's first.

    The result differs from ``flash_attn_paged_varlen_func`` on the same tables by rounding only (the two partial
    outputs are rounded to q's dtype before the merge). ``prefix_len == 0`` IS ``flash_attn_paged_varlen_func``,
    bit for bit. Returns ``out`` [total_q, Hq, D], or ``(out, lse)`` with the merged LSE [Hq, total_q]. It is an
    explicit call: nothing dispatches to it. Measured crossover against the one-launch call: not measured."""
    prefix_len = int(prefix_len)
    page_size = k_cache.size(2)
    if prefix_len < 0 or prefix_len % page_size != 0:
        raise ValueError(f"prefix_len ({prefix_len}) must be a non-negative multiple of page_size ({page_size})")
    if q.dim() != 3:
        raise ValueError(f"ragged q must be [total_q, Hq, D] (got {tuple(q.shape)})")
    b = cu_seqlens_q.numel() - 1
    c = b if group_size is None else int(group_size)
    if group_size is not None and c < 1:
        raise ValueError(f"group_size ({c}) must be at least 1")
    if prefix_len == 0:
        return flash_attn_paged_varlen_func(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table,
                                            cache_seqlens, softmax_scale, causal, -1, sinks, return_lse)
    n_pre = prefix_len // page_size
    if n_pre > block_table.size(1):
        raise ValueError(f"prefix_len ({prefix_len}) exceeds the block table's capacity "
                         f"({block_table.size(1) * page_size})")
    if block_table.dim() != 2 or block_table.size(0) != b or cache_seqlens.numel() != b:
        raise ValueError(f"block_table must have, and cache_seqlens be, one row per sequence ({b})")
    softmax_scale = _default_scale(q, softmax_scale)
    if sinks is not None:
        sinks = _sinks_arg(sinks, q)
    _paged_varlen_unsupported(q, k_cache, v_cache)
    total_q, hq, d = q.shape
    if b <= 0 or total_q == 0:
        out = torch.empty_like(q)
        return (out, q.new_empty((hq, total_q), dtype=torch.float32)) if return_lse else out
    c = min(max(c, 1), b)
    n_groups = (b + c - 1) // c
    if _check_shared_prefix_enabled() and not torch.compiler.is_compiling() and not (
            q.is_cuda and torch.cuda.is_current_stream_capturing()):
        _check_shared_prefix_table(block_table, n_pre, [(i * c, min((i + 1) * c, b)) for i in range(n_groups)])
    if q.stride(-1) != 1:
        q = q.contiguous()
    if block_table.stride(1) != 1:
        block_table = block_table.contiguous()

    # the two states, side by side so that the merge reads them where the launches wrote them: [0] the prefix
    # phase, [1] the suffix phase
    outs = torch.empty((2, total_q, hq, d), dtype=q.dtype, device=q.device)
    lses = torch.empty((2, hq, total_q), dtype=torch.float32, device=q.device)
    # prefix phase: the group boundaries (one device op), each group's first table row, prefix_len keys each
    cu_groups = cu_seqlens_q if c == 1 else torch.cat([cu_seqlens_q[0:b:c], cu_seqlens_q[b:b + 1]])
    _varlen_lse_into(q, k_cache, v_cache, cu_groups, c * int(max_seqlen_q), block_table[::c, :n_pre],
                     cache_seqlens[:n_groups], None, softmax_scale, False, outs[0], lses[0])
    # suffix phase: every sequence's own keys (a table without suffix columns: 0 keys, no entry is read)
    if n_pre < block_table.size(1):
        table, lens = block_table[:, n_pre:], cache_seqlens - prefix_len
    else:
        table, lens = block_table[:, :1], torch.zeros_like(cache_seqlens)
    _varlen_lse_into(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, table, lens, sinks, softmax_scale, causal,
                     outs[1], lses[1])
    return flash_attn_merge_states(outs, lses, return_lse)
