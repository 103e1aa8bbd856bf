"""The argument checks of the torch binding (csrc/flash_attention_api.cpp): one table of (entry, one
malformed argument) -> the substring of the message it raises. Every row violates one condition and
raises before any launch. With CPU tensors everything up to each entry's ``is_cuda`` check is reachable;
the rows marked ``gpu`` cover the checks behind it (still before any launch: no kernel runs)."""
from __future__ import annotations

import re

import pytest
import torch

from flash_attention_cute_amd import flash_attention as fam

B, HQ, HKV, S, D = 2, 4, 2, 8, 64
PAGES, PAGE = 4, 32
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def z(*shape, dtype=F16, dev="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=dev)


def i32(vals, dev="cpu", dtype=torch.int32):
    return torch.tensor(vals, dtype=dtype, device=dev)


def qkv(dev="cpu", b=B, hq=HQ, hkv=HKV, sq=S, sk=S, d=D, dtype=F16):
    return [z(b, hq, sq, d, dtype=dtype, dev=dev), z(b, hkv, sk, d, dtype=dtype, dev=dev),
            z(b, hkv, sk, d, dtype=dtype, dev=dev)]


def replaced(args, **by_index):
    args = list(args)
    for i, val in by_index.items():
        args[int(i[1:])] = val
    return args


# ---- valid argument lists of each entry (a row replaces one argument) ----------------------------------------
def fwd(dev="cpu", **kw):
    return [*qkv(dev, **kw), 0.125, False]


def window(dev="cpu", window_left=2):
    return [*qkv(dev), window_left, 0.125, True]


def rope_apply(dev="cpu", dtype=F16):
    return [z(B, HQ, S, D, dtype=dtype, dev=dev), z(S, D, dtype=dtype, dev=dev), z(S, D, dtype=dtype, dev=dev)]


def rope_fwd(dev="cpu"):
    return [*qkv(dev), z(S, D, dev=dev), z(S, D, dev=dev), 0.125, True]


def varlen(dev="cpu", d=D):
    cu = i32([0, S, 2 * S], dev)
    return [z(B * S, HQ, d, dev=dev), z(B * S, HKV, d, dev=dev), z(B * S, HKV, d, dev=dev), cu, cu.clone(), S, S,
            0.125, True, -1]


def padded(dev="cpu", **kw):
    return [*qkv(dev, **kw), None, None, i32([0, 1], dev), i32([S, S - 1], dev), 0.125, True, -1]


def paged(dev="cpu", page=PAGE):
    return [z(B, HQ, 1, D, dev=dev), z(PAGES, HKV, page, D, dev=dev), z(PAGES, HKV, page, D, dev=dev),
            i32([[0, 1], [2, 3]], dev), i32([40, 7], dev), 0.125, False]


def kvcache(dev="cpu", dtype=F16):
    # k_cache, v_cache, k, v, cache_seqlens, block_table, q, rotary_cos, rotary_sin
    return [z(PAGES, HKV, PAGE, D, dtype=dtype, dev=dev), z(PAGES, HKV, PAGE, D, dtype=dtype, dev=dev),
            z(B, HKV, 1, D, dtype=dtype, dev=dev), z(B, HKV, 1, D, dtype=dtype, dev=dev), i32([40, 7], dev),
            i32([[0, 1], [2, 3]], dev), z(B, HQ, 1, D, dtype=dtype, dev=dev), z(64, D, dtype=dtype, dev=dev),
            z(64, D, dtype=dtype, dev=dev)]


CPU_ROWS = [
    ("fwd-3d-q", "flash_attention_fwd", lambda: replaced(fwd(), a0=z(B, S, D)), "must be 4-D"),
    ("fwd-batch", "flash_attention_fwd", lambda: replaced(fwd(), a0=z(B + 1, HQ, S, D)), "same batch size"),
    ("fwd-kv-heads", "flash_attention_fwd", lambda: replaced(fwd(), a2=z(B, 1, S, D)),
     "k, v must have the same number of heads"),
    ("fwd-kv-len", "flash_attention_fwd", lambda: replaced(fwd(), a2=z(B, HKV, 2 * S, D)), "same sequence length"),
    ("fwd-d-mismatch", "flash_attention_fwd", lambda: replaced(fwd(), a0=z(B, HQ, S, 32)), "same hidden dimension"),
    ("fwd-sk-0", "flash_attention_fwd", lambda: fwd(sk=0), "at least one element"),
    ("fwd-hq-lt-hkv", "flash_attention_fwd", lambda: fwd(hq=2, hkv=4), "greater or equal"),
    ("fwd-hq-3-hkv-2", "flash_attention_fwd", lambda: fwd(hq=3, hkv=2), "multiple of number of heads"),
    ("fwd-mixed-dtype", "flash_attention_fwd", lambda: replaced(fwd(), a1=z(B, HKV, S, D, dtype=BF16)),
     "same data type"),
    ("fwd-fp32", "flash_attention_fwd", lambda: fwd(dtype=F32), "only support fp16 or bf16"),
    ("fwd-q-strided", "flash_attention_fwd", lambda: replaced(fwd(), a0=z(B, HQ, S, 2 * D)[..., ::2]),
     "q must be contiguous in the last dimension"),
    ("fwd-d-12", "flash_attention_fwd", lambda: fwd(d=12), "multiple of 8"),
    ("fwd-d-136", "flash_attention_fwd", lambda: fwd(d=136), "<= 128"),
    ("fwd-valid-cpu", "flash_attention_fwd", lambda: fwd(), "must be on CUDA device"),
    ("window-negative", "flash_attention_window_fwd", lambda: window(window_left=-1), "window_left must be >= 0"),
    ("rope-apply-3d", "rope_apply", lambda: replaced(rope_apply(), a0=z(B, S, D)), "x must be 4-D"),
    ("rope-apply-fp32", "rope_apply", lambda: rope_apply(dtype=F32), "RoPE supports fp16 or bf16"),
    ("rope-apply-valid-cpu", "rope_apply", lambda: rope_apply(), "x must be on CUDA device"),
    # a CPU q is never "fused": the entry rotates with rope_apply first
    ("rope-fwd-valid-cpu", "flash_attention_rope_fwd", lambda: rope_fwd(), "x must be on CUDA device"),
    ("varlen-4d", "flash_attention_varlen_fwd", lambda: replaced(varlen(), a0=z(B, S, HQ, D)), "must be 3-D"),
    ("varlen-d-12", "flash_attention_varlen_fwd", lambda: varlen(d=12), "multiple of 8"),
    ("varlen-valid-cpu", "flash_attention_varlen_fwd", lambda: varlen(), "on CUDA device"),
    ("padded-hq-3-hkv-2", "flash_attention_padded_fwd", lambda: padded(hq=3, hkv=2), "multiple of number of heads"),
    ("padded-valid-cpu", "flash_attention_padded_fwd", lambda: padded(), "on CUDA device"),
    ("paged-cache-shapes", "flash_attention_paged_fwd", lambda: replaced(paged(), a2=z(PAGES + 1, HKV, PAGE, D)),
     "k_cache, v_cache must have the same shape"),
    ("paged-page-48", "flash_attention_paged_fwd", lambda: paged(page=48), "positive multiple of 32"),
    ("paged-valid-cpu", "flash_attention_paged_fwd", lambda: paged(), "on CUDA device"),
    ("kvcache-3d-cache", "flash_attention_kvcache_append",
     lambda: replaced(kvcache(), a0=z(HKV, PAGE, D), a1=z(HKV, PAGE, D)), "the caches must be 4-D"),
    ("kvcache-fp32", "flash_attention_kvcache_append", lambda: kvcache(dtype=F32), "only support fp16 or bf16"),
    ("kvcache-valid-cpu", "flash_attention_kvcache_append", lambda: kvcache(), "same CUDA device"),
]

GPU_ROWS = [
    ("varlen-cu-int64", "flash_attention_varlen_fwd",
     lambda dev: replaced(varlen(dev), a3=i32([0, S, 2 * S], dev, torch.int64)), "cu_seqlens must be int32"),
    ("varlen-cu-lengths", "flash_attention_varlen_fwd",
     lambda dev: replaced(varlen(dev), a4=i32([0, S, 2 * S, 2 * S], dev)), "batch_size + 1 entries"),
    ("padded-q-start-alone", "flash_attention_padded_fwd", lambda dev: replaced(padded(dev), a3=i32([0, 0], dev)),
     "given together"),
    ("padded-k-start-int64", "flash_attention_padded_fwd",
     lambda dev: replaced(padded(dev), a5=i32([0, 1], dev, torch.int64)), "k_start must be int32 [batch]"),
    ("paged-table-batch", "flash_attention_paged_fwd", lambda dev: replaced(paged(dev), a3=i32([[0, 1]], dev)),
     "block_table must be int32 [batch, max_pages]"),
    ("paged-seqlens-int64", "flash_attention_paged_fwd",
     lambda dev: replaced(paged(dev), a4=i32([40, 7], dev, torch.int64)), "cache_seqlens must be int32 [batch]"),
    ("kvcache-k-without-v", "flash_attention_kvcache_append", lambda dev: replaced(kvcache(dev), a3=None),
     "k and v must be given together"),
    ("kvcache-q-without-tables", "flash_attention_kvcache_append",
     lambda dev: replaced(kvcache(dev), a7=None, a8=None), "needs rotary_cos / rotary_sin"),
    ("kvcache-dense-batch", "flash_attention_kvcache_append", lambda dev: replaced(kvcache(dev), a5=None),
     "a dense cache must have"),
    ("kvcache-cos-columns", "flash_attention_kvcache_append",
     lambda dev: replaced(kvcache(dev), a7=z(64, D + 2, dev=dev)), "must be [max_pos,"),
    ("rope-apply-table-layouts", "rope_apply", lambda dev: replaced(rope_apply(dev), a2=z(B, S, D, dev=dev)),
     "cos and sin must have the same layout"),
]


ROWS = ([pytest.param(*r[1:], False, id=r[0]) for r in CPU_ROWS] +
        [pytest.param(*r[1:], True, id=r[0], marks=pytest.mark.gpu) for r in GPU_ROWS])


@pytest.mark.parametrize("entry,make,message,gpu", ROWS)
def test_binding_rejects(entry, make, message, gpu, request):
    if fam.flash_attention_cuda is None:
        pytest.skip(f"extension not built: {fam._load_error!r}")
    args = make(request.getfixturevalue("device")) if gpu else make()
    with pytest.raises(RuntimeError, match=re.escape(message)):
        getattr(fam.flash_attention_cuda, entry)(*args)
