"""The argument checks of the torch binding (csrc/flash_attention_api.cpp): one table of (entry, one
malformed argument) -> the substring of the message it raises. Every row violates one condition and
raises before any launch. With CPU tensors everything up to each entry's ``is_cuda`` check is reachable;
the rows marked ``gpu`` cover the checks behind it (still before any launch: no kernel runs).

The entries differ on purpose in what they accept (a strided block table is copied by some and refused by
others, ``cache_seqlens`` is optional in one, one writes into the caller's tensors): the tests below the table
pin that, on the GPU, at the table's sizes."""
from __future__ import annotations

import re

import pytest
import torch

from flash_attention_cute_amd import flash_attention as fam

B, HQ, HKV, S, D = 2, 4, 2, 8, 64
PAGES, PAGE = 4, 32
F16, BF16, F32, FP8 = torch.float16, torch.bfloat16, torch.float32, torch.float8_e4m3fn


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


def paged_fp8(dev="cpu", dtype=FP8):
    # q, k_cache, v_cache, block_table, cache_seqlens, k_descale, v_descale, softmax_scale, causal
    return [*paged(dev)[:1], z(PAGES, HKV, PAGE, D, dtype=dtype, dev=dev), z(PAGES, HKV, PAGE, D, dtype=dtype, dev=dev),
            *paged(dev)[3:5], None, None, 0.125, False]


def paged_window(dev="cpu", page=PAGE, hq=HQ):
    # q, k_cache, v_cache, block_table, cache_seqlens, window_left, softmax_scale, causal (the prefill entry: the same)
    return [z(B, hq, 1, D, dev=dev), *paged(dev, page)[1:5], 16, 0.125, False]


def paged_lse(dev="cpu"):
    # q, k_cache, v_cache, block_table, cache_seqlens, seqlen_offset, k_descale, v_descale, softmax_scale, causal,
    # out, lse_out
    return [*paged(dev)[:5], 0, None, None, 0.125, False, None, None]


def paged_varlen(dev="cpu", page=2 * PAGE):
    # q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, block_table, cache_seqlens, window_left, softmax_scale, causal
    return [z(3, HQ, D, dev=dev), *paged(dev, page)[1:3], i32([0, 1, 3], dev), 2, *paged(dev)[3:5], -1, 0.125, True]


def kvcache_fp8(dev="cpu", dtype=FP8):
    # the arguments of kvcache() with caches of their own dtype, then k_descale, v_descale
    return [z(PAGES, HKV, PAGE, D, dtype=dtype, dev=dev), z(PAGES, HKV, PAGE, D, dtype=dtype, dev=dev),
            *kvcache(dev)[2:], None, None]


def kvcache_varlen(dev="cpu", dtype=F16):
    # k_cache, v_cache, k, v, cu_seqlens_new, cache_seqlens, block_table, rotary_cos, rotary_sin, q, cu_seqlens_q
    cu = i32([0, 1, 3], dev)
    return [z(PAGES, HKV, PAGE, D, dtype=dtype, dev=dev), z(PAGES, HKV, PAGE, D, dtype=dtype, dev=dev),
            z(3, HKV, D, dtype=dtype, dev=dev), z(3, HKV, D, dtype=dtype, dev=dev), cu, i32([40, 7], dev),
            i32([[0, 1], [2, 3]], dev), z(64, D, dtype=dtype, dev=dev), z(64, D, dtype=dtype, dev=dev),
            z(3, HQ, D, dtype=dtype, dev=dev), cu.clone()]


def strided_table(dev="cpu"):
    """The table of paged() as a view with column stride 2."""
    return i32([[0, 9, 1, 9], [2, 9, 3, 9]], dev)[:, ::2]


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
    ("paged-fp8-fp16-caches", "flash_attention_paged_fp8_fwd", lambda: paged_fp8(dtype=F16),
     "the fp8 caches must be torch.float8_e4m3fn"),
    ("paged-window-page-48", "flash_attention_paged_window_fwd", lambda: paged_window(page=48),
     "positive multiple of 32"),
    ("paged-prefill-hq-3-hkv-2", "flash_attention_paged_prefill_fwd", lambda: paged_window(hq=3),
     "multiple of number of heads"),
    ("paged-lse-cache-shapes", "flash_attention_paged_lse_fwd",
     lambda: replaced(paged_lse(), a2=z(PAGES + 1, HKV, PAGE, D)), "k_cache, v_cache must have the same shape"),
    ("paged-lse-descale-16-bit", "flash_attention_paged_lse_fwd",
     lambda: replaced(paged_lse(), a6=z(B, HKV, dtype=F32)), "k_descale / v_descale go with an fp8 cache"),
    ("paged-lse-valid-cpu", "flash_attention_paged_lse_fwd", lambda: paged_lse(), "on CUDA device"),
    ("paged-varlen-4d-q", "flash_attention_paged_varlen_fwd", lambda: replaced(paged_varlen(), a0=z(1, 3, HQ, D)),
     "ragged q must be 3-D"),
    ("paged-varlen-page-32", "flash_attention_paged_varlen_fwd", lambda: paged_varlen(page=PAGE),
     "positive multiple of 64"),
    ("paged-varlen-valid-cpu", "flash_attention_paged_varlen_fwd", lambda: paged_varlen(), "on CUDA device"),
    ("kvcache-fp8-fp16-caches", "flash_attention_kvcache_append_fp8", lambda: kvcache_fp8(dtype=F16),
     "the fp8 caches must be torch.float8_e4m3fn"),
    ("kvcache-varlen-fp32", "flash_attention_kvcache_append_varlen", lambda: kvcache_varlen(dtype=F32),
     "only support fp16 or bf16"),
    ("kvcache-varlen-valid-cpu", "flash_attention_kvcache_append_varlen", lambda: kvcache_varlen(),
     "same CUDA device"),
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
    ("paged-lse-table-strided", "flash_attention_paged_lse_fwd",
     lambda dev: replaced(paged_lse(dev), a3=strided_table(dev)), "block_table rows must be contiguous"),
    ("paged-lse-seqlens-int64", "flash_attention_paged_lse_fwd",
     lambda dev: replaced(paged_lse(dev), a4=i32([40, 7], dev, torch.int64)), "cache_seqlens must be int32 [batch]"),
    ("paged-lse-out-shape", "flash_attention_paged_lse_fwd",
     lambda dev: replaced(paged_lse(dev), a10=z(B, HQ, 2, D, dev=dev)), "out must have q's shape"),
    ("paged-lse-lse-out-fp16", "flash_attention_paged_lse_fwd",
     lambda dev: replaced(paged_lse(dev), a11=z(B, HQ, 1, dev=dev)), "lse_out must be fp32"),
    ("paged-varlen-table-strided", "flash_attention_paged_varlen_fwd",
     lambda dev: replaced(paged_varlen(dev), a5=strided_table(dev)), "block_table rows must be contiguous"),
    ("paged-varlen-cu-int64", "flash_attention_paged_varlen_fwd",
     lambda dev: replaced(paged_varlen(dev), a3=i32([0, 1, 3], dev, torch.int64)), "cu_seqlens_q must be int32"),
    ("paged-varlen-table-batch", "flash_attention_paged_varlen_fwd",
     lambda dev: replaced(paged_varlen(dev), a5=i32([[0, 1]], dev)), "block_table must be int32 [batch, max_pages]"),
    ("paged-fp8-descale-1d", "flash_attention_paged_fp8_fwd",
     lambda dev: replaced(paged_fp8(dev), a5=z(B, dtype=F32, dev=dev)), "k_descale must be fp32 [batch, kv heads]"),
    # (behind the entry's is_cuda check: with CPU tensors "same CUDA device" fires first)
    ("kvcache-varlen-q-without-cu", "flash_attention_kvcache_append_varlen",
     lambda dev: replaced(kvcache_varlen(dev), a10=None), "q and cu_seqlens_q must be given together"),
    ("kvcache-varlen-cu-new-entries", "flash_attention_kvcache_append_varlen",
     lambda dev: replaced(kvcache_varlen(dev), a4=i32([0, 3], dev)),
     "cu_seqlens_new must be int32 with batch + 1 entries"),
    ("kvcache-varlen-cos-columns", "flash_attention_kvcache_append_varlen",
     lambda dev: replaced(kvcache_varlen(dev), a7=z(64, D + 2, dev=dev)), "must be [max_pos,"),
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


# ---- what the entries accept: they differ on purpose (still the file's tiny sizes, Sq 1) ---------------------------
def rand(*shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(F16).to(dev)


def ext():
    if fam.flash_attention_cuda is None:
        pytest.skip(f"extension not built: {fam._load_error!r}")
    return fam.flash_attention_cuda


def same_bits(a, b):
    as_int = {2: torch.int16, 4: torch.int32}
    return (a.shape == b.shape and a.dtype == b.dtype and
            torch.equal(a.contiguous().view(as_int[a.element_size()]), b.contiguous().view(as_int[b.element_size()])))


@pytest.mark.gpu
def test_paged_fwd_copies_a_strided_table(device):
    """flash_attention_paged_fwd takes a table whose column stride is not 1 (it is copied): the same bits."""
    args = replaced(paged(device), a0=rand(B, HQ, 1, D, dev=device, seed=1),
                    a1=rand(PAGES, HKV, PAGE, D, dev=device, seed=2), a2=rand(PAGES, HKV, PAGE, D, dev=device, seed=3))
    want = ext().flash_attention_paged_fwd(*args)
    table = strided_table(device)
    assert table.stride(1) == 2 and torch.equal(table, args[3])
    got = ext().flash_attention_paged_fwd(*replaced(args, a3=table))
    assert same_bits(got, want) and got.float().abs().max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("entry,make,table_at", [("flash_attention_kvcache_append", kvcache, 5),
                                                 ("flash_attention_kvcache_append_varlen", kvcache_varlen, 6)])
def test_append_copies_a_strided_table(entry, make, table_at, device):
    """Both 16-bit appends take a table whose column stride is not 1 (it is copied): the same caches, lengths and
    rotated q as with the contiguous table."""
    def run(table):
        args = make(device)
        for i, t in enumerate(args):  # the same random tensors for both calls; the caches are written in place
            if torch.is_tensor(t) and t.dtype == F16:
                args[i] = rand(*t.shape, dev=device, seed=10 + i)
        args[table_at] = table
        new_seqlens, q_rot = getattr(ext(), entry)(*args)
        return args[0], args[1], new_seqlens, q_rot

    table = strided_table(device)
    want = run(make(device)[table_at])
    assert table.stride(1) == 2 and torch.equal(table, make(device)[table_at])
    got = run(table)
    for g, w in zip(got, want):
        assert same_bits(g, w)
    assert got[2].tolist() == ([41, 8] if make is kvcache else [41, 9])  # 1 + 1 new rows, or 1 + 2


@pytest.mark.gpu
def test_paged_lse_without_cache_seqlens(device):
    """flash_attention_paged_lse_fwd with cache_seqlens=None and seqlen_offset n: bit for bit the call with
    cache_seqlens all zero and the same offset."""
    args = replaced(paged_lse(device), a0=rand(B, HQ, 1, D, dev=device, seed=1),
                    a1=rand(PAGES, HKV, PAGE, D, dev=device, seed=2), a2=rand(PAGES, HKV, PAGE, D, dev=device, seed=3),
                    a5=40)
    o_zero, lse_zero = ext().flash_attention_paged_lse_fwd(*replaced(args, a4=i32([0, 0], device)))
    o_none, lse_none = ext().flash_attention_paged_lse_fwd(*replaced(args, a4=None))
    assert same_bits(o_none, o_zero) and same_bits(lse_none, lse_zero)
    assert torch.isfinite(lse_none).all() and o_none.float().abs().max() > 0


@pytest.mark.gpu
def test_paged_lse_writes_into_the_callers_tensors(device):
    """flash_attention_paged_lse_fwd returns the caller's out / lse_out themselves, written in place."""
    args = replaced(paged_lse(device), a0=rand(B, HQ, 1, D, dev=device, seed=1),
                    a1=rand(PAGES, HKV, PAGE, D, dev=device, seed=2), a2=rand(PAGES, HKV, PAGE, D, dev=device, seed=3))
    o_own, lse_own = ext().flash_attention_paged_lse_fwd(*args)
    out = torch.full((B, HQ, 1, D), float("nan"), dtype=F16, device=device)
    lse_out = torch.full((B, HQ, 1), float("nan"), dtype=F32, device=device)
    o, lse = ext().flash_attention_paged_lse_fwd(*replaced(args, a10=out, a11=lse_out))
    assert o.data_ptr() == out.data_ptr() and lse.data_ptr() == lse_out.data_ptr()
    assert same_bits(out, o_own) and same_bits(lse_out, lse_own)
