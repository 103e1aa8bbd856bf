"""Shared-prefix (cascade) decode on the paged cache: ``flash_attn_paged_shared_prefix_func`` and
``flash_attn_with_kvcache(shared_prefix_len=...)``.

No reference counterpart. A batch whose sequences share their first ``prefix_len`` keys -- their block tables point
at the same physical pages -- is served by streaming the prefix once per GROUP of c sequences (one batch row of the
LSE decode kernel, the group's queries as its positions), each sequence's own keys by the LSE decode kernel, and one
``flash_attn_merge_states``. Pinned here, with the poisoned pools and shuffled tables of tests/test_paged.py:

* parity with the float64 oracle on the dense keys within tests/test_gpu_parity.py TOL (fp16 2e-3 + 2e-3|ref|,
  bf16 1.6e-2 + 1.6e-2|ref|) and with ``flash_attn_paged_func`` on the same table within twice that bound (both
  sit inside one bound of the oracle), for batches that hold a full group and a non-empty tail (g 4: c = 8, B 11;
  g 8: c = 4, B 7), suffix lengths 0, 1, 31, 32, 33, 70, a split prefix (fused and unfused) and an FP8 pool;
* a needle at the seam: keys prefix_len - 1 and prefix_len carry the weight, with distinct one-hot V rows --
  dropping either, or counting it twice, moves the output by O(1);
* prefix_len = 0 is ``flash_attn_paged_func`` bit for bit;
* what is never read: the prefix entries of every row but a group's first, and entries past a sequence's end;
* one captured step replays bit-equal; ``flash_attn_with_kvcache`` equals the explicit composition bit for bit.
"""
from __future__ import annotations

import warnings

import pytest
import torch

from test_fp8_kvcache import make_fp8_paged, pow2_descales
from test_padded import oracle_padded
from test_paged import make_paged

F16, BF16 = torch.float16, torch.bfloat16
GROUP_ROWS = 32  # flash_attention._SHARED_PREFIX_GROUP_ROWS: c = 32 // g


def check_bound(out, ref, dtype, factor=1.0, what=""):
    """The elementwise bound of tests/test_gpu_parity.py TOL, times ``factor``."""
    from tests.test_gpu_parity import TOL

    atol, rtol, _ = TOL[dtype]
    got, ref = out.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    worst = (err - factor * (atol + rtol * ref.abs())).max().item()
    assert worst <= 0, f"{what}: max err {err.max().item():.3e} exceeds the bound by {worst:.3e}"


def share_prefix(k, v, kc, vc, table, prefix, page, c):
    """Make rows [i c, (i + 1) c) of the batch share the first row's prefix: the dense keys are copied, the table
    entries point at the first row's pages, and the pages no longer referenced are poisoned again."""
    n_pre = prefix // page
    nan = float("nan") if kc.dtype.is_floating_point and kc.dtype != torch.float8_e4m3fn else None
    for i in range(table.size(0)):
        first = i // c * c
        if i == first:
            continue
        k[i, :, :prefix], v[i, :, :prefix] = k[first, :, :prefix], v[first, :, :prefix]
        for j in range(n_pre):
            if nan is not None:
                kc[table[i, j]], vc[table[i, j]] = nan, nan
            else:
                kc.view(torch.uint8)[table[i, j]], vc.view(torch.uint8)[table[i, j]] = 0x7F, 0x7F
            table[i, j] = table[first, j]


def make_shared(b, hq, hkv, page, prefix, suffixes, d, dtype, seed, layout="phsd"):
    g = hq // hkv
    c = max(1, GROUP_ROWS // g)
    lens = [prefix + suffixes[i % len(suffixes)] for i in range(b)]
    cap = (max(lens) + page - 1) // page * page + page  # (one spare, unused table column)
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, 1, page, cap, d, dtype, seed, layout)
    share_prefix(k, v, kc, vc, table, prefix, page, c)
    return q, k, v, kc, vc, table, sl, c


# ------------------------------------------------------------------------------------------- CPU
def test_shared_prefix_cpu_default_matches_oracle():
    from flash_attention_cute_amd import flash_attn_paged_func, flash_attn_paged_shared_prefix_func

    q, k, v, kc, vc, table, sl, c = make_shared(11, 8, 2, 32, 96, (0, 1, 31, 32, 33, 70), 64, F16, 3)
    assert 11 // c >= 1 and 11 % c
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, lse = flash_attn_paged_shared_prefix_func(q.float(), kc.float(), vc.float(), table, sl, 96, return_lse=True)
        plain, plain_lse = flash_attn_paged_func(q.float(), kc.float(), vc.float(), table, sl, return_lse=True)
        zero = flash_attn_paged_shared_prefix_func(q.float(), kc.float(), vc.float(), table, sl, 0)
    ref = oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, 64 ** -0.5, False).float()
    torch.testing.assert_close(out, ref, atol=3e-3, rtol=3e-3)
    torch.testing.assert_close(out, plain, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(lse, plain_lse, atol=1e-5, rtol=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert torch.equal(zero, flash_attn_paged_func(q.float(), kc.float(), vc.float(), table, sl))


def test_shared_prefix_wrapper_errors(monkeypatch):
    from flash_attention_cute_amd import (flash_attn_paged_func, flash_attn_paged_shared_prefix_func,
                                          flash_attn_with_kvcache)

    q, _, _, kc, vc, table, sl, _ = make_shared(3, 8, 2, 32, 64, (5,), 64, F16, 1)
    kc, vc = kc.float().nan_to_num(0), vc.float().nan_to_num(0)
    q = q.float()
    with pytest.raises(ValueError, match="multiple of page_size"):
        flash_attn_paged_shared_prefix_func(q, kc, vc, table, sl, 48)
    with pytest.raises(ValueError, match="multiple of page_size"):
        flash_attn_paged_shared_prefix_func(q, kc, vc, table, sl, -32)
    with pytest.raises(ValueError, match="capacity"):
        flash_attn_paged_shared_prefix_func(q, kc, vc, table, sl, 32 * (table.size(1) + 1))
    with pytest.raises(ValueError, match="decode steps"):
        flash_attn_paged_shared_prefix_func(q.expand(-1, -1, 2, -1), kc, vc, table, sl, 64)
    with pytest.raises(NotImplementedError, match="window"):
        flash_attn_paged_func(q, kc, vc, table, sl, window_left=3, return_lse=True)
    dense = torch.zeros(3, 2, 128, 64)
    with pytest.raises(ValueError, match="paged cache"):
        flash_attn_with_kvcache(q, dense, dense, cache_seqlens=sl, shared_prefix_len=64)
    with pytest.raises(ValueError, match="Sq == 1"):
        flash_attn_with_kvcache(q.expand(-1, -1, 2, -1), kc, vc, cache_seqlens=sl, block_table=table,
                                shared_prefix_len=64)
    with pytest.raises(ValueError, match="window_left"):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=sl, block_table=table, shared_prefix_len=64, window_left=7)
    # the eager check, read per call: rows of a group that differ in a prefix entry
    bad = table.clone()
    bad[1, 0] = bad[1, 0] + 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flash_attn_paged_shared_prefix_func(q, kc, vc, bad, sl, 64)  # off by default
        monkeypatch.setenv("FA_CHECK_SHARED_PREFIX", "1")
        flash_attn_paged_shared_prefix_func(q, kc, vc, table, sl, 64)
        with pytest.raises(ValueError, match="same page ids"):
            flash_attn_paged_shared_prefix_func(q, kc, vc, bad, sl, 64)


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def ops(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam
    from flash_attention_cute_amd import flash_attn_paged_func, flash_attn_paged_shared_prefix_func

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    assert fam._SHARED_PREFIX_GROUP_ROWS == GROUP_ROWS
    _debug.set_knobs()
    _debug.set_dec_fuse(None)
    yield flash_attn_paged_shared_prefix_func, flash_attn_paged_func, _debug
    _debug.set_dec_fuse(None)


SUFFIXES = (0, 1, 31, 32, 33, 70)
# (B, Hq, Hkv, page, prefix, D, dtype, layout): g 4 -> c 8, B 11 = a group of 8 and a tail of 3; g 8 -> c 4, B 7 = a
# group of 4 and a tail of 3
CASES = [
    (11, 8, 2, 32, 96, 64, F16, "phsd"),
    (11, 8, 2, 64, 128, 128, BF16, "pshd"),
    (7, 8, 1, 32, 128, 128, F16, "pshd"),
    (7, 8, 1, 64, 128, 64, BF16, "phsd"),
]
CASE_IDS = [f"b{b}-g{hq // hkv}-p{p}-pre{pre}-d{d}-{'f16' if t == F16 else 'bf16'}" for b, hq, hkv, p, pre, d, t, _ in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_shared_prefix_parity_groups_and_tail(ops, device, ci):
    shared, paged, _ = ops
    b, hq, hkv, page, prefix, d, dtype, layout = CASES[ci]
    q, k, v, kc, vc, table, sl, c = make_shared(b, hq, hkv, page, prefix, SUFFIXES, d, dtype, 500 + ci, layout)
    assert b // c >= 1 and b % c  # a full group and a non-empty tail
    dq, dkc, dvc, dt, dsl = (t.to(device) for t in (q, kc, vc, table, sl))
    out, lse = shared(dq, dkc, dvc, dt, dsl, prefix, return_lse=True)
    plain, plain_lse = paged(dq, dkc, dvc, dt, dsl, return_lse=True)
    ref = oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, False)
    check_bound(out, ref, dtype, 1.0, "oracle")
    check_bound(out, plain, dtype, 2.0, "paged")
    assert (lse - plain_lse).abs().max().item() <= 2.0 ** -11  # (each within 2^-12 of the exact value)
    assert torch.equal(shared(dq, dkc, dvc, dt, dsl, prefix), out)  # without the lse: the same bits
    # prefix_len = 0 is the paged call itself
    assert torch.equal(shared(dq, dkc, dvc, dt, dsl, 0), paged(dq, dkc, dvc, dt, dsl))
    # a sequence shorter than the prefix is treated as exactly the prefix
    short = dsl.clone()
    short[1] = prefix - 5
    exact = dsl.clone()
    exact[1] = prefix
    assert torch.equal(shared(dq, dkc, dvc, dt, short, prefix), shared(dq, dkc, dvc, dt, exact, prefix))


@pytest.mark.gpu
@pytest.mark.parametrize("ci", [0, 3], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_shared_prefix_entries_that_are_never_read(ops, device, ci):
    """Out-of-range ids in the prefix entries of every row but a group's first, and in every entry past a sequence's
    last page (the prefix phase's view ends at prefix_len / page_size): the bits of the clean table."""
    shared, _, _ = ops
    b, hq, hkv, page, prefix, d, dtype, layout = CASES[ci]
    q, _, _, kc, vc, table, sl, c = make_shared(b, hq, hkv, page, prefix, SUFFIXES, d, dtype, 500 + ci, layout)
    poisoned = table.clone()
    for i in range(b):
        if i % c:
            poisoned[i, :prefix // page] = 2 ** 31 - 1 - i
        poisoned[i, (int(sl[i]) + page - 1) // page:] = -(2 ** 31) + i
    assert not torch.equal(poisoned, table)
    dq, dkc, dvc, dsl = (t.to(device) for t in (q, kc, vc, sl))
    clean = shared(dq, dkc, dvc, table.to(device), dsl, prefix)
    out = shared(dq, dkc, dvc, poisoned.to(device), dsl, prefix)
    assert torch.isfinite(out.float()).all() and torch.equal(out, clean)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", [None, 0], ids=["fused", "unfused"])
def test_shared_prefix_split_prefix_phase(ops, device, fuse):
    """prefix 2048, B 2: the prefix phase (one group, Hkv units) splits its keys, merged in the kernel or by the
    combine launch."""
    shared, paged, _debug = ops
    page, prefix, d = 64, 2048, 128
    q, k, v, kc, vc, table, sl, c = make_shared(2, 8, 2, page, prefix, (33, 70), d, BF16, 61)
    dq, dkc, dvc, dt, dsl = (t.to(device) for t in (q, kc, vc, table, sl))
    _debug.set_dec_fuse(fuse)
    # the prefix phase on its own, as the function launches it: it splits
    o, l = torch.ops.flash_attention.paged_forward_lse(dq.view(1, 2, 8, d).transpose(1, 2), dkc, dvc,
                                                       dt[:1, :prefix // page], None, prefix, d ** -0.5, False)
    assert _debug.last_path() == "decode_paged_split" and _debug.last_dec_fused() == (fuse is None)
    out = shared(dq, dkc, dvc, dt, dsl, prefix)
    ref = oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, False)
    check_bound(out, ref, BF16, 1.0, "oracle")
    check_bound(out, paged(dq, dkc, dvc, dt, dsl), BF16, 2.0, "paged")


@pytest.mark.gpu
def test_shared_prefix_fp8_pool(ops, device):
    from test_fp8_kvcache import fp8_oracle

    shared, paged, _ = ops
    b, hq, hkv, page, prefix, d = 11, 8, 2, 64, 128, 128
    c = GROUP_ROWS // (hq // hkv)
    lens = [prefix + SUFFIXES[i % len(SUFFIXES)] for i in range(b)]
    cap = (max(lens) + page - 1) // page * page
    # the same descales for every row (rows of a group must share them); distinct per kv-head
    kd, vd = pow2_descales(1, hkv).expand(b, hkv).contiguous(), pow2_descales(1, hkv, 2).expand(b, hkv).contiguous()
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, 1, page, cap, d, BF16, 71, kd=kd, vd=vd)
    share_prefix(k8, v8, kc8, vc8, table, prefix, page, c)
    dv = lambda t: t.to(device)  # noqa: E731
    out = shared(dv(q), dv(kc8), dv(vc8), dv(table), dv(sl), prefix, k_descale=dv(kd), v_descale=dv(vd))
    plain = paged(dv(q), dv(kc8), dv(vc8), dv(table), dv(sl), k_descale=dv(kd), v_descale=dv(vd))
    check_bound(out, fp8_oracle(q, k8, v8, sl, kd, vd, False), BF16, 1.0, "oracle")
    check_bound(out, plain, BF16, 2.0, "paged")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_needle_at_the_seam(ops, device, dtype):
    """Keys prefix_len - 1 (the last of the prefix phase) and prefix_len (the first of the suffix phase) carry logit
    8 against 0 for the rest, with V rows e_1 and e_2: the output is ~0.49 on each of the two columns. A phase that
    drops its needle gives ~(0, 0.97) or (0.97, 0); one that counts it twice ~(0.65, 0.33)."""
    shared, _, _ = ops
    b, hq, hkv, page, prefix, d = 9, 8, 2, 32, 96, 64
    q, k, v, kc, vc, table, sl, c = make_shared(b, hq, hkv, page, prefix, (1, 33, 70), d, dtype, 81)
    q.zero_(), k.zero_(), v.zero_()
    q[..., 0] = 8.0
    for n, col in ((prefix - 1, 1), (prefix, 2)):
        k[:, :, n, 0] = 8.0
        v[:, :, n, col] = 1.0
    for i in range(b):  # the pool from the dense keys (the shared prefix pages hold the same rows for every sequence)
        for j in range((int(sl[i]) + page - 1) // page):
            rows = min(int(sl[i]), (j + 1) * page) - j * page
            kc[table[i, j], :, :rows] = k[i, :, j * page:j * page + rows]
            vc[table[i, j], :, :rows] = v[i, :, j * page:j * page + rows]
    out = shared(*(t.to(device) for t in (q, kc, vc, table, sl)), prefix).float().cpu()
    ref = oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, False).float()
    assert 0.45 < ref[0, 0, 0, 1] < 0.5 and 0.45 < ref[0, 0, 0, 2] < 0.5  # both needles carry the row
    check_bound(out, ref, dtype, 1.0, "needle")


@pytest.mark.gpu
def test_shared_prefix_graph_capture(ops, device):
    """No host synchronisation, no allocation outside the caching allocator: one captured step replays twice with
    the same bits and matches the eager call within the bound (under capture the split merge is not fused)."""
    shared, _, _ = ops
    b, hq, hkv, page, prefix, d = 11, 8, 2, 64, 2048, 128
    q, k, v, kc, vc, table, sl, c = make_shared(b, hq, hkv, page, prefix, SUFFIXES, d, BF16, 91)
    dq, dkc, dvc, dt, dsl = (t.to(device) for t in (q, kc, vc, table, sl))
    eager = shared(dq, dkc, dvc, dt, dsl, prefix)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = shared(dq, dkc, dvc, dt, dsl, prefix)
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.equal(out, first)
    check_bound(out, eager, BF16, 1.0, "eager")
    check_bound(out, oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, False), BF16, 1.0, "oracle")


@pytest.mark.gpu
def test_with_kvcache_shared_prefix_equals_the_composition(ops, device):
    from flash_attention_cute_amd import flash_attn_kvcache_append, flash_attn_with_kvcache

    shared, paged, _ = ops
    b, hq, hkv, page, prefix, d = 11, 8, 2, 32, 96, 64
    q, k, v, kc, vc, table, sl, c = make_shared(b, hq, hkv, page, prefix, (1, 31, 32, 33, 70), d, F16, 95)
    g = torch.Generator().manual_seed(5)
    k_new, v_new = (torch.randn(b, hkv, 1, d, generator=g).to(F16).to(device) for _ in range(2))
    dq, dt = q.to(device), table.to(device)
    before = (sl - 1).to(device)  # the step appends each sequence's last key
    kc1, vc1, kc2, vc2 = (t.to(device).nan_to_num(0.0) for t in (kc, vc, kc, vc))
    out, new = flash_attn_with_kvcache(dq, kc1, vc1, k_new, v_new, cache_seqlens=before, block_table=dt,
                                       shared_prefix_len=prefix, return_seqlens=True)
    lens2 = flash_attn_kvcache_append(kc2, vc2, k_new, v_new, before, dt)
    want = shared(dq, kc2, vc2, dt, lens2, prefix)
    assert torch.equal(new, lens2) and torch.equal(new.cpu(), sl)
    assert torch.equal(kc1, kc2) and torch.equal(out, want)
    # the default is the call as it was
    plain = flash_attn_with_kvcache(dq, kc1, vc1, cache_seqlens=new, block_table=dt)
    assert torch.equal(plain, flash_attn_with_kvcache(dq, kc1, vc1, cache_seqlens=new, block_table=dt, shared_prefix_len=0))
    assert torch.equal(plain, paged(dq, kc1, vc1, dt, new))
