"""Ragged queries, the ragged append and the step on the paged KV cache (GPU).

``flash_attn_paged_varlen_func`` runs the paged fa_fwd_w4 with per-sequence query ranges (C-ABI
``fa_fwd_gfx950_paged_varlen``, include/fa_gfx950_paged_varlen.h). The ragged paged launch walks the same
256-row blocks and the same 64-key tiles in the same order, through the same arithmetic, as
``flash_attn_varlen_func`` on the gathered keys packed densely (the same kernel body with q / k ranges), so
every attention case asserts, in this order: (1) ``torch.equal`` with that call, (2) agreement with the float
oracle (``test_padded.oracle_padded`` per sequence) within tests/test_gpu_parity.py TOL, (3) a finite output and
the path labels (``last_path() == "w4"`` with ``last_prefill_paged()``).

Pools are built as tests/test_paged.py ``make_paged`` builds them: a shuffled table, NaN in every unused row
and unreferenced page, -1 in unused entries. ``flash_attn_kvcache_append_varlen`` is held, bit for bit, to the
existing ``flash_attn_kvcache_append`` called once per sequence with B = 1.
"""
from __future__ import annotations

import functools

import pytest
import torch

from test_kvcache import PATTERN, rope_tables
from test_padded import check_padded, oracle_padded
from test_paged import make_paged

F16, BF16 = torch.float16, torch.bfloat16
DEV = "cuda:0"
I32 = torch.int32


def dv(*ts):
    return tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in ts)


def cu_of(counts):
    out = [0]
    for n in counts:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=I32)


class Ragged:
    """One ragged case on the host: ``pairs`` of (Sq_b, L_b); q packed [total_q, Hq, D] and the dense keys
    [B, Hkv, cap, D] of make_paged, scattered into its NaN-poisoned pool through its shuffled table."""

    def __init__(self, pairs, hq, hkv, page, cap, d, dtype, seed, layout="phsd"):
        self.sqs, self.lens = [p[0] for p in pairs], [p[1] for p in pairs]
        self.max_q, self.dtype, self.d = max(self.sqs), dtype, d
        q4, self.k, self.v, self.kc, self.vc, self.table, self.sl = make_paged(
            self.lens, hq, hkv, max(self.max_q, 1), page, cap, d, dtype, seed, layout)
        self.q4 = q4
        self.q = torch.cat([q4[b, :, :s].transpose(0, 1) for b, s in enumerate(self.sqs)]).contiguous()
        self.cu_q = cu_of(self.sqs)

    def packed_keys(self):
        kp = torch.cat([self.k[b, :, :n].transpose(0, 1) for b, n in enumerate(self.lens)]).contiguous()
        vp = torch.cat([self.v[b, :, :n].transpose(0, 1) for b, n in enumerate(self.lens)]).contiguous()
        return kp, vp, cu_of(self.lens)

    def oracle(self, causal, w=-1):
        """test_padded.oracle_padded per sequence, packed."""
        out = torch.zeros_like(self.q)
        for b, (s, n) in enumerate(zip(self.sqs, self.lens)):
            if s == 0:
                continue
            r0 = int(self.cu_q[b])
            one = oracle_padded(self.q4[b:b + 1, :, :s], self.k[b:b + 1], self.v[b:b + 1], torch.tensor([0], dtype=I32),
                                torch.tensor([n], dtype=I32), None, None, self.d ** -0.5, causal, window_left=w)
            out[r0:r0 + s] = one[0].transpose(0, 1)
        return out


@pytest.fixture
def fam(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    yield fam
    _debug.set_knobs()


def ragged_launch(c, causal, w=-1, q=None, kc=None, vc=None, table=None, cu_q=None, max_q=None):
    """One ragged paged launch on the device: (output on the host, last_path, last_prefill_paged)."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_varlen_func

    q = c.q.to(DEV) if q is None else q
    kc, vc, table = (c.kc if kc is None else kc), (c.vc if vc is None else vc), (c.table if table is None else table)
    out = flash_attn_paged_varlen_func(q, *dv(kc, vc, c.cu_q if cu_q is None else cu_q),
                                       c.max_q if max_q is None else max_q, *dv(table, c.sl), causal=causal,
                                       window_left=w)
    labels = _debug.last_path(), _debug.last_prefill_paged()
    torch.cuda.synchronize()
    return (out.cpu(), *labels)


def dense_varlen(c, causal, w=-1):
    """The reference for bit-identity: flash_attn_varlen_func on the gathered keys packed densely."""
    from flash_attention_cute_amd import _debug, flash_attn_varlen_func

    kp, vp, cu_k = c.packed_keys()
    out = flash_attn_varlen_func(*dv(c.q, kp, vp, c.cu_q, cu_k), c.max_q, max(c.lens), causal=causal, window_left=w)
    assert _debug.last_path() == "w4" and not _debug.last_prefill_paged()
    torch.cuda.synchronize()
    return out.cpu()


def check_case(c, causal, w=-1):
    """The three checks of every attention case, in the order the module docstring gives; returns the output."""
    out, path, in_place = ragged_launch(c, causal, w)
    assert torch.equal(out, dense_varlen(c, causal, w))
    check_padded(out, c.oracle(causal, w), c.dtype)
    assert torch.isfinite(out.float()).all()
    assert path == "w4" and in_place
    return out


# 1. the base grid: an empty query range; one row; no keys; fewer keys than queries (causal: the first three rows
# 0); exactly one q-tile with L == Sq; one row into the second q-tile with a full table; a tile tail one key past
# the queries. (page, dtype, layout) cycle as test_paged_prefill.BASE does.
BASE_PAIRS = ((0, 300), (1, 449), (40, 0), (40, 37), (256, 256), (257, 512), (300, 301))
BASE = [(64, F16, "phsd"), (128, BF16, "pshd"), (256, F16, "pshd"), (64, BF16, "pshd"), (128, F16, "phsd"),
        (256, BF16, "phsd")]


@functools.lru_cache(maxsize=None)
def base_case(page, dtype, layout):
    return Ragged(BASE_PAIRS, 8, 2, page, 512, 128, dtype, 1900 + page, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("page,dtype,layout", BASE, ids=[f"p{p}-{'f16' if t == F16 else 'bf16'}-{lay}" for p, t, lay in BASE])
def test_base_grid(fam, page, dtype, layout, causal):
    c = base_case(page, dtype, layout)
    out = check_case(c, causal)
    r = c.cu_q.tolist()
    assert (out[r[2]:r[3]] == 0).all()  # no keys: 0 rows, no table entry read
    if causal:
        assert (out[r[3]:r[3] + 3] == 0).all()  # 37 keys under 40 queries: the first three rows see none
        assert not (out[r[3] + 3] == 0).all()


# 2. the tie to the existing public op: a sequence alone (B = 1) through flash_attn_paged_func's paged prefill
@pytest.mark.gpu
@pytest.mark.parametrize("causal,w", [(False, -1), (True, -1), (True, 100)], ids=["full", "causal", "causal-w100"])
@pytest.mark.parametrize("page,dtype,layout", BASE[:2], ids=["p64-f16-phsd", "p128-bf16-pshd"])
def test_each_sequence_equals_the_uniform_paged_op_alone(fam, page, dtype, layout, causal, w):
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    c = base_case(page, dtype, layout)
    out, path, in_place = ragged_launch(c, causal, w)
    assert path == "w4" and in_place
    tied = 0
    for b, s in enumerate(c.sqs):
        if 8 // 2 * s <= 64:
            continue  # (a decode shape: another kernel)
        one = flash_attn_paged_func(*dv(c.q4[b:b + 1, :, :s].contiguous(), c.kc, c.vc, c.table[b:b + 1], c.sl[b:b + 1]),
                                    causal=causal, window_left=w)
        assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
        r0 = int(c.cu_q[b])
        assert torch.equal(out[r0:r0 + s], one[0].transpose(0, 1).cpu()), b
        tied += 1
    assert tied == 5


# 3. other shapes: head dims 64 and 96, g 1 and 4
@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("hq,d,dtype", [(2, 64, F16), (8, 96, BF16), (2, 96, F16), (8, 64, BF16)],
                         ids=["g1-d64", "g4-d96", "g1-d96", "g4-d64"])
def test_other_head_dims_and_groups(fam, hq, d, dtype, causal):
    c = Ragged(((300, 700), (0, 100), (1, 1), (257, 300), (65, 64), (40, 768)), hq, 2, 128, 768, d, dtype, 1910 + hq + d)
    check_case(c, causal)


# q as a strided slice of a fused [total, Hq + 2 Hkv, D] projection, read in place (no copy: the same storage)
@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_q_slice_of_a_fused_qkv_projection(fam, causal):
    c = base_case(64, BF16, "pshd")
    hq, hkv = 8, 2
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(c.q.size(0), hq + 2 * hkv, 128, generator=g).to(BF16)
    qkv[:, :hq] = c.q
    qkv_d = qkv.to(DEV)
    q_view = qkv_d[:, :hq]
    assert not q_view.is_contiguous() and q_view.stride(0) == (hq + 2 * hkv) * 128
    from flash_attention_cute_amd import _debug, flash_attn_paged_varlen_func

    kc, vc, cu_q, table, sl = dv(c.kc, c.vc, c.cu_q, c.table, c.sl)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = flash_attn_paged_varlen_func(q_view, kc, vc, cu_q, c.max_q, table, sl, causal=causal)
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    q_bytes = c.q.numel() * 2
    print(f"peak rise {rise} bytes; q {q_bytes} bytes")
    assert rise < q_bytes + q_bytes // 2  # the output, and no contiguous copy of q beside it
    assert torch.equal(out.cpu(), check_case(c, causal))


# 4. many rounds per workgroup: 6 sequences x 2 heads x 2 q-tiles = 24 blocks on 8 workgroups, so a workgroup's
# consecutive blocks belong to different sequences with different Sq_b -- the next block's Q and first K tile,
# staged under the drain, go through ANOTHER row range, table row and length. Two launches give the same bits.
ROUNDS_PAIRS = ((300, 700), (40, 64), (257, 301), (0, 50), (129, 129), (1, 512))


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_many_rounds_per_workgroup_and_determinism(fam, causal):
    from flash_attention_cute_amd import _debug

    c = Ragged(ROUNDS_PAIRS, 2, 2, 64, 768, 128, BF16, 1920)
    plain = check_case(c, causal)
    with _debug.knobs(w4_grid=8):
        walked, path, in_place = ragged_launch(c, causal)
        again, _, _ = ragged_launch(c, causal)
    assert path == "w4" and in_place
    assert torch.equal(walked, plain) and torch.equal(again, walked)


# 5. the window, per sequence with its own Sq_b: the pages wholly below max(0, L_b - Sq_b - W) // 64 * 64, and their
# table entries, may hold anything
WIN_PAIRS = ((0, 300), (1, 449), (40, 37), (40, 640), (256, 768), (300, 640), (17, 768))


@pytest.mark.gpu
@pytest.mark.parametrize("w,page,causal", [(0, 64, True), (63, 128, False), (100, 64, True), (100, 64, False),
                                           (63, 64, True), (0, 128, False)],
                         ids=["w0-p64-causal", "w63-p128-full", "w100-p64-causal", "w100-p64-full", "w63-p64-causal",
                              "w0-p128-full"])
def test_window_and_freed_pages(fam, w, page, causal):
    c = Ragged(WIN_PAIRS, 8, 2, page, 768, 128, F16, 1930 + w + page, "pshd")
    out = check_case(c, causal, w)
    freed_any = 0
    for bad in (-1, 2 ** 31 - 1):
        kc, vc, table = c.kc.clone(), c.vc.clone(), c.table.clone()
        for b, (s, n) in enumerate(zip(c.sqs, c.lens)):
            for j in range(max(0, n - s - w) // 64 * 64 // page):
                kc[int(table[b, j])], vc[int(table[b, j])] = float("nan"), float("nan")
                table[b, j] = bad
                freed_any += 1
        got, path, in_place = ragged_launch(c, causal, w, kc=kc, vc=vc, table=table)
        assert path == "w4" and in_place
        assert torch.isfinite(got.float()).all() and torch.equal(got, out)
    assert freed_any >= 8  # (the case does free pages)


# 6. never read or written: a larger max_seqlen_q only launches empty q-tiles
@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_a_larger_max_seqlen_q_gives_the_same_bits(fam, causal):
    c = base_case(128, F16, "phsd")
    out = check_case(c, causal)
    for max_q in (301, 512, 1500):
        got, path, in_place = ragged_launch(c, causal, max_q=max_q)
        assert path == "w4" and in_place and torch.equal(got, out), max_q


@pytest.mark.gpu
def test_an_empty_step_launches_nothing(fam):
    """Batch 0 (cu_seqlens_q with one entry) and total_q 0: the attention returns an empty / untouched output as the
    append takes the same step, instead of raising."""
    from flash_attention_cute_amd import flash_attn_kvcache_append_varlen, flash_attn_paged_varlen_func

    c = Ragged(((40, 64), (17, 100)), 8, 2, 64, 128, 128, F16, 1945)
    kc, vc = dv(c.kc, c.vc)
    none = dict(device=DEV, dtype=I32)
    cu0, table0, sl0 = torch.zeros(1, **none), torch.zeros(0, 2, **none), torch.zeros(0, **none)
    out = flash_attn_paged_varlen_func(c.q[:0].to(DEV), kc, vc, cu0, 0, table0, sl0, causal=True)
    assert out.shape == (0, 8, 128)
    out = flash_attn_paged_varlen_func(c.q.to(DEV), kc, vc, cu0, 40, table0, sl0, causal=True)  # rows of no sequence
    assert out.shape == c.q.shape
    new = flash_attn_kvcache_append_varlen(kc, vc, c.q[:0, :2].to(DEV), c.q[:0, :2].to(DEV), cu0, sl0, table0)
    torch.cuda.synchronize()
    assert new.shape == (0,)
    out = flash_attn_paged_varlen_func(c.q[:0].to(DEV), kc, vc, *dv(torch.zeros(3, dtype=I32)), 0, *dv(c.table, c.sl))
    assert out.shape == (0, 8, 128)


@pytest.mark.gpu
def test_unsupported_layouts_name_the_alternative(fam):
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    c = Ragged(((40, 64), (17, 96)), 8, 2, 32, 96, 128, F16, 1940)
    with pytest.raises(NotImplementedError, match="flash_attn_paged_func"):
        flash_attn_paged_varlen_func(*dv(c.q, c.kc, c.vc, c.cu_q), c.max_q, *dv(c.table, c.sl))
    c = Ragged(((40, 64), (17, 100)), 8, 2, 64, 128, 128, F16, 1941)
    k8 = c.kc.nan_to_num(0.0).to(torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="FP8"):
        flash_attn_paged_varlen_func(*dv(c.q, k8, k8, c.cu_q), c.max_q, *dv(c.table, c.sl))
    c = Ragged(((40, 64), (17, 100)), 8, 2, 64, 128, 68, F16, 1942)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        flash_attn_paged_varlen_func(*dv(c.q, c.kc, c.vc, c.cu_q), c.max_q, *dv(c.table, c.sl))


# ------------------------------------------------------------------------------------------- the append
def ragged_cache(lens, news, hkv, page, cap, d, dtype, seed, layout="phsd"):
    """A cache that holds ``lens`` keys per sequence with room for ``news[b]`` more: test_kvcache.make_cache with a
    per-sequence token count (the pool and shuffled table of make_paged for the lengths after the append, rows
    without a key set to PATTERN)."""
    after = tuple(min(max(n, 0) + m, cap) for n, m in zip(lens, news))
    _, _, _, kc, vc, table, _ = make_paged(after, hkv, hkv, 1, page, cap, d, dtype, seed, layout)
    for c in (kc, vc):
        c[c.isnan()] = PATTERN
    return kc, vc, table, torch.tensor(lens, dtype=I32)


def packed_rows(total, h, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(total, h, d, generator=g).to(dtype)


def per_sequence_append(kc, vc, k, v, cu_new, sl, table, cos, sin, q, cu_q):
    """The existing flash_attn_kvcache_append op called once per sequence with B = 1, on clones: (k_cache,
    v_cache, new_seqlens, q_rot)."""
    kc, vc = kc.clone(), vc.clone()
    cn = cu_new.tolist()
    cq = cu_q.tolist() if cu_q is not None else None
    new, q_rot = [], (torch.empty_like(q) if q is not None else None)
    for b in range(sl.numel()):
        kb = k[cn[b]:cn[b + 1]].transpose(0, 1)[None]
        vb = v[cn[b]:cn[b + 1]].transpose(0, 1)[None]
        kb, vb = (kb, vb) if kb.size(2) else (None, None)
        qb = None
        if q is not None and cq[b + 1] > cq[b]:
            qb = q[cq[b]:cq[b + 1]].transpose(0, 1)[None]
        if kb is None and qb is None:
            new.append(sl[b:b + 1].clamp(0, table.size(1) * kc.size(2)))
            continue
        n1, qr = torch.ops.flash_attention.kvcache_append(kc, vc, kb, vb, sl[b:b + 1], table[b:b + 1], qb, cos, sin)
        new.append(n1)
        if qb is not None:
            q_rot[cq[b]:cq[b + 1]] = qr[0].transpose(0, 1)
    return kc, vc, torch.cat(new), q_rot


APPEND_LENS = (63, 64, 30, 100, 0, 250)  # tokens land on page edges (63 + 1, 64 + 40, 100 + 300 = 400 ...)
APPEND_NEWS = (1, 40, 0, 300, 300, 40)
APPEND_SQS = (1, 40, 7, 300, 301, 17)  # 301 > 300 keys after the append: a sequence shorter than its Sq_b


@pytest.mark.gpu
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("page,dtype,layout", [(64, F16, "phsd"), (128, BF16, "pshd"), (32, BF16, "phsd")],
                         ids=["p64-f16", "p128-bf16-pshd", "p32-bf16"])
def test_append_equals_per_sequence_appends(fam, page, dtype, layout, rope):
    from flash_attention_cute_amd import flash_attn_kvcache_append_varlen

    hq, hkv, cap, d = 8, 2, 512, 128
    kc, vc, table, sl = dv(*ragged_cache(APPEND_LENS, APPEND_NEWS, hkv, page, cap, d, dtype, 1950 + page, layout))
    cu_new, cu_q = dv(cu_of(APPEND_NEWS), cu_of(APPEND_SQS))
    k, v = dv(packed_rows(sum(APPEND_NEWS), hkv, d, dtype, 1), packed_rows(sum(APPEND_NEWS), hkv, d, dtype, 2))
    q = packed_rows(sum(APPEND_SQS), hq, d, dtype, 3).to(DEV) if rope else None
    cos, sin = dv(*rope_tables(cap, d, dtype)) if rope else (None, None)
    kc_ref, vc_ref, new_ref, q_ref = per_sequence_append(kc, vc, k, v, cu_new, sl, table, cos, sin, q, cu_q if rope else None)
    kc0, vc0 = kc.clone(), vc.clone()
    got = flash_attn_kvcache_append_varlen(kc, vc, k, v, cu_new, sl, table, cos, sin, q, cu_q if rope else None)
    torch.cuda.synchronize()
    new, q_rot = got if rope else (got, None)
    assert new.tolist() == [min(n + m, cap) for n, m in zip(APPEND_LENS, APPEND_NEWS)] and torch.equal(new, new_ref)
    # the whole pool, as int16: every target row holds the per-sequence append's bits and every other row is untouched
    for c, ref, c0 in ((kc, kc_ref, kc0), (vc, vc_ref, vc0)):
        assert torch.equal(c.view(torch.int16), ref.view(torch.int16))
        changed = (c.view(torch.int16) != c0.view(torch.int16)).any(dim=-1)
        assert int(changed.sum()) <= sum(APPEND_NEWS) * hkv and int(changed.sum()) > 0
    assert (kc.cpu() == PATTERN).all(dim=-1).any()  # (poisoned rows stay poisoned: some are left)
    if rope:
        assert torch.equal(q_rot.view(torch.int16), q_ref.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
def test_append_drop_rules(fam, rope):
    """A sequence that overflows its capacity loses only the overflowing tokens; a page id of -1 or num_pages under
    a new token drops that token only."""
    from flash_attention_cute_amd import flash_attn_kvcache_append_varlen

    hkv, page, cap, d, dtype = 2, 64, 256, 64, F16
    lens, news = (250, 60, 0, 100), (40, 70, 130, 0)  # 250 + 40 > 256: 6 written, 34 dropped
    kc, vc, table, sl = ragged_cache(lens, news, hkv, page, cap, d, dtype, 1960)
    table[1, 1] = -1                # sequence 1's tokens at positions 64 .. 127: dropped; 60 .. 63 and 128, 129 written
    table[2, 0] = kc.size(0)        # sequence 2's tokens at 0 .. 63: dropped; 64 .. 129 written
    kc, vc, table, sl = dv(kc, vc, table, sl)
    cu_new = cu_of(news).to(DEV)
    k, v = dv(packed_rows(sum(news), hkv, d, dtype, 4), packed_rows(sum(news), hkv, d, dtype, 5))
    cos, sin = dv(*rope_tables(cap, d, dtype)) if rope else (None, None)
    kc_ref, vc_ref, new_ref, _ = per_sequence_append(kc, vc, k, v, cu_new, sl, table, cos, sin, None, None)
    kc0 = kc.clone()
    new = flash_attn_kvcache_append_varlen(kc, vc, k, v, cu_new, sl, table, cos, sin)
    torch.cuda.synchronize()
    assert new.tolist() == [256, 130, 130, 100] and torch.equal(new, new_ref)
    assert torch.equal(kc.view(torch.int16), kc_ref.view(torch.int16))
    assert torch.equal(vc.view(torch.int16), vc_ref.view(torch.int16))
    written = int((kc.view(torch.int16) != kc0.view(torch.int16)).any(dim=-1).sum())
    assert written == (6 + (4 + 2) + 66) * hkv  # exactly the surviving tokens' rows


# ------------------------------------------------------------------------------------------- the step
STEP_LENS = (70, 0, 33, 200, 449)
STEP_NEWS = (40, 300, 1, 0, 63)


def step_inputs(dtype, seed, page=64, cap=512, hq=8, hkv=2, d=128):
    kc, vc, table, sl = ragged_cache(STEP_LENS, STEP_NEWS, hkv, page, cap, d, dtype, seed)
    total = sum(STEP_NEWS)
    return dict(kc=kc, vc=vc, table=table, sl=sl, cu=cu_of(STEP_NEWS), k=packed_rows(total, hkv, d, dtype, seed + 1),
                v=packed_rows(total, hkv, d, dtype, seed + 2), q=packed_rows(total, hq, d, dtype, seed + 3),
                cos_sin=rope_tables(cap, d, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("causal,w", [(True, -1), (False, -1), (True, 100)], ids=["causal", "full", "causal-w100"])
def test_step_equals_append_then_attention_and_the_oracle(fam, causal, w):
    from flash_attention_cute_amd import _debug

    s = step_inputs(BF16, 1970)
    kc, vc, table, sl, cu, k, v, q = dv(s["kc"], s["vc"], s["table"], s["sl"], s["cu"], s["k"], s["v"], s["q"])
    cos, sin = dv(*s["cos_sin"])
    kc2, vc2 = kc.clone(), vc.clone()
    out, new = fam.flash_attn_varlen_with_kvcache(q, kc, vc, cu, max(STEP_NEWS), k, v, rotary_cos=cos, rotary_sin=sin,
                                                  cache_seqlens=sl, block_table=table, causal=causal, window_left=w,
                                                  return_seqlens=True)
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
    new2, q_rot = fam.flash_attn_kvcache_append_varlen(kc2, vc2, k, v, cu, sl, table, cos, sin, q, cu)
    ref = fam.flash_attn_paged_varlen_func(q_rot, kc2, vc2, cu, max(STEP_NEWS), table, new2, causal=causal, window_left=w)
    torch.cuda.synchronize()
    assert new.tolist() == [a + b for a, b in zip(STEP_LENS, STEP_NEWS)] and torch.equal(new, new2)
    assert torch.equal(kc.view(torch.int16), kc2.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc2.view(torch.int16))
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)
    # the oracle on the post-append cache: the dense keys gathered back from the pool, q as the append rotated it
    kc_h, vc_h, tab, qr = kc.cpu(), vc.cpu(), s["table"], q_rot.cpu()
    want = torch.zeros_like(qr)
    r = s["cu"].tolist()
    for b, n in enumerate(new.tolist()):
        sq = STEP_NEWS[b]
        if sq == 0:
            continue
        ids = tab[b, :(n + 63) // 64].long()
        kd = kc_h[ids].transpose(0, 1).flatten(1, 2)[None, :, :n]
        vd = vc_h[ids].transpose(0, 1).flatten(1, 2)[None, :, :n]
        one = oracle_padded(qr[r[b]:r[b + 1]].transpose(0, 1)[None], kd, vd, torch.tensor([0], dtype=I32),
                            torch.tensor([n], dtype=I32), None, None, 128 ** -0.5, causal, window_left=w)
        want[r[b]:r[b + 1]] = one[0].transpose(0, 1)
    check_padded(out, want, BF16)


# graph capture: the step captured once, replayed on new lengths, table contents and cu_seqlens_q (same shapes)
@pytest.mark.gpu
def test_step_graph_capture(fam):
    from flash_attention_cute_amd import _debug

    s = step_inputs(BF16, 1980)
    kc, vc, table, sl, cu, k, v, q = dv(s["kc"], s["vc"], s["table"], s["sl"], s["cu"], s["k"], s["v"], s["q"])
    cos, sin = dv(*s["cos_sin"])
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)
    max_q = 320  # (an upper bound of both rounds' chunks)

    def step():
        return fam.flash_attn_varlen_with_kvcache(q, kc, vc, cu, max_q, k, v, rotary_cos=cos, rotary_sin=sin,
                                                  cache_seqlens=sl, block_table=table, causal=True, return_seqlens=True)

    kc_start, vc_start = kc.clone(), vc.clone()
    step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, new = step()
    # the replayed step: other chunk lengths (the same total), other cache lengths, the table re-dealt
    gen = torch.Generator().manual_seed(7)
    news2 = (300, 0, 63, 40, 1)
    lens2 = (100, 449, 0, 64, 33)
    kc.copy_(kc_start)
    vc.copy_(vc_start)
    q.copy_(torch.randn(q.shape, generator=gen).to(BF16))
    cu.copy_(cu_of(news2))
    sl.copy_(torch.tensor(lens2, dtype=I32))
    table.copy_(torch.randperm(kc.size(0), generator=gen)[:table.numel()].reshape(table.shape).to(I32))
    g.replay()
    torch.cuda.synchronize()
    got, got_new, kc_g, vc_g = out.clone(), new.clone(), kc.clone(), vc.clone()
    kc.copy_(kc_start)
    vc.copy_(vc_start)
    eager, eager_new = step()
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
    torch.cuda.synchronize()
    assert got_new.tolist() == [a + b for a, b in zip(lens2, news2)] and torch.equal(got_new, eager_new)
    assert torch.equal(kc_g.view(torch.int16), kc.view(torch.int16)) and torch.equal(vc_g.view(torch.int16), vc.view(torch.int16))
    assert torch.isfinite(got.float()).all() and torch.equal(got, eager)
