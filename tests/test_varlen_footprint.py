"""What the ragged paged attention and the ragged append write (tests/footprint.py, as tests/test_footprint.py).

Every device buffer of a launch is carved from one arena under the three byte patterns: the attention writes only
the rows of ``out`` that some sequence covers, the append only the target cache rows, ``new_seqlens`` and the
covered rows of ``q_rotated``, and the results are bit-identical under all three patterns. A ``cu_seqlens_q``
whose entries lie outside ``[0, total_q]`` is clamped: run inside the arena, with slack regions around q / out
that are larger than anything the bad entries could reach, a stray access would be a data mismatch, never a fault.
"""
from __future__ import annotations

import ctypes

import pytest
import torch

from footprint import PATTERNS  # noqa: F401  (Launch.run goes through all three)
from test_footprint import BF16, F16, I32, LARGE, Launch, abi, code, log2e_scale, seeded  # noqa: F401  (abi: a fixture)
from test_kvcache import PATTERN, rope_tables
from test_kvcache_varlen_abi import FaKvcacheVarlenParams
from test_paged_abi import FaPagedParams
from test_paged_varlen import Ragged, cu_of, packed_rows, per_sequence_append, ragged_cache
from test_paged_varlen_abi import FaPagedVarlenParams

gpu = pytest.mark.gpu
RHC = ("row", "head", "col")
_P, _I, _C = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def bind(abi):
    lib = abi.lib
    lib.fa_fwd_gfx950_paged_varlen.argtypes = [_P, _C, _C, _I, _P, _I, _P]
    lib.fa_fwd_gfx950_paged_varlen.restype = _C
    lib.fa_fwd_gfx950_paged_varlen_workspace_size.argtypes = [_P, _C, _C, _I]
    lib.fa_fwd_gfx950_paged_varlen_workspace_size.restype = _I
    lib.fa_kvcache_append_varlen_gfx950.argtypes = [_P, _C, _P]
    lib.fa_kvcache_append_varlen_gfx950.restype = _C
    return lib


def attention_launch(abi, c, cu, lead, tail, max_q, window_left, slack=0, covered=None):
    """The buffers of one fa_fwd_gfx950_paged_varlen launch in the arena. q / o have ``lead`` rows before and
    ``tail`` rows after the rows of c.q that no sequence owns; ``slack`` > 0 carves that many undeclared bytes
    before and after q and o; ``covered``: the rows of o a launch may write (default: c.q's). Returns (launch,
    params, o, total rows)."""
    from test_abi import FaFwdParams

    L = Launch(abi, LARGE)
    hq, d = c.q.size(1), c.q.size(2)
    g = torch.Generator().manual_seed(99)
    q_all = torch.cat([torch.randn(lead, hq, d, generator=g).to(c.dtype), c.q, torch.randn(tail, hq, d, generator=g).to(c.dtype)])
    total = q_all.size(0)
    if slack:
        L.arena.carve(slack, "slack before q")
    qd = L.inp("q", q_all, dims=RHC)
    if slack:
        L.arena.carve(slack, "slack after q")
    kcd, vcd = L.inp("k_cache", c.kc), L.inp("v_cache", c.vc)
    td, sld = L.inp("block_table", c.table, dims=("batch", "entry")), L.inp("cache_seqlens", c.sl, dims=("batch",))
    cud = L.inp("cu_seqlens_q", cu, dims=("entry",))
    if slack:
        L.arena.carve(slack, "slack before o")
    lo, hi = (lead, lead + c.q.size(0)) if covered is None else covered
    o = L.out("o", c.dtype, q_all.shape, dims=RHC, written=lambda t: [t[lo:hi]])
    if slack:
        L.arena.carve(slack, "slack after o")
    base = FaFwdParams()
    base.q_ptr, base.k_ptr, base.v_ptr, base.o_ptr = qd.data_ptr(), kcd.data_ptr(), vcd.data_ptr(), o.data_ptr()
    base.batch_size, base.num_heads_q, base.num_heads_kv = cu.numel() - 1, hq, c.kc.size(1)
    base.seqlen_q, base.seqlen_kv, base.headdim = max_q, c.table.size(1) * c.kc.size(2), d
    base.head_q_per_group = hq // c.kc.size(1)
    base.q_head_stride, base.o_head_stride = qd.stride(1), o.stride(1)
    base.q_seqlen_stride, base.o_seqlen_stride = qd.stride(0), o.stride(0)
    base.k_batch_stride, base.v_batch_stride = kcd.stride(0), vcd.stride(0)
    base.k_head_stride, base.v_head_stride = kcd.stride(1), vcd.stride(1)
    base.k_seqlen_stride, base.v_seqlen_stride = kcd.stride(2), vcd.stride(2)
    base.softmax_scale = log2e_scale(d ** -0.5)
    paged = FaPagedParams(base, td.data_ptr(), td.stride(0), c.table.size(1), c.kc.size(0), c.kc.size(2), sld.data_ptr())
    return L, FaPagedVarlenParams(paged, cud.data_ptr(), total), o, total


PAIRS = ((0, 100), (1, 65), (40, 37), (257, 301), (20, 512))


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("window_left", [-1, 100])
def test_attention_writes_only_the_covered_rows(abi, window_left, dtype):
    """Three rows before cu[0] and five after cu[B] belong to no sequence: they keep the pattern. Workspace size 0
    and NULL; d = 72 (a D tile that is not filled)."""
    from test_padded import check_padded

    lib = bind(abi)
    c = Ragged(PAIRS, 4, 2, 64, 512, 72, dtype, seeded("vf", window_left, str(dtype)))
    lead, tail = 3, 5
    L, p, o, total = attention_launch(abi, c, c.cu_q + lead, lead, tail, c.max_q, window_left)
    dt = code(dtype)
    assert lib.fa_fwd_gfx950_paged_varlen_workspace_size(ctypes.byref(p), dt, 1, window_left) == 0
    call = lambda: lib.fa_fwd_gfx950_paged_varlen(ctypes.byref(p), dt, 1, window_left, None, 0, abi.stream())  # noqa: E731

    def expect():
        assert abi.dbg.last_path() == "w4" and abi.dbg.last_prefill_paged()

    (got,) = L.run(call, expect)
    check_padded(got, c.oracle(True, window_left), dtype)
    dev = lambda *ts: tuple(t.to(abi.device) for t in ts)  # noqa: E731  (the pin: the Python op on the same tensors)
    ref = abi.m.flash_attn_paged_varlen_func(*dev(c.q, c.kc, c.vc, c.cu_q), c.max_q, *dev(c.table, c.sl), causal=True,
                                             window_left=window_left)
    assert torch.equal(got, ref.cpu())


@gpu
@pytest.mark.parametrize("bad", ["past_total", "negative", "descending"])
def test_a_bad_cu_seqlens_q_is_clamped_inside_the_arena(abi, bad):
    """Entries outside [0, total_q] are clamped (a start into [0, total_q], an end into [start, total_q]): the
    launch equals the one with the clamped array, and nothing outside ``o`` is written. Unclamped, the worst entry
    would reach 2000 rows (1.2 MB) past or before q / o: the slack regions around them are 2 MiB each, inside the
    arena, and any byte written there is reported."""
    lib = bind(abi)
    dtype = BF16
    c = Ragged(((40, 37), (257, 301), (20, 512)), 4, 2, 64, 512, 72, dtype, seeded("vc", bad))
    total = c.q.size(0)
    cu = c.cu_q.clone()  # [0, 40, 297, 317]
    if bad == "past_total":
        cu[2], cu[3] = total + 700, total + 2000    # clamped: [0, 40, 317, 317]
    elif bad == "negative":
        cu[0], cu[1] = -2000, -5                     # clamped: [0, 0, 297, 317]
    else:
        cu[0], cu[1] = 300, 100                      # clamped: [300, 300), [100, 297), [297, 317): an end below its start
    clamped = []
    for b in range(3):
        q0 = min(max(int(cu[b]), 0), total)
        clamped.append((q0, min(max(int(cu[b + 1]), q0), total)))
    lo = min(q0 for q0, q1 in clamped if q1 > q0)  # (the ranges chosen here do not overlap and leave no hole above lo)
    assert total * 4 * 72 * 2 < (2 << 20) and 2000 * 4 * 72 * 2 < (2 << 20)
    L, p, o, _ = attention_launch(abi, c, cu, 0, 0, 320, -1, slack=2 << 20, covered=(lo, total))
    call = lambda: lib.fa_fwd_gfx950_paged_varlen(ctypes.byref(p), code(dtype), 1, -1, None, 0, abi.stream())  # noqa: E731
    (got,) = L.run(call)
    dev = lambda *ts: tuple(t.to(abi.device) for t in ts)  # noqa: E731
    kc, vc, table, sl = dev(c.kc, c.vc, c.table, c.sl)
    checked = 0
    for b, (q0, q1) in enumerate(clamped):  # every sequence's clamped range, alone (B = 1) through the Python op
        if q1 == q0:
            continue
        one = abi.m.flash_attn_paged_varlen_func(c.q[q0:q1].to(abi.device), kc, vc, cu_of([q1 - q0]).to(abi.device),
                                                 q1 - q0, table[b:b + 1], sl[b:b + 1], causal=True)
        assert torch.equal(got[q0 - lo:q1 - lo], one.cpu()), (bad, b)
        checked += q1 - q0
    assert checked == total - lo


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
def test_append_writes_only_its_targets(abi, rope, dtype):
    """The pools, new_seqlens and q_rotated in the arena: only the target rows of the pools (with a dropped page id
    and an overflow among them), new_seqlens and the covered rows of q_rotated are written."""
    lib = bind(abi)
    hq, hkv, page, cap, d = 4, 2, 64, 256, 64
    lens, news, sqs = (250, 60, 0, 100, 63), (40, 70, 130, 0, 1), (3, 70, 131, 0, 1)
    kc, vc, table, sl = ragged_cache(lens, news, hkv, page, cap, d, dtype, seeded("va", rope, str(dtype)))
    table[1, 1] = -1
    num_pages = kc.size(0)
    cu_new, cu_q = cu_of(news), cu_of(sqs) + 2  # (two rows of q before cu_q[0], four after cu_q[B]: no sequence's)
    k, v = packed_rows(sum(news), hkv, d, dtype, 41), packed_rows(sum(news), hkv, d, dtype, 42)
    q = packed_rows(sum(sqs) + 6, hq, d, dtype, 43)
    cos, sin = rope_tables(cap, d, dtype)
    # the target rows, by the header's rule on the host
    tgt = torch.zeros(num_pages, hkv, page, dtype=torch.bool)
    for b, (n0, m) in enumerate(zip(lens, news)):
        for i in range(m):
            n = n0 + i
            pg = int(table[b, n // page]) if n < cap else -1
            if 0 <= pg < num_pages:
                tgt[pg, :, n % page] = True

    L = Launch(abi, LARGE)
    kd, vd = L.inp("k", k, dims=RHC), L.inp("v", v, dims=RHC)
    cnd, td, sld = L.inp("cu_seqlens_new", cu_new), L.inp("block_table", table), L.inp("cache_seqlens", sl)
    # the pools are inputs AND outputs: their target rows join the write set, every other row must keep its value
    kcd = L.arena.tensor("k_cache", dtype, kc.shape, dims=("page", "head", "row", "col"))
    vcd = L.arena.tensor("v_cache", dtype, vc.shape, dims=("page", "head", "row", "col"))
    for t, value in ((kcd, kc), (vcd, vc)):
        L.arena.declare_input(t)
        L.inputs.append((t, value))
    new_d = L.out("new_seqlens", I32, (len(lens),), dims=("batch",))
    p = FaKvcacheVarlenParams()
    p.k_new, p.v_new = kd.data_ptr(), vd.data_ptr()
    p.kn_row_stride, p.kn_head_stride, p.vn_row_stride, p.vn_head_stride = kd.stride(0), kd.stride(1), vd.stride(0), vd.stride(1)
    p.cu_seqlens_new, p.total_new = cnd.data_ptr(), k.size(0)
    if rope:
        qd, cqd = L.inp("q", q, dims=RHC), L.inp("cu_seqlens_q", cu_q)
        cd, sd = L.inp("cos", cos), L.inp("sin", sin)
        qo = L.out("q_rotated", dtype, q.shape, dims=RHC, written=lambda t: [t[2:2 + sum(sqs)]])
        p.q, p.q_out, p.cu_seqlens_q, p.total_q = qd.data_ptr(), qo.data_ptr(), cqd.data_ptr(), q.size(0)
        p.q_row_stride, p.q_head_stride, p.qo_row_stride, p.qo_head_stride = qd.stride(0), qd.stride(1), qo.stride(0), qo.stride(1)
        p.cos, p.sin, p.cs_row_stride, p.max_pos = cd.data_ptr(), sd.data_ptr(), cd.stride(0), cap
        p.num_heads_q = hq
    p.k_cache, p.v_cache = kcd.data_ptr(), vcd.data_ptr()
    p.k_page_stride, p.k_head_stride, p.k_row_stride = kcd.stride(0), kcd.stride(1), kcd.stride(2)
    p.v_page_stride, p.v_head_stride, p.v_row_stride = vcd.stride(0), vcd.stride(1), vcd.stride(2)
    p.block_table, p.block_table_stride, p.max_pages, p.num_pages, p.page_size = td.data_ptr(), td.stride(0), table.size(1), num_pages, page
    p.seqlens_k, p.seqlens_out = sld.data_ptr(), new_d.data_ptr()
    p.batch_size, p.num_heads_kv, p.headdim = len(lens), hkv, d

    # under every pattern: the launch, then the pools against the per-sequence appends, the untouched rows against
    # the inputs, and the arena's own check of everything that is not a pool (Launch.run)
    dev = lambda *ts: tuple(t.to(abi.device) if t is not None else None for t in ts)  # noqa: E731
    ref = per_sequence_append(*dev(kc, vc, k, v, cu_new, sl, table, cos if rope else None, sin if rope else None,
                                   q[2:2 + sum(sqs)].contiguous() if rope else None, cu_of(sqs) if rope else None))
    pools = []

    def call():
        rc = lib.fa_kvcache_append_varlen_gfx950(ctypes.byref(p), code(dtype), abi.stream())
        pools.append((kcd.clone(), vcd.clone()))
        # (the pools' written rows are put back so that Launch.run's input check sees only the rows the launch
        # must not touch; the clones above keep what was written)
        kcd.copy_(torch.where(tgt.to(abi.device)[..., None], kc.to(abi.device), kcd))
        vcd.copy_(torch.where(tgt.to(abi.device)[..., None], vc.to(abi.device), vcd))
        return rc

    outs = L.run(call)
    assert outs[0].tolist() == [256, 130, 130, 100, 64] and torch.equal(outs[0], ref[2].cpu())
    for kg, vg in pools:  # bit-identical under the three patterns, and the per-sequence appends' bits
        assert torch.equal(kg.view(torch.int16), ref[0].view(torch.int16))
        assert torch.equal(vg.view(torch.int16), ref[1].view(torch.int16))
    assert (pools[0][0].cpu() == PATTERN).all(dim=-1).any()
    if rope:
        assert torch.equal(outs[1].view(torch.int16), ref[3].cpu().view(torch.int16))
