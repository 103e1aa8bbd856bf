"""The softmax log-sum-exp from the ragged paged prefill (include/fa_gfx950_paged_varlen_lse.h).

``flash_attn_paged_varlen_func(..., return_lse=True)`` and ``flash_attn_varlen_with_kvcache(..., return_lse=True)``
return ``(out, lse)``, lse fp32 [Hq, total_q] in natural-log units, ``ln(sum_n exp(s_n) + exp(sinks[h]))`` over the
row's visible keys. The reference is float64: tests/test_paged_varlen_sink.py's ``row_lse`` with the sink folded in by
``logaddexp``; the bound is tests/test_paged_lse.py's ``LSE_TOL`` (2^-12 absolute, the decode's), which this kernel's
arithmetic stays far inside (DESIGN.md section 5 has the budget). Cases are tests/test_paged_varlen.py's ``Ragged``
over ``BASE_PAIRS`` (an empty range, one row, a sequence with no key, one shorter than its Sq_b, a block that ends
inside a tile) and sinks are ``make_sinks``': head 0 30 above every logit, head 1 30 below, head 2 -inf.

Every GPU case asserts (1) ``out`` is ``torch.equal`` to the same call without ``return_lse`` -- without sinks that is
the unsinked op's launch, with sinks the sinked op's -- and (2) the LSE: ``-inf`` exactly where a row has neither a
visible key nor a sink, ``sinks[h]`` where it has the sink alone, within LSE_TOL everywhere else.
"""
from __future__ import annotations

import functools
import warnings

import pytest
import torch

from test_paged_lse import LSE_TOL, check_lse, merge_oracle
from test_paged_sink import make_sinks
from test_paged_varlen import BASE_PAIRS, ROUNDS_PAIRS, WIN_PAIRS, Ragged, cu_of, dv
from test_paged_varlen_sink import PLAIN_SCHEMA, SINK_SCHEMA, ragged_oracle, row_lse

F16, BF16 = torch.float16, torch.bfloat16
DEV = "cuda:0"
I32 = torch.int32
NEG_INF = float("-inf")

LSE_SCHEMA = ("flash_attention::paged_varlen_forward_lse(Tensor q, Tensor k_cache, Tensor v_cache, "
              "Tensor cu_seqlens_q, SymInt max_seqlen_q, Tensor block_table, Tensor cache_seqlens, Tensor? sinks=None, "
              "float softmax_scale=None, bool causal=False, SymInt window_left=-1) -> (Tensor, Tensor)")
MERGE_SCHEMA = ("flash_attention::merge_states(Tensor outs, Tensor lses, bool return_lse=False) -> (Tensor, Tensor)")
PACKED_SCHEMA = ("flash_attention::merge_states_packed(Tensor outs, Tensor lses, bool return_lse=False) -> "
                 "(Tensor, Tensor)")


def quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


def lse_ref(c, sinks, causal, w=-1):
    """float64 [Hq, total_q]: row_lse with the sink (at or below -1e30: none) folded in; -inf: neither key nor sink."""
    l = row_lse(c, causal, w).transpose(0, 1)
    if sinks is None:
        return l
    s = sinks.double().masked_fill(sinks.double() <= -1e30, NEG_INF)[:, None].expand_as(l)
    both = (l == NEG_INF) & (s == NEG_INF)
    return torch.logaddexp(l.masked_fill(both, 0), s.masked_fill(both, 0)).masked_fill(both, NEG_INF)


# ------------------------------------------------------------------------------------------- CPU
def test_schemas_fake_and_export():
    import flash_attention_cute_amd as m

    ops = torch.ops.flash_attention
    assert str(ops.paged_varlen_forward_lse.default._schema) == LSE_SCHEMA
    assert str(ops.paged_varlen_forward_sink.default._schema) == SINK_SCHEMA  # (the two ragged ops keep theirs)
    assert str(ops.paged_varlen_forward.default._schema) == PLAIN_SCHEMA
    assert str(ops.merge_states.default._schema) == MERGE_SCHEMA
    assert str(ops.merge_states_packed.default._schema) == PACKED_SCHEMA
    for name in ("flash_attention_paged_varlen_forward_lse", "flash_attention_merge_states_packed",
                 "flash_attn_paged_varlen_shared_prefix_func"):
        assert name in m.__all__ and callable(getattr(m, name))
    c = Ragged(((0, 30), (3, 49), (5, 0), (7, 5)), 4, 2, 64, 128, 16, torch.float32, 1)
    kc, vc = c.kc.nan_to_num(0.0), c.vc.nan_to_num(0.0)
    sinks = torch.tensor([0.5, -1.0, NEG_INF, 3.0])
    for args in ((c.q, kc, vc, c.cu_q, c.max_q, c.table, c.sl, sinks, 0.25, True, 3),
                 (c.q, kc, vc, c.cu_q, c.max_q, c.table, c.sl, None, 0.125, False, -1),
                 (c.q, kc, vc, c.cu_q, c.max_q, c.table, c.sl)):
        quiet(torch.library.opcheck, ops.paged_varlen_forward_lse.default, args,
              test_utils=("test_schema", "test_faketensor"))
    outs, lses = torch.randn(3, 15, 4, 16), torch.randn(3, 4, 15)
    for flag in (False, True):
        quiet(torch.library.opcheck, ops.merge_states_packed.default, (outs, lses, flag),
              test_utils=("test_schema", "test_faketensor"))
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode() as mode:
        fo, fl = ops.paged_varlen_forward_lse(*(mode.from_tensor(t) for t in (c.q, kc, vc, c.cu_q)), c.max_q,
                                              *(mode.from_tensor(t) for t in (c.table, c.sl)))
    assert fo.shape == c.q.shape and fo.dtype == c.q.dtype
    assert fl.shape == (4, 15) and fl.dtype == torch.float32 and fl.is_contiguous()

    def step(q, cu, table, sl):  # export: the op survives tracing with its two results
        return ops.paged_varlen_forward_lse(q, kc, vc, cu, 7, table, sl, sinks, 0.25, True, -1)

    ep = quiet(torch.export.export, _Wrap(step), (c.q, c.cu_q, c.table, c.sl))
    assert "paged_varlen_forward_lse" in str(ep.graph)
    for name in ("flash_attn_paged_varlen_func", "flash_attn_varlen_with_kvcache"):
        assert "return_lse" in getattr(m, name).__doc__
    assert "PACKED" in m.flash_attn_merge_states.__doc__


class _Wrap(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, *args):
        return self.fn(*args)


CPU_PAIRS = ((0, 96), (1, 33), (5, 0), (40, 37), (70, 96))


@pytest.mark.parametrize("w", [-1, 20])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sinked", [False, True], ids=["plain", "sinks"])
def test_cpu_default_matches_float64(sinked, causal, w):
    """The CPU default computes in fp32 on fp32 copies of the 16-bit inputs: 1e-5 + 1e-5 |ref| is fp32's own error
    over a 64-term dot product and a 96-term sum (eps 6e-8 each), with a wide margin (test_paged_varlen_sink's
    bound for out, applied to the LSE too)."""
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    c = Ragged(CPU_PAIRS, 4, 2, 64, 128, 64, F16, 46)
    sinks = make_sinks(c.q4, c.k, c.lens, 5) if sinked else None
    args = (c.q.float(), c.kc.float(), c.vc.float(), c.cu_q, c.max_q, c.table, c.sl)
    out, lse = quiet(flash_attn_paged_varlen_func, *args, causal=causal, window_left=w, sinks=sinks, return_lse=True)
    assert lse.shape == (4, c.q.size(0)) and lse.dtype == torch.float32 and lse.is_contiguous()
    assert torch.equal(out, quiet(flash_attn_paged_varlen_func, *args, causal=causal, window_left=w, sinks=sinks))
    ref = lse_ref(c, sinks, causal, w)
    empty = ref == NEG_INF
    assert torch.equal(lse == NEG_INF, empty)
    r = c.cu_q.tolist()
    dead = slice(r[2], r[3])  # (a sequence without keys: -inf without sinks, the sink itself with them)
    if sinked:
        assert not empty[[0, 1, 3]].any() and empty[2, dead].all()  # (only the head whose sink is -inf)
        assert torch.equal(lse[3, dead], sinks[3].expand(5)) and torch.equal(lse[0, dead], sinks[0].expand(5))
    else:
        assert empty[:, dead].all() and (not causal or empty[:, r[3]:r[3] + 3].all())
    torch.testing.assert_close(lse[~empty].double(), ref[~empty], atol=1e-5, rtol=1e-5)


def test_return_lse_false_is_the_old_call_and_the_wrappers_errors():
    from flash_attention_cute_amd import flash_attn_paged_varlen_func, flash_attn_varlen_with_kvcache
    from test_paged_varlen import packed_rows, ragged_cache

    c = Ragged(CPU_PAIRS, 4, 2, 64, 128, 64, F16, 41)
    sinks = make_sinks(c.q4, c.k, c.lens, 5)
    for kw in ({}, {"sinks": sinks}, {"causal": True, "window_left": 20}):
        a = quiet(flash_attn_paged_varlen_func, c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl, **kw)
        b = quiet(flash_attn_paged_varlen_func, c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl, return_lse=False, **kw)
        assert isinstance(b, torch.Tensor) and torch.equal(a, b)
    # the step: (out, lse), (out, lse, new_seqlens); the errors of the attention half come before the append
    hq, hkv, page, cap, d = 4, 2, 64, 128, 16
    lens, news = (0, 31, 95, 60), (5, 3, 0, 20)
    kc, vc, table, sl = ragged_cache(lens, news, hkv, page, cap, d, F16, 42)
    cu = cu_of(news)
    k, v, q = packed_rows(28, hkv, d, F16, 43), packed_rows(28, hkv, d, F16, 44), packed_rows(28, hq, d, F16, 45)
    kc2, vc2, kc3, vc3 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    a = quiet(flash_attn_varlen_with_kvcache, q, kc, vc, cu, 20, k, v, cache_seqlens=sl, block_table=table, causal=True)
    o2, l2 = quiet(flash_attn_varlen_with_kvcache, q, kc2, vc2, cu, 20, k, v, cache_seqlens=sl, block_table=table,
                   causal=True, return_lse=True)
    o3, l3, n3 = quiet(flash_attn_varlen_with_kvcache, q, kc3, vc3, cu, 20, k, v, cache_seqlens=sl, block_table=table,
                       causal=True, return_lse=True, return_seqlens=True)
    assert torch.equal(a, o2) and torch.equal(a, o3) and torch.equal(l2, l3) and l2.shape == (hq, 28)
    assert torch.equal(n3, sl + torch.tensor(news, dtype=I32)) and torch.equal(kc, kc2) and torch.equal(kc, kc3)
    for bad in (torch.zeros(3), 0.5, torch.zeros(4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sinks"):
            flash_attn_paged_varlen_func(c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl, sinks=bad, return_lse=True)
    kc32, vc32, table32, sl32 = ragged_cache(lens, news, hkv, 32, cap, d, F16, 53)
    kc1 = kc32.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="page_size"):
            flash_attn_varlen_with_kvcache(q, kc32, vc32, cu, 20, k, v, cache_seqlens=sl32, block_table=table32,
                                           return_lse=True)
        assert torch.equal(kc32.view(torch.int16), kc1.view(torch.int16))  # (refused before anything is appended)
        k8 = c.kc.nan_to_num(0.0).to(torch.float8_e4m3fn)
        with pytest.raises(NotImplementedError, match="FP8"):
            flash_attn_paged_varlen_func(c.q, k8, k8, c.cu_q, c.max_q, c.table, c.sl, return_lse=True)


def test_packed_merge_cpu():
    """The packed merge against the float64 oracle and against the 5-D merge of the same states."""
    from flash_attention_cute_amd import flash_attn_merge_states

    g = torch.Generator().manual_seed(3)
    n, t, h, d = 3, 37, 4, 16
    outs = torch.randn(n, t, h, d, generator=g).to(BF16)
    lses = 3 * torch.randn(n, h, t, generator=g)
    lses[:, 0, 0] = NEG_INF  # every part empty
    lses[0, 1, :] = NEG_INF  # one part empty
    out, lse = quiet(flash_attn_merge_states, outs, lses, True)
    assert out.shape == (t, h, d) and out.is_contiguous() and lse.shape == (h, t) and out.dtype == BF16
    ro, rl = merge_oracle(outs.transpose(1, 2), lses)  # [N, H, T, D] against [N, H, T]
    torch.testing.assert_close(out.double(), ro.transpose(0, 1), atol=2 ** -8, rtol=2 ** -8)  # (bf16's rounding)
    assert lse[0, 0] == NEG_INF and (out[0, 0] == 0).all()
    fin = rl != NEG_INF
    torch.testing.assert_close(lse[fin].double(), rl[fin], atol=1e-5, rtol=1e-5)
    o5, l5 = quiet(flash_attn_merge_states, outs.transpose(1, 2)[:, None], lses[:, None], True)  # [N, 1, H, T, D]
    assert torch.equal(o5[0].transpose(0, 1), out) and torch.equal(l5[0], lse)
    only = quiet(flash_attn_merge_states, list(outs), list(lses))  # (sequences of N tensors; no lse)
    assert torch.equal(only, out)
    with pytest.raises(ValueError, match="packed outs"):
        flash_attn_merge_states(outs, lses.transpose(1, 2))


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def fam(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    yield fam
    _debug.set_knobs()


def launch(c, causal, w=-1, sinks=None, return_lse=True):
    """One ragged paged launch on the device: (out, lse) on the host, or out alone."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_varlen_func

    kw = {} if sinks is None else {"sinks": sinks.to(DEV)}
    res = flash_attn_paged_varlen_func(*dv(c.q, c.kc, c.vc, c.cu_q), c.max_q, *dv(c.table, c.sl), causal=causal,
                                       window_left=w, return_lse=return_lse, **kw)
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
    torch.cuda.synchronize()
    return (res[0].cpu(), res[1].cpu()) if return_lse else res.cpu()


def check_both(c, sinks, causal, w, what, min_keyless):
    """The two checks of the module docstring, without sinks and with them; returns the two LSE errors."""
    errs = []
    for s in (None, sinks):
        out, lse = launch(c, causal, w, s)
        assert lse.shape == (c.q.size(1), c.q.size(0)) and lse.dtype == torch.float32 and lse.is_contiguous()
        assert torch.equal(out, launch(c, causal, w, s, return_lse=False))  # 1.
        ref = lse_ref(c, s, causal, w)
        errs.append(check_lse(lse, ref, f"{what} {'sinks' if s is not None else 'plain'}"))  # 2.
        keyless = row_lse(c, causal, w).transpose(0, 1) == NEG_INF
        assert int(keyless[0].sum()) >= min_keyless  # (the case does have rows without a visible key)
        if s is None:
            assert (lse[keyless] == NEG_INF).all()
        else:  # the sink alone: its own value, exactly; -inf on the head without one
            assert (lse[2][keyless[2]] == NEG_INF).all()
            for h in (0, 1, 3):
                assert (lse[h][keyless[h]] == s[h]).all()
    return errs


@functools.lru_cache(maxsize=None)
def base_case(d, dtype, page):
    hq, hkv = 8, 2
    c = Ragged(BASE_PAIRS, hq, hkv, page, 512, d, dtype, 2200 + d + page + (dtype == BF16))
    return c, make_sinks(c.q4, c.k, c.lens, 27)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_grid(fam, d, dtype, page, causal):
    c, sinks = base_case(d, dtype, page)
    check_both(c, sinks, causal, -1, f"d{d} {dtype} p{page} causal={causal}", 43 if causal else 40)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("w", [0, 63, 100])
def test_window(fam, w, causal):
    c = Ragged(WIN_PAIRS, 8, 2, 64, 768, 128, F16, 2300 + w)
    check_both(c, make_sinks(c.q4, c.k, c.lens, 27), causal, w, f"w{w} causal={causal}", 3 if causal else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", [-1, 0x7B7B7B7B], ids=["nan", "finite"])
def test_what_the_launch_writes(fam, pattern):
    """lse as an as_strided view [Hq, total_q] with a row stride of 2 and a padded head pitch inside a poisoned buffer
    with guard bands on both sides: after the launch only the elements of owned rows differ from the poison, and
    they hold the LSE. cu_seqlens_q leaves 5 rows before the first sequence unowned, and its last entry lies far
    past total_q, so the last sequence is clamped to the 7 rows that remain (its queries are its first 7). The odd
    elements between the rows and the pitch gap between the heads are the unowned elements in the middle. Two
    poison patterns: an owned element that was never written would show one of them."""
    hq, hkv, d = 8, 2, 64
    c = Ragged(((40, 37), (257, 300), (0, 100), (1, 449), (30, 200)), hq, hkv, 64, 512, d, BF16, 2400)
    sinks = make_sinks(c.q4, c.k, c.lens, 7)
    lead, kept = 5, 7  # (of the last sequence's 30 rows)
    n_own = c.q.size(0) - 30 + kept
    total = lead + n_own
    q = torch.cat([torch.full((lead, hq, d), float("nan"), dtype=BF16), c.q[:n_own]])
    cu = c.cu_q + lead
    cu[-1] = 2 ** 31 - 1
    guard, pitch = 4096, 2 * total + 24
    buf = torch.full((2 * guard + hq * pitch,), pattern, dtype=I32, device=DEV)
    view = buf.view(torch.float32).as_strided((hq, total), (pitch, 2), guard)
    before = buf.clone()
    o, l = fam._paged_varlen_lse_cuda(*dv(q, c.kc, c.vc, cu), c.max_q, *dv(c.table, c.sl), sinks.to(DEV), d ** -0.5, True,
                                      100, None, view)
    torch.cuda.synchronize()
    assert l.data_ptr() == view.data_ptr()
    owned = torch.zeros_like(buf, dtype=torch.bool)
    owned.as_strided((hq, n_own), (pitch, 2), guard + 2 * lead).fill_(True)
    assert torch.equal(buf[~owned], before[~owned])  # nothing else of the array is touched
    # the owned rows hold the LSE: the case with its last sequence cut to its first 7 queries over the same 200 keys
    # (bottom-right alignment: a sequence of 7 rows, not the first 7 of 30)
    cut = Ragged(((40, 37), (257, 300), (0, 100), (1, 449), (kept, 200)), hq, hkv, 64, 512, d, BF16, 2400)
    cut.q4[4, :, :kept] = c.q4[4, :, :kept]
    cut.q = c.q[:n_own].clone()
    ref = lse_ref(cut, sinks, True, 100)
    check_lse(view[:, lead:].cpu(), ref, f"footprint {pattern:#x}")
    ro = ragged_oracle(cut, sinks, True, 100)
    from test_padded import check_padded

    check_padded(o[lead:].cpu(), ro, BF16)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_many_rounds_per_workgroup_and_determinism(fam, causal):
    """24 blocks on 8 workgroups: a workgroup runs several blocks in a row, so every block's O and LSE stores are
    in flight under the next block's loads -- the case a wrong store count in the prologue's counted wait would
    break. Two runs give the same bits, equal to the full grid's, and both match the oracle."""
    from flash_attention_cute_amd import _debug

    c = Ragged(ROUNDS_PAIRS, 2, 2, 64, 768, 128, BF16, 2500)
    sinks = torch.tensor([0.5, NEG_INF])
    for s in (None, sinks):
        full_o, full_l = launch(c, causal, -1, s)
        with _debug.knobs(w4_grid=8):
            o1, l1 = launch(c, causal, -1, s)
            o2, l2 = launch(c, causal, -1, s)
        assert torch.equal(o1, o2) and torch.equal(l1.view(I32), l2.view(I32))
        assert torch.equal(o1, full_o) and torch.equal(l1.view(I32), full_l.view(I32))
        check_lse(l1, lse_ref(c, s, causal), f"rounds causal={causal}")
        from test_padded import check_padded

        check_padded(o1, ragged_oracle(c, s if s is not None else torch.full((2,), NEG_INF), causal), BF16)


@pytest.mark.gpu
def test_packed_merge_of_two_key_sets_is_the_one_launch_call(fam):
    """What the LSE is for: a chunk computed against two halves of its keys (two tables) and merged equals, within
    rounding, the chunk over all its keys; the sink sits in exactly one state."""
    from flash_attention_cute_amd import flash_attn_merge_states, flash_attn_paged_varlen_func
    from test_padded import check_padded

    hq, hkv, d, page = 8, 2, 128, 64
    c = Ragged(((40, 512), (257, 512), (1, 512)), hq, hkv, page, 512, d, BF16, 2600)
    sinks = make_sinks(c.q4, c.k, c.lens, 27)
    q, kc, vc, cu, table, sinks_d = dv(c.q, c.kc, c.vc, c.cu_q, c.table, sinks)
    half = torch.full((3,), 256, dtype=I32, device=DEV)
    o0, l0 = flash_attn_paged_varlen_func(q, kc, vc, cu, c.max_q, table[:, :4].contiguous(), half, return_lse=True)
    o1, l1 = flash_attn_paged_varlen_func(q, kc, vc, cu, c.max_q, table[:, 4:].contiguous(), half, return_lse=True,
                                          sinks=sinks_d)
    out, lse = flash_attn_merge_states([o0, o1], [l0, l1], return_lse=True)
    torch.cuda.synchronize()
    assert out.shape == c.q.shape and out.is_contiguous() and lse.shape == (hq, c.q.size(0))
    check_padded(out.cpu(), ragged_oracle(c, sinks, False), BF16)
    check_lse(lse, lse_ref(c, sinks, False), "merged")
    ro, rl = merge_oracle(torch.stack([o0, o1]).cpu().transpose(1, 2), torch.stack([l0, l1]).cpu())
    torch.testing.assert_close(out.cpu().double(), ro.transpose(0, 1), atol=2 ** -8, rtol=2 ** -8)
