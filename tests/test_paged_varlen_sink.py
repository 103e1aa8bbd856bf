"""Attention sinks in the ragged paged prefill (include/fa_gfx950_paged_varlen_sink.h).

``flash_attn_paged_varlen_func(..., sinks=S)`` and ``flash_attn_varlen_with_kvcache(..., sinks=S)``: S is one fp32
logit per q-head that joins every row's softmax denominator and contributes no value (the formula and the units are
tests/test_paged_sink.py's, whose float64 ``sink_oracle`` is the reference here, per sequence). Cases are
tests/test_paged_varlen.py's ``Ragged`` (NaN-poisoned pool, shuffled table) and sinks are ``make_sinks``': 2 randn(Hq)
with head 0 set 30 above the largest logit, head 1 30 below the smallest and head 2 -inf.

Every GPU case asserts, in this order: (1) head 2's rows are ``torch.equal`` to the same launch without sinks, and so
are head 1's -- OBSERVED on the MI355X and expected from the arithmetic: the row's sum L is relative to a reference
at most the row's max, so L >= 1, and a sink 30 below every logit adds at most 2^-43 to it, less than half an ulp
of 1; (2) agreement with the oracle within tests/test_gpu_parity.py TOL; (3) a finite output, rows without a visible
key exactly 0, also under head 0's large sink; (4) the path labels.

The condition on the inputs: the sink's share of a row's weight, sigmoid(S[h] - lse_row) from the float64 scores,
has a median between 1 % and 90 % over the randomly drawn heads' rows. 2 randn draws most heads a sink that holds
far less than 1 % of a row of several hundred keys (lse ~ ln n + 0.5), so the sink seeds below are CHOSEN, by a
search on the CPU from seed 0 upward for the first one that meets the condition in all four (causal, window)
cases of a geometry (38, 27 and 4); the condition itself is asserted in every case.
"""
from __future__ import annotations

import ctypes
import functools
import warnings

import pytest
import torch

from test_padded import check_padded
from test_paged import make_paged
from test_paged_sink import make_sinks, scores, sink_oracle
from test_paged_varlen import BASE_PAIRS, Ragged, cu_of, dv, packed_rows, ragged_cache, step_inputs, STEP_NEWS

F16, BF16 = torch.float16, torch.bfloat16
DEV = "cuda:0"
I32 = torch.int32
NEG_INF = float("-inf")

SINK_SCHEMA = ("flash_attention::paged_varlen_forward_sink(Tensor q, Tensor k_cache, Tensor v_cache, "
               "Tensor cu_seqlens_q, SymInt max_seqlen_q, Tensor block_table, Tensor cache_seqlens, Tensor sinks, "
               "float softmax_scale=None, bool causal=False, SymInt window_left=-1) -> Tensor")
PLAIN_SCHEMA = ("flash_attention::paged_varlen_forward(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, "
                "SymInt max_seqlen_q, Tensor block_table, Tensor cache_seqlens, float softmax_scale=None, "
                "bool causal=False, SymInt window_left=-1) -> Tensor")


def quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


def ragged_oracle(c, sinks, causal, w=-1, scale=None):
    """test_paged_sink.sink_oracle per sequence, packed [total_q, Hq, D] (fp32)."""
    out = torch.zeros(c.q.shape, dtype=torch.float32)
    for b, (s, n) in enumerate(zip(c.sqs, c.lens)):
        if s == 0:
            continue
        r0 = int(c.cu_q[b])
        one = sink_oracle(c.q4[b:b + 1, :, :s], c.k[b:b + 1], c.v[b:b + 1], [n], sinks, causal, w, scale)
        out[r0:r0 + s] = one[0].transpose(0, 1)
    return out


def visible(s, n, causal, w):
    m, j = torch.arange(s)[:, None], torch.arange(n)[None, :]
    vis = torch.ones(s, n, dtype=torch.bool)
    if w >= 0:
        vis &= j >= m + n - s - w
    if causal:
        vis &= j <= m + n - s
    return vis


def row_lse(c, causal, w=-1):
    """float64 log-sum-exp of every packed row's visible scaled scores, [total_q, Hq]; -inf: no visible key."""
    out = torch.full((c.q.size(0), c.q.size(1)), NEG_INF, dtype=torch.float64)
    for b, (s, n) in enumerate(zip(c.sqs, c.lens)):
        if s == 0 or n == 0:
            continue
        r0 = int(c.cu_q[b])
        sc = scores(c.q4[b:b + 1, :, :s], c.k[b:b + 1], [n])[0].masked_fill(~visible(s, n, causal, w)[None], NEG_INF)
        out[r0:r0 + s] = torch.logsumexp(sc, dim=-1).transpose(0, 1)
    return out


def median_share(c, sinks, causal, w=-1):
    """The median, over the rows with a visible key of the randomly drawn heads (3 ..), of the sink's share of the
    row's softmax weight: exp(S) / (exp(S) + sum_n exp(s_n)) = sigmoid(S - lse)."""
    lse = row_lse(c, causal, w)[:, 3:]
    share = torch.sigmoid(sinks.double()[None, 3:] - lse)
    return share[torch.isfinite(lse)].median().item()


def outside_tol(got, ref, dtype):
    """Whether ``got`` misses test_padded.check_padded's elementwise bound against ``ref`` somewhere."""
    from tests.test_gpu_parity import TOL

    atol, rtol, _ = TOL[dtype]
    return bool(((got - ref).abs() > atol + rtol * ref.abs()).any())


# ------------------------------------------------------------------------------------------- CPU
def test_schemas_fake_and_export():
    import flash_attention_cute_amd as m

    ops = torch.ops.flash_attention
    assert str(ops.paged_varlen_forward_sink.default._schema) == SINK_SCHEMA
    assert str(ops.paged_varlen_forward.default._schema) == PLAIN_SCHEMA
    assert "flash_attention_paged_varlen_forward_sink" in m.__all__
    assert callable(m.flash_attention_paged_varlen_forward_sink)
    c = Ragged(((0, 30), (3, 49), (5, 0), (7, 5)), 4, 2, 64, 128, 16, torch.float32, 1)
    kc, vc = c.kc.nan_to_num(0.0), c.vc.nan_to_num(0.0)
    sinks = torch.tensor([0.5, -1.0, NEG_INF, 3.0])
    for args in ((c.q, kc, vc, c.cu_q, c.max_q, c.table, c.sl, sinks, 0.25, True, 3),
                 (c.q, kc, vc, c.cu_q, c.max_q, c.table, c.sl, sinks)):
        quiet(torch.library.opcheck, ops.paged_varlen_forward_sink.default, args,
              test_utils=("test_schema", "test_faketensor"))
    from torch._subclasses.fake_tensor import FakeTensorMode

    strided = c.q.transpose(0, 1).contiguous().transpose(0, 1)  # (a strided q: empty_like keeps its layout)
    want = torch.empty_like(strided)
    assert not strided.is_contiguous()
    with FakeTensorMode() as mode:
        fake = ops.paged_varlen_forward_sink(*(mode.from_tensor(t) for t in (strided, kc, vc, c.cu_q)), c.max_q,
                                             *(mode.from_tensor(t) for t in (c.table, c.sl, sinks)))
    assert fake.shape == want.shape and fake.stride() == want.stride() and fake.dtype == want.dtype
    for name in ("flash_attn_paged_varlen_func", "flash_attn_varlen_with_kvcache"):
        assert "sinks" in getattr(m, name).__doc__
    assert "cu_seqlens_q" in m.flash_attn_paged_varlen_func.__doc__.split("sinks", 1)[1]  # (the uniform chunk's way)


CPU_PAIRS = ((0, 96), (1, 33), (5, 0), (40, 37), (70, 96))


def test_sinks_none_is_the_call_without_the_argument():
    from flash_attention_cute_amd import flash_attn_paged_varlen_func, flash_attn_varlen_with_kvcache

    c = Ragged(CPU_PAIRS, 4, 2, 64, 128, 64, F16, 41)
    for causal, w in ((False, -1), (True, 20)):
        a = quiet(flash_attn_paged_varlen_func, c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl, causal=causal, window_left=w)
        b = quiet(flash_attn_paged_varlen_func, c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl, causal=causal, window_left=w,
                  sinks=None)
        assert torch.equal(a, b)
    hq, hkv, page, cap, d = 4, 2, 64, 128, 16
    lens, news = (0, 31, 95, 60), (5, 3, 0, 20)
    kc, vc, table, sl = ragged_cache(lens, news, hkv, page, cap, d, F16, 42)
    cu = cu_of(news)
    k, v, q = packed_rows(28, hkv, d, F16, 43), packed_rows(28, hkv, d, F16, 44), packed_rows(28, hq, d, F16, 45)
    kc2, vc2 = kc.clone(), vc.clone()
    a = quiet(flash_attn_varlen_with_kvcache, q, kc, vc, cu, 20, k, v, cache_seqlens=sl, block_table=table, causal=True)
    b = quiet(flash_attn_varlen_with_kvcache, q, kc2, vc2, cu, 20, k, v, cache_seqlens=sl, block_table=table, causal=True,
              sinks=None)
    assert torch.equal(a, b) and torch.equal(kc, kc2) and torch.equal(vc, vc2)


@pytest.mark.parametrize("w", [-1, 20])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_cpu_default_matches_float64(causal, w):
    """The CPU default computes in fp32 on fp32 copies of the 16-bit inputs: 1e-5 + 1e-5 |ref| is fp32's own error
    over a 64-term dot product and a 96-term sum (eps 6e-8 each), with a wide margin (test_paged_sink's bound)."""
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    c = Ragged(CPU_PAIRS, 4, 2, 64, 128, 64, F16, 46)
    sinks = make_sinks(c.q4, c.k, c.lens, 5)
    out = quiet(flash_attn_paged_varlen_func, c.q.float(), c.kc.float(), c.vc.float(), c.cu_q, c.max_q, c.table, c.sl,
                causal=causal, window_left=w, sinks=sinks)
    ref = ragged_oracle(c, sinks, causal, w)
    r = c.cu_q.tolist()
    assert torch.isfinite(out).all() and (out[r[2]:r[3]] == 0).all()  # (a sequence without keys)
    if causal:
        assert (out[r[3]:r[3] + 3] == 0).all()  # 37 keys under 40 queries
    torch.testing.assert_close(out, ref, atol=1e-5, rtol=1e-5)
    assert ref[:, 0].abs().max() < 1e-9 and ref[:, 3].abs().max() > 1e-2  # (the sink of head 0 dominates)
    share = median_share(c, sinks, causal, w)
    assert 0.01 <= share <= 0.9, share


def test_wrapper_errors():
    from flash_attention_cute_amd import flash_attn_paged_varlen_func, flash_attn_varlen_with_kvcache

    c = Ragged(((4, 64), (7, 100)), 4, 2, 64, 128, 32, torch.float32, 47)
    bads = (torch.zeros(3), torch.zeros(4, 1), 0.5, torch.zeros(4, dtype=torch.float64))
    for bad in bads:
        with pytest.raises(ValueError, match="sinks"):
            flash_attn_paged_varlen_func(c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl, sinks=bad)
    # the step: the error comes before the cache is written
    hq, hkv, page, cap, d = 4, 2, 64, 128, 16
    kc, vc, table, sl = ragged_cache((0, 31, 95, 60), (5, 3, 0, 20), hkv, page, cap, d, F16, 48)
    cu = cu_of((5, 3, 0, 20))
    k, v, q = packed_rows(28, hkv, d, F16, 49), packed_rows(28, hkv, d, F16, 50), packed_rows(28, hq, d, F16, 51)
    kc0, vc0 = kc.clone(), vc.clone()
    for bad in bads:
        with pytest.raises(ValueError, match="sinks"):
            flash_attn_varlen_with_kvcache(q, kc, vc, cu, 20, k, v, cache_seqlens=sl, block_table=table, sinks=bad)
        assert torch.equal(kc.view(torch.int16), kc0.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc0.view(torch.int16))
    ok = torch.zeros(4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        k8 = c.kc.nan_to_num(0.0).to(torch.float8_e4m3fn)
        with pytest.raises(NotImplementedError, match="FP8.*flash_attn_paged_func"):
            flash_attn_paged_varlen_func(c.q, k8, k8, c.cu_q, c.max_q, c.table, c.sl, sinks=ok)
        c32 = Ragged(((4, 64), (7, 96)), 4, 2, 32, 96, 32, torch.float32, 52)
        with pytest.raises(NotImplementedError, match="page_size.*flash_attn_paged_func"):
            flash_attn_paged_varlen_func(c32.q, c32.kc, c32.vc, c32.cu_q, c32.max_q, c32.table, c32.sl, sinks=ok)
        kc32, vc32, table32, sl32 = ragged_cache((0, 31, 95, 60), (5, 3, 0, 20), hkv, 32, cap, d, F16, 53)
        kc1 = kc32.clone()
        with pytest.raises(NotImplementedError, match="page_size"):
            flash_attn_varlen_with_kvcache(q, kc32, vc32, cu, 20, k, v, cache_seqlens=sl32, block_table=table32, sinks=ok)
        assert torch.equal(kc32.view(torch.int16), kc1.view(torch.int16))


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def fam(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    yield fam
    _debug.set_knobs()


def launch(c, causal, w=-1, sinks=None, scale=None):
    """One ragged paged launch on the device: (output on the host, last_path, last_prefill_paged)."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_varlen_func

    kw = {} if sinks is None else {"sinks": sinks.to(DEV)}
    out = flash_attn_paged_varlen_func(*dv(c.q, c.kc, c.vc, c.cu_q), c.max_q, *dv(c.table, c.sl), softmax_scale=scale,
                                       causal=causal, window_left=w, **kw)
    labels = _debug.last_path(), _debug.last_prefill_paged()
    torch.cuda.synchronize()
    return (out.cpu(), *labels)


def no_key_rows(c, causal, w):
    return ~torch.isfinite(row_lse(c, causal, w)[:, 0])


# geometry -> (Hq, Hkv, D, page, dtype, case seed, SINK SEED: the module docstring's search)
GEOS = {
    "gptoss-g8-d64-p64-f16": (16, 2, 64, 64, F16, 2101, 38),
    "gptoss-g8-d64-p64-bf16": (16, 2, 64, 64, BF16, 2102, 38),
    "llama-g4-d128-p64-bf16": (8, 2, 128, 64, BF16, 2103, 27),
    "llama-g4-d128-p128-f16": (8, 2, 128, 128, F16, 2104, 27),
    "llama-g4-d128-p256-bf16": (8, 2, 128, 256, BF16, 2105, 27),
    "odd-g3-d128-p64-f16": (6, 2, 128, 64, F16, 2106, 4),
}
MASKS = [(False, -1), (True, -1), (False, 127), (True, 127)]
MASK_IDS = ["full", "causal", "full-w127", "causal-w127"]


@functools.lru_cache(maxsize=None)
def geo_case(geo):
    hq, hkv, d, page, dtype, seed, sink_seed = GEOS[geo]
    c = Ragged(BASE_PAIRS, hq, hkv, page, 512, d, dtype, seed)
    return c, make_sinks(c.q4, c.k, c.lens, sink_seed)


@pytest.mark.parametrize("causal,w", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("geo", list(GEOS))
def test_the_chosen_sink_seeds_meet_the_condition(geo, causal, w):
    """CPU: the condition of the GPU grid on its inputs (the module docstring), on the committed seeds."""
    c, sinks = geo_case(geo)
    share = median_share(c, sinks, causal, w)
    print(f"SINK_SHARE {geo} causal={causal} w={w} median={share:.4f}")
    assert 0.01 <= share <= 0.9, share
    assert sinks[2] == NEG_INF and sinks[0] > sinks[3:].max() + 25 and sinks[1] < sinks[3:].min() - 25
    # what the condition is for: a kernel that ignored the sink, doubled it (applied before the pair sum), or
    # indexed it by kv-head or by the previous block's q-head lies outside TOL of the oracle somewhere
    if (causal, w) not in ((False, -1), (True, 127)):  # (the smallest and the largest shares: the oracle is slow)
        return
    ref = ragged_oracle(c, sinks, causal, w)
    hq, g = sinks.numel(), sinks.numel() // c.k.size(1)
    wrongs = {"ignored": torch.full((hq,), NEG_INF), "doubled": sinks + 0.6931471805599453,
              "by kv-head": sinks[torch.arange(hq) // g], "the previous head's": sinks.roll(1)}
    for what, wrong in wrongs.items():
        assert outside_tol(ragged_oracle(c, wrong, causal, w), ref, c.dtype), what


@pytest.mark.gpu
@pytest.mark.parametrize("causal,w", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("geo", list(GEOS))
def test_grid(fam, geo, causal, w):
    c, sinks = geo_case(geo)
    share = median_share(c, sinks, causal, w)
    assert 0.01 <= share <= 0.9, share
    out, path, in_place = launch(c, causal, w, sinks)
    plain, _, _ = launch(c, causal, w)
    assert torch.equal(out[:, 2], plain[:, 2])  # 1. -inf: no sink on this head
    ulps = (out[:, 1].view(torch.int16).int() - plain[:, 1].view(torch.int16).int()).abs().max().item()
    print(f"HEAD1 {geo} causal={causal} w={w} max ulp distance {ulps}")
    assert torch.equal(out[:, 1], plain[:, 1])  # (observed 0 ulps everywhere; see the module docstring)
    ref = ragged_oracle(c, sinks, causal, w)
    check_padded(out, ref, c.dtype)  # 2.
    assert torch.isfinite(out.float()).all()  # 3.
    dead = no_key_rows(c, causal, w)
    assert int(dead.sum()) >= (43 if causal else 40) and (out[dead] == 0).all()
    assert not (plain[~dead][:, 0] == 0).all() and out[:, 0].float().abs().max() < 1e-6  # (head 0: the sink takes all)
    assert path == "w4" and in_place  # 4.


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_cross_kernel_agreement(fam, dtype):
    """A sequence short enough for the decode kernel (Sq 8, g 8: 64 rows) through both kernels."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    c = Ragged(((8, 449),), 16, 2, 64, 512, 64, dtype, 2110)
    sinks = make_sinks(c.q4, c.k, c.lens, 3)
    ref = ragged_oracle(c, sinks, True)
    dec = flash_attn_paged_func(*dv(c.q4, c.kc, c.vc, c.table, c.sl), causal=True, sinks=sinks.to(DEV))
    assert _debug.last_path().startswith("decode_paged")
    out, path, in_place = launch(c, True, -1, sinks)
    assert path == "w4" and in_place
    check_padded(dec[0].transpose(0, 1), ref, dtype)
    check_padded(out, ref, dtype)


@pytest.mark.gpu
def test_dynamic_range(fam):
    """Logits far from the sink on either side, and sinks beyond the clamp: q = a k-aligned direction, so that
    every logit of a sequence sits near a chosen value."""
    hq, hkv, d = 8, 2, 64
    c = Ragged(((300, 449), (40, 37)), hq, hkv, 64, 512, d, F16, 2120)
    # every key equal to one unit-ish vector u, q = t u: logits t |u|^2 / sqrt(d) for every key
    u = torch.randn(d, generator=torch.Generator().manual_seed(1)).to(F16)
    uu = float((u.float() ** 2).sum()) * d ** -0.5
    for target, sink, near_zero in ((-200.0, 50.0, True), (200.0, -50.0, False)):
        cc = Ragged(((300, 449), (40, 37)), hq, hkv, 64, 512, d, F16, 2120)
        cc.k[:] = u
        for b, n in enumerate(cc.lens):  # the pool's keys (the values stay random)
            for j in range((n + 63) // 64):
                rows = min(n, 64 * j + 64) - 64 * j
                cc.kc[int(cc.table[b, j]), :, :rows] = u
        cc.q4[:] = (u.float() * (target / uu)).to(F16)
        cc.q = torch.cat([cc.q4[b, :, :s].transpose(0, 1) for b, s in enumerate(cc.sqs)]).contiguous()
        sinks = torch.full((hq,), sink)
        out, path, _ = launch(cc, True, -1, sinks)
        assert path == "w4" and torch.isfinite(out.float()).all()
        want = torch.zeros_like(out, dtype=torch.float32) if near_zero else ragged_oracle(cc, torch.full((hq,), NEG_INF), True)
        check_padded(out, want, F16)
        check_padded(out, ragged_oracle(cc, sinks, True), F16)
    for big in (float("inf"), 3e38, -3e38):  # the clamp rule: +-1e30 on the bits
        sinks = torch.full((hq,), big)
        out, _, _ = launch(c, True, -1, sinks)
        assert torch.isfinite(out.float()).all()
        if big > 0:
            assert (out == 0).all()
        else:
            assert torch.equal(out, launch(c, True)[0])


@pytest.mark.gpu
def test_sinks_is_read_at_its_heads_only(fam):
    """sinks as a [Hq] view in the middle of a NaN-filled buffer: the same bits."""
    c, sinks = geo_case("llama-g4-d128-p64-bf16")
    out, _, _ = launch(c, True, 127, sinks)
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    buf = torch.full((64,), float("nan"), device=DEV)
    buf[29:37] = sinks.to(DEV)
    got = flash_attn_paged_varlen_func(*dv(c.q, c.kc, c.vc, c.cu_q), c.max_q, *dv(c.table, c.sl), causal=True,
                                       window_left=127, sinks=buf[29:37])
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all() and torch.equal(got.cpu(), out)


from test_footprint import abi  # noqa: E402,F401  (the fixture: the C-ABI library and the debug labels)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_footprint(abi, dtype):  # noqa: F811
    """The C entry with every buffer in tests/footprint.py's arena: only rows [cu[0], cu[B]) of o are written (q / o
    have 5 rows before and 7 after them), under three fill patterns, and q, the pools, the table, the lengths, the
    cumulative array and the sinks are bit-identical after the call."""
    from test_footprint import LARGE, Launch, code, dense_params
    from test_paged_abi import FaPagedParams
    from test_paged_varlen_abi import FaPagedVarlenParams
    from test_paged_varlen_sink_abi import FaPagedVarlenSinkParams

    hq, hkv, d, page = 6, 2, 64, 64
    c = Ragged(((40, 37), (257, 300), (0, 100), (1, 449)), hq, hkv, page, 512, d, dtype, 2130)
    sinks = make_sinks(c.q4, c.k, c.lens, 7)
    lead, tail = 5, 7
    total = lead + c.q.size(0) + tail
    q = torch.cat([torch.full((lead, hq, d), float("nan"), dtype=dtype), c.q, torch.full((tail, hq, d), float("nan"), dtype=dtype)])
    cu = c.cu_q + lead
    L = Launch(abi, LARGE)
    qd = L.inp("q", q, dims=("row", "head", "col"))
    kcd, vcd = L.inp("k_cache", c.kc), L.inp("v_cache", c.vc)
    td, sld = L.inp("block_table", c.table, dims=("batch", "entry")), L.inp("cache_seqlens", c.sl, dims=("batch",))
    cud, sd = L.inp("cu_seqlens_q", cu, dims=("entry",)), L.inp("sinks", sinks, dims=("head",))
    o = L.out("o", dtype, q.shape, dims=("row", "head", "col"), written=lambda t: [t[lead:total - tail]])
    # the dense description of [1, Hq, total, D] views of the packed q / o, then the paged fields
    as4 = lambda t: t.transpose(0, 1)[None]  # noqa: E731
    base = dense_params(as4(qd), kcd, vcd, as4(o), hq // hkv, d ** -0.5)
    base.batch_size, base.seqlen_q, base.seqlen_kv = len(c.sqs), c.max_q, 512
    base.k_seqlen_stride, base.v_seqlen_stride = kcd.stride(2), vcd.stride(2)
    pp = FaPagedParams(base, td.data_ptr(), td.stride(0), c.table.size(1), c.kc.size(0), page, sld.data_ptr())
    sp = FaPagedVarlenSinkParams(FaPagedVarlenParams(pp, cud.data_ptr(), total), sd.data_ptr())
    lib, I64, P, C = abi.lib, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    lib.fa_fwd_gfx950_paged_varlen_sink.argtypes = [P, C, C, I64, P, I64, P]
    lib.fa_fwd_gfx950_paged_varlen_sink_workspace_size.argtypes = [P, C, C, I64]
    lib.fa_fwd_gfx950_paged_varlen_sink_workspace_size.restype = I64
    dt = code(dtype)
    assert lib.fa_fwd_gfx950_paged_varlen_sink_workspace_size(ctypes.byref(sp), dt, 1, 127) == 0, lib.fa_last_error()
    call = lambda: lib.fa_fwd_gfx950_paged_varlen_sink(ctypes.byref(sp), dt, 1, 127, None, 0, abi.stream())  # noqa: E731

    def expect():
        assert abi.dbg.last_path() == "w4" and abi.dbg.last_prefill_paged()

    (got,) = L.run(call, expect)  # (asserts: nothing outside the declared rows written, no input changed)
    check_padded(got, ragged_oracle(c, sinks, True, 127), dtype)
    ref, _, _ = launch(c, True, 127, sinks)  # the pin: the Python op on the same tensors
    assert torch.equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("causal,w", [(True, -1), (True, 100)], ids=["causal", "causal-w100"])
def test_step_equals_append_then_attention(fam, causal, w):
    from flash_attention_cute_amd import _debug

    s = step_inputs(BF16, 2140)
    kc, vc, table, sl, cu, k, v, q = dv(s["kc"], s["vc"], s["table"], s["sl"], s["cu"], s["k"], s["v"], s["q"])
    cos, sin = dv(*s["cos_sin"])
    sinks = (2 * torch.randn(8, generator=torch.Generator().manual_seed(9))).to(DEV)
    sinks[2] = NEG_INF
    kc2, vc2 = kc.clone(), vc.clone()
    out, new = fam.flash_attn_varlen_with_kvcache(q, kc, vc, cu, max(STEP_NEWS), k, v, rotary_cos=cos, rotary_sin=sin,
                                                  cache_seqlens=sl, block_table=table, causal=causal, window_left=w,
                                                  return_seqlens=True, sinks=sinks)
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
    new2, q_rot = fam.flash_attn_kvcache_append_varlen(kc2, vc2, k, v, cu, sl, table, cos, sin, q, cu)
    ref = fam.flash_attn_paged_varlen_func(q_rot, kc2, vc2, cu, max(STEP_NEWS), table, new2, causal=causal, window_left=w,
                                           sinks=sinks)
    plain = fam.flash_attn_paged_varlen_func(q_rot, kc2, vc2, cu, max(STEP_NEWS), table, new2, causal=causal, window_left=w)
    torch.cuda.synchronize()
    assert torch.equal(new, new2)
    assert torch.equal(kc.view(torch.int16), kc2.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc2.view(torch.int16))
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)
    assert torch.equal(out[:, 2], plain[:, 2]) and not torch.equal(out[:, 3], plain[:, 3])  # (the sinks did arrive)


@pytest.mark.gpu
def test_step_graph_capture(fam):
    """The sinked step captured once and replayed once on other sinks (same shapes): the eager bits."""
    s = step_inputs(BF16, 2150)
    kc, vc, table, sl, cu, k, v, q = dv(s["kc"], s["vc"], s["table"], s["sl"], s["cu"], s["k"], s["v"], s["q"])
    cos, sin = dv(*s["cos_sin"])
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)
    sinks = torch.zeros(8, device=DEV)

    def step():
        return fam.flash_attn_varlen_with_kvcache(q, kc, vc, cu, 320, k, v, rotary_cos=cos, rotary_sin=sin,
                                                  cache_seqlens=sl, block_table=table, causal=True, sinks=sinks)

    kc_start, vc_start = kc.clone(), vc.clone()
    step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    kc.copy_(kc_start)
    vc.copy_(vc_start)
    sinks.copy_(2 * torch.randn(8, generator=torch.Generator().manual_seed(11)))
    g.replay()
    torch.cuda.synchronize()
    got, kc_g = out.clone(), kc.clone()
    kc.copy_(kc_start)
    vc.copy_(vc_start)
    eager = step()
    torch.cuda.synchronize()
    assert torch.equal(kc_g.view(torch.int16), kc.view(torch.int16))
    assert torch.isfinite(got.float()).all() and torch.equal(got, eager)
    sinks.zero_()
    kc.copy_(kc_start)
    vc.copy_(vc_start)
    assert not torch.equal(step(), eager)  # (the replay read the sinks of its own time)
