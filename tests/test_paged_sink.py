"""Attention sinks on the paged decode, 16-bit and FP8 pools, windowed or not (include/fa_gfx950_sink.h).

``flash_attn_paged_func(..., sinks=S)`` and ``flash_attn_with_kvcache(..., sinks=S)``: S is one fp32 logit per q-head
that joins the softmax denominator and contributes no value,

    out = (v_descale) sum_n exp(s_n - mu) v_n / (sum_n exp(s_n - mu) + exp(S[h] - mu)),  mu = max(max_n s_n, S[h]),

with s_n the scaled, masked scores of the row's visible keys; S is in final-logit units (no softmax_scale, no
k_descale). The oracle is that formula in float64 over the same 16-bit (or widened e4m3) inputs, within
tests/test_gpu_parity.py TOL (fp16 2e-3 + 2e-3|ref|, bf16 1.6e-2 + 1.6e-2|ref|): a sink only shrinks outputs, so
the bar of the kernels without sinks holds by construction.

Every case draws the sinks as 2 randn(Hq) and fixes three heads by hand: head 0 has a sink 30 above the largest
logit of the case, head 1 one 30 below the smallest, head 2 has -inf (no sink). Pools are test_paged.make_paged's:
shuffled tables, every unused row NaN, every unused entry -1.
"""
from __future__ import annotations

import functools
import warnings

import pytest
import torch

from test_fp8_kvcache import FP8, NAN_BYTE, make_fp8_paged, schema_holds
from test_kvcache import make_cache, new_tokens, rope_tables
from test_padded import check_padded
from test_paged import KINDS, make_paged
from test_paged_window import SPLIT, free_pages_below_the_window

F16, BF16 = torch.float16, torch.bfloat16
DEV = "cuda:0"
NEG_INF = float("-inf")


def quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


def descales(b, hkv, shift=0):
    """Distinct powers of two per (b, h), none of them 1: 2^-3 .. 2^-1, 2^1 .. 2^3, fp32 [B, Hkv]."""
    e = (torch.arange(b * hkv).reshape(b, hkv) + shift) % 6 - 3
    return torch.pow(2.0, torch.where(e >= 0, e + 1, e).float())


def scores(q, k, lens, scale=None, kd=None):
    """float64 scaled scores of every sequence over ITS keys: list of [Hq, Sq, n_b]."""
    g = q.size(1) // k.size(1)
    scale = q.size(-1) ** -0.5 if scale is None else scale
    out = []
    for b, n in enumerate(lens):
        s = torch.matmul(q[b].double(), k[b, :, :n].double().repeat_interleave(g, dim=0).transpose(1, 2)) * scale
        if kd is not None:
            s = s * kd[b].double().repeat_interleave(g)[:, None, None]
        out.append(s)
    return out


def make_sinks(q, k, lens, seed, scale=None, kd=None):
    """2 randn(Hq) with heads 0 / 1 / 2 fixed: 30 above the largest logit, 30 below the smallest, -inf."""
    flat = torch.cat([s.flatten() for s in scores(q, k, lens, scale, kd)] + [torch.zeros(1, dtype=torch.float64)])
    sinks = 2 * torch.randn(q.size(1), generator=torch.Generator().manual_seed(seed))
    sinks[0], sinks[1], sinks[2] = flat.max().item() + 30, flat.min().item() - 30, NEG_INF
    return sinks


def sink_oracle(q, k, v, lens, sinks, causal, w=-1, scale=None, kd=None, vd=None):
    """The float64 softmax with the extra column over the dense keys [B, Hkv, cap, D] (16-bit, or e4m3 widened)."""
    bsz, hq, sq, d = q.shape
    g = hq // k.size(1)
    out = torch.zeros(bsz, hq, sq, d, dtype=torch.float64)
    col = sinks.double()[:, None, None].expand(hq, sq, 1)
    for b, (n, s) in enumerate(zip(lens, scores(q, k, lens, scale, kd))):
        if n == 0:
            continue
        m, j = torch.arange(sq)[:, None], torch.arange(n)[None, :]
        vis = torch.ones(sq, n, dtype=torch.bool)
        if w >= 0:
            vis &= j >= m + n - sq - w
        if causal:
            vis &= j <= m + n - sq
        s = s.masked_fill(~vis[None], NEG_INF)
        p = torch.nan_to_num(torch.softmax(torch.cat([s, col], dim=-1), dim=-1)[..., :n], nan=0.0)
        o = torch.matmul(p, v[b, :, :n].double().repeat_interleave(g, dim=0))
        if vd is not None:
            o = o * vd[b].double().repeat_interleave(g)[:, None, None]
        out[b] = o
    return out.float()


# ------------------------------------------------------------------------------------------- CPU
CPU_LENS, CPU_GEO = (96, 0, 33, 1, 64), (4, 2, 32, 96, 64)  # lens; Hq, Hkv, page, capacity, D

SINK_SCHEMA = ("flash_attention::paged_forward_sink(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, "
               "Tensor cache_seqlens, Tensor sinks, SymInt window_left=-1, float softmax_scale=None, "
               "bool causal=False) -> Tensor")
SINK_FP8_SCHEMA = ("flash_attention::paged_forward_sink_fp8(Tensor q, Tensor k_cache, Tensor v_cache, "
                   "Tensor block_table, Tensor cache_seqlens, Tensor sinks, SymInt window_left=-1, "
                   "Tensor? k_descale=None, Tensor? v_descale=None, float softmax_scale=None, bool causal=False) "
                   "-> Tensor")
OLD_SCHEMAS = {
    "paged_forward": "flash_attention::paged_forward(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, "
                     "Tensor cache_seqlens, float softmax_scale=None, bool causal=False) -> Tensor",
    "paged_window_forward": "flash_attention::paged_window_forward(Tensor q, Tensor k_cache, Tensor v_cache, "
                            "Tensor block_table, Tensor cache_seqlens, SymInt window_left, float softmax_scale=None, "
                            "bool causal=False) -> Tensor",
    "paged_forward_fp8": "flash_attention::paged_forward_fp8(Tensor q, Tensor k_cache, Tensor v_cache, "
                         "Tensor block_table, Tensor cache_seqlens, Tensor? k_descale=None, Tensor? v_descale=None, "
                         "float softmax_scale=None, bool causal=False) -> Tensor",
    "paged_window_forward_fp8": "flash_attention::paged_window_forward_fp8(Tensor q, Tensor k_cache, Tensor v_cache, "
                                "Tensor block_table, Tensor cache_seqlens, SymInt window_left, Tensor? k_descale=None, "
                                "Tensor? v_descale=None, float softmax_scale=None, bool causal=False) -> Tensor",
}


def test_sink_ops_registration_fakes_and_exports():
    import flash_attention_cute_amd as m

    ops = torch.ops.flash_attention
    assert str(ops.paged_forward_sink.default._schema) == SINK_SCHEMA
    assert str(ops.paged_forward_sink_fp8.default._schema) == SINK_FP8_SCHEMA
    for name, sch in OLD_SCHEMAS.items():
        assert str(getattr(ops, name).default._schema) == sch
        assert "sink" not in sch
    for name in ("flash_attention_paged_forward_sink", "flash_attention_paged_forward_sink_fp8"):
        assert name in m.__all__ and hasattr(m, name)
    q, _, _, kc, vc, table, lens = make_paged((40, 7), 4, 2, 2, 32, 64, 32, torch.float32, 1)
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)
    sinks = torch.tensor([0.5, -1.0, NEG_INF, 3.0])
    quiet(torch.library.opcheck, ops.paged_forward_sink.default, (q, kc, vc, table, lens, sinks, 9, 0.125, True),
          test_utils=("test_schema", "test_faketensor"))
    quiet(torch.library.opcheck, ops.paged_forward_sink.default, (q, kc, vc, table, lens, sinks),
          test_utils=("test_schema", "test_faketensor"))
    q8, _, _, kc8, vc8, table8, lens8 = make_fp8_paged((40, 7), 4, 2, 2, 32, 64, 32, F16, 1)
    kc8 = kc8.view(torch.uint8).masked_fill(kc8.view(torch.uint8) == NAN_BYTE, 0).view(FP8)
    vc8 = vc8.view(torch.uint8).masked_fill(vc8.view(torch.uint8) == NAN_BYTE, 0).view(FP8)
    args8 = (q8, kc8, vc8, table8, lens8, sinks, 9, descales(2, 2), None, 0.125, True)
    quiet(torch.library.opcheck, ops.paged_forward_sink_fp8.default, args8, test_utils=("test_faketensor",))
    quiet(schema_holds, ops.paged_forward_sink_fp8.default, args8, mutated=())  # ("test_schema" cannot run on float8)


@pytest.mark.parametrize("w", [-1, 0, 31, 33])
@pytest.mark.parametrize("causal,sq", [(False, 3), (True, 3), (False, 1)], ids=["full_sq3", "causal_sq3", "sq1"])
def test_sink_cpu_default_matches_float64(w, causal, sq):
    """The CPU default computes in fp32 on fp32 copies of the 16-bit inputs: 1e-5 + 1e-5 |ref| is fp32's own error
    over a 64-term dot product and a 96-term sum (eps 6e-8 each), with a wide margin."""
    from flash_attention_cute_amd import flash_attn_paged_func

    hq, hkv, page, cap, d = CPU_GEO
    q, k, v, kc, vc, table, sl = make_paged(CPU_LENS, hq, hkv, sq, page, cap, d, F16, 3)
    sinks = make_sinks(q, k, CPU_LENS, 5)
    out = quiet(flash_attn_paged_func, q.float(), kc.float(), vc.float(), table, sl, causal=causal, window_left=w,
                sinks=sinks)
    assert torch.isfinite(out).all() and (out[1] == 0).all()  # (a sequence without keys)
    ref = sink_oracle(q, k, v, CPU_LENS, sinks, causal, w)
    torch.testing.assert_close(out, ref, atol=1e-5, rtol=1e-5)
    assert ref[:, 0].abs().max() < 1e-9 and ref[:, 3].abs().max() > 1e-2  # (the sink of head 0 dominates)
    # sinks all -inf: the call without sinks (its SDPA orders the fp32 sums differently: fp32's error again)
    none = quiet(flash_attn_paged_func, q.float(), kc.float(), vc.float(), table, sl, causal=causal, window_left=w,
                 sinks=torch.full((hq,), NEG_INF))
    plain = quiet(flash_attn_paged_func, q.float(), kc.float(), vc.float(), table, sl, causal=causal, window_left=w)
    torch.testing.assert_close(none, plain, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("w", [-1, 31])
def test_sink_fp8_cpu_default_matches_float64(w):
    """An FP8 pool with descales != 1: the sink is scaled by neither. The default returns q's dtype: fp16's bar."""
    from flash_attention_cute_amd import flash_attn_paged_func

    hq, hkv, page, cap, d = CPU_GEO
    kd, vd = descales(5, hkv), descales(5, hkv, 2)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(CPU_LENS, hq, hkv, 3, page, cap, d, F16, 3, kd=kd, vd=vd)
    sinks = make_sinks(q, k8.float(), CPU_LENS, 5, kd=kd)
    out = quiet(flash_attn_paged_func, q, kc8, vc8, table, sl, causal=True, k_descale=kd, v_descale=vd, window_left=w,
                sinks=sinks.half())  # (a 16-bit sinks tensor is converted once)
    ref = sink_oracle(q, k8.float(), v8.float(), CPU_LENS, sinks.half().float(), True, w, kd=kd, vd=vd)
    check_padded(out, ref, F16)
    wrong = sink_oracle(q, k8.float(), v8.float(), CPU_LENS, sinks.half().float() * d ** -0.5, True, w, kd=kd, vd=vd)
    assert (wrong - ref).abs().max() > 0.05  # (the case tells a scaled sink from an unscaled one)


def test_sink_wrapper_errors():
    from flash_attention_cute_amd import flash_attn_paged_func, flash_attn_with_kvcache

    q, _, _, kc, vc, table, sl = make_paged((40, 7), 4, 2, 2, 32, 64, 64, torch.float32, 1)
    for bad in (torch.zeros(3), torch.zeros(4, 1), torch.zeros(2), 0.5, torch.zeros(4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sinks"):
            flash_attn_paged_func(q, kc, vc, table, sl, sinks=bad)
    ok = torch.zeros(4)
    with pytest.raises(NotImplementedError, match="return_lse"):
        flash_attn_paged_func(q, kc, vc, table, sl, sinks=ok, return_lse=True)
    big = torch.zeros(2, 4, 33, 64)  # g 2 x Sq 33 = 66 rows
    with pytest.raises(NotImplementedError, match="decode shapes"):
        flash_attn_paged_func(big, kc, vc, table, sl, sinks=ok)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        flash_attn_paged_func(q[..., :60], kc[..., :60], vc[..., :60], table, sl, sinks=ok)
    # flash_attn_with_kvcache: a dense cache goes through an identity table, so its length must allow that
    dense = torch.zeros(2, 2, 40, 64)
    with pytest.raises(ValueError, match="multiple of 32"):
        flash_attn_with_kvcache(q, dense, dense.clone(), cache_seqlens=sl, sinks=ok)
    with pytest.raises(ValueError, match="shared_prefix_len"):
        flash_attn_with_kvcache(q[:, :, :1], kc, vc, cache_seqlens=sl, block_table=table, sinks=ok, shared_prefix_len=32)
    with pytest.raises(NotImplementedError, match="decode shapes"):  # before anything is appended
        flash_attn_with_kvcache(big, kc, vc, big[:, :2], big[:, :2], cache_seqlens=sl, block_table=table, sinks=ok)
    assert sl.tolist() == [40, 7]


def test_with_kvcache_sinks_on_a_dense_cache_cpu():
    """A dense 16-bit cache with sinks is read through an identity table (batch row b is page b)."""
    from flash_attention_cute_amd import flash_attn_with_kvcache

    lens, hq, hkv, cap, d, sq = (60, 0, 33, 90), 4, 2, 96, 64, 2
    kc, vc, _, sl = make_cache(lens, sq, hkv, 32, cap, d, F16, 7, dense=True)
    kn, vn, q = new_tokens(4, hkv, sq, d, F16, 1), new_tokens(4, hkv, sq, d, F16, 2), new_tokens(4, hq, sq, d, F16, 3)
    kc, vc = kc.float(), vc.float()
    new_lens = [n + sq for n in lens]
    sinks = torch.tensor([1.0, -2.0, NEG_INF, 0.25])
    out, new = quiet(flash_attn_with_kvcache, q.float(), kc, vc, kn.float(), vn.float(), cache_seqlens=sl, causal=True,
                     return_seqlens=True, window_left=40, sinks=sinks)
    assert new.tolist() == new_lens
    torch.testing.assert_close(out, sink_oracle(q, kc, vc, new_lens, sinks, True, 40), atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def ops(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    _debug.set_dec_fuse(None)
    yield fam
    _debug.set_dec_fuse(None)


def dv(*ts):
    return tuple(t.to(DEV) for t in ts)


def launch(q, kc, vc, table, sl, sinks, causal=False, w=-1, fuse=None, **kw):
    """One paged launch on the device: (output on the host, path, fused). sinks None: the call without them."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    _debug.set_knobs()
    _debug.set_dec_fuse(fuse)
    try:
        if sinks is not None:
            kw["sinks"] = sinks
        out = flash_attn_paged_func(*dv(q, kc, vc, table, sl), causal=causal, window_left=w,
                                    **{n: t.to(DEV) for n, t in kw.items()})
        path, fused = _debug.last_path(), _debug.last_dec_fused()
        torch.cuda.synchronize()
    finally:
        _debug.set_dec_fuse(None)
    return out.cpu(), path, fused


def want_path(kind, fp8=False):
    return ("decode_paged_fp8" if fp8 else "decode_paged") + ("_split" if kind.startswith("split") else "")


# 1. oracle parity on every path. (kind, page, D, dtype, layout, lengths): the kinds and shapes of test_paged
CASES = [
    ("unsplit", 32, 128, F16, "phsd", (0, 1, 31)),
    ("unsplit", 64, 72, BF16, "pshd", (32, 33, 256)),
    ("split", 32, 128, BF16, "phsd", (2048, 33)),
    ("split", 64, 64, F16, "pshd", (65, 2047)),
    ("split_unfused", 32, 72, F16, "phsd", (32, 1999)),
    ("split_unfused", 64, 128, BF16, "pshd", (2048, 33)),
    ("sq3_causal", 32, 128, F16, "pshd", (0, 1, 33)),
    ("sq3_causal", 256, 64, BF16, "pshd", (2, 256, 32)),
    ("g8_sq5", 32, 64, F16, "phsd", (31, 32, 256)),
    ("g8_sq5", 64, 128, BF16, "pshd", (5, 65, 0)),
]
CASE_IDS = [f"{k}-p{p}-d{d}-{'f16' if t == F16 else 'bf16'}" for k, p, d, t, _, _ in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_sink_decode_matches_the_oracle(ops, ci):
    kind, page, d, dtype, layout, lens = CASES[ci]
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 1100 + ci, layout)
    sinks = make_sinks(q, k, lens, ci)
    fuse = 0 if kind == "split_unfused" else None
    out, path, fused = launch(q, kc, vc, table, sl, sinks, causal, -1, fuse)
    assert path == want_path(kind) and fused == (kind == "split")
    ref = sink_oracle(q, k, v, lens, sinks, causal)
    check_padded(out, ref, dtype)
    plain, _, _ = launch(q, kc, vc, table, sl, None, causal, -1, fuse)
    assert torch.equal(out[:, 2::hq], plain[:, 2::hq])  # head 2 has no sink: the unsinked bits
    assert torch.equal(out[:, 1::hq], plain[:, 1::hq])  # a sink 30 below every score: e == 1, L' == L
    assert (out[:, 0].float().abs() <= 1e-9).all()      # a sink 30 above every score: e^-30 of the row
    assert not torch.equal(out[:, 3:], plain[:, 3:])


# 2. windowed parity. Sq == 1: the lengths and windows of test_paged_window (tile and page edges); page size, D, dtype
# and layout cycle so that each value meets each window and each triple
LENS1 = [(0, 1, 31), (32, 33, 256), (64, 65, 200)]
WINDOWS1 = [0, 1, 31, 32, 33, 100]
PAGES, DIMS = (32, 64, 256), (64, 128, 72)
CASES1 = [(li, w, PAGES[(li + wi) % 3], DIMS[(li + 2 * wi + wi // 3) % 3], (F16, BF16)[(li + wi) % 2],
           ("phsd", "pshd")[(wi + wi // 2) % 2]) for li in range(3) for wi, w in enumerate(WINDOWS1)]
IDS1 = [f"L{li}-w{w}-p{p}-d{d}-{'f16' if t == F16 else 'bf16'}-{lay}" for li, w, p, d, t, lay in CASES1]


@functools.lru_cache(maxsize=None)
def run1(ci):
    li, w, page, d, dtype, layout = CASES1[ci]
    q, k, v, kc, vc, table, sl = make_paged(LENS1[li], 8, 2, 1, page, 256, d, dtype, 1500 + ci, layout)
    sinks = make_sinks(q, k, LENS1[li], ci)
    out, path, _ = launch(q, kc, vc, table, sl, sinks, False, w)
    return out, path, sink_oracle(q, k, v, LENS1[li], sinks, False, w), (q, kc, vc, table, sl, sinks)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES1)), ids=IDS1)
def test_sink_window_decode_matches_the_oracle(ops, ci):
    out, path, ref, _ = run1(ci)
    assert path == "decode_paged"
    check_padded(out, ref, CASES1[ci][4])


@pytest.mark.gpu
@pytest.mark.parametrize("w,page,d,dtype,lens", [(0, 32, 64, F16, (31, 32, 256)), (31, 64, 128, BF16, (5, 65, 200)),
                                                 (33, 256, 72, F16, (256, 4, 33)), (100, 32, 128, BF16, (130, 101, 0))])
def test_sink_window_rows_whose_windows_start_in_different_tiles(ops, w, page, d, dtype, lens):
    """g 8 x Sq 5: 40 rows in two row blocks, each position with its own lower bound."""
    b, hq, hkv, sq, cap, causal = KINDS["g8_sq5"]
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 1600 + w)
    sinks = make_sinks(q, k, lens, w)
    out, path, _ = launch(q, kc, vc, table, sl, sinks, causal, w)
    assert path == "decode_paged"
    check_padded(out, sink_oracle(q, k, v, lens, sinks, causal, w), dtype)


@functools.lru_cache(maxsize=None)
def split_inputs(fp8=False):
    s = SPLIT
    if fp8:
        kd, vd = descales(2, s["hkv"]), descales(2, s["hkv"], 2)
        return make_fp8_paged(s["lens"], s["hq"], s["hkv"], 1, s["page"], s["cap"], s["d"], s["dtype"], 77, "phsd", kd,
                              vd) + (kd, vd)
    return make_paged(s["lens"], s["hq"], s["hkv"], 1, s["page"], s["cap"], s["d"], s["dtype"], 77)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", [None, 0], ids=["fused", "unfused"])
def test_sink_window_split_decode(ops, fuse):
    q, k, v, kc, vc, table, sl = split_inputs()
    sinks = make_sinks(q, k, SPLIT["lens"], 9)
    out, path, fused = launch(q, kc, vc, table, sl, sinks, False, SPLIT["w"], fuse)
    assert path == "decode_paged_split" and fused == (fuse is None)
    check_padded(out, sink_oracle(q, k, v, SPLIT["lens"], sinks, False, SPLIT["w"]), SPLIT["dtype"])


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [2 ** 31 - 1, -1])
@pytest.mark.parametrize("ci", [13, 14], ids=[IDS1[13], IDS1[14]])
def test_sink_window_freed_pages_are_never_read(ops, ci, bad):
    li, w, page, _, _, _ = CASES1[ci]
    out, _, _, (q, kc, vc, table, sl, sinks) = run1(ci)
    lens = LENS1[li]
    assert max(n - 1 - w for n in lens) >= 64 and page < 256
    kc2, vc2, table2, freed = free_pages_below_the_window(kc, vc, table, lens, 1, w, page, bad, float("nan"))
    assert freed >= 2
    got, _, _ = launch(q, kc2, vc2, table2, sl, sinks, False, w)
    assert torch.isfinite(got.float()).all() and torch.equal(got, out)


# 3. an FP8 pool with power-of-two descales != 1: a sink scaled by k_descale or softmax_scale misses the bar
FP8_CASES = [("unsplit", 64, 128, BF16, (64, 65, 200), -1), ("unsplit", 32, 64, F16, (32, 33, 256), 31),
             ("split", 64, 128, BF16, (2048, 33), -1), ("split", 32, 64, F16, (65, 2047), -1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,page,d,dtype,lens,w", FP8_CASES, ids=[f"{c[0]}-d{c[2]}-w{c[5]}" for c in FP8_CASES])
def test_sink_fp8_pool(ops, kind, page, d, dtype, lens, w):
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    kd, vd = descales(b, hkv), descales(b, hkv, 2)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, sq, page, cap, d, dtype, 1900, "pshd", kd, vd)
    sinks = make_sinks(q, k8.float(), lens, 3, kd=kd)
    out, path, _ = launch(q, kc8, vc8, table, sl, sinks, causal, w, k_descale=kd, v_descale=vd)
    assert path == want_path(kind, True)
    ref = sink_oracle(q, k8.float(), v8.float(), lens, sinks, causal, w, kd=kd, vd=vd)
    check_padded(out, ref, dtype)
    for wrong in (sinks * d ** -0.5, sinks * kd[0, 0]):  # (the case tells a scaled sink from an unscaled one)
        bad = sink_oracle(q, k8.float(), v8.float(), lens, wrong, causal, w, kd=kd, vd=vd)
        atol = 2e-3 if dtype == F16 else 1.6e-2
        assert ((bad - ref).abs() - 2 * (atol + atol * ref.abs())).max() > 0


@pytest.mark.gpu
def test_sink_fp8_window_split_decode(ops):
    q, k8, v8, kc8, vc8, table, sl, kd, vd = split_inputs(True)
    sinks = make_sinks(q, k8.float(), SPLIT["lens"], 4, kd=kd)
    out, path, fused = launch(q, kc8, vc8, table, sl, sinks, False, SPLIT["w"], k_descale=kd, v_descale=vd)
    assert path == "decode_paged_fp8_split" and fused
    ref = sink_oracle(q, k8.float(), v8.float(), SPLIT["lens"], sinks, False, SPLIT["w"], kd=kd, vd=vd)
    check_padded(out, ref, SPLIT["dtype"])


# 4. no-op sinks (-inf, -1e30) on all four kernel families, unsplit / split fused / split unfused: the bits of the
# call without sinks. 6. extremes: +-1e4 and +-3e38 are finite; the positive ones give rows of exactly 0, the
# negative ones the unsinked bits; a sequence without keys stays 0.
def family_inputs(fp8, window, split):
    """(inputs, window_left, descale kwargs) of one kernel family: lengths include a sequence without keys."""
    if split and window:
        lens, page, cap, d, w = (4096, 0, 2300), 64, 4096, 128, 2047
    elif split:
        lens, page, cap, d, w = (2048, 0, 33), 32, 2048, 64, -1
    else:
        lens, page, cap, d, w = (64, 0, 200), 64, 256, 128, (100 if window else -1)
    if fp8:
        kd, vd = descales(3, 2), descales(3, 2, 2)
        q, _, _, kc, vc, table, sl = make_fp8_paged(lens, 8, 2, 1, page, cap, d, BF16, 2100, "phsd", kd, vd)
        return (q, kc, vc, table, sl), w, dict(k_descale=kd, v_descale=vd)
    q, _, _, kc, vc, table, sl = make_paged(lens, 8, 2, 1, page, cap, d, BF16, 2100)
    return (q, kc, vc, table, sl), w, {}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["unsplit", "split_fused", "split_unfused"])
@pytest.mark.parametrize("window", [False, True], ids=["full", "window"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_noop_and_extreme_sinks(ops, fp8, window, mode):
    args, w, ds = family_inputs(fp8, window, mode != "unsplit")
    fuse = 0 if mode == "split_unfused" else None
    plain, path, fused = launch(*args, None, False, w, fuse, **ds)
    assert path == want_path("split" if mode != "unsplit" else "unsplit", fp8) and fused == (mode == "split_fused")
    assert torch.isfinite(plain.float()).all() and (plain[1] == 0).all() and plain[0].float().abs().max() > 0
    for value in (NEG_INF, -1e30, -1e4, -3e38):
        out, path2, fused2 = launch(*args, torch.full((8,), value), False, w, fuse, **ds)
        assert (path2, fused2) == (path, fused)
        assert torch.equal(out, plain), value
    for value in (1e4, 3e38):
        out, _, _ = launch(*args, torch.full((8,), value), False, w, fuse, **ds)
        assert torch.isfinite(out.float()).all() and (out == 0).all(), value


# 5. the sink is applied once per row: the fused and the separate merge agree (bit for bit at D 128, within one
# output ulp at D 64, the documented v_fma_mix difference of the two merges) and both meet the oracle on the
# (2048, 33) case, where the sink dominates the 33-key row
@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype", [(128, BF16), (64, F16), (128, F16), (64, BF16)])
def test_sink_is_applied_once_in_either_merge(ops, d, dtype):
    lens = (2048, 33)
    q, k, v, kc, vc, table, sl = make_paged(lens, 8, 2, 1, 32, 2048, d, dtype, 2300 + d)
    sinks = 2 * torch.randn(8, generator=torch.Generator().manual_seed(d))
    s33 = scores(q, k, lens)[1]
    sinks[3] = s33[3].max().item() + 4  # on the 33-key row of head 3 the sink outweighs every key
    fused, path, f1 = launch(q, kc, vc, table, sl, sinks, False, -1, None)
    sep, path2, f0 = launch(q, kc, vc, table, sl, sinks, False, -1, 0)
    assert path == path2 == "decode_paged_split" and f1 and not f0
    ref = sink_oracle(q, k, v, lens, sinks, False)
    assert ref[1, 3].abs().max() < 0.5 * sink_oracle(q, k, v, lens, torch.full((8,), NEG_INF), False)[1, 3].abs().max()
    check_padded(fused, ref, dtype)
    check_padded(sep, ref, dtype)
    if d == 128:
        assert torch.equal(fused, sep)
    else:
        ulp = 2.0 ** (-10 if dtype == F16 else -7)
        a, b = fused.float(), sep.float()
        assert ((a - b).abs() <= ulp * torch.maximum(a.abs(), b.abs())).all()


# 7. the identity on the device: a sinked row is the unsinked row times sigmoid(lse - sink)
@pytest.mark.gpu
@pytest.mark.parametrize("ci", [0, 2, 5, 7], ids=[CASE_IDS[i] for i in (0, 2, 5, 7)])
def test_sink_equals_the_lse_rescaled_row(ops, ci):
    from flash_attention_cute_amd import flash_attn_paged_func

    kind, page, d, dtype, layout, lens = CASES[ci]
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 1100 + ci, layout)
    sinks = make_sinks(q, k, lens, ci)
    out, _, _ = launch(q, kc, vc, table, sl, sinks, causal)
    plain, lse = flash_attn_paged_func(*dv(q, kc, vc, table, sl), causal=causal, return_lse=True)
    torch.cuda.synchronize()
    factor = torch.nan_to_num(torch.sigmoid(lse.cpu().double() - sinks.double()[None, :, None]), nan=0.0)
    check_padded(out, (plain.cpu().double() * factor[..., None]).float(), dtype)


# 8. flash_attn_with_kvcache(sinks=): the composed step, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_with_kvcache_sinks_equals_the_composed_step(ops, device, fp8):
    fam = ops
    lens, hq, hkv, page, cap, d, w = (200, 0, 33, 255), 8, 2, 32, 256, 128, 127
    kc, vc, table, sl = dv(*make_cache(lens, 1, hkv, page, cap, d, BF16, 21))
    kn, vn, q = dv(new_tokens(4, hkv, 1, d, BF16, 1), new_tokens(4, hkv, 1, d, BF16, 2), new_tokens(4, hq, 1, d, BF16, 3))
    cos, sin = dv(*rope_tables(cap, d, BF16))
    sinks = (2 * torch.randn(hq, generator=torch.Generator().manual_seed(8))).to(DEV)
    ds = {}
    if fp8:
        kd, vd = dv(descales(4, hkv), descales(4, hkv, 2))
        kc, vc = fam.quantize_e4m3(kc.nan_to_num(0.0), 1.0), fam.quantize_e4m3(vc.nan_to_num(0.0), 1.0)
        ds = dict(k_descale=kd, v_descale=vd)
    kc2, vc2 = kc.clone(), vc.clone()
    out, new = fam.flash_attn_with_kvcache(q, kc, vc, kn, vn, cos, sin, cache_seqlens=sl, block_table=table, causal=True,
                                           return_seqlens=True, window_left=w, sinks=sinks, **ds)
    if fp8:
        new2, q_rot = torch.ops.flash_attention.kvcache_append_fp8(kc2, vc2, kn, vn, sl, table, q, cos, sin, kd, vd)
    else:
        new2, q_rot = torch.ops.flash_attention.kvcache_append(kc2, vc2, kn, vn, sl, table, q, cos, sin)
    ref = fam.flash_attn_paged_func(q_rot, kc2, vc2, table, new2, causal=True, window_left=w, sinks=sinks, **ds)
    torch.cuda.synchronize()
    assert torch.equal(new, new2) and torch.equal(kc.view(torch.uint8), kc2.view(torch.uint8))
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)
    unsinked = fam.flash_attn_paged_func(q_rot, kc2, vc2, table, new2, causal=True, window_left=w, **ds)
    assert not torch.equal(out, unsinked)


@pytest.mark.gpu
def test_with_kvcache_sinks_on_a_dense_cache(ops, device):
    """A dense 16-bit cache with sinks is read by the paged sink kernel through an identity table."""
    from flash_attention_cute_amd import _debug

    fam = ops
    lens, hq, hkv, cap, d, w, sq = (70, 0, 33, 100), 8, 2, 128, 128, 40, 3
    kc, vc, _, sl = make_cache(lens, sq, hkv, 32, cap, d, F16, 22, dense=True)
    kn, vn, q = new_tokens(4, hkv, sq, d, F16, 1), new_tokens(4, hkv, sq, d, F16, 2), new_tokens(4, hq, sq, d, F16, 3)
    kg, vg = dv(kc, vc)
    sinks = 2 * torch.randn(hq, generator=torch.Generator().manual_seed(9))
    out, new = fam.flash_attn_with_kvcache(*dv(q), kg, vg, *dv(kn, vn), cache_seqlens=sl.to(DEV), causal=True,
                                           return_seqlens=True, window_left=w, sinks=sinks.to(DEV))
    assert _debug.last_path() == "decode_paged"
    torch.cuda.synchronize()
    assert new.tolist() == [n + sq for n in lens]
    check_padded(out, sink_oracle(q, kg.cpu(), vg.cpu(), new.tolist(), sinks, True, w), F16)


# 9. one gpt-oss-shaped step under graph capture: the replay follows lengths, table and sinks updated in place
@pytest.mark.gpu
@pytest.mark.parametrize("w", [127, -1], ids=["window", "full"])
def test_gpt_oss_step_graph_capture(ops, device, w):
    fam = ops
    b, hq, hkv, page, cap, d = 4, 64, 8, 64, 512, 64
    q, _, _, kc, vc, table, sl = dv(*make_paged([cap] * b, hq, hkv, 1, page, cap, d, BF16, 31))
    sl.copy_(torch.tensor([300, 128, 5, 0], dtype=torch.int32))
    sinks = (2 * torch.randn(hq, generator=torch.Generator().manual_seed(10))).to(DEV)
    eager = fam.flash_attn_paged_func(q, kc, vc, table, sl, window_left=w, sinks=sinks)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fam.flash_attn_paged_func(q, kc, vc, table, sl, window_left=w, sinks=sinks)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and (out[3] == 0).all()
    sl.add_(1)
    table.copy_(table.flip(0))
    sinks.add_(1.5)
    g.replay()
    torch.cuda.synchronize()
    fresh = fam.flash_attn_paged_func(q, kc, vc, table, sl, window_left=w, sinks=sinks)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.equal(out, fresh) and not torch.equal(out, eager)


# 10. what a split windowed FP8 launch writes: its output and its workspace, nothing else (tests/footprint.py)
from test_footprint import abi  # noqa: E402,F401  (the fixture)


@pytest.mark.gpu
def test_sink_launch_writes_its_output_and_workspace_only(abi):  # noqa: F811
    import ctypes

    from test_footprint import _C, _I, _P, code, expect_path, paged_case
    from test_sink_abi import FaPagedFp8SinkParams

    w, dtype = 1000, BF16
    L, _, cpu, _, _ = paged_case(abi, "paged_window_fp8", "sq1_g4", 64, 128, dtype, window_left=w)
    assert L.need > 0
    sinks = make_sinks(cpu["q"], cpu["k"].float(), cpu["sl"].tolist(), 6, kd=cpu["kd"])
    sd = L.inp("sinks", sinks, dims=("head",))
    p = FaPagedFp8SinkParams(L.keep, sd.data_ptr())
    lib = abi.lib
    lib.fa_fwd_gfx950_paged_sink_fp8.argtypes = [_P, _C, _C, _I, _P, _I, _P]
    lib.fa_fwd_gfx950_paged_sink_fp8_workspace_size.argtypes = [_P, _C, _C, _I]
    lib.fa_fwd_gfx950_paged_sink_fp8_workspace_size.restype = _I
    assert lib.fa_fwd_gfx950_paged_sink_fp8_workspace_size(ctypes.byref(p), code(dtype), 0, w) == L.need
    ws = L.arena.buf.data_ptr() + L.ws_region.offset
    call = lambda: lib.fa_fwd_gfx950_paged_sink_fp8(ctypes.byref(p), code(dtype), 0, w, ws, L.need, abi.stream())  # noqa: E731
    (got,) = L.run(call, expect_path(abi, "decode_paged_fp8", split=True), split=True)
    ref = sink_oracle(cpu["q"], cpu["k"].float(), cpu["v"].float(), cpu["sl"].tolist(), sinks, False, w, kd=cpu["kd"],
                      vd=cpu["vd"])
    check_padded(got.reshape(cpu["q"].shape), ref, dtype)
