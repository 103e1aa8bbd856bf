"""LSE output of the paged split-KV decode and the merge of partial attention states
(include/fa_gfx950_lse.h; ``flash_attn_paged_func(return_lse=True)``, ``flash_attn_merge_states``).

No reference counterpart. What is pinned here:

* O of the LSE kernels equals ``flash_attn_paged_func``'s BIT FOR BIT -- unsplit, split with the fused merge,
  split with the separate combine launch, 16-bit and FP8 pools;
* the LSE is ``ln sum_n exp(scale q . k_n)`` over a row's visible keys in natural log units, ``-inf`` for a
  row without one, within 2^-12 ABSOLUTE of a float64 logsumexp over the same (16-bit or widened e4m3)
  inputs. The bound is a condition, not a measurement: an LSE error eps moves a merge weight by a factor
  e^eps, and 2^-12 keeps that under half an fp16 output ulp. Each case prints the error it measured;
* the merge kernel against a float64 merge of the same 16-bit partials within tests/test_gpu_parity.py TOL
  (fp16 2e-3 + 2e-3|ref|, bf16 1.6e-2 + 1.6e-2|ref|), its LSE within 2^-12, with -inf parts, all -inf rows
  and a strided input.

The cases follow tests/test_paged.py (``make_paged``: shuffled table, NaN-poisoned pool, -1 in unused entries).
"""
from __future__ import annotations

import functools
import math
import warnings

import pytest
import torch

from test_fp8_kvcache import make_fp8_paged, pow2_descales
from test_paged import KINDS, make_paged

F16, BF16 = torch.float16, torch.bfloat16
LSE_TOL = 2.0 ** -12
NEG_INF = float("-inf")


def lse_oracle(q, k, lens, scale, causal, kd=None):
    """float64 logsumexp of scale * q . k over each row's visible keys (bottom-right causal per sequence); k
    dense [B, Hkv, cap, D] (widened bytes for an FP8 pool, kd [B, Hkv] then scales the logits); -inf without keys."""
    b, hq, sq, _ = q.shape
    g = hq // k.size(1)
    out = torch.full((b, hq, sq), NEG_INF, dtype=torch.float64)
    for i, n in enumerate(lens):
        if n == 0:
            continue
        kb = k[i, :, :n].double().repeat_interleave(g, dim=0)
        s = torch.matmul(q[i].double(), kb.transpose(1, 2)) * scale
        if kd is not None:
            s = s * kd[i].double().repeat_interleave(g)[:, None, None]
        if causal:
            key, pos = torch.arange(n)[None, :], torch.arange(sq)[:, None]
            s = s.masked_fill((key > pos + n - sq)[None], NEG_INF)
        out[i] = torch.logsumexp(s, dim=-1)
    return out


def check_lse(lse, ref, what=""):
    """-inf exactly where the oracle has it; every other value within 2^-12 absolute. Returns the max error."""
    lse = lse.double().cpu()
    empty = ref == NEG_INF
    assert torch.equal(lse == NEG_INF, empty), f"{what}: -inf rows differ"
    assert torch.isfinite(lse[~empty]).all()
    err = (lse[~empty] - ref[~empty]).abs().max().item() if (~empty).any() else 0.0
    print(f"LSE_ERR {what} max_abs_err={err:.3e} bound={LSE_TOL:.3e} max_abs_lse={ref[~empty].abs().max().item() if (~empty).any() else 0:.2f}")
    assert err <= LSE_TOL, f"{what}: lse error {err:.3e} exceeds 2^-12"
    return err


# ------------------------------------------------------------------------------------------- CPU
def test_lse_ops_registration_and_fakes():
    import flash_attention_cute_amd  # noqa: F401

    ops = torch.ops.flash_attention
    assert str(ops.paged_forward_lse.default._schema) == (
        "flash_attention::paged_forward_lse(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, "
        "Tensor? cache_seqlens, SymInt seqlen_offset=0, float softmax_scale=None, bool causal=False) -> (Tensor, Tensor)")
    assert str(ops.paged_forward_lse_fp8.default._schema) == (
        "flash_attention::paged_forward_lse_fp8(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, "
        "Tensor? cache_seqlens, Tensor? k_descale=None, Tensor? v_descale=None, SymInt seqlen_offset=0, "
        "float softmax_scale=None, bool causal=False) -> (Tensor, Tensor)")
    assert str(ops.merge_states.default._schema) == (
        "flash_attention::merge_states(Tensor outs, Tensor lses, bool return_lse=False) -> (Tensor, Tensor)")
    # the existing schemas did not move
    for old in (ops.paged_forward, ops.paged_forward_fp8):
        assert "seqlen_offset" not in str(old.default._schema) and str(old.default._schema).endswith("-> Tensor")
    q, _, _, kc, vc, table, lens = make_paged((40, 7), 4, 2, 2, 32, 64, 32, torch.float32, 1)
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)
    outs, lses = torch.randn(2, 2, 4, 2, 32).half(), torch.randn(2, 2, 4, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for args in ((q, kc, vc, table, lens, 0, 0.125, True), (q, kc, vc, table, None, 33, 0.125, False)):
            torch.library.opcheck(ops.paged_forward_lse.default, args, test_utils=("test_schema", "test_faketensor"))
        for rl in (False, True):
            torch.library.opcheck(ops.merge_states.default, (outs, lses, rl), test_utils=("test_schema", "test_faketensor"))
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        fq = torch.empty(3, 8, 2, 64, dtype=BF16)
        fk = torch.empty(9, 2, 32, 64, dtype=BF16)
        o, l = ops.paged_forward_lse(fq, fk, fk, torch.empty(3, 3, dtype=torch.int32), torch.empty(3, dtype=torch.int32))
        assert o.shape == fq.shape and o.dtype == BF16 and l.shape == (3, 8, 2) and l.dtype == torch.float32
        f8 = torch.empty(9, 2, 32, 64, dtype=torch.float8_e4m3fn)
        o, l = ops.paged_forward_lse_fp8(fq, f8, f8, torch.empty(3, 3, dtype=torch.int32), None)
        assert o.shape == fq.shape and o.dtype == BF16 and l.shape == (3, 8, 2) and l.dtype == torch.float32
        o, l = ops.merge_states(torch.empty(3, 2, 4, 1, 64, dtype=F16), torch.empty(3, 2, 4, 1), True)
        assert o.shape == (2, 4, 1, 64) and o.dtype == F16 and l.shape == (2, 4, 1) and l.dtype == torch.float32


def test_new_functions_are_exported():
    import flash_attention_cute_amd as m

    for name in ("flash_attn_merge_states", "flash_attn_paged_shared_prefix_func", "flash_attention_merge_states",
                 "flash_attention_paged_forward_lse", "flash_attention_paged_forward_lse_fp8"):
        assert name in m.__all__ and hasattr(m, name)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq", [1, 3])
def test_lse_op_cpu_default_matches_float64(causal, sq):
    from flash_attention_cute_amd import flash_attn_paged_func
    from test_padded import oracle_padded

    lens, hq, hkv, page, cap, d = (96, 0, 33, 1, 64), 4, 2, 32, 96, 64
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, F16, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, lse = flash_attn_paged_func(q.float(), kc.float(), vc.float(), table, sl, causal=causal, return_lse=True)
        plain = flash_attn_paged_func(q.float(), kc.float(), vc.float(), table, sl, causal=causal)
        # the two length options: clamp(lens + offset), and clamp(offset) without lens
        _, lse_off = torch.ops.flash_attention.paged_forward_lse(q.float(), kc.float().nan_to_num(0), vc.float().nan_to_num(0),
                                                                 table, sl, -32, d ** -0.5, causal)
        _, lse_all = torch.ops.flash_attention.paged_forward_lse(q[:1].float(), kc.float().nan_to_num(0), vc.float().nan_to_num(0),
                                                                 table[:1, :1], None, 32, d ** -0.5, causal)
    assert torch.isfinite(out).all()
    ref = oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, causal).float()
    torch.testing.assert_close(out, ref, atol=3e-3, rtol=3e-3)
    torch.testing.assert_close(out, plain, atol=1e-5, rtol=1e-5)
    want = lse_oracle(q, k, lens, d ** -0.5, causal)
    assert torch.equal(lse == NEG_INF, want == NEG_INF)
    torch.testing.assert_close(lse.double()[want != NEG_INF], want[want != NEG_INF], atol=1e-4, rtol=0)
    want_off = lse_oracle(q, k, [max(n - 32, 0) for n in lens], d ** -0.5, causal)
    torch.testing.assert_close(lse_off.double().nan_to_num(neginf=-1e9), want_off.nan_to_num(neginf=-1e9), atol=1e-4, rtol=0)
    want_all = lse_oracle(q[:1], k[:1], [32], d ** -0.5, causal)
    torch.testing.assert_close(lse_all.double(), want_all, atol=1e-4, rtol=0)


def test_lse_fp8_op_cpu_default_matches_float64():
    from flash_attention_cute_amd import flash_attn_paged_func

    lens, hq, hkv, page, cap, d = (96, 0, 33), 4, 2, 32, 96, 64
    kd, vd = pow2_descales(3, hkv), pow2_descales(3, hkv, 1)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, 1, page, cap, d, BF16, 5, kd=kd, vd=vd)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, lse = flash_attn_paged_func(q, kc8, vc8, table, sl, k_descale=kd, v_descale=vd, return_lse=True)
        plain = flash_attn_paged_func(q, kc8, vc8, table, sl, k_descale=kd, v_descale=vd)
    torch.testing.assert_close(out.float(), plain.float(), atol=2e-2, rtol=2e-2)
    want = lse_oracle(q, k8.float(), lens, d ** -0.5, False, kd)
    assert torch.equal(lse == NEG_INF, want == NEG_INF)
    torch.testing.assert_close(lse.double()[want != NEG_INF], want[want != NEG_INF], atol=1e-4, rtol=0)


def merge_oracle(outs, lses):
    """float64 merge of the given partials: (out, lse)."""
    l = lses.double()
    mx = l.max(dim=0).values
    w = torch.exp(l - mx.masked_fill(mx == NEG_INF, 0))
    sw = w.sum(dim=0)
    o = (w[..., None] * outs.double()).sum(dim=0) / sw.masked_fill(sw == 0, 1)[..., None]
    return o.masked_fill((sw == 0)[..., None], 0), (mx + torch.log(sw)).masked_fill(sw == 0, NEG_INF)


def make_states(n, b, h, s, d, dtype, seed):
    """n partial states; row (0, 0, 0) has every part -inf, rows (b > 0, h = 1) have part 0 -inf, row (b, 2) only
    part n - 1 finite."""
    g = torch.Generator().manual_seed(seed)
    outs = torch.randn(n, b, h, s, d, generator=g).to(dtype)
    lses = (4.0 * torch.randn(n, b, h, s, generator=g)).float()
    lses[:, 0, 0, 0] = NEG_INF
    lses[0, 1:, 1] = NEG_INF
    lses[:n - 1, :, 2] = NEG_INF
    return outs, lses


@pytest.mark.parametrize("n", [1, 2, 3, 16])
def test_merge_op_cpu_default_matches_float64(n):
    from flash_attention_cute_amd import flash_attn_merge_states

    outs, lses = make_states(n, 2, 4, 2, 64, F16, 7 + n)
    o, l = flash_attn_merge_states(outs, lses, return_lse=True)
    ro, rl = merge_oracle(outs, lses)
    torch.testing.assert_close(o.double(), ro, atol=2e-3, rtol=2e-3)
    assert torch.equal(l == NEG_INF, rl == NEG_INF) and (o[0, 0, 0] == 0).all()
    torch.testing.assert_close(l.double()[rl != NEG_INF], rl[rl != NEG_INF], atol=1e-5, rtol=0)
    o2 = flash_attn_merge_states(list(outs), list(lses))  # sequences of tensors, and no lse
    assert torch.equal(o2, o)


def test_lse_wrapper_errors():
    from flash_attention_cute_amd import flash_attn_merge_states, flash_attn_paged_func

    q, _, _, kc, vc, table, sl = make_paged((40, 7), 8, 2, 1, 32, 64, 64, F16, 1)
    with pytest.raises(NotImplementedError, match="window"):
        flash_attn_paged_func(q, kc, vc, table, sl, window_left=5, return_lse=True)
    big = torch.zeros(2, 8, 17, 64, dtype=F16)  # g 4 x Sq 17 = 68 rows
    with pytest.raises(NotImplementedError, match="decode shapes"):
        flash_attn_paged_func(big, kc, vc, table, sl, return_lse=True)
    with pytest.raises(ValueError, match="1 to 16"):
        flash_attn_merge_states(torch.zeros(17, 1, 1, 1, 8, dtype=F16), torch.zeros(17, 1, 1, 1))
    with pytest.raises(ValueError, match="multiple of 8"):
        flash_attn_merge_states(torch.zeros(2, 1, 1, 1, 12, dtype=F16), torch.zeros(2, 1, 1, 1))
    with pytest.raises(ValueError, match="outs must be"):
        flash_attn_merge_states(torch.zeros(2, 1, 1, 1, 8, dtype=F16), torch.zeros(2, 1, 1, 2))


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def ops(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam
    from flash_attention_cute_amd import flash_attn_merge_states, flash_attn_paged_func

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    _debug.set_dec_fuse(None)
    yield flash_attn_paged_func, flash_attn_merge_states, _debug
    _debug.set_dec_fuse(None)


# (kind of tests/test_paged.py KINDS, page_size, D, dtype, lengths): page 32 and 64, D 64 / 72 / 128 and both dtypes
# across the list; lengths 0, 1, 31, 32, 33, 256 for the unsplit kind, (2048, 33) for the split ones
CASES = [
    ("unsplit", 32, 128, F16, (0, 1, 31)),
    ("unsplit", 64, 64, BF16, (32, 33, 256)),
    ("unsplit", 64, 72, F16, (256, 0, 33)),
    ("split", 32, 128, BF16, (2048, 33)),
    ("split", 64, 64, F16, (2048, 33)),
    ("split_unfused", 32, 72, F16, (2048, 33)),
    ("split_unfused", 64, 128, BF16, (2048, 33)),
    ("sq3_causal", 32, 128, F16, (0, 1, 33)),
    ("sq3_causal", 64, 72, BF16, (31, 32, 256)),
    ("g8_sq5", 32, 64, F16, (31, 32, 256)),
    ("g8_sq5", 64, 128, BF16, (4, 33, 0)),
]
CASE_IDS = [f"{k}-p{p}-d{d}-{'f16' if t == F16 else 'bf16'}" for k, p, d, t, _ in CASES]


@functools.lru_cache(maxsize=None)
def run_case(ci):
    """The LSE launch, the launch without it and the float64 lse, once per case (never modified)."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    kind, page, d, dtype, lens = CASES[ci]
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 300 + ci)
    dv = lambda t: t.to("cuda:0")  # noqa: E731
    _debug.set_knobs()
    _debug.set_dec_fuse(0 if kind == "split_unfused" else None)
    try:
        out, lse = flash_attn_paged_func(dv(q), dv(kc), dv(vc), dv(table), dv(sl), causal=causal, return_lse=True)
        path, fused = _debug.last_path(), _debug.last_dec_fused()
        plain = flash_attn_paged_func(dv(q), dv(kc), dv(vc), dv(table), dv(sl), causal=causal)
        plain_path = _debug.last_path()
        torch.cuda.synchronize()
    finally:
        _debug.set_dec_fuse(None)
    return out.cpu(), lse.cpu(), plain.cpu(), path, fused, plain_path, lse_oracle(q, k, lens, d ** -0.5, causal)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_lse_kernel_output_is_bit_identical_and_lse_matches_float64(ops, ci):
    kind = CASES[ci][0]
    out, lse, plain, path, fused, plain_path, ref = run_case(ci)
    split = kind.startswith("split")
    assert path == plain_path == ("decode_paged_split" if split else "decode_paged")
    if split:
        assert fused == (kind == "split")
    assert lse.dtype == torch.float32 and lse.shape == out.shape[:3]
    assert torch.isfinite(out.float()).all() and torch.equal(out, plain)
    check_lse(lse, ref, CASE_IDS[ci])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["unsplit", "split", "split_unfused"])
def test_lse_fp8_pool(ops, device, kind):
    """An FP8 pool with descales != 1: k_descale is part of the scale, v_descale is not part of the lse."""
    paged, _, _debug = ops
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    lens = (2048, 33) if b == 2 else (256, 0, 33)
    kd, vd = pow2_descales(b, hkv), pow2_descales(b, hkv, 2)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, sq, 64, cap, 128, BF16, 41, kd=kd, vd=vd)
    dv = lambda t: t.to(device)  # noqa: E731
    _debug.set_dec_fuse(0 if kind == "split_unfused" else None)
    out, lse = paged(dv(q), dv(kc8), dv(vc8), dv(table), dv(sl), k_descale=dv(kd), v_descale=dv(vd), return_lse=True)
    path = _debug.last_path()
    plain = paged(dv(q), dv(kc8), dv(vc8), dv(table), dv(sl), k_descale=dv(kd), v_descale=dv(vd))
    assert path == _debug.last_path() == ("decode_paged_fp8" if kind == "unsplit" else "decode_paged_fp8_split")
    assert torch.isfinite(out.float()).all() and torch.equal(out, plain)
    check_lse(lse, lse_oracle(q, k8.float(), lens, 128 ** -0.5, causal, kd), f"fp8-{kind}")


@pytest.mark.gpu
def test_lse_length_options(ops, device):
    """seqlen_offset and a missing cache_seqlens give the bits of the explicit lengths (table entries past the
    shortened sequences are then unused: poisoned)."""
    from flash_attention_cute_amd import flash_attn_paged_func  # noqa: F401

    lens, hq, hkv, page, cap, d = (200, 64, 31), 8, 2, 32, 256, 128
    q, _, _, kc, vc, table, sl = (t.to(device) for t in make_paged(lens, hq, hkv, 1, page, cap, d, F16, 77))
    op = torch.ops.flash_attention.paged_forward_lse
    for off in (-64, -31, -1, -1000):  # (a positive offset would reach the poisoned rows past each sequence's end)
        want_o, want_l = op(q, kc, vc, table, (sl + off).clamp(min=0), 0, d ** -0.5, False)
        o, l = op(q, kc, vc, table, sl, off, d ** -0.5, False)
        assert torch.equal(o, want_o) and torch.equal(l, want_l), off
    o, l = op(q, kc, vc, table, None, 31, d ** -0.5, False)
    want_o, want_l = op(q, kc, vc, table, torch.full_like(sl, 31), 0, d ** -0.5, False)
    assert torch.equal(o, want_o) and torch.equal(l, want_l) and torch.isfinite(l).all()


MERGE_CASES = [(2, 64, F16), (2, 128, BF16), (3, 72, F16), (3, 128, F16), (2, 72, BF16), (3, 64, BF16)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,dtype", MERGE_CASES, ids=[f"n{n}-d{d}-{'f16' if t == F16 else 'bf16'}" for n, d, t in MERGE_CASES])
@pytest.mark.parametrize("layout", ["bhsd", "bshd"])
def test_merge_kernel_matches_float64(ops, device, n, d, dtype, layout):
    from test_padded import check_padded

    _, merge, _ = ops
    b, h, s = 3, 5, 2
    outs, lses = make_states(n, b, h, s, d, dtype, 900 + n + d)
    if layout == "bshd":  # a transposed view: head stride D, seq stride H * D
        dev_outs = outs.transpose(2, 3).contiguous().to(device).transpose(2, 3)
        dev_lses = lses.transpose(2, 3).contiguous().to(device).transpose(2, 3)
        assert not dev_outs.is_contiguous()
    else:
        dev_outs, dev_lses = outs.to(device), lses.to(device)
    o, l = merge(dev_outs, dev_lses, return_lse=True)
    o_only = merge(dev_outs, dev_lses)
    ro, rl = merge_oracle(outs, lses)
    assert torch.equal(o, o_only)
    check_padded(o, ro, dtype)
    assert (o[0, 0, 0] == 0).all()  # every part -inf
    check_lse(l, rl, f"merge-n{n}-d{d}-{layout}")
    # a part that weighs 0 leaves the other parts' result: rows (b > 0, h = 1) are the merge of parts 1..
    if n == 2:
        assert torch.equal(o[1:, 1].cpu(), outs[1, 1:, 1])


@pytest.mark.gpu
def test_two_key_sets_merge_to_the_whole(ops, device):
    """The LSE decode over two disjoint key sets (a prefix of whole pages and the rest), merged, equals the
    decode over all keys within the parity bound, and its lse within 2^-12."""
    from test_padded import check_padded, oracle_padded

    paged, merge, _ = ops
    lens, hq, hkv, page, cap, d = (200, 129, 128), 8, 2, 64, 256, 128
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, 1, page, cap, d, F16, 55)
    dq, dkc, dvc, dt, dsl = (t.to(device) for t in (q, kc, vc, table, sl))
    op = torch.ops.flash_attention.paged_forward_lse
    o1, l1 = op(dq, dkc, dvc, dt[:, :2], None, 128, d ** -0.5, False)
    o2, l2 = op(dq, dkc, dvc, dt[:, 2:], dsl, -128, d ** -0.5, False)
    o, l = merge([o1, o2], [l1, l2], return_lse=True)
    check_padded(o, oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, False), F16)
    check_lse(l, lse_oracle(q, k, lens, d ** -0.5, False), "two-sets")
    assert (l2[2] == NEG_INF).all() and (o2[2] == 0).all()  # the third sequence has no suffix
