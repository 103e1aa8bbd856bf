"""softmax_scale and extreme logit ranges on every attention path, against a float64 softmax.

Why. Outside the dense prefill every GPU parity test runs at ``softmax_scale = D ** -0.5`` on inputs whose logits
stay within a few tens of log2 units of zero. The kernels' online softmax depends on two things no test varied: the
scale (threaded by hand through every op, multiplied by ``k_descale`` in the FP8 bodies, and the divisor of
``thr_raw = kRescaleThr / sc``) and the magnitude of the scores (the sentinel ``kNeg``, the first-key ``alpha``, the
merge weights ``exp2(m_w - M)`` of waves and splits).

The machinery is tests/test_edge_weight.py's, imported: its case builders (shapes, masks, sentinels, pools), its
``attend`` / ``excess`` / ``check_edge`` and its launch helpers. A case of this file is one of that file's cases
with the q / k / v generator swapped (``make``) and a scale of its own (``RangeCase``). Inputs are rounded to the io
dtype first; the yardstick is ``attend`` in float64 on the rounded values, under the elementwise bound of
tests/test_gpu_parity.py ``TOL`` -- NOT the C oracle, which at these ranges is itself under test (pinned against
``attend`` by the CPU self-tests below).

Families (``FAMS``; T in log2 units, ``u`` the fixed unit vector of test_edge_weight):

* ``off+300`` / ``off-300`` -- ``q = 0.25 randn + a u``, ``k = 0.25 randn +- a u``, ``a = sqrt(|T| / (scale log2e))``:
  every logit carries the common offset T over a spread of a few nats. T = -300 is the cold start: a row's first
  visible key gives ``exp2(0 - m sc) = 2^300``.
* ``steep_rise`` / ``steep_fall`` -- test_edge_weight's ramp at gamma 4: the running max moves ~185 log2 units per
  32-key tile, so every rescale's ``alpha`` underflows to 0, the later tiles of a fall have P exactly 0 and ~98 %
  of every row's weight sits on its edge key.
* ``hot`` -- the needle family with the needle's own logit at 200 nat instead of 14, on both sides of every 32-key
  tile boundary: whichever wave or split holds the needle, every other partial gets merge weight exactly 0.
* ``scale1`` / ``scale_quarter`` / ``scale_milli`` -- ``randn`` at ``softmax_scale`` 1.0 (``thr_raw`` 5.5 raw units
  under logits of sigma 16 log2 units: a near one-hot softmax, rescales on most tiles), 0.25 D^-0.5, and 1e-3
  (``thr_raw`` 5545: no rescale after the first key).
* ``off+300@1`` / ``off-300@1`` / ``slow@1`` -- the offsets and test_edge_weight's "slow" ramp rebuilt for a scale
  of 1.0 (``a`` and ``beta`` depend on it).

FP8 pools take power-of-two descales chosen per family so that K stays inside 448 descale (asserted by ``build``).

Bit-exact identities (section 3 below, ``torch.equal``): a power-of-two factor moved between q and the scale, between
``k_descale`` and the scale, or onto v / ``v_descale`` and the output commutes with every rounding in the kernels.
Elements whose result is a subnormal number of the io dtype are left out (rounding there does not commute with a
power of two); they must be under 1 % of the output.

The scale contract (``softmax_scale`` finite and > 0) is tested on the CPU in tests/test_abi.py, test_paged_abi.py,
test_fp8_abi.py, test_paged_window_abi.py, test_paged_prefill_abi.py and test_op_cpu.py.

CPU self-tests (``test_range_data_*``, not marked gpu), one representative per (case group, family, dtype): the honest
kernel model ``attend(..., emul=dtype)`` and the C oracle stay inside the bound against float64, the family's defining
property holds, and fp32 torch models of the mistakes this data is for leave the bound or go non-finite. Measured by
them over ``SELF``:
    honest model, max(err - bound) over every family:  fp16 -2.01e-3 .. -1.50e-3 (FP8 pools -2.00e-3 .. -1.42e-3);
        bf16 -1.61e-2 .. -1.30e-2 (FP8 pools -1.60e-2 .. -1.37e-2);  off+-1000: fp16 -1.87e-3, bf16 -1.53e-2
    C oracle against float64, max(err - bound):  fp16 -2.01e-3 .. -1.58e-3;  bf16 -1.61e-2 .. -1.30e-2
    steep: the max of consecutive 32-key tiles moves by 158 .. 177 log2 units (FP8 pools: 129 .. 174)
    offset: every logit within +-13.7 log2 units of T at the default scale (+-19.0 at T = +-1000), +-45.1 at scale 1.0
    hot: a visible needle holds > 0.999 of its row
    shifted edge, min over the affected rows of max(err - bound):  steep_rise 0.55, steep_fall 1.76, hot 1.93
    the default scale in place of the given one overshoots by >= 0.1 on 100 % (scale1), >= 91.9 % (scale_quarter)
        and >= 98.4 % (scale_milli) of the rows with 2 .. 512 keys; counting the 2047- and 2048-key rows too, on
        60 % in the 2048-key decode groups (see ``SEPARABLE_KEYS``)
(the bound is 2e-3 + 2e-3 |ref| for fp16 and 1.6e-2 + 1.6e-2 |ref| for bf16).
"""
from __future__ import annotations

import copy
import functools
import math

import pytest
import torch

import test_edge_weight as E
from test_edge_weight import (BF16, DEV, F16, FORMS, GUARDS, LENGTHS, MIN_OVERSHOOT, NAMES, PP_LENS, PREFILL_SHAPES,
                              SHORT_LENGTHS, VARLEN_LENS, Case, affected_rows, attend, check_edge, crc, dv, excess, pow2,
                              to_pool, unit, window_lens)
from test_edge_weight import dbg  # noqa: F401  (the fixture)
from test_fp8_kvcache import NAN_BYTE, quant
from test_kvcache import new_tokens
from test_padded import oracle_padded
from test_paged_window import free_pages_below_the_window

LOG2E = 1.4426950408889634
KNEG = -1e30  # the kernels' mask sentinel (csrc/fa_fwd_kernels.hpp kNeg)
HOT_LOGIT = 200.0  # nat: the needle's own logit in the "hot" family
STEEP_GAMMA = 4.0  # nat per key along the ramp: 32 gamma log2e ~ 185 log2 units per 32-key tile
DEFAULT = lambda d: d ** -0.5  # noqa: E731
# With randn v, the softmax of n keys at logit sigma 1 (the default scale) and the near-uniform one of the two small
# scales differ by ~sqrt((e - 1) / n) per element: ~0.23 at 32 keys, ~0.03 at 2048 -- above the bound, below
# MIN_OVERSHOOT. The 90 % share of rows that overshoot by MIN_OVERSHOOT is asked of the rows up to this many keys;
# 90 % of all rows with two keys or more must still leave the bound.
SEPARABLE_KEYS = 512


# ------------------------------------------------------------------------------------------------
# the families: generators with the signature of test_edge_weight.ramp_qkv after its family argument
# ------------------------------------------------------------------------------------------------
def offset_qkv(scale, t, b, bk, hq, hkv, sq, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    a = math.sqrt(abs(t) / (scale * LOG2E))
    q = 0.25 * torch.randn(b, hq, sq, d, generator=g) + a * unit(d)
    k = 0.25 * torch.randn(bk, hkv, n, d, generator=g) + math.copysign(a, t) * unit(d)
    return q, k, torch.randn(bk, hkv, n, d, generator=g)


def ramp_qkv(scale, s, gamma, b, bk, hq, hkv, sq, n, d, seed):
    """test_edge_weight.ramp_qkv at another gamma and scale: ``beta = gamma / (scale RAMP_A)``."""
    g = torch.Generator().manual_seed(seed)
    beta = gamma / (scale * E.RAMP_A)
    q = 0.25 * torch.randn(b, hq, sq, d, generator=g) + E.RAMP_A * unit(d)
    pos = torch.arange(n, dtype=torch.float32) - n / 2
    k = 0.25 * torch.randn(bk, hkv, n, d, generator=g) + s * beta * pos[:, None] * unit(d)
    return q, k, torch.randn(bk, hkv, n, d, generator=g)


def randn_qkv(scale, b, bk, hq, hkv, sq, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*s, generator=g) for s in ((b, hq, sq, d), (bk, hkv, n, d), (bk, hkv, n, d)))


GEN = {"offset": offset_qkv, "ramp": ramp_qkv, "randn": randn_qkv}
# family -> ((kind, its arguments ...), scale as a function of D)
FAMS = {
    "off+300": (("offset", 300.0), DEFAULT),
    "off-300": (("offset", -300.0), DEFAULT),
    "steep_rise": (("ramp", 1.0, STEEP_GAMMA), DEFAULT),
    "steep_fall": (("ramp", -1.0, STEEP_GAMMA), DEFAULT),
    "hot": (("needle",), DEFAULT),
    "scale1": (("randn",), lambda d: 1.0),
    "scale_quarter": (("randn",), lambda d: 0.25 * d ** -0.5),
    "scale_milli": (("randn",), lambda d: 1e-3),
    "off+300@1": (("offset", 300.0), lambda d: 1.0),
    "off-300@1": (("offset", -300.0), lambda d: 1.0),
    "slow@1": (("ramp", 1.0, 0.05), lambda d: 1.0),
    "randn": (("randn",), DEFAULT),  # (the identities' data; not one of ALL)
    "off+1000": (("offset", 1000.0), DEFAULT),  # (CPU self-tests only)
    "off-1000": (("offset", -1000.0), DEFAULT),
}
ALL = tuple(f for f in FAMS if f not in ("randn", "off+1000", "off-1000"))
SCALES = ("scale1", "scale_quarter", "scale_milli")
RAMP_GUARDS = {"steep_rise": GUARDS["rise"], "steep_fall": GUARDS["fall"], "hot": GUARDS["needle"]}
FAM = object()  # the place of the family argument in a call passed to ``make``


class RangeCase(Case):
    """A test_edge_weight Case with a scale of its own, judged against the float64 softmax."""

    @property
    def scale(self):
        return self.softmax_scale

    @functools.cached_property
    def ref(self):
        return attend(self.q, self.k, self.v, *self.lohi(), self.scale)[0].float()


def hot_needles(k, c, hq, dtype, scale):
    """test_edge_weight.set_needles at HOT_LOGIT and this scale."""
    b, hkv, n, d = k.shape
    kk = k.repeat_interleave(hq // hkv, 1)
    q = torch.gather(kk, 2, c[..., None].expand(-1, -1, -1, d)).float()
    return (q * (HOT_LOGIT / (scale * q.pow(2).sum(-1, keepdim=True)))).to(dtype)


def make(fam, case_fn, *args, **kw):
    """``case_fn(*args, **kw)`` -- a case builder of test_edge_weight, ``FAM`` standing where it takes its family --
    with this file's family: the builder runs with test_edge_weight's ramp generator swapped for the family's (so the
    shapes, masks, sentinel rows, FP8 round trip and needle placement stay that file's), "hot" takes its needle
    case and rescales the needle rows."""
    spec, scale_of = FAMS[fam]
    kind = spec[0]
    # (the family's name is part of the builder's seed; any name but "needle" reaches the swapped generator)
    args = [("needle" if kind == "needle" else fam) if a is FAM else a for a in args]
    theirs = E.ramp_qkv
    if kind != "needle":
        E.ramp_qkv = lambda _fam, *a: GEN[kind](scale_of(a[6]), *spec[1:], *a)  # a: (b, bk, hq, hkv, sq, n, d, seed)
    try:
        case = case_fn(*args, **kw)
    finally:
        E.ramp_qkv = theirs
    case.__class__ = RangeCase
    case.fam, case.kind, case.softmax_scale = fam, kind, scale_of(case.q.size(-1))
    if kind == "needle":
        case.q = hot_needles(case.k, case.c, case.q.size(1), case.dtype, case.scale)
    return case


def descales_for(fam, b, cap):
    """Distinct power-of-two (k, v) descales per (b, kv-head) that keep the family's K inside 448 descale: the
    steep ramps reach |k| ~ beta cap / 2 max|u|."""
    e = {256: 0, 2048: 3}[cap] if fam.startswith("steep") else -1
    return pow2(b, 2, e, e + 3), pow2(b, 2, -1, 2, 1)


def logits2(case):
    """[B, Hq, Sq, N] float64: every score of the buffer in log2 units (no mask)."""
    b, hq, sq, d = case.q.shape
    hkv = case.k.size(1)
    s = torch.matmul(case.q.reshape(b, hkv, -1, d).double(), case.k.double().transpose(-1, -2))
    return s.reshape(b, hq, sq, -1) * (case.scale * LOG2E)


def visible(case):
    lo, hi = case.lohi()
    pos = torch.arange(case.k.size(2))
    return ((pos >= lo[:, :, None]) & (pos < hi[:, :, None]))[:, None]  # [B, 1, Sq, N]


def check(out, case, *what):
    """check_edge against ``attend`` in float64; rows with no visible key are exactly 0."""
    lo, hi = case.lohi()
    got = out.detach().float().cpu()
    dead = (hi <= lo)[:, None, :, None].expand_as(got)
    assert (got[dead] == 0).all(), "a row with no visible key is not exactly 0"
    check_edge(out, case.ref, case.dtype, " ".join(str(x) for x in (case.fam, NAMES[case.dtype], *what)))


# ------------------------------------------------------------------------------------------------
# fp32 torch models of the mistakes this data is for
# ------------------------------------------------------------------------------------------------
def masked_logits(case):
    """fp32 [B, Hkv, g Sq, N] in log2 units, KNEG where masked; v [B, Hkv, N, D] fp32."""
    b, hq, sq, d = case.q.shape
    hkv = case.k.size(1)
    g = hq // hkv
    s = torch.matmul(case.q.reshape(b, hkv, g * sq, d).float(), case.k.float().transpose(-1, -2))
    s = s * (case.scale * LOG2E)
    vis = visible(case).repeat(1, 1, g, 1)
    return torch.where(vis, s, torch.tensor(KNEG)), case.v.float()


def online_model(case, tile=64, first_key_guard=True):
    """The tile-by-tile recurrence of the prefill bodies in fp32: ``m`` starts at the sentinel and ``msc`` at 0;
    ``first_key_guard=False`` is fa_fwd_w8 before its fix, ``alpha = exp2(0 - m sc)`` times O = l = 0 on a row's
    first visible key."""
    s, v = masked_logits(case)
    m = torch.full(s.shape[:-1], KNEG)
    msc, l = torch.zeros_like(m), torch.zeros_like(m)
    o = torch.zeros(*s.shape[:-1], v.size(-1))
    for j in range(0, s.size(-1), tile):
        sj = s[..., j:j + tile]
        m_new = torch.maximum(m, sj.amax(-1))
        msc_new = torch.where(m_new <= 0.5 * KNEG, torch.zeros_like(m), m_new)
        alpha = torch.exp2(msc - msc_new)
        if first_key_guard:
            alpha = torch.where(m <= 0.5 * KNEG, torch.zeros_like(m), alpha)
        p = torch.exp2(sj - msc_new[..., None])
        o = o * alpha[..., None] + torch.matmul(p, v[:, :, j:j + tile])
        l = l * alpha + p.sum(-1)
        m, msc = m_new, msc_new
    out = torch.where(l[..., None] > 0, o / l[..., None], torch.zeros(()))
    return out.reshape(case.q.shape).double()


def no_max_model(case):
    """A softmax without the max subtraction."""
    s, v = masked_logits(case)
    p = torch.exp2(s)
    return (torch.matmul(p, v) / p.sum(-1, keepdim=True)).reshape(case.q.shape).double()


def merge_model(case, mistake, tile=32):
    """Per-tile partials (max, sum, unnormalised O) merged as the decode kernels merge waves and splits.
    "own_l": each partial is normalised by its own l first, 0 / 0 where the partial saw no key. "no_guard": an
    empty partial reports the max 0 it started with and is weighted by ``exp2`` like the others, so it outvotes
    every partial whose scores are far below zero. None: the kernels' merge."""
    s, v = masked_logits(case)
    parts = []
    for j in range(0, s.size(-1), tile):
        sj = s[..., j:j + tile]
        mx = sj.amax(-1)
        empty = mx <= 0.5 * KNEG
        msc = torch.where(empty, torch.zeros_like(mx), mx)
        p = torch.exp2(sj - msc[..., None])
        parts.append((torch.where(empty, torch.tensor(0.0 if mistake == "no_guard" else KNEG), msc), empty,
                      p.sum(-1), torch.matmul(p, v[:, :, j:j + tile])))
    big = torch.stack([x[0] for x in parts]).amax(0)
    acc, tot = 0.0, 0.0
    for mw, empty, lw, ow in parts:
        w = torch.exp2(mw - big)
        if mistake is None:
            w = torch.where(empty, torch.zeros_like(w), w)
        if mistake == "own_l":
            ow = ow / lw[..., None] * lw[..., None]
        acc, tot = acc + w[..., None] * ow, tot + w * lw
    out = torch.where(tot[..., None] > 0, acc / tot[..., None], torch.zeros(()))
    return out.reshape(case.q.shape).double()


def leaves_the_bound(got, case):
    return (not torch.isfinite(got).all()) or excess(got, case.ref.double(), case.dtype).max().item() > 0


# ------------------------------------------------------------------------------------------------
# the cases, shared by the CPU self-tests and the GPU tests
# ------------------------------------------------------------------------------------------------
def fp8_decode_case(fam, lens, cap, sq, g, dtype, w=-1, tag=""):
    return make(fam, E.decode_case, lens, cap, sq, g, 128, dtype, FAM, w, descales=descales_for(fam, len(lens), cap),
                tag=tag)


def groups(fam, dt):
    """(group, thunk): one representative of every case group the GPU tests run this family through."""
    mk = functools.partial(functools.partial, make, fam)
    out = [
        ("prefill-d128", mk(E.prefill_case, PREFILL_SHAPES[0], 128, dt, True, FAM)),
        ("prefill-d64", mk(E.prefill_case, PREFILL_SHAPES[2], 64, dt, True, FAM)),
        ("prefill_full", mk(E.prefill_case, PREFILL_SHAPES[1], 128, dt, False, FAM)),
        ("layout", mk(E.prefill_case, (1, 8, 2, 200, 333), 128 if dt == F16 else 64, dt, True, FAM, piece_edges=True)),
        ("varlen-w40", mk(E.varlen_case, dt, True, FAM, 40)),
        ("varlen-full", mk(E.varlen_case, dt, False, FAM, -1)),
        ("padded37", mk(E.padded_case, 37, "mixed", dt, True, FAM)),
        ("padded1", mk(E.padded_case, 1, "left", dt, False, FAM)),
        ("window_prefill-w63", mk(E.prefill_case, (1, 4, 2, 300, 300), 128, dt, True, FAM, 63)),
        ("decode256", mk(E.decode_case, SHORT_LENGTHS, 256, 3, 4, 128, dt, FAM)),
        ("decode2048", mk(E.decode_case, LENGTHS, 2048, 1, 4, 128, dt, FAM)),
        ("decode2048_sq3-d64", mk(E.decode_case, LENGTHS, 2048, 3, 8, 64, dt, FAM)),
        ("window_decode_sq3-w100", mk(E.decode_case, window_lens(100, 3), 256, 3, 4, 128, dt, FAM, 100)),
        ("paged_prefill40-w64", mk(E.paged_prefill_case, 40, dt, True, FAM, 64)),
        ("paged_prefill300", mk(E.paged_prefill_case, 300, dt, False, FAM, -1)),
        ("fp8_decode256", functools.partial(fp8_decode_case, fam, SHORT_LENGTHS, 256, 1, 4, dt)),
        ("fp8_decode2048", functools.partial(fp8_decode_case, fam, LENGTHS, 2048, 3, 4, dt)),
        ("fp8_window_decode-w32", functools.partial(fp8_decode_case, fam, window_lens(32, 1), 256, 1, 4, dt, 32)),
    ]
    return out


SELF = [(f"{grp}-{fam}-{NAMES[dt]}", thunk) for dt in (F16, BF16) for fam in ALL for grp, thunk in groups(fam, dt)]
SELF += [(f"prefill-d128-{fam}-{NAMES[dt]}", functools.partial(make, fam, E.prefill_case, PREFILL_SHAPES[0], 128, dt, True, FAM))
         for dt in (F16, BF16) for fam in ("off+1000", "off-1000")]


@pytest.mark.parametrize("name,thunk", SELF, ids=[s[0] for s in SELF])
def test_range_data_can_fail_and_honest_arithmetic_passes(name, thunk):
    """For this (group, family, dtype): the honest kernel model and the C oracle stay inside the elementwise bound
    against float64; the family's defining property holds; the fp32 models of the mistakes the family is for leave
    the bound or go non-finite."""
    case = thunk()
    lo, hi = case.lohi()
    ref = case.ref.double()
    vis = visible(case)
    assert vis.any()
    oracle = oracle_padded(case.q, case.k, case.v, case.ks, case.ke, case.qs, case.qe, case.scale, case.causal,
                           window_left=case.w)
    o_margin = excess(oracle, ref, case.dtype).max().item()
    honest, p = attend(case.q, case.k, case.v, lo, hi, case.scale, emul=case.dtype)
    margin = excess(honest, ref, case.dtype).max().item()
    print(f"{name}: honest model max(err - bound) = {margin:.3e}, C oracle {o_margin:.3e}")
    assert torch.isfinite(oracle.float()).all() and o_margin <= 0
    assert torch.isfinite(honest).all() and margin <= 0
    for model in (online_model(case), merge_model(case, None)):  # (the guarded recurrences are themselves right)
        assert not leaves_the_bound(model, case)
    s2 = logits2(case)
    fam, kind = case.fam, case.kind
    if kind == "offset":
        t = FAMS[fam][0][1]
        # (the two a u . noise terms have sigma 0.25 sqrt(|T| scale log2e) log2 units each, 1.55 at the default
        # scale, and a row's and a key's extremes add. At scale 1.0 that sigma is 5.2, +-40 is 7.7 sigma of one
        # term and up to 45.1 was measured over these cases: +-60 there)
        spread = (s2 - t).abs().max().item()
        print(f"{name}: every logit within +-{spread:.1f} log2 units of {t:+.0f}")
        assert spread <= (60 if fam.endswith("@1") else 40), spread
        if t > 0:
            assert leaves_the_bound(no_max_model(case), case)  # (b)
        assert leaves_the_bound(online_model(case, first_key_guard=False), case) == (t < 0)  # (a)
    if fam.startswith("steep"):
        tiles = s2[..., :s2.size(-1) // 32 * 32].unflatten(-1, (-1, 32)).amax(-1)
        step = ((tiles[..., 1:] - tiles[..., :-1]) * FAMS[fam][0][1]).min().item()
        print(f"{name}: the running max moves by >= {step:.1f} log2 units per 32-key tile")
        assert step >= 128
    if kind == "needle":
        seen = (case.c >= lo[:, None]) & (case.c < hi[:, None])
        weight = torch.gather(p, 3, case.c[..., None])[..., 0]
        assert seen.any() and weight[seen].min().item() > 0.999, weight[seen].min().item()
    if fam.startswith("steep") or kind == "needle":  # (d), (e)
        # (a partial can only be empty where some 32-key tile of the buffer holds no key the row sees; an empty
        # partial's max of 0 can only outvote a row whose own scores all underflow against it)
        empty = ~visible(case).expand(-1, case.q.size(1), -1, -1)
        empty = torch.nn.functional.pad(empty, (0, -empty.size(-1) % 32), value=True).unflatten(-1, (-1, 32)).all(-1).any(-1)
        live = (hi > lo)[:, None]
        if (empty & live).any():
            assert leaves_the_bound(merge_model(case, "own_l"), case)
        cold = empty & live & (s2.masked_fill(~visible(case), -math.inf).amax(-1) < -160)
        if cold.any():
            assert leaves_the_bound(merge_model(case, "no_guard"), case)
        guarded = 0
        for shift, dlo, dhi in RAMP_GUARDS[fam]:
            rows = affected_rows(case, shift) if kind != "needle" else _needle_rows(case, shift)
            if not rows.any():
                continue
            moved, _ = attend(case.q, case.k, case.v, lo + dlo, hi + dhi, case.scale)
            over = excess(moved, ref, case.dtype).amax(-1)[rows].min().item()
            print(f"{name}: {shift}: {int(rows.sum())} rows, min overshoot {over:.3f}")
            assert over >= MIN_OVERSHOOT, (shift, over)
            guarded += 1
        assert guarded >= (2 if kind == "needle" else 1)
    if fam in SCALES:  # (c)
        wrong, _ = attend(case.q, case.k, case.v, lo, hi, DEFAULT(case.q.size(-1)))
        over = excess(wrong, ref, case.dtype).amax(-1)
        keys = (hi - lo)[:, None].expand(-1, case.q.size(1), -1)
        # (one key: softmax == 1 at any scale; of the others, nearly every row leaves the bound)
        assert (over[keys >= 2] > 0).float().mean().item() >= 0.9
        rows = (keys >= 2) & (keys <= SEPARABLE_KEYS)
        share = (over[rows] >= MIN_OVERSHOOT).float().mean().item()
        print(f"{name}: the default scale in place of {case.scale:.4g} overshoots by >= {MIN_OVERSHOOT} on "
              f"{100 * share:.1f} % of the rows with 2 .. {SEPARABLE_KEYS} keys, "
              f"{100 * (over[keys >= 2] >= MIN_OVERSHOOT).float().mean().item():.1f} % of all with two or more")
        assert share >= 0.9, share


def _needle_rows(case, shift):
    """test_edge_weight.affected_rows for a needle case under this file's family name."""
    twin = copy.copy(case)
    twin.fam = "needle"
    return affected_rows(twin, shift)


# ------------------------------------------------------------------------------------------------
# GPU: every family through every path, each asserting the path it took
# ------------------------------------------------------------------------------------------------
def launch_paged(dbg, case, pool, fuse=None):
    """test_edge_weight.paged_launch with the case's scale (that helper passes none)."""
    from flash_attention_cute_amd import flash_attn_paged_func

    kc, vc, table, sl = pool
    kw = {}
    if case.descales is not None:
        kw = dict(k_descale=case.descales[0].to(DEV), v_descale=case.descales[1].to(DEV))
    dbg.set_dec_fuse(fuse)
    try:
        out = flash_attn_paged_func(*dv(case.q, kc, vc, table, sl), softmax_scale=case.scale, causal=case.causal,
                                    window_left=case.w, **kw)
        labels = dbg.last_path(), dbg.last_dec_fused(), dbg.last_prefill_paged()
        torch.cuda.synchronize()
    finally:
        dbg.set_dec_fuse(None)
    return (out.cpu(), *labels)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("shape", PREFILL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prefill_ranges(dbg, shape, d, dtype):
    """flash_attn_func on fa_fwd_w4, causal and full."""
    from flash_attention_cute_amd import flash_attn_func

    for causal in (False, True):
        for fam in ALL:
            case = make(fam, E.prefill_case, shape, d, dtype, causal, FAM)
            out = flash_attn_func(*dv(case.q, case.k, case.v), softmax_scale=case.scale, causal=causal)
            assert dbg.last_path() == "w4"
            check(out, case, "causal" if causal else "full")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("layout,si", E.LAYOUT_CASES,
                         ids=[f"{lay}-{'x'.join(map(str, E.LAYOUT_SHAPES[si]))}" for lay, si in E.LAYOUT_CASES])
def test_prefill_ranges_under_forced_layouts(dbg, layout, si, dtype):
    """Zigzag, head-packed and key-split causal blocks, forced as test_prefill_edges_under_forced_layouts forces
    them: the key-split pieces merge partials whose maxima are hundreds of log2 units apart."""
    import flash_attention_cute_amd as m

    split, zigzag, head_pack = E.LAYOUT_KNOBS[layout]
    d = 128 if dtype == F16 else 64
    m.split_errors(reset=True)
    for fam in ALL:
        case = make(fam, E.prefill_case, E.LAYOUT_SHAPES[si], d, dtype, True, FAM, piece_edges=True)
        dbg.set_split(split)
        dbg.set_zigzag(zigzag)
        dbg.set_head_pack(head_pack)
        out = m.flash_attn_func(*dv(case.q, case.k, case.v), softmax_scale=case.scale, causal=True)
        assert dbg.last_path() == "w4"
        assert dbg.last_layout() == layout.split("_")[0], dbg.last_layout()
        assert dbg.last_head_pack() == ("headpack" in layout)
        torch.cuda.synchronize()
        check(out, case, layout)
    assert m.split_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ALL)
@pytest.mark.parametrize("variant", ["p8", "w8", "w4slow", "m32", "m16"])
def test_prefill_ranges_on_the_debug_bodies(dbg, variant, fam):
    """The other bodies with their own softmax recurrence, through _debug.forward. fa_fwd_w8 with ``off-300`` is the
    case that found its first-key ``alpha = exp2(0 - m sc)`` = +inf times O = 0."""
    dtype = BF16 if variant in ("w8", "m16") else F16
    try:
        for causal in (True, False):
            case = make(fam, E.prefill_case, PREFILL_SHAPES[0], 128, dtype, causal, FAM)
            out = dbg.forward(*dv(case.q, case.k, case.v), case.scale, causal, variant=variant)
            assert dbg.last_path(debug=True) == variant
            check(out, case, variant, "causal" if causal else "full")
    finally:
        dbg.set_knobs(debug=True)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_varlen_ranges(dbg, dtype, causal):
    """Packed sequences, causal / full / windowed: a neighbour's keys next door carry the same offsets and ramps."""
    from flash_attention_cute_amd import flash_attn_varlen_func

    cu = torch.tensor([0, 65, 66, 256], dtype=torch.int32)
    pack = lambda t: torch.cat([t[i, :, :n].transpose(0, 1) for i, n in enumerate(VARLEN_LENS)]).contiguous()  # noqa: E731
    for w in (-1, 0, 40):
        for fam in ALL:
            case = make(fam, E.varlen_case, dtype, causal, FAM, w)
            kp, vp = (t[0].transpose(0, 1).contiguous() for t in (case.k, case.v))
            out = flash_attn_varlen_func(*dv(pack(case.q), kp, vp, cu, cu), max(VARLEN_LENS), max(VARLEN_LENS),
                                         softmax_scale=case.scale, causal=causal, window_left=w)
            assert dbg.last_path() == "w4"
            check_edge(out, pack(case.ref), dtype, f"{fam} varlen w{w}")  # (every packed row sees a key)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("side", ["left", "right", "mixed"])
@pytest.mark.parametrize("sq", [37, 1])
def test_padded_ranges(dbg, sq, side, dtype):
    from flash_attention_cute_amd import flash_attn_padded_func

    for causal in (False, True):
        for fam in ALL:
            case = make(fam, E.padded_case, sq, side, dtype, causal, FAM)
            rng = (case.ks, case.ke) if sq == 1 else (case.ks, case.ke, case.qs, case.qe)
            out = flash_attn_padded_func(*dv(case.q, case.k, case.v, *rng), softmax_scale=case.scale, causal=causal)
            assert dbg.last_path() == ("decode" if sq == 1 else "w4")
            check(out, case, side)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 4, 2, 300, 300), (1, 4, 2, 40, 333)], ids=["300x300", "40x333"])
def test_window_prefill_ranges(dbg, shape, dtype):
    """The window mask of fa_fwd_w4: a row's first visible tile is not the block's first tile, so under ``off-300``
    the all-masked tiles before it must leave the cold start intact."""
    from flash_attention_cute_amd import flash_attn_window_func

    for w in (0, 63, 100):
        for fam in ALL:
            case = make(fam, E.prefill_case, shape, 128, dtype, True, FAM, w)
            out = flash_attn_window_func(*dv(case.q, case.k, case.v), w, softmax_scale=case.scale, causal=True)
            assert dbg.last_path() == "w4"
            check(out, case, f"w{w}")


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_rope_fused_scale(dbg, dtype, causal):
    """flash_attn_rope_func, the one op test_edge_weight does not drive, with the scale family only: the other
    families place their structure in q . k, which the rotation of q alone would scatter. The reference rotates q
    with the oracle of the stand-alone kernel (tests/test_rope.py: bit-exact with it)."""
    from flash_attention_cute_amd import flash_attn_rope_func
    from test_rope import oracle_rope, tables

    for fam in SCALES:
        for d in (128, 64):
            case = make(fam, E.prefill_case, PREFILL_SHAPES[0], d, dtype, causal, FAM)
            cos, sin = tables(1, case.q.size(2), d, dtype, crc("rope", fam, d))
            out = flash_attn_rope_func(*dv(case.q, case.k, case.v, cos, sin), softmax_scale=case.scale, causal=causal)
            assert dbg.last_path() == "w4"
            case.q = oracle_rope(case.q, cos, sin)
            check(out, case, "rope", d)


DEC_GEO = E.DEC_GEO


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("sq,g", DEC_GEO, ids=[f"sq{s}-g{g}" for s, g in DEC_GEO])
def test_dense_decode_ranges(dbg, sq, g, dtype):
    """flash_attn_func on few rows per kv-head, unsplit and split."""
    from flash_attention_cute_amd import flash_attn_func

    d = 128 if (sq + g) % 2 else 64
    for n in (33, 256, 2047, 2048):
        for fam in ALL:
            case = make(fam, E.decode_case, (n, n), n, sq, g, d, dtype, FAM)
            out = flash_attn_func(*dv(case.q, case.k, case.v), softmax_scale=case.scale, causal=case.causal)
            assert dbg.last_path() == ("decode_split" if n >= 2047 else "decode"), (n, dbg.last_path())
            check(out, case, n)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("sq,g", DEC_GEO, ids=[f"sq{s}-g{g}" for s, g in DEC_GEO])
@pytest.mark.parametrize("form", list(FORMS))
def test_padded_decode_ranges(dbg, form, sq, g, dtype):
    """seqlens against the capacity on the dense decode kernel, unsplit, fused and unfused: the wave merge and the
    split merge when one partial holds all the weight and the others' maxima are hundreds of log2 units below."""
    from flash_attention_cute_amd import flash_attn_padded_func

    lens, cap, fuse = FORMS[form]
    d = 64 if (sq + g) % 2 else 128
    for fam in ALL:
        case = make(fam, E.decode_case, lens, cap, sq, g, d, dtype, FAM)
        dbg.set_dec_fuse(fuse)
        out = flash_attn_padded_func(*dv(case.q, case.k, case.v, case.ks, case.ke), softmax_scale=case.scale,
                                     causal=case.causal)
        assert dbg.last_path() == ("decode" if form == "unsplit" else "decode_split")
        if form != "unsplit":
            assert dbg.last_dec_fused() == (fuse is None)
        check(out, case, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form,page,geo,dtype,layout", E.PAGED_DEC,
                         ids=[f"{f}-p{p}-sq{s}-g{g}-{NAMES[t]}" for f, p, (s, g), t, _ in E.PAGED_DEC])
def test_paged_decode_ranges(dbg, form, page, geo, dtype, layout):
    (sq, g), (lens, cap, fuse) = geo, FORMS[form]
    for fam in ALL:
        case = make(fam, E.decode_case, lens, cap, sq, g, 128, dtype, FAM)
        out, path, fused, _ = launch_paged(dbg, case, to_pool(case, lens, page, crc(form, page, fam), layout), fuse)
        assert path == ("decode_paged" if form == "unsplit" else "decode_paged_split")
        if form != "unsplit":
            assert fused == (fuse is None)
        check(out, case, form, page)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("form,page,sq,g", [("unsplit", 32, 1, 4), ("unsplit", 64, 3, 8), ("fused", 256, 1, 8),
                                            ("unfused", 64, 3, 4)])
def test_fp8_decode_ranges(dbg, form, page, sq, g, dtype):
    """The FP8 body, whose scale is ``softmax_scale * k_descale[b, h]``, with distinct power-of-two descales per (b,
    kv-head) (the reference reads the widened bytes times the descale: exact)."""
    lens, cap, fuse = FORMS[form]
    for fam in ALL:
        case = fp8_decode_case(fam, lens, cap, sq, g, dtype)
        out, path, fused, _ = launch_paged(dbg, case, to_pool(case, lens, page, crc("fp8", form, fam), "pshd"), fuse)
        assert path == ("decode_paged_fp8" if form == "unsplit" else "decode_paged_fp8_split")
        if form != "unsplit":
            assert fused == (fuse is None)
        check(out, case, form, "fp8")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("form", ["unsplit", "fused"])
def test_fp8_decode_with_descales_that_are_no_powers_of_two(dbg, form, dtype):
    """``softmax_scale = 1.0`` times k_descale 0.37, v_descale 1.9, as test_fp8_kvcache.fp8_oracle(..., pow2=False)
    folds them: k_descale into the reference's scale, v_descale onto its result (the kernel multiplies in fp32)."""
    lens, cap, fuse = FORMS[form]
    kd, vd = 0.37, 1.9
    case = make("scale1", E.decode_case, lens, cap, 1, 4, 128, dtype, FAM,
                descales=(torch.ones(len(lens), 2), torch.ones(len(lens), 2)))
    pool = to_pool(case, lens, 64, crc("fp8-nonpow2", form))
    case.descales = (torch.full((len(lens), 2), kd), torch.full((len(lens), 2), vd))
    out, path, _, _ = launch_paged(dbg, case, pool, fuse)
    assert path == ("decode_paged_fp8" if form == "unsplit" else "decode_paged_fp8_split")
    lo, hi = case.lohi()
    ref = attend(case.q, case.k, case.v, lo, hi, case.scale * float(torch.tensor(kd)))[0] * float(torch.tensor(vd))
    check_edge(out, ref.float(), dtype, f"fp8 descales ({kd}, {vd}) at scale 1.0, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("sq,page,dtype", [(1, 32, F16), (3, 64, BF16), (1, 64, BF16), (3, 32, F16)],
                         ids=["sq1-p32-f16", "sq3-p64-bf16", "sq1-p64-bf16", "sq3-p32-f16"])
def test_window_decode_ranges(dbg, sq, page, dtype, fp8):
    """The windowed paged decode: rows whose window starts in a later tile than row 0's meet an all-masked tile
    first. Then the same launch with the pages below the window freed: the same bits."""
    for w in (31, 100):
        lens = window_lens(w, sq)
        for fam in ALL:
            case = fp8_decode_case(fam, lens, 256, sq, 4, dtype, w) if fp8 else \
                make(fam, E.decode_case, lens, 256, sq, 4, 128, dtype, FAM, w)
            kc, vc, table, sl = to_pool(case, lens, page, crc("win", w, fam))
            out, path, _, _ = launch_paged(dbg, case, (kc, vc, table, sl))
            assert path == ("decode_paged_fp8" if fp8 else "decode_paged")
            check(out, case, f"w{w}", "fp8" if fp8 else "16bit")
            kc2, vc2, table2, freed = free_pages_below_the_window(kc, vc, table, lens, sq, w, page, -1,
                                                                  NAN_BYTE if fp8 else float("nan"))
            assert freed >= 2
            got, _, _, _ = launch_paged(dbg, case, (kc2, vc2, table2, sl))
            assert torch.isfinite(got.float()).all() and torch.equal(got, out)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq,page,dtype", [(40, 64, F16), (40, 128, BF16), (300, 64, BF16), (300, 128, F16)],
                         ids=["sq40-p64-f16", "sq40-p128-bf16", "sq300-p64-bf16", "sq300-p128-f16"])
def test_paged_prefill_ranges(dbg, sq, page, dtype, causal):
    """The paged fa_fwd_w4, with and without a window."""
    for w in (-1, 64):
        for fam in ALL:
            case = make(fam, E.paged_prefill_case, sq, dtype, causal, FAM, w)
            out, path, _, in_place = launch_paged(dbg, case, to_pool(case, PP_LENS, page, crc("pp", w, fam), "pshd"))
            assert path == "w4" and in_place
            check(out, case, f"w{w}", page)


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_with_kvcache_takes_the_scale(dbg, fp8):
    """One flash_attn_with_kvcache step (append, then the paged read) at ``softmax_scale = 1.0``, which the wrapper
    takes and passes on. No rotation, so the reference's q is the q given; its keys are the cache before the step
    with row L replaced on the host (the FP8 write formula for an FP8 pool)."""
    from flash_attention_cute_amd import flash_attention as fam

    lens, hq, hkv, page, cap, d, dtype = (70, 0, 33, 127, 63), 8, 2, 32, 128, 128, BF16
    b, g = len(lens), hq // hkv
    after = tuple(n + 1 for n in lens)
    ds = (pow2(b, hkv, -1, 2), pow2(b, hkv, -1, 2, 1)) if fp8 else None
    case = make("scale1", E.decode_case, after, cap, 1, g, d, dtype, FAM, descales=ds, tag="kvcache")
    kc, vc, table, _ = to_pool(case, after, page, 31)
    kn, vn = new_tokens(b, hkv, 1, d, dtype, 1), new_tokens(b, hkv, 1, d, dtype, 2)
    kw = dict(k_descale=ds[0].to(DEV), v_descale=ds[1].to(DEV)) if fp8 else {}
    out, new = fam.flash_attn_with_kvcache(*dv(case.q, kc, vc, kn, vn), cache_seqlens=torch.tensor(lens, dtype=torch.int32).to(DEV),
                                           block_table=table.to(DEV), softmax_scale=case.scale, causal=True,
                                           return_seqlens=True, **kw)
    assert dbg.last_path() == ("decode_paged_fp8" if fp8 else "decode_paged")
    torch.cuda.synchronize()
    assert new.tolist() == list(after)
    k_row, v_row = kn, vn
    if fp8:
        k_row = quant(kn, ds[0][:, :, None, None]).to(dtype) * ds[0][:, :, None, None].to(dtype)
        v_row = quant(vn, ds[1][:, :, None, None]).to(dtype) * ds[1][:, :, None, None].to(dtype)
    case.k, case.v = case.k.clone(), case.v.clone()
    for i, n in enumerate(lens):
        case.k[i, :, n], case.v[i, :, n] = k_row[i, :, 0], v_row[i, :, 0]
    check(out, case, "with_kvcache", "fp8" if fp8 else "16bit")
    wrong, _ = attend(case.q, case.k, case.v, *case.lohi(), d ** -0.5)
    assert excess(wrong, case.ref.double(), dtype).max().item() > MIN_OVERSHOOT  # (the default scale would show)


# ------------------------------------------------------------------------------------------------
# bit-exact rescaling identities: powers of two commute with every rounding in the kernels
# ------------------------------------------------------------------------------------------------
def _dense(dbg, c, op, **kw):
    out = op(*dv(c.q, c.k, c.v), softmax_scale=c.scale, causal=c.causal, **kw)
    return out.cpu()


def _run_prefill(dbg, c):
    from flash_attention_cute_amd import flash_attn_func

    out = _dense(dbg, c, flash_attn_func)
    assert dbg.last_path() == "w4"
    return out


def _run_w8(dbg, c):
    try:
        out = dbg.forward(*dv(c.q, c.k, c.v), c.scale, c.causal, variant="w8")
        assert dbg.last_path(debug=True) == "w8"
        return out.cpu()
    finally:
        dbg.set_knobs(debug=True)


def _run_varlen(dbg, c):
    from flash_attention_cute_amd import flash_attn_varlen_func

    cu = torch.tensor([0, 65, 66, 256], dtype=torch.int32)
    pack = lambda t: torch.cat([t[i, :, :n].transpose(0, 1) for i, n in enumerate(VARLEN_LENS)]).contiguous()  # noqa: E731
    kp, vp = (t[0].transpose(0, 1).contiguous() for t in (c.k, c.v))
    out = flash_attn_varlen_func(*dv(pack(c.q), kp, vp, cu, cu), max(VARLEN_LENS), max(VARLEN_LENS),
                                 softmax_scale=c.scale, causal=c.causal, window_left=c.w)
    assert dbg.last_path() == "w4"
    return out.cpu()


def _run_padded(dbg, c):
    from flash_attention_cute_amd import flash_attn_padded_func

    out = flash_attn_padded_func(*dv(c.q, c.k, c.v, c.ks, c.ke, c.qs, c.qe), softmax_scale=c.scale, causal=c.causal)
    assert dbg.last_path() == "w4"
    return out.cpu()


def _run_decode(path):
    def run(dbg, c):
        from flash_attention_cute_amd import flash_attn_func

        out = _dense(dbg, c, flash_attn_func)
        assert dbg.last_path() == path
        return out
    return run


def _run_paged(path, page, prefill=False):
    def run(dbg, c):
        lens = c.ke.tolist()
        out, got, _, in_place = launch_paged(dbg, c, to_pool(c, lens, page, 77, "pshd"))
        assert got == path and (in_place or not prefill)
        return out
    return run


# path -> (case thunk taking the dtype, runner)
IDENT = {
    "prefill": (lambda dt: make("randn", E.prefill_case, PREFILL_SHAPES[2], 128, dt, True, FAM), _run_prefill),
    "prefill_w8": (lambda dt: make("randn", E.prefill_case, PREFILL_SHAPES[0], 128, dt, True, FAM), _run_w8),
    "varlen": (lambda dt: make("randn", E.varlen_case, dt, True, FAM, 40), _run_varlen),
    "padded": (lambda dt: make("randn", E.padded_case, 37, "mixed", dt, True, FAM), _run_padded),
    "decode": (lambda dt: make("randn", E.decode_case, (256, 256), 256, 3, 4, 128, dt, FAM), _run_decode("decode")),
    "decode_split": (lambda dt: make("randn", E.decode_case, (2047, 2047), 2047, 1, 8, 128, dt, FAM),
                     _run_decode("decode_split")),
    "paged_decode": (lambda dt: make("randn", E.decode_case, LENGTHS, 2048, 3, 4, 128, dt, FAM),
                     _run_paged("decode_paged_split", 64)),
    "window_decode": (lambda dt: make("randn", E.decode_case, window_lens(100, 3), 256, 3, 4, 128, dt, FAM, 100),
                      _run_paged("decode_paged", 32)),
    "paged_prefill": (lambda dt: make("randn", E.paged_prefill_case, 40, dt, True, FAM, 64),
                      _run_paged("w4", 64, prefill=True)),
}
IDENT_FP8 = {
    "fp8_decode": (lambda dt: fp8_decode_case("randn", LENGTHS, 2048, 3, 4, dt), _run_paged("decode_paged_fp8_split", 64)),
    "fp8_window_decode": (lambda dt: fp8_decode_case("randn", window_lens(32, 1), 256, 1, 4, dt, 32),
                          _run_paged("decode_paged_fp8", 32)),
}


def variant(case, **kw):
    alt = copy.copy(case)
    alt.__dict__.pop("ref", None)
    alt.__dict__.update(kw)
    return alt


def times_pow2(x, j, dtype):
    """2^j x in the io dtype, asserted exact."""
    y = x.float() * 2.0 ** j
    assert torch.equal(y.to(dtype).float(), y), f"2^{j} x is not exact in {dtype}"
    return y.to(dtype)


def assert_pow2_of(scaled, base, j, dtype, what):
    """scaled == 2^j base bit for bit wherever both are normal numbers of the io dtype (or 0): a subnormal result has
    lost bits that the other side keeps. Such elements must be rare, and stay within one subnormal step."""
    fi = torch.finfo(dtype)
    want = base.float() * 2.0 ** j
    assert torch.isfinite(scaled.float()).all() and want.abs().max().item() <= fi.max, what
    normal = ((base.float().abs() >= fi.tiny) & (want.abs() >= fi.tiny)) | (base == 0)
    assert normal.float().mean().item() > 0.99, (what, normal.float().mean().item())
    assert torch.equal(scaled.float()[normal], want[normal]), what
    step = fi.tiny * fi.eps * max(1.0, 2.0 ** j)
    assert ((scaled.float() - want).abs() <= step).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("path", list(IDENT))
def test_a_power_of_two_moves_between_q_and_the_scale(dbg, path, dtype):
    """op(2^j q, k, v, scale 2^-j) == op(q, k, v, scale), j in {-3, 5}: the scores, ``sc`` and ``thr_raw = 8 / sc``
    scale exactly, so every comparison and every exp2 argument is the same. fp16 q is put on a 2^-10 grid first, so
    that 2^-3 q has no subnormal element."""
    thunk, run = IDENT[path]
    case = thunk(dtype)
    case.q = ((case.q.float() * 1024).round() / 1024).to(dtype)
    base = run(dbg, case)
    assert torch.isfinite(base.float()).all() and base.float().abs().max().item() > 0
    for j in (-3, 5):
        got = run(dbg, variant(case, q=times_pow2(case.q, j, dtype), softmax_scale=case.scale * 2.0 ** -j))
        assert torch.equal(got, base), (path, j)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("path", list(IDENT))
def test_a_power_of_two_on_v_comes_out_on_the_output(dbg, path, dtype):
    """op(q, k, 2^j v) == 2^j op(q, k, v): fp16 j = 13 with V clamped to +-7 (7 * 2^13 < 65504), bf16 j = +-60."""
    thunk, run = IDENT[path]
    case = thunk(dtype)
    if dtype == F16:
        case.v = case.v.clamp(-7, 7)
    base = run(dbg, case)
    for j in ((13,) if dtype == F16 else (60, -60)):
        got = run(dbg, variant(case, v=times_pow2(case.v, j, dtype)))
        assert_pow2_of(got, base, j, dtype, (path, j))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("path", list(IDENT_FP8))
def test_a_power_of_two_moves_between_the_descales_the_scale_and_the_output(dbg, path, dtype):
    """FP8: ``sc = softmax_scale * k_descale`` is one fp32 product, exact under 2^j on one factor and 2^-j on the
    other; ``v_descale 2^j`` comes out as 2^j on the output."""
    thunk, run = IDENT_FP8[path]
    case = thunk(dtype)
    kd, vd = case.descales
    base = run(dbg, case)
    assert torch.isfinite(base.float()).all() and base.float().abs().max().item() > 0
    for j in (-3, 5):
        got = run(dbg, variant(case, descales=(kd * 2.0 ** j, vd), softmax_scale=case.scale * 2.0 ** -j))
        assert torch.equal(got, base), (path, "k_descale", j)
        got = run(dbg, variant(case, descales=(kd, vd * 2.0 ** j)))
        assert_pow2_of(got, base, j, dtype, (path, "v_descale", j))
