"""Mask edges that carry weight: needle and ramp inputs for every kernel body, against the CPU oracle.

Why. The other GPU parity tests draw q, k and v from ``randn``. At D = 128 the softmax is then diffuse, one key
holds O(1 / Sk) of a row's weight, and tests/test_gpu_parity.py ``TOL`` (sized for honest rounding) is wider than
one key's contribution: a kernel that gains or drops one key at a mask edge can pass. The data here gives the key
AT each edge a large share of the softmax, so a gained or lost key moves the output by O(|v|).

Two input families (plain seeded functions, CPU tensors; ``build``):

* needle -- k, v ``randn``; every query row (b, q-head, m) is the stored key ``k[b, kv-head, c]`` of a position
  ``c`` the test chooses, rounded as stored and scaled so that its own logit is 14 (``NEEDLE_LOGIT``; x ~1.24 at
  D = 128, x ~1.75 at D = 64 -- the plain key's ~11.3 / ~8 left a short key among 2048 others at 87 % of the
  weight); for an FP8 pool the key is the widened byte row times ``k_descale``; for the RoPE-fused append the
  rotated key. Noise has sigma ~1.2 - 1.75, so the row's output is ~``v[c]`` when ``c`` is visible. The rows of
  one launch take, in turn (``assign_needles``): the last visible key, the key one past it, the first visible
  key, the key one below it, then a list of absolute positions (tile, page and piece boundaries 32j - 1 / 32j,
  64j - 1 / 64j). Keys that exist in the buffer and belong to nobody (rows outside ``[k_start, k_end)``, rows
  below every row's decode window) hold V = 8 in every dim; a neighbour sequence's keys in a packed batch and
  the NaN rows of a pool stay what they are.
* ramp -- ``q = 0.25 randn + 8 u``, ``k[n] = 0.25 randn + s beta (n - N / 2) u`` with u a fixed unit vector,
  ``beta = gamma / (8 scale)`` and n the PHYSICAL position in the buffer (the packed index for varlen), v
  ``randn``. "rise" (s = +1, gamma 0.7) puts ~1 - e^-0.7 of EVERY row's weight on its last visible key (right
  edges: the causal diagonal, the length, ``k_end``) and lets a neighbour past the edge outscore everything
  visible; "fall" (s = -1) does the same for left edges (the window, ``k_start``). gamma 0.7 raises the running max
  by 32 log2 units per 32-key tile, so every tile takes the rescale; "slow" (s = +1, gamma 0.05) raises it by 2.3
  per 32-key and 4.6 per 64-key tile against ``kRescaleThr = 8``, so the deferred branch is skipped on some tiles
  and taken on others.

What is compared. The GPU output against the oracle (``oracle_padded``, i.e. ``fa_oracle_c.forward_varlen``) under
the ELEMENTWISE bound ``atol + rtol |ref|`` of ``TOL`` only (``check_edge``). The absolute ``mean_tol`` of ``TOL``
is NOT applied: it was calibrated on ``randn`` outputs of ~0.03, and with outputs of O(1) an honest kernel
(fp32 scores, P rounded to the io dtype, fp32 sum, rounded output) already sits at 0.94 - 1.11 of it (fp16,
"rise"), so it would measure the data, not the kernel.

CPU self-tests (``test_data_*``, not marked gpu) pin that the GPU tests can fail: for every (case group, family)
used below, a float64 reference with the guarded edge moved by one key (``hi`` +-1: length, ``k_end``, diagonal;
``lo`` +-1: window, ``k_start``) exceeds the elementwise bound by at least 0.1 on EVERY affected row, while a torch
model of the honest kernel stays inside it, and a visible needle holds > 90 % of its row's weight. Measured by
them over the cases listed in ``SELF``:
    honest model, max(err - bound):  fp16 needle -1.85e-3, ramp -1.20e-3;  bf16 needle -1.45e-2, ramp -1.04e-2;
        FP8 pools: fp16 needle -1.97e-3, ramp -1.89e-3;  bf16 needle -1.57e-2, ramp -1.42e-2
    shifted reference, min over the affected rows of max(err - bound):  needle 1.56, rise 0.61, fall 0.84;
        FP8 pools: needle 2.06, rise 0.76, fall 0.80
(the bound is 2e-3 + 2e-3 |ref| for fp16 and 1.6e-2 + 1.6e-2 |ref| for bf16).

The last section pins a contract of ``flash_attn_paged_func`` no GPU test covered: lengths outside
``[0, max_pages * page_size]`` are clamped on the device by every read kernel.
"""
from __future__ import annotations

import functools
import zlib

import pytest
import torch

from accuracy import attend, span  # noqa: F401  (moved there unchanged)
from test_fp8_kvcache import NAN_BYTE, empty_pool, make_fp8_paged, quant
from test_kvcache import new_tokens, rope_tables
from test_gpu_parity import TOL
from test_padded import oracle_padded, ranges
from test_paged import make_paged
from test_paged_window import free_pages_below_the_window

F16, BF16 = torch.float16, torch.bfloat16
DEV = "cuda:0"
SENTINEL = 8.0  # V of buffer rows that belong to no sequence: including one moves the output by several units
RAMPS = {"rise": (1.0, 0.7), "fall": (-1.0, 0.7), "slow": (1.0, 0.05)}  # family -> (s, gamma)
RAMP_A = 8.0
NEEDLE_LOGIT = 14.0  # scale * q . k[c] of a needle row, against noise of sigma ~1.2 (D 128) / ~1.75 (D 64)
MIN_OVERSHOOT = 0.1  # a reference with an edge moved by one key must exceed the bound by this on every affected row
NAMES = {F16: "f16", BF16: "bf16"}


def crc(*key):
    return zlib.crc32(repr(key).encode())


def dv(*ts):
    return tuple(t.to(DEV) for t in ts)


# ------------------------------------------------------------------------------------------------
# the elementwise check (the mask as key ranges ``span`` and the float64 / honest-arithmetic reference ``attend``
# on them live in tests/accuracy.py)
# ------------------------------------------------------------------------------------------------
def excess(got, ref, dtype):
    """err - (atol + rtol |ref|), elementwise: positive means outside the bound of TOL."""
    atol, rtol, _ = TOL[dtype]
    got, ref = got.double(), ref.double()
    return (got - ref).abs() - (atol + rtol * ref.abs())


def check_edge(out, ref, dtype, what=""):
    """The elementwise bound of tests/test_gpu_parity.py TOL. NOT its absolute mean_tol: that was calibrated on
    randn outputs of ~0.03; these outputs are O(1), where the honest model of ``attend`` already sits at 0.94 -
    1.11 of it (fp16, "rise"), so it would judge the data and not the kernel."""
    got = out.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    ex = excess(got, ref, dtype)
    worst = ex.max().item()
    if worst > 0:
        i = tuple(int(x) for x in torch.unravel_index(ex.argmax(), ex.shape))
        raise AssertionError(f"{what}: at {i} kernel {got[i].item():.5f} oracle {ref.float()[i].item():.5f}: "
                             f"outside the bound by {worst:.3e}")


# ------------------------------------------------------------------------------------------------
# the two families
# ------------------------------------------------------------------------------------------------
def unit(d):
    u = torch.randn(d, generator=torch.Generator().manual_seed(4242))
    return u / u.norm()


def ramp_qkv(fam, b, bk, hq, hkv, sq, n, d, seed):
    """fp32 q [B, Hq, Sq, D], k / v [Bk, Hkv, N, D]: the ramp along u over the buffer position n."""
    s, gamma = RAMPS[fam]
    g = torch.Generator().manual_seed(seed)
    u = unit(d)
    beta = gamma / (d ** -0.5 * RAMP_A)
    q = 0.25 * torch.randn(b, hq, sq, d, generator=g) + RAMP_A * u
    pos = torch.arange(n, dtype=torch.float32) - n / 2
    k = 0.25 * torch.randn(bk, hkv, n, d, generator=g) + s * beta * pos[:, None] * u
    v = torch.randn(bk, hkv, n, d, generator=g)
    return q, k, v


def needle_qkv(b, bk, hq, hkv, sq, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, hq, sq, d, generator=g)  # (replaced row by row: set_needles)
    return q, torch.randn(bk, hkv, n, d, generator=g), torch.randn(bk, hkv, n, d, generator=g)


def assign_needles(lo, hi, n, hq, extras=None):
    """c [B, Hq, Sq]: the live rows of the launch take in turn (one running counter over (b, m, q-head)) the last
    visible key hi - 1, the key past it hi (when the buffer has one), the first visible key lo, the key below it
    lo - 1 (when there is one), then the sequence's ``extras`` (absolute buffer positions)."""
    b, sq = lo.shape
    c = torch.zeros(b, hq, sq, dtype=torch.long)
    r = 0
    for i in range(b):
        ex = list(extras[i]) if extras is not None else []
        for m in range(sq):
            l_, h_ = int(lo[i, m]), int(hi[i, m])
            if h_ <= l_:
                continue
            for h in range(hq):
                slot = r % (4 + len(ex))
                r += 1
                c[i, h, m] = (h_ - 1, h_ if h_ < n else h_ - 1, l_, l_ - 1 if l_ > 0 else l_)[slot] if slot < 4 \
                    else ex[slot - 4]
    return c


def set_needles(k, c, hq, dtype):
    """q [B, Hq, Sq, D] in the io dtype: row (b, h, m) is the stored key k[b, h // g, c[b, h, m]], scaled so that
    its own logit is NEEDLE_LOGIT (x ~1.24 at D 128, x ~1.75 at D 64: the plain key's logit, ~11.3 and ~8, leaves
    a short key among 2048 others below 90 % of the weight)."""
    b, hkv, n, d = k.shape
    g = hq // hkv
    kk = k.repeat_interleave(g, 1) if g > 1 else k  # [B, Hq, N, D]
    q = torch.gather(kk, 2, c[..., None].expand(-1, -1, -1, d)).float()
    return (q * (NEEDLE_LOGIT / (d ** -0.5 * q.pow(2).sum(-1, keepdim=True)))).to(dtype)


class Case:
    """One launch's inputs in the dense form every entry reduces to: q [B, Hq, Sq, D], key buffers k / v [B, Hkv,
    N, D] as the kernel reads them (dequantized for an FP8 pool), the ranges, the mask."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def scale(self):
        return self.q.size(-1) ** -0.5

    def lohi(self):
        return span(self.ks, self.ke, self.q.size(2), self.causal, self.w, self.qs, self.qe)

    @functools.cached_property
    def ref(self):
        """The oracle the GPU tests compare with, float32 on the host."""
        return oracle_padded(self.q, self.k, self.v, self.ks, self.ke, self.qs, self.qe, self.scale, self.causal,
                             window_left=self.w).float()


def build(fam, b, hq, hkv, sq, n, d, dtype, seed, ks, ke, causal, w=-1, qs=None, qe=None, extras=None, shared=False,
          descales=None, sentinel_below=None):
    """A Case of family ``fam`` ("needle", "rise", "fall", "slow"). shared: one key buffer for all sequences (a
    packed varlen batch; no sentinel). descales (kd, vd) fp32 [B, Hkv]: k / v go through the FP8 write formula and
    come back widened times the descale (exact: powers of two), with k8 / v8 kept for the pool.
    sentinel_below [B]: rows below that position hold the sentinel V too (keys below every row's window)."""
    t = lambda x: torch.as_tensor(x, dtype=torch.int32)  # noqa: E731
    ks, ke = t(ks), t(ke)
    qs, qe = (None if x is None else t(x) for x in (qs, qe))
    bk = 1 if shared else b
    q, k, v = needle_qkv(b, bk, hq, hkv, sq, n, d, seed) if fam == "needle" else ramp_qkv(fam, b, bk, hq, hkv, sq, n, d,
                                                                                           seed)
    if not shared:
        pos = torch.arange(n)[None]
        nobody = (pos < ks[:, None]) | (pos >= ke[:, None])
        if sentinel_below is not None:
            nobody |= pos < t(sentinel_below)[:, None]
        v = torch.where(nobody[:, None, :, None], torch.tensor(SENTINEL), v)
    k8 = v8 = None
    if descales is not None:
        kd, vd = descales
        assert (k.abs().amax(dim=(2, 3)) <= 448.0 * kd).all(), "the ramp leaves the e4m3 range of this descale"
        k8, v8 = quant(k, kd[:, :, None, None]), quant(v, vd[:, :, None, None])
        k, v = k8.to(dtype) * kd[:, :, None, None].to(dtype), v8.to(dtype) * vd[:, :, None, None].to(dtype)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    if shared:
        k, v = k.expand(b, -1, -1, -1), v.expand(b, -1, -1, -1)
    case = Case(fam=fam, q=q, k=k, v=v, ks=ks, ke=ke, qs=qs, qe=qe, causal=causal, w=w, dtype=dtype, c=None, k8=k8,
                v8=v8, descales=descales)
    if fam == "needle":
        lo, hi = case.lohi()
        case.c = assign_needles(lo, hi, n, hq, extras)
        case.q = set_needles(k, case.c, hq, dtype)
    return case


def edges(step, upto):
    """Both sides of every multiple of ``step`` below ``upto``: step j - 1 and step j."""
    return [p for j in range(1, (upto - 1) // step + 1) for p in (step * j - 1, step * j) if p < upto]


# ------------------------------------------------------------------------------------------------
# the cases, shared by the CPU self-tests and the GPU tests
# ------------------------------------------------------------------------------------------------
PREFILL_SHAPES = [(1, 4, 2, 100, 333), (1, 2, 2, 333, 100), (2, 4, 1, 300, 300)]  # (B, Hq, Hkv, Sq, Sk)


def prefill_case(shape, d, dtype, causal, fam, w=-1, piece_edges=False):
    b, hq, hkv, sq, sk = shape
    extras = [edges(64, sk)] * b if piece_edges else None
    return build(fam, b, hq, hkv, sq, sk, d, dtype, crc("prefill", shape, d, NAMES[dtype], causal, fam, w), [0] * b,
                 [sk] * b, causal, w, extras=extras)


VARLEN_LENS = (65, 1, 190)


def varlen_case(dtype, causal, fam, w):
    """Three sequences packed back to back (Sq == Sk each); the ramp runs over the packed index, and the needle
    slots "one past the last" / "one below the first" are the neighbour sequences' adjacent keys."""
    cu = [0, 65, 66, 256]
    return build(fam, 3, 4, 2, max(VARLEN_LENS), cu[-1], 128, dtype, crc("varlen", NAMES[dtype], causal, fam, w), cu[:-1],
                 cu[1:], causal, w, qs=[0, 0, 0], qe=list(VARLEN_LENS), shared=True)


def padded_case(sq, side, dtype, causal, fam):
    b, hq, hkv, sk, d = 4, 8, 2, 200, 128
    seed = crc("padded", sq, side, NAMES[dtype], causal, fam)
    ks, ke, qs, qe = ranges(b, sq, sk, seed % 1000, side, min_len=1)
    if sq == 1:
        qs = qe = None  # the decode step: every sequence's one query row
    return build(fam, b, hq, hkv, sq, sk, d, dtype, seed, ks, ke, causal, qs=qs, qe=qe)


LENGTHS = (1, 31, 32, 33, 2047, 2048)
SHORT_LENGTHS = (1, 31, 32, 33, 255, 256)


def decode_case(lens, cap, sq, g, d, dtype, fam, w=-1, descales=None, tag=""):
    """A decode step over caches of capacity ``cap``: sequence b holds keys [0, lens[b]). Needle extras: both
    sides of every 32-key tile boundary of the sequence."""
    b, hkv = len(lens), 2
    causal = sq > 1
    extras = [edges(32, n) for n in lens]
    below = [max(0, n - sq - w) if w >= 0 else 0 for n in lens]
    return build(fam, b, hkv * g, hkv, sq, cap, d, dtype, crc("decode", lens, cap, sq, g, d, NAMES[dtype], fam, w, tag),
                 [0] * b, list(lens), causal, w, extras=extras, descales=descales, sentinel_below=below)


def pow2(b, hkv, lo_exp, hi_exp, shift=0):
    """Distinct powers of two 2^lo_exp .. 2^hi_exp per (b, h), cyclic; fp32 [B, Hkv]."""
    e = (torch.arange(b * hkv).reshape(b, hkv) + shift) % (hi_exp - lo_exp + 1) + lo_exp
    return torch.pow(2.0, e.float())


def window_lens(w, sq):
    """Lengths that put row 0's first visible key at 95 = 32 * 3 - 1 and at 96, and one shorter than the window."""
    return (w + sq + 95, w + sq + 96, min(w, 20) + sq)


PP_LENS = (37, 64, 65, 449)


def paged_prefill_case(sq, dtype, causal, fam, w):
    b, hq, hkv, cap, d = len(PP_LENS), 8, 2, 512, 128
    extras = [edges(64, n) for n in PP_LENS]
    return build(fam, b, hq, hkv, sq, cap, d, dtype, crc("pp", sq, NAMES[dtype], causal, fam, w), [0] * b, list(PP_LENS),
                 causal, w, extras=extras)


# (group, thunk): one representative of every (case group, family, dtype) the GPU tests use
SELF = []
for _dt in (F16, BF16):
    for _fam in ("needle", "rise", "fall", "slow"):
        SELF += [
            (f"prefill-{_fam}-d128-{NAMES[_dt]}", functools.partial(prefill_case, PREFILL_SHAPES[0], 128, _dt, True, _fam)),
            (f"prefill-{_fam}-d64-{NAMES[_dt]}", functools.partial(prefill_case, PREFILL_SHAPES[2], 64, _dt, True, _fam)),
            (f"prefill_full-{_fam}-{NAMES[_dt]}", functools.partial(prefill_case, PREFILL_SHAPES[1], 128, _dt, False, _fam)),
            (f"layout-{_fam}-{NAMES[_dt]}",
             functools.partial(prefill_case, (1, 8, 2, 200, 333), 128 if _dt == F16 else 64, _dt, True, _fam, piece_edges=True)),
            (f"decode256-{_fam}-{NAMES[_dt]}", functools.partial(decode_case, SHORT_LENGTHS, 256, 3, 4, 128, _dt, _fam)),
            (f"decode2048-{_fam}-{NAMES[_dt]}", functools.partial(decode_case, LENGTHS, 2048, 1, 4, 128, _dt, _fam)),
            (f"decode2048_sq3-{_fam}-d64-{NAMES[_dt]}", functools.partial(decode_case, LENGTHS, 2048, 3, 8, 64, _dt, _fam)),
        ]
    for _fam in ("needle", "rise", "fall"):
        SELF += [
            (f"split_pieces-{_fam}-{NAMES[_dt]}",
             functools.partial(prefill_case, PREFILL_SHAPES[2], 128, _dt, True, _fam, piece_edges=True)),
            (f"varlen-{_fam}-w40-{NAMES[_dt]}", functools.partial(varlen_case, _dt, True, _fam, 40)),
            (f"varlen-{_fam}-w0-full-{NAMES[_dt]}", functools.partial(varlen_case, _dt, False, _fam, 0)),
            (f"varlen-{_fam}-{NAMES[_dt]}", functools.partial(varlen_case, _dt, True, _fam, -1)),
            (f"padded37-{_fam}-{NAMES[_dt]}", functools.partial(padded_case, 37, "mixed", _dt, True, _fam)),
            (f"padded1-{_fam}-{NAMES[_dt]}", functools.partial(padded_case, 1, "left", _dt, False, _fam)),
            (f"window_prefill-{_fam}-w63-{NAMES[_dt]}",
             functools.partial(prefill_case, (1, 4, 2, 300, 300), 128, _dt, True, _fam, 63)),
            (f"window_prefill-{_fam}-w100-{NAMES[_dt]}",
             functools.partial(prefill_case, (1, 4, 2, 40, 333), 128, _dt, True, _fam, 100)),
            (f"window_decode-{_fam}-w31-{NAMES[_dt]}",
             functools.partial(decode_case, window_lens(31, 1), 256, 1, 4, 128, _dt, _fam, 31)),
            (f"window_decode_sq3-{_fam}-w100-{NAMES[_dt]}",
             functools.partial(decode_case, window_lens(100, 3), 256, 3, 4, 128, _dt, _fam, 100)),
            (f"paged_prefill40-{_fam}-w64-{NAMES[_dt]}", functools.partial(paged_prefill_case, 40, _dt, True, _fam, 64)),
            (f"paged_prefill300-{_fam}-{NAMES[_dt]}", functools.partial(paged_prefill_case, 300, _dt, False, _fam, -1)),
            (f"fp8_decode-{_fam}-{NAMES[_dt]}",
             functools.partial(decode_case, SHORT_LENGTHS, 256, 1, 4, 128, _dt, _fam,
                               descales=(pow2(6, 2, -1, 2), pow2(6, 2, -1, 2, 1)))),
            (f"fp8_window_decode-{_fam}-w32-{NAMES[_dt]}",
             functools.partial(decode_case, window_lens(32, 1), 256, 1, 4, 128, _dt, _fam, 32,
                               descales=(pow2(3, 2, -1, 2), pow2(3, 2, -1, 2, 1)))),
        ]
    SELF += [
        (f"every_tile_boundary-needle-{NAMES[_dt]}",
         functools.partial(decode_case, (2048, 2047) * 5, 2048, 1, 8, 128, _dt, "needle", tag="all")),
        (f"fp8_decode2048-needle-{NAMES[_dt]}",
         functools.partial(decode_case, LENGTHS, 2048, 1, 4, 128, _dt, "needle",
                           descales=(pow2(6, 2, -1, 2), pow2(6, 2, -1, 2, 1)))),
        (f"fp8_decode2048-slow-{NAMES[_dt]}",
         functools.partial(decode_case, LENGTHS, 2048, 1, 4, 128, _dt, "slow",
                           descales=(pow2(6, 2, -1, 2), pow2(6, 2, -1, 2, 1)))),
    ]

# the shifts a family guards: (name, d lo, d hi)
GUARDS = {"rise": [("hi-1", 0, -1), ("hi+1", 0, 1)], "fall": [("lo+1", 1, 0), ("lo-1", -1, 0)], "slow": [],
          "needle": [("hi-1", 0, -1), ("hi+1", 0, 1), ("lo+1", 1, 0), ("lo-1", -1, 0)]}


def affected_rows(case, name):
    """[B, Hq, Sq] bool: the rows on which moving that edge by one key must show. Ramp: every live row whose
    gained key exists in the buffer. Needle: the rows whose needle IS the key gained or lost."""
    lo, hi = case.lohi()
    n = case.k.size(2)
    live = hi > lo
    key, ok = {"hi-1": (hi - 1, live), "hi+1": (hi, live & (hi < n)), "lo+1": (lo, live),
               "lo-1": (lo - 1, live & (lo > 0))}[name]
    rows = ok[:, None].expand(-1, case.q.size(1), -1)
    if case.fam == "needle":
        rows = rows & (case.c == key[:, None])
    return rows


@pytest.mark.parametrize("name,thunk", SELF, ids=[s[0] for s in SELF])
def test_data_can_fail_and_honest_arithmetic_passes(name, thunk):
    """For this (group, family): the oracle's input with a guarded edge moved by one key exceeds the elementwise
    bound by >= 0.1 on every affected row (so a kernel that gains or drops that key fails the GPU test); the honest
    kernel model stays inside the bound; visible needles hold > 90 % of their row's weight."""
    case = thunk()
    lo, hi = case.lohi()
    ref = case.ref
    f64, p = attend(case.q, case.k, case.v, lo, hi, case.scale)
    assert excess(f64, ref, case.dtype).max().item() <= 0  # (the C oracle is the float64 softmax on this mask)
    honest, _ = attend(case.q, case.k, case.v, lo, hi, case.scale, emul=case.dtype)
    margin = excess(honest, ref, case.dtype).max().item()
    print(f"{name}: honest model max(err - bound) = {margin:.3e}")
    assert margin <= 0
    if case.fam == "needle":
        vis = (case.c >= lo[:, None]) & (case.c < hi[:, None])
        weight = torch.gather(p, 3, case.c[..., None])[..., 0]
        assert vis.any() and weight[vis].min().item() > 0.9, weight[vis].min().item()
    guarded = 0
    for shift, dlo, dhi in GUARDS[case.fam]:
        rows = affected_rows(case, shift)
        if not rows.any():
            continue
        moved, _ = attend(case.q, case.k, case.v, lo + dlo, hi + dhi, case.scale)
        over = excess(moved, ref, case.dtype).amax(-1)[rows].min().item()
        print(f"{name}: {shift}: {int(rows.sum())} rows, min overshoot {over:.3f}")
        assert over >= MIN_OVERSHOOT, (shift, over)
        guarded += 1
    assert guarded >= (0 if case.fam == "slow" else 2 if case.fam == "needle" else 1)


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def dbg(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"

    def reset():
        _debug.set_knobs()
        _debug.set_dec_fuse(None)
        _debug.set_split()
        _debug.set_split_pairs()
        _debug.set_zigzag()
        _debug.set_head_pack()

    reset()
    yield _debug
    reset()


def to_pool(case, lens, page, seed, layout="phsd"):
    """The case's dense keys scattered into a poisoned pool through a shuffled table, as test_paged.make_paged
    does: every pool row that holds no key is NaN (0x7F in an e4m3 pool), the rows of a last page past the
    length included, every unused table entry -1. Returns (k pool, v pool, table, lengths)."""
    b, hkv, cap, d = case.k.shape
    max_pages = cap // page
    g = torch.Generator().manual_seed(seed)
    num_pages = b * max_pages + 3
    ids = torch.randperm(num_pages, generator=g).tolist()
    table = torch.full((b, max_pages), -1, dtype=torch.int32)
    fp8 = case.k8 is not None
    ksrc, vsrc = (case.k8, case.v8) if fp8 else (case.k, case.v)

    def pool():
        if fp8:
            return empty_pool(num_pages, hkv, page, d, layout)
        if layout == "pshd":
            return torch.full((num_pages, page, hkv, d), float("nan"), dtype=case.dtype).transpose(1, 2)
        return torch.full((num_pages, hkv, page, d), float("nan"), dtype=case.dtype)

    kc, vc = pool(), pool()
    for i, n in enumerate(lens):
        for j in range((n + page - 1) // page):
            pg, n0 = ids.pop(), j * page
            rows = min(n, n0 + page) - n0
            table[i, j] = pg
            kc[pg, :, :rows] = ksrc[i, :, n0:n0 + rows]
            vc[pg, :, :rows] = vsrc[i, :, n0:n0 + rows]
    return kc, vc, table, torch.tensor(lens, dtype=torch.int32)


def paged_launch(dbg, case, pool, fuse=None):
    """flash_attn_paged_func on a pool of to_pool: (output on the host, last_path, last_dec_fused)."""
    from flash_attention_cute_amd import flash_attn_paged_func

    kc, vc, table, sl = pool
    kw = {}
    if case.descales is not None:
        kw = dict(k_descale=case.descales[0].to(DEV), v_descale=case.descales[1].to(DEV))
    dbg.set_dec_fuse(fuse)
    try:
        out = flash_attn_paged_func(*dv(case.q, kc, vc, table, sl), causal=case.causal, window_left=case.w, **kw)
        labels = dbg.last_path(), dbg.last_dec_fused(), dbg.last_prefill_paged()
        torch.cuda.synchronize()
    finally:
        dbg.set_dec_fuse(None)
    return (out.cpu(), *labels)


def label(case, *more):
    return " ".join(str(x) for x in (case.fam, NAMES[case.dtype], "causal" if case.causal else "full", f"w{case.w}") + more)


# ---- prefill: flash_attn_func ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("shape", PREFILL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prefill_edges(dbg, shape, d, dtype):
    """The diagonal (Sq < Sk, Sq > Sk, Sq == Sk), the 64-key tile tail and the last q-tile, on fa_fwd_w4."""
    from flash_attention_cute_amd import flash_attn_func

    for causal in (False, True):
        for fam in ("rise", "fall", "slow", "needle"):
            case = prefill_case(shape, d, dtype, causal, fam)
            out = flash_attn_func(*dv(case.q, case.k, case.v), causal=causal)
            assert dbg.last_path() == "w4"
            check_edge(out, case.ref, dtype, label(case))


LAYOUT_KNOBS = {"zigzag": (0, 2, 0), "headpack": (0, 0, 2), "split": (2, None, 0), "split_headpack": (2, None, 2)}
# (zigzag and key-split blocks take launches of more than 128 query rows only -- fa_launch.h use_zigzag, use_split --
# so the Sq < Sk shape has 200 rows here, and g = 4 so that it can be head-packed too)
LAYOUT_SHAPES = [(1, 8, 2, 200, 333)] + PREFILL_SHAPES[1:]
LAYOUT_CASES = [(lay, si) for lay in LAYOUT_KNOBS for si in range(len(LAYOUT_SHAPES))
                if "headpack" not in lay or (LAYOUT_SHAPES[si][1] // LAYOUT_SHAPES[si][2]) % 4 == 0]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("layout,si", LAYOUT_CASES, ids=[f"{lay}-{'x'.join(map(str, LAYOUT_SHAPES[si]))}" for lay, si in LAYOUT_CASES])
def test_prefill_edges_under_forced_layouts(dbg, layout, si, dtype):
    """The causal block layouts, forced with the knobs as tests/test_gpu_parity.py forces them: zigzag, head-packed
    (g % 4 == 0) and key-split blocks (plain and head-packed pieces). The needle rows also probe both sides of
    every 64-key boundary, so whatever piece boundary the key-split plan picks is probed from both sides."""
    import flash_attention_cute_amd as m

    split, zigzag, head_pack = LAYOUT_KNOBS[layout]
    shape = LAYOUT_SHAPES[si]
    d = 128 if dtype == F16 else 64
    m.split_errors(reset=True)
    for fam in ("rise", "fall", "slow", "needle"):
        case = prefill_case(shape, d, dtype, True, fam, piece_edges=True)
        dbg.set_split(split)
        dbg.set_zigzag(zigzag)
        dbg.set_head_pack(head_pack)
        out = m.flash_attn_func(*dv(case.q, case.k, case.v), causal=True)
        assert dbg.last_path() == "w4"
        assert dbg.last_layout() == layout.split("_")[0], dbg.last_layout()
        assert dbg.last_head_pack() == ("headpack" in layout)
        torch.cuda.synchronize()
        check_edge(out, case.ref, dtype, label(case, layout))
    assert m.split_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["p8", "w8", "w4slow", "m32", "m16"])
def test_prefill_edges_on_the_debug_bodies(dbg, variant):
    """The other bodies that carry the deferred rescale and their own mask code, through _debug.forward."""
    dtype = BF16 if variant in ("w8", "m16") else F16
    try:
        for causal, fam in ((True, "rise"), (True, "slow"), (False, "slow"), (True, "fall"), (True, "needle")):
            case = prefill_case(PREFILL_SHAPES[0], 128, dtype, causal, fam)
            out = dbg.forward(*dv(case.q, case.k, case.v), None, causal, variant=variant)
            assert dbg.last_path(debug=True) == variant
            check_edge(out, case.ref, dtype, label(case, variant))
    finally:
        dbg.set_knobs(debug=True)


# ---- varlen ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_varlen_edges(dbg, dtype, causal):
    """cu_seqlens boundaries with a neighbour's finite keys next door: the ramp over the PACKED index makes the
    neighbour's adjacent key outscore everything visible, in both directions; needles sit on those keys."""
    from flash_attention_cute_amd import flash_attn_varlen_func

    cu = torch.tensor([0, 65, 66, 256], dtype=torch.int32)
    pack = lambda t: torch.cat([t[i, :, :n].transpose(0, 1) for i, n in enumerate(VARLEN_LENS)]).contiguous()  # noqa: E731
    for w in (-1, 0, 40):
        for fam in ("rise", "fall", "needle"):
            case = varlen_case(dtype, causal, fam, w)
            kp, vp = (t[0].transpose(0, 1).contiguous() for t in (case.k, case.v))
            out = flash_attn_varlen_func(*dv(pack(case.q), kp, vp, cu, cu), max(VARLEN_LENS), max(VARLEN_LENS),
                                         causal=causal, window_left=w)
            assert dbg.last_path() == "w4"
            check_edge(out, pack(case.ref), dtype, label(case))


# ---- padded op ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("side", ["left", "right", "mixed"])
@pytest.mark.parametrize("sq", [37, 1])
def test_padded_edges(dbg, sq, side, dtype):
    """k_start / k_end inside dense tensors; the rows outside hold finite keys that outscore every visible one
    under the ramp, and V = 8."""
    from flash_attention_cute_amd import flash_attn_padded_func

    for causal in (False, True):
        for fam in ("rise", "fall", "needle"):
            case = padded_case(sq, side, dtype, causal, fam)
            rng = (case.ks, case.ke) if sq == 1 else (case.ks, case.ke, case.qs, case.qe)
            out = flash_attn_padded_func(*dv(case.q, case.k, case.v, *rng), causal=causal)
            assert dbg.last_path() == ("decode" if sq == 1 else "w4")
            check_edge(out, case.ref, dtype, label(case, side))


# ---- window prefill -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 4, 2, 300, 300), (1, 4, 2, 40, 333)], ids=["300x300", "40x333"])
def test_window_prefill_edges(dbg, shape, dtype):
    """The window's left edge at, one below and one above a 64-key tile edge: the fall ramp weighs every row's
    first visible key; q-heads 2 and 3 of every row are needles on that key and on the one below it."""
    from flash_attention_cute_amd import flash_attn_window_func

    for w in (0, 63, 64, 100):
        for fam in ("fall", "rise", "needle"):
            case = prefill_case(shape, 128, dtype, True, fam, w)
            out = flash_attn_window_func(*dv(case.q, case.k, case.v), w, causal=True)
            assert dbg.last_path() == "w4"
            check_edge(out, case.ref, dtype, label(case))


# ---- 16-bit decode: dense, padded, paged ----------------------------------------------------
DEC_GEO = [(1, 4), (3, 4), (1, 8), (3, 8)]  # (Sq, g); Hkv 2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("sq,g", DEC_GEO, ids=[f"sq{s}-g{g}" for s, g in DEC_GEO])
def test_dense_decode_edges(dbg, sq, g, dtype):
    """flash_attn_func on few rows per kv-head: one key, the 32-key tile tail on both sides, the split plan."""
    from flash_attention_cute_amd import flash_attn_func

    d = 128 if (sq + g) % 2 else 64
    for n in LENGTHS:
        for fam in ("needle", "rise", "slow"):
            case = decode_case((n, n), n, sq, g, d, dtype, fam)
            out = flash_attn_func(*dv(case.q, case.k, case.v), causal=case.causal)
            assert dbg.last_path() == ("decode_split" if n >= 2047 else "decode"), (n, dbg.last_path())
            check_edge(out, case.ref, dtype, label(case, n))


FORMS = {"unsplit": (SHORT_LENGTHS, 256, None), "fused": (LENGTHS, 2048, None), "unfused": (LENGTHS, 2048, 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("sq,g", DEC_GEO, ids=[f"sq{s}-g{g}" for s, g in DEC_GEO])
@pytest.mark.parametrize("form", list(FORMS))
def test_padded_decode_edges(dbg, form, sq, g, dtype):
    """seqlens against the capacity on the dense decode kernel: the rows past each length hold keys that outscore
    every visible one under the ramp, and V = 8. Split forms: the merge when one split holds all the weight."""
    from flash_attention_cute_amd import flash_attn_padded_func

    lens, cap, fuse = FORMS[form]
    d = 64 if (sq + g) % 2 else 128
    for fam in ("needle", "rise", "slow"):
        case = decode_case(lens, cap, sq, g, d, dtype, fam)
        dbg.set_dec_fuse(fuse)
        out = flash_attn_padded_func(*dv(case.q, case.k, case.v, case.ks, case.ke), causal=case.causal)
        assert dbg.last_path() == ("decode" if form == "unsplit" else "decode_split")
        if form != "unsplit":
            assert dbg.last_dec_fused() == (fuse is None)
        check_edge(out, case.ref, dtype, label(case, form))


PAGED_DEC = [(form, page, DEC_GEO[(fi + pi) % 4], (F16, BF16)[(fi + pi) % 2], ("phsd", "pshd")[pi % 2])
             for fi, form in enumerate(FORMS) for pi, page in enumerate((32, 64, 256))]


@pytest.mark.gpu
@pytest.mark.parametrize("form,page,geo,dtype,layout", PAGED_DEC,
                         ids=[f"{f}-p{p}-sq{s}-g{g}-{NAMES[t]}" for f, p, (s, g), t, _ in PAGED_DEC])
def test_paged_decode_edges(dbg, form, page, geo, dtype, layout):
    """The same through shuffled tables into NaN-poisoned pools (page edges, the last page's tail)."""
    (sq, g), (lens, cap, fuse) = geo, FORMS[form]
    for fam in ("needle", "rise", "slow"):
        case = decode_case(lens, cap, sq, g, 128, dtype, fam)
        out, path, fused, _ = paged_launch(dbg, case, to_pool(case, lens, page, crc(form, page, fam), layout), fuse)
        assert path == ("decode_paged" if form == "unsplit" else "decode_paged_split")
        if form != "unsplit":
            assert fused == (fuse is None)
        check_edge(out, case.ref, dtype, label(case, form, page))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("fuse", [None, 0], ids=["fused", "unfused"])
def test_every_decode_tile_boundary_holds_a_needle(dbg, fuse, dtype):
    """160 (b, q-head) rows over lengths 2048 and 2047: one needle on each side of EVERY 32-key tile boundary (and so
    of every split and wave-share boundary of the plan), on the first key and on the last; padded and paged."""
    from flash_attention_cute_amd import flash_attn_padded_func

    lens = (2048, 2047) * 5
    case = decode_case(lens, 2048, 1, 8, 128, dtype, "needle", tag="all")
    placed = set(case.c.flatten().tolist())
    assert set(edges(32, 2047)) | {0, 2047} <= placed and 2048 not in placed
    dbg.set_dec_fuse(fuse)
    out = flash_attn_padded_func(*dv(case.q, case.k, case.v, case.ks, case.ke))
    assert dbg.last_path() == "decode_split" and dbg.last_dec_fused() == (fuse is None)
    check_edge(out, case.ref, dtype, label(case, "padded"))
    out, path, fused, _ = paged_launch(dbg, case, to_pool(case, lens, 64, 5), fuse)
    assert path == "decode_paged_split" and fused == (fuse is None)
    check_edge(out, case.ref, dtype, label(case, "paged"))


# ---- FP8 decode -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("form,page,sq,g", [("unsplit", 32, 1, 4), ("unsplit", 64, 3, 8), ("fused", 256, 1, 8),
                                            ("unfused", 64, 3, 4)])
def test_fp8_decode_edges(dbg, form, page, sq, g, dtype):
    """The FP8 body through e4m3 pools with power-of-two descales (the oracle reads the widened bytes times the
    descale: exact). The ramp must stay inside 448 * descale (asserted by ``build``), so the steep ramps run at
    capacity 256 and the split forms take the needles and the slow ramp."""
    lens, cap, fuse = FORMS[form]
    b = len(lens)
    ds = (pow2(b, 2, -1, 2), pow2(b, 2, -1, 2, 1))
    for fam in ("needle", "slow") + (("rise",) if form == "unsplit" else ()):
        case = decode_case(lens, cap, sq, g, 128, dtype, fam, descales=ds)
        out, path, fused, _ = paged_launch(dbg, case, to_pool(case, lens, page, crc("fp8", form, fam), "pshd"), fuse)
        assert path == ("decode_paged_fp8" if form == "unsplit" else "decode_paged_fp8_split")
        if form != "unsplit":
            assert fused == (fuse is None)
        check_edge(out, case.ref, dtype, label(case, form, "fp8"))


# ---- window decode, 16-bit and FP8 ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("sq,page,dtype", [(1, 32, F16), (3, 64, BF16), (1, 64, BF16), (3, 32, F16)],
                         ids=["sq1-p32-f16", "sq3-p64-bf16", "sq1-p64-bf16", "sq3-p32-f16"])
def test_window_decode_edges(dbg, sq, page, dtype, fp8):
    """The window's first key at 32j - 1 and at 32j: the fall ramp weighs it, two needle rows sit on it and on the
    key below it (which holds V = 8 where no row sees it). Then the same launch with the pages below the window
    freed -- NaN pages, -1 in their entries: the same bits."""
    for w in (0, 31, 32, 100):
        lens = window_lens(w, sq)
        assert [(n - sq - w) % 32 for n in lens[:2]] == [31, 0]
        ds = (pow2(3, 2, -1, 2), pow2(3, 2, -1, 2, 1)) if fp8 else None
        for fam in ("fall", "needle", "rise"):
            case = decode_case(lens, 256, sq, 4, 128, dtype, fam, w, descales=ds)
            kc, vc, table, sl = to_pool(case, lens, page, crc("win", w, fam))
            out, path, _, _ = paged_launch(dbg, case, (kc, vc, table, sl))
            assert path == ("decode_paged_fp8" if fp8 else "decode_paged")
            check_edge(out, case.ref, dtype, label(case, "fp8" if fp8 else "16bit"))
            kc2, vc2, table2, freed = free_pages_below_the_window(kc, vc, table, lens, sq, w, page, -1,
                                                                  NAN_BYTE if fp8 else float("nan"))
            assert freed >= 2
            got, _, _, _ = paged_launch(dbg, case, (kc2, vc2, table2, sl))
            assert torch.isfinite(got.float()).all() and torch.equal(got, out)


# ---- paged prefill --------------------------------------------------------------------------
PP_WF = [(-1, "rise"), (-1, "fall"), (-1, "needle"), (0, "fall"), (0, "needle"), (64, "fall"), (64, "needle"),
         (100, "rise"), (100, "fall")]


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq,page,dtype", [(40, 64, F16), (40, 128, BF16), (300, 64, BF16), (300, 128, F16)],
                         ids=["sq40-p64-f16", "sq40-p128-bf16", "sq300-p64-bf16", "sq300-p128-f16"])
def test_paged_prefill_edges(dbg, sq, page, dtype, causal):
    """The paged fa_fwd_w4: fewer keys than queries, a page edge, one key past it, a tile tail; needles on both
    sides of every 64-key (page and tile) edge. Beside the oracle, the bits of the padded op on the dense keys."""
    from flash_attention_cute_amd import flash_attn_padded_func

    for w, fam in PP_WF:
        case = paged_prefill_case(sq, dtype, causal, fam, w)
        out, path, _, in_place = paged_launch(dbg, case, to_pool(case, PP_LENS, page, crc("pp", w, fam), "pshd"))
        assert path == "w4" and in_place
        check_edge(out, case.ref, dtype, label(case, page))
        dense = flash_attn_padded_func(*dv(case.q, case.k, case.v, case.ks, case.ke), causal=causal, window_left=w)
        assert dbg.last_path() == "w4" and not dbg.last_prefill_paged()
        assert torch.equal(out, dense.cpu())


# ---- flash_attn_with_kvcache: the needle is the key the step itself appends -----------------
@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_with_kvcache_needle_on_the_appended_key(dbg, fp8):
    """One decode step with the RoPE-fused append: q is the new key itself (scaled to NEEDLE_LOGIT), rotated at the
    same position, so the row's output is the new value IF the append landed where the read looks. The oracle's
    keys are the cache before the step with row L replaced on the host (_rope_reference, the FP8 write formula),
    its q the rotated q of the append op."""
    from flash_attention_cute_amd import flash_attention as fam

    lens, hq, hkv, page, cap, d, dtype = (70, 0, 33, 127, 63), 8, 2, 32, 128, 128, BF16
    b, g = len(lens), hq // hkv
    after = tuple(n + 1 for n in lens)
    ds = (pow2(b, hkv, -1, 2), pow2(b, hkv, -1, 2, 1)) if fp8 else None
    case = decode_case(after, cap, 1, g, d, dtype, "needle", descales=ds, tag="kvcache")  # (its k / v: the old cache)
    kc, vc, table, _ = to_pool(case, after, page, 31)  # row L of every sequence still holds another key
    kn, vn = new_tokens(b, hkv, 1, d, dtype, 1), new_tokens(b, hkv, 1, d, dtype, 2)
    q = kn.float().repeat_interleave(g, 1)
    q = (q * (NEEDLE_LOGIT / (d ** -0.5 * q.pow(2).sum(-1, keepdim=True)))).to(dtype)
    cos, sin = rope_tables(cap, d, dtype)
    sl = torch.tensor(lens, dtype=torch.int32)
    kw = dict(k_descale=ds[0].to(DEV), v_descale=ds[1].to(DEV)) if fp8 else {}
    kc_d, vc_d, table_d, sl_d, cos_d, sin_d = dv(kc, vc, table, sl, cos, sin)
    kc2, vc2 = kc_d.clone(), vc_d.clone()
    out, new = fam.flash_attn_with_kvcache(*dv(q), kc_d, vc_d, *dv(kn, vn), cos_d, sin_d, cache_seqlens=sl_d,
                                           block_table=table_d, causal=True, return_seqlens=True, **kw)
    assert dbg.last_path() == ("decode_paged_fp8" if fp8 else "decode_paged")
    append = torch.ops.flash_attention.kvcache_append_fp8 if fp8 else torch.ops.flash_attention.kvcache_append
    _, q_rot = append(kc2, vc2, *dv(kn, vn), sl_d, table_d, *dv(q), cos_d, sin_d, *kw.values())
    torch.cuda.synchronize()
    assert new.tolist() == list(after)
    pos = torch.tensor(lens)
    k_row, v_row = fam._rope_reference(kn, cos[pos][:, None], sin[pos][:, None]), vn
    if fp8:
        k_row = quant(k_row, ds[0][:, :, None, None]).to(dtype) * ds[0][:, :, None, None].to(dtype)
        v_row = quant(v_row, ds[1][:, :, None, None]).to(dtype) * ds[1][:, :, None, None].to(dtype)
    k, v = case.k.clone(), case.v.clone()
    for i, n in enumerate(lens):
        k[i, :, n], v[i, :, n] = k_row[i, :, 0], v_row[i, :, 0]
    ref = oracle_padded(q_rot.cpu(), k, v, case.ks, case.ke, None, None, d ** -0.5, True).float()
    _, p = attend(q_rot.cpu(), k, v, *span(case.ks, case.ke, 1, True), d ** -0.5)
    weight = torch.stack([p[i, :, 0, n] for i, n in enumerate(lens)])
    assert weight.min().item() > 0.9, weight.min().item()  # (the oracle's own probabilities: the new key is the needle)
    check_edge(out, ref, dtype, "with_kvcache " + ("fp8" if fp8 else "16bit"))


# ------------------------------------------------------------------------------------------------
# lengths outside [0, max_pages * page_size] are clamped on the device (flash_attn_paged_func's contract)
# ------------------------------------------------------------------------------------------------
CLAMP = {  # kernel -> (Sq, window, fp8, path)
    "decode": (1, -1, False, "decode_paged"),
    "decode_fp8": (1, -1, True, "decode_paged_fp8"),
    "window_decode": (3, 40, False, "decode_paged"),
    "window_decode_fp8": (3, 40, True, "decode_paged_fp8"),
    "prefill": (40, -1, False, "w4"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(CLAMP))
def test_out_of_range_lengths_are_clamped_to_the_table(dbg, kernel):
    """Lengths (-3, cap + 1, cap + page + 5, 2^31 - 1, -2^31) give the bits of (0, cap, cap, cap, 0). The table is
    the first max_pages columns of a WIDER int32 tensor (a row stride != max_pages) whose further columns name
    NaN-poisoned pages: a length that escaped the clamp would walk into them and show as NaN, not as an access
    outside the table. (The clamps: fa_decode_paged.hpp PagedSeq::key_range, fa_fwd_kernels.hpp set_block -- each
    precedes every use of the length.)"""
    from flash_attention_cute_amd import flash_attn_paged_func

    sq, w, fp8, want_path = CLAMP[kernel]
    page, cap, hq, hkv, d, dtype = 64, 256, 8, 2, 128, F16
    full = (cap,) * 5
    kw = {}
    if fp8:
        kd, vd = pow2(5, hkv, -1, 2), pow2(5, hkv, -1, 2, 1)
        q, _, _, kc, vc, table, _ = make_fp8_paged(full, hq, hkv, sq, page, cap, d, dtype, 41, "phsd", kd, vd)
        kw = dict(k_descale=kd.to(DEV), v_descale=vd.to(DEV))
        assert (kc.view(torch.uint8) == NAN_BYTE).flatten(1).all(1).sum() == 3  # (the spare pages: all NaN)
    else:
        q, _, _, kc, vc, table, _ = make_paged(full, hq, hkv, sq, page, cap, d, dtype, 41)
    spare = sorted(set(range(kc.size(0))) - set(table.flatten().tolist()))
    assert len(spare) == 3
    wide = torch.cat([table, torch.tensor(spare[:2], dtype=torch.int32).expand(5, 2)], dim=1).contiguous().to(DEV)
    view = wide[:, :cap // page]
    assert view.stride(0) == cap // page + 2 and not view.is_contiguous()
    bad = torch.tensor([-3, cap + 1, cap + page + 5, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    good = torch.tensor([0, cap, cap, cap, 0], dtype=torch.int32)
    qd, kcd, vcd = dv(q, kc, vc)
    got = flash_attn_paged_func(qd, kcd, vcd, view, bad.to(DEV), causal=sq > 1, window_left=w, **kw)
    assert dbg.last_path() == want_path and (kernel != "prefill" or dbg.last_prefill_paged())
    ref = flash_attn_paged_func(qd, kcd, vcd, view, good.to(DEV), causal=sq > 1, window_left=w, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all() and torch.equal(got, ref)
    assert (got[0] == 0).all() and (got[4] == 0).all() and got[1:4].float().abs().max().item() > 0
