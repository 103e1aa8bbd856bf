"""Every attention path's error against what honest arithmetic costs (tests/accuracy.py).

Why. Every other GPU parity test hangs on tests/test_gpu_parity.py ``TOL``, which an honest kernel fills to about
a tenth (tests/test_edge_weight.py measured it). A kernel could be several times less accurate than it should be
and pass all of them. Here each path's output is measured against a float64 reference (``accuracy.model`` with
``dtype=None``) and the three numbers of ``accuracy.measure`` are compared with the same numbers of the honest
model on the SAME data (``model(..., dtype)``: fp32 scores, P rounded to nearest even, fp32 sums, one rounding):

    rms_kernel  <= RMS_CAP  * rms_honest      (families centered, sharp)
    emax_kernel <= EMAX_CAP * emax_honest     (families centered, sharp)
    |bias_kernel| <= eps / 16                 (family offset; eps 2^-11 fp16, 2^-8 bf16)

The caps are conditions derived from CPU models, never from a kernel (``caps``): per (family, dtype), over one
representative shape per kernel class (``CLASSES``), RMS_CAP is the geometric mean of the worst ratio of an honest
form ("tiled", "split") to the "row" form and the weakest ratio of a planted defect; EMAX_CAP the same against the
"O kept in 16 bits" defect. The CPU part of this file (not marked gpu) shows that the GPU tests can fail and that
an honest kernel cannot fail them: every cap sits at least 1.15 x above every honest form and 1.15 x below every
defect it is built from. Figures the CPU part measured (``test_caps`` prints them):

    RMS_CAP   centered f16 1.27 (honest <= 1.05, defects >= 1.52)  bf16 1.26 (1.05, 1.52)
              sharp    f16 1.45 (honest <= 1.21, defects >= 1.73)  bf16 1.46 (1.21, 1.76)
    EMAX_CAP  centered f16 2.03 (honest <= 1.56, o16 >= 2.64)      bf16 2.01 (1.39, 2.90)
              sharp    f16 2.89 (honest <= 1.84, o16 >= 4.55)      bf16 2.53 (1.99, 3.22)

Four things the models showed that the plan for this file had not expected, all properties of the arithmetic and
none of a kernel (the MI355X run agrees: every fa_fwd_w4 layout sits at 1.06 - 1.16 x the row form on ``sharp``):

* the "tiled" honest form is NOT within 1.05 of the "row" form: 1.02 - 1.055 x in rms on ``centered`` and 1.15 -
  1.21 x on ``sharp`` (emax up to 2 x). The row form gives the key that holds the row's max P = exp(0) = 1
  EXACTLY, so the dominant term of a sharp row carries no rounding error at all, while under the deferred rescale
  (fa_fwd_kernels.hpp kRescaleThr) P is taken relative to a stale max and that term is rounded like any other. The
  1.05 bound is therefore asserted for the "split" form, and for both forms on ``offset`` (where the output
  rounding dominates); the cap rule takes the worst honest ratio as it is, and the 1.15 x separation of every cap
  from the honest forms below it and the defects above it is asserted everywhere;
* emax is the maximum of >= 16384 errors and moves by tens of percent between two honest forms on the same data,
  so no 1.05 bound is asserted on it; EMAX_CAP takes the worst honest emax ratio as measured;
* one dropped key is 17 - 186 x on ``centered`` (asserted) but a lottery on ``sharp``, where most keys of a row
  weigh nothing (1.6 x to 450 x over the classes): ``centered`` is the family on which a lost key shows;
* partials rounded to the io dtype before the merge cost 1.21 - 1.37 x in rms (one more output rounding), which is
  BELOW the caps: this defect is measured and shown to stand 1.15 x clear of the honest split form, but the caps
  cannot see it. ``flash_attn_paged_shared_prefix_func`` does exactly this by design (its docstring: "the two
  partial outputs are rounded to q's dtype before the merge"), so its honest model rounds the partials too.

The honest |bias| <= eps / 64 holds on the self-test shapes; at 16384 keys in bf16 (outputs all next to 2.0, where
the bf16 grid changes) the honest model itself has -1.5e-4 = eps / 26, and the kernels the same figure.

The GPU part prints one line per case, ``ACCURACY <path> <family> <dtype> rms_ratio=... emax_ratio=... bias=...``.
"""
from __future__ import annotations

import functools
import math
import zlib

import pytest
import torch

import accuracy as A
from accuracy import BF16, EPS, F16, NAMES

DEV = "cuda:0"
FP8 = torch.float8_e4m3fn
SEPARATION = 1.15
DTYPES = [F16, BF16]
DT_IDS = ["f16", "bf16"]


def crc(*key):
    return zlib.crc32(repr(key).encode())


def dv(*ts):
    return tuple(t.to(DEV) for t in ts)


def descales(b, hkv, seed):
    """FP8 descales that are NOT powers of two: 0.011 (1 + rand) per (b, kv-head), fp32 [B, Hkv]."""
    return 0.011 * (1 + torch.rand(b, hkv, generator=torch.Generator().manual_seed(seed)))


def quant(x, descale):
    """The FP8 write formula on the host (tests/test_fp8_kvcache.py quant)."""
    return (x.float() / descale[:, :, None, None]).clamp(-448.0, 448.0).to(FP8)


def sink_logits(hq, seed):
    """randn + 2: the sink holds a real share of every row's weight."""
    return torch.randn(hq, generator=torch.Generator().manual_seed(seed)) + 2.0


class Problem:
    """One launch's inputs in the dense form every entry reduces to, with its reference and honest model (each
    computed once and never modified): q [B, Hq, Sq, D], the key buffers k / v [B | 1, Hkv, N, D] as the MODELS
    read them (an FP8 pool: the widened bytes, with ``kscale`` / ``vscale``), the rows' key ranges."""

    def __init__(self, fam, dtype, q, k, v, lo, hi, sinks=None, kscale=None, vscale=None, k8=None, v8=None):
        self.fam, self.dtype, self.q, self.k, self.v, self.lo, self.hi = fam, dtype, q, k, v, lo, hi
        self.kw = dict(sinks=sinks, kscale=kscale, vscale=vscale)
        self.sinks, self.kscale, self.vscale, self.k8, self.v8 = sinks, kscale, vscale, k8, v8
        self.scale = q.size(-1) ** -0.5

    def run(self, dtype=None, **kw):
        return A.model(self.q, self.k, self.v, self.lo, self.hi, self.scale, dtype, **kw, **self.kw)

    @functools.cached_property
    def ref(self):
        return self.run()

    @functools.cached_property
    def honest(self):
        return self.run(self.dtype)

    def measure(self, out):
        return A.measure(out, self.ref[0], self.lo, self.hi)


def problem(fam, dtype, b, hq, hkv, sq, n, d, seed, ks, ke, causal, w=-1, qs=None, qe=None, shared=False, fp8=False,
            sinks=False, prefix=0):
    """A Problem of family ``fam``. shared: one key buffer for all sequences (a packed varlen batch). fp8: k / v
    go through the FP8 write formula with ``descales`` and the models read the widened bytes. prefix: the first
    ``prefix`` keys of every sequence are sequence 0's."""
    t = lambda x: None if x is None else torch.as_tensor(x, dtype=torch.int32)  # noqa: E731
    q, k, v = A.family(fam, b, 1 if shared else b, hq, hkv, sq, n, d, dtype, seed)
    if prefix:
        k[:, :, :prefix], v[:, :, :prefix] = k[:1, :, :prefix], v[:1, :, :prefix]
    lo, hi = A.span(t(ks), t(ke), sq, causal, w, t(qs), t(qe))
    kw = {}
    if fp8:
        kd, vd = descales(b, hkv, seed + 1), descales(b, hkv, seed + 2)
        k8, v8 = quant(k, kd), quant(v, vd)
        k, v = k8.float(), v8.float()
        kw = dict(kscale=kd, vscale=vd, k8=k8, v8=v8)
    if sinks:
        kw["sinks"] = sink_logits(hq, seed + 3)
    return Problem(fam, dtype, q, k, v, lo, hi, **kw)


# ------------------------------------------------------------------------------------------------
# CPU: the models, the caps, and that the caps separate honest arithmetic from every planted defect
# ------------------------------------------------------------------------------------------------
DEC_LENS = (750, 768, 350, 555, 449, 700, 512, 640)
CLASSES = {  # one representative shape per kernel class
    "prefill": dict(b=1, hq=4, hkv=2, sq=128, n=600, ke=[600], causal=True),
    "decode_split": dict(b=8, hq=32, hkv=8, sq=1, n=768, ke=DEC_LENS, causal=False),
    "fp8": dict(b=8, hq=32, hkv=8, sq=1, n=768, ke=DEC_LENS, causal=False, fp8=True),
    "sink": dict(b=8, hq=32, hkv=8, sq=1, n=768, ke=DEC_LENS, causal=False, sinks=True),
}
MIN_ELEMENTS = 16384  # below that the sampling noise of a ratio eats the margin
RMS_DEFECTS = {"centered": ("trunc", "o16", "exp", "drop"), "sharp": ("o16", "exp")}  # (truncation on sharp: the bias)


def class_problem(cls, fam, dtype):
    c = dict(CLASSES[cls])
    b, ke = c.pop("b"), c.pop("ke")
    return problem(fam, dtype, b, c.pop("hq"), c.pop("hkv"), c.pop("sq"), c.pop("n"), 128, crc(cls, fam, NAMES[dtype]),
                   [0] * b, list(ke), c.pop("causal"), **c)


@functools.lru_cache(maxsize=None)
def ratios(cls, fam, dtype):
    """{model name: (rms / rms_row, emax / emax_row, bias)} of the honest forms and the planted defects on this
    class's shape; "row" holds its absolute (rms, emax, bias)."""
    p = class_problem(cls, fam, dtype)
    assert p.ref[0].numel() >= MIN_ELEMENTS, p.ref[0].numel()
    rms, bias, emax = p.measure(p.honest[0])
    out = {"row": (rms, emax, bias)}
    runs = [("tiled", dict(variant="tiled")), ("split", dict(variant="split")), ("trunc", dict(defect="trunc"))]
    if fam != "offset":
        runs += [(name, dict(defect=name)) for name in ("o16", "exp", "drop", "partials")]
    for name, kw in runs:
        r, bi, e = p.measure(p.run(dtype, **kw)[0])
        out[name] = (r / rms, e / emax, bi)
    return out


@functools.lru_cache(maxsize=None)
def caps(fam, dtype):
    """(RMS_CAP, EMAX_CAP, worst honest rms ratio, weakest defect rms ratio, worst honest emax ratio, weakest "o16"
    emax ratio) of this (family, dtype) over CLASSES: each cap the geometric mean of the two figures it separates."""
    tabs = [ratios(cls, fam, dtype) for cls in CLASSES]
    h_rms = max(max(t["tiled"][0], t["split"][0], 1.0) for t in tabs)
    d_rms = min(t[name][0] for t in tabs for name in RMS_DEFECTS[fam])
    h_emax = max(max(t["tiled"][1], t["split"][1], 1.0) for t in tabs)
    d_emax = min(t["o16"][1] for t in tabs)
    return math.sqrt(h_rms * d_rms), math.sqrt(h_emax * d_emax), h_rms, d_rms, h_emax, d_emax


def test_the_reference_and_the_row_form_are_attend():
    """``model`` with dtype None is the float64 ``attend``; its "row" form is ``attend(emul=dtype)`` up to the
    summation order of an fp32 matmul. GQA, a window and a causal diagonal in one case."""
    p = problem("centered", F16, 2, 4, 2, 40, 300, 64, 11, [0, 20], [300, 250], True, w=100)
    ref, _ = A.attend(p.q, p.k, p.v, p.lo, p.hi, p.scale)
    assert (p.ref[0] - ref).abs().max().item() < 1e-12
    want = A.measure(A.attend(p.q, p.k, p.v, p.lo, p.hi, p.scale, emul=F16)[0], ref, p.lo, p.hi)
    got = p.measure(p.honest[0])
    assert abs(got[0] / want[0] - 1) < 0.02 and abs(got[2] / want[2] - 1) < 0.25, (got, want)
    lse = torch.logsumexp((p.q[1, 3].double() @ p.k[1, 1].double().T * p.scale)[5, int(p.lo[1, 5]):int(p.hi[1, 5])], 0)
    assert abs(p.ref[1][1, 3, 5].item() - lse.item()) < 1e-12
    assert abs(A.lse_fp32(p.q, p.k, p.lo, p.hi, p.scale)[1, 3, 5].item() - lse.item()) < 1e-5


def test_a_sink_joins_the_denominator_only_in_every_form():
    p = problem("centered", BF16, 2, 8, 2, 1, 200, 64, 12, [0, 0], [200, 77], False, sinks=True)
    plain, lse = A.model(p.q, p.k, p.v, p.lo, p.hi, p.scale)
    share = torch.exp(lse) / (torch.exp(lse) + torch.exp(p.sinks.double())[None, :, None])
    assert share.min().item() < 0.9 and share.max().item() < 0.999  # (the sink holds 0.1 % to over 10 % of a row)
    assert (p.ref[0] - plain * share[..., None]).abs().max().item() < 1e-12
    for variant in ("tiled", "split"):
        got = A.model(p.q, p.k, p.v, p.lo, p.hi, p.scale, variant=variant, sinks=p.sinks)[0]
        assert (got - p.ref[0]).abs().max().item() < 1e-12, variant


def test_truncation_rounds_toward_zero():
    x = torch.rand(4096, generator=torch.Generator().manual_seed(1)) * 3
    for dtype in DTYPES:
        t = A.toward_zero(x, dtype).float()
        assert (t <= x).all() and ((x - t) < 2 * EPS[dtype] * x + 1e-30).all() and (t < x.to(dtype).float()).any()


SELF = [(cls, fam, dt) for cls in CLASSES for fam in ("centered", "sharp") for dt in DTYPES]


@pytest.mark.parametrize("cls,fam,dtype", SELF, ids=[f"{c}-{f}-{NAMES[t]}" for c, f, t in SELF])
def test_caps_separate_honest_forms_from_planted_defects(cls, fam, dtype):
    """On this class's shape: every honest form stays 1.15 x below both caps (rms within 1.05 of the row form on
    ``centered``); every defect a cap is built from, and the dropped key, exceeds it by 1.15 x."""
    tab = ratios(cls, fam, dtype)
    rms_cap, emax_cap = caps(fam, dtype)[:2]
    for name, (r, e, bi) in tab.items():
        print(f"MODEL {cls} {fam} {NAMES[dtype]} {name}: rms {r:.3e} emax {e:.3e} bias {bi:.2e}")
    for name in ("tiled", "split"):
        r, e, _ = tab[name]
        assert r * SEPARATION <= rms_cap and e * SEPARATION <= emax_cap, (name, r, e, rms_cap, emax_cap)
    assert tab["split"][0] <= 1.05
    for name in RMS_DEFECTS[fam]:
        assert tab[name][0] >= SEPARATION * rms_cap, (name, tab[name][0], rms_cap)
    assert tab["o16"][1] >= SEPARATION * emax_cap, (tab["o16"][1], emax_cap)
    # (one more rounding of the partials: clear of the honest split form, but below the caps -- see the docstring)
    assert tab["partials"][0] >= SEPARATION * tab["split"][0], (tab["partials"][0], tab["split"][0])


@pytest.mark.parametrize("fam", ["centered", "sharp"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_caps(fam, dtype):
    rms_cap, emax_cap, h_rms, d_rms, h_emax, d_emax = caps(fam, dtype)
    print(f"CAPS {fam} {NAMES[dtype]} RMS_CAP={rms_cap:.3f} (honest <= {h_rms:.3f}, defects >= {d_rms:.3f}) "
          f"EMAX_CAP={emax_cap:.3f} (honest <= {h_emax:.3f}, o16 >= {d_emax:.3f})")
    assert d_rms / rms_cap >= SEPARATION and rms_cap / h_rms >= SEPARATION
    assert d_emax / emax_cap >= SEPARATION and emax_cap / h_emax >= SEPARATION


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bias_separates_truncation_from_rounding(cls, dtype):
    """``offset``: every honest form's |bias| is at most eps / 64 and rms within 1.05 of the row form; a truncated
    P gives at least eps / 4. The cap of the GPU tests, eps / 16, lies a factor 4 from both."""
    tab = ratios(cls, "offset", dtype)
    eps = EPS[dtype]
    for name in ("row", "tiled", "split", "trunc"):
        print(f"MODEL {cls} offset {NAMES[dtype]} {name}: bias {tab[name][2]:.3e} (eps/64 {eps / 64:.3e}, eps/4 {eps / 4:.3e})")
    for name in ("row", "tiled", "split"):
        assert abs(tab[name][2]) <= eps / 64, (name, tab[name][2])
    assert tab["tiled"][0] <= 1.05 and tab["split"][0] <= 1.05  # (outputs of O(1): the output rounding dominates)
    assert abs(tab["trunc"][2]) >= eps / 4, tab["trunc"][2]


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


def judge(path, p, out, honest=None):
    """The three assertions of the module docstring on one launch's output, after printing its ACCURACY line."""
    got = out.detach().cpu().double()
    assert got.shape == p.ref[0].shape, (path, got.shape)
    assert torch.isfinite(got).all(), f"{path}: non-finite output"
    rms, bias, emax = p.measure(got)
    h_rms, _, h_emax = p.measure(p.honest[0] if honest is None else honest)
    print(f"ACCURACY {path} {p.fam} {NAMES[p.dtype]} rms_ratio={rms / h_rms:.3f} emax_ratio={emax / h_emax:.3f} "
          f"bias={bias:.2e} (rms {rms:.3e} emax {emax:.3e})")
    if p.fam == "offset":
        assert abs(bias) <= EPS[p.dtype] / 16, f"{path}: bias {bias:.3e} exceeds eps / 16 = {EPS[p.dtype] / 16:.3e}"
    else:
        rms_cap, emax_cap = caps(p.fam, p.dtype)[:2]
        assert rms <= rms_cap * h_rms, f"{path}: rms {rms:.3e} is {rms / h_rms:.3f} x the honest model's (cap {rms_cap:.3f})"
        assert emax <= emax_cap * h_emax, f"{path}: emax {emax:.3e} is {emax / h_emax:.3f} x the honest model's (cap {emax_cap:.3f})"


def judge_lse(path, p, lse):
    """max |lse - lse64| against 4 x the same error of the fp32 torch model (fp32 scores, float32 logsumexp): the
    kernel's log2-domain form (M + log2 L) ln 2 adds two fp32 roundings and an exp2 / log2 pair to the model's one."""
    err = A.lse_error(lse.cpu(), p.ref[1])
    base = A.lse_error(A.lse_fp32(p.q, p.k, p.lo, p.hi, p.scale, p.kscale), p.ref[1])
    print(f"ACCURACY_LSE {path} {p.fam} {NAMES[p.dtype]} max_abs_err={err:.3e} fp32_model={base:.3e} ratio={err / base:.2f}")
    assert err <= 4 * base, f"{path}: lse error {err:.3e} exceeds 4 x the fp32 model's {base:.3e}"


FAMS = list(A.FAMILIES)

# ---- dense fa_fwd_w4 ------------------------------------------------------------------------
# layout -> (shape (B, Hq, Hkv, Sq, Sk), causal, (split, zigzag, head_pack, split_pairs), last_layout, head-packed, pairs)
DENSE = {
    "plain": ((2, 4, 2, 300, 300), False, (None, None, None, None), "plain", False, False),
    "zigzag": ((1, 4, 2, 1024, 1024), True, (0, 2, 0, None), "zigzag", False, False),
    "headpack": ((1, 8, 2, 600, 600), True, (0, 0, 2, None), "headpack", True, False),
    "split_halves": ((1, 4, 2, 1024, 1024), True, (2, None, 0, 0), "split", False, False),
    "split_pairs": ((1, 16, 8, 2304, 2304), True, (2, None, 0, 1), "split", False, True),
    "headpack_split": ((1, 8, 2, 1024, 1024), True, (2, None, 2, 0), "split", True, False),
}


@functools.lru_cache(maxsize=2)
def dense_problem(shape, d, dtype, fam, causal, w=-1):
    b, hq, hkv, sq, sk = shape
    return problem(fam, dtype, b, hq, hkv, sq, sk, d, crc("dense", shape, d, NAMES[dtype], fam), [0] * b, [sk] * b, causal, w)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("layout", list(DENSE))
def test_dense_prefill(dbg, layout, d, dtype, fam):
    """flash_attn_func on fa_fwd_w4 under every block layout, the causal ones forced with the knobs."""
    import flash_attention_cute_amd as m

    shape, causal, (split, zigzag, head_pack, pairs), want, hp, want_pairs = DENSE[layout]
    p = dense_problem(shape, d, dtype, fam, causal)
    m.split_errors(reset=True)
    try:
        dbg.set_split(split)
        dbg.set_zigzag(zigzag)
        dbg.set_head_pack(head_pack)
        dbg.set_split_pairs(pairs)
        out = m.flash_attn_func(*dv(p.q, p.k, p.v), causal=causal)
        labels = dbg.last_path(), dbg.last_layout(), dbg.last_head_pack(), dbg.last_split_pairs()
        torch.cuda.synchronize()
    finally:
        dbg.set_split()
        dbg.set_zigzag()
        dbg.set_head_pack()
        dbg.set_split_pairs()
    assert labels == ("w4", want, hp, want_pairs), labels
    assert m.split_errors() == 0
    judge(f"w4-{layout}-d{d}", p, out)


# ---- the entries that share that body but address differently ----------------------------
VARLEN_LENS = (190, 65, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_varlen(dbg, dtype, fam):
    """flash_attn_varlen_func: 3 ragged sequences packed back to back, causal."""
    from flash_attention_cute_amd import flash_attn_varlen_func

    cu = [0, 190, 255, 555]
    p = problem(fam, dtype, 3, 4, 2, max(VARLEN_LENS), cu[-1], 128, crc("varlen", NAMES[dtype], fam), cu[:-1], cu[1:], True,
                qs=[0, 0, 0], qe=list(VARLEN_LENS), shared=True)
    pack = lambda t: torch.cat([t[i, :, :n].transpose(0, 1) for i, n in enumerate(VARLEN_LENS)]).contiguous()  # noqa: E731
    unpack = torch.zeros(p.q.shape, dtype=torch.float64)
    kp, vp = (t[0].transpose(0, 1).contiguous() for t in (p.k, p.v))
    cu_t = torch.tensor(cu, dtype=torch.int32)
    out = flash_attn_varlen_func(*dv(pack(p.q), kp, vp, cu_t, cu_t), max(VARLEN_LENS), max(VARLEN_LENS), causal=True)
    assert dbg.last_path() == "w4"
    out = out.cpu().double()
    for i, n in enumerate(VARLEN_LENS):
        unpack[i, :, :n] = out[cu[i]:cu[i + 1]].transpose(0, 1)
    judge("w4-varlen", p, unpack)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_padded_left(dbg, dtype, fam):
    """flash_attn_padded_func with left padding: sequence b's keys and queries are the LAST rows of its tensors."""
    from flash_attention_cute_amd import flash_attn_padded_func

    b, s, pad = 3, 300, [0, 77, 236]
    p = problem(fam, dtype, b, 8, 2, s, s, 128, crc("padded", NAMES[dtype], fam), pad, [s] * b, True, qs=pad, qe=[s] * b)
    rng = [torch.tensor(x, dtype=torch.int32) for x in (pad, [s] * b, pad, [s] * b)]
    out = flash_attn_padded_func(*dv(p.q, p.k, p.v, *rng), causal=True)
    assert dbg.last_path() == "w4"
    live = (p.hi > p.lo)[:, None, :, None]
    out = torch.where(live, out.cpu().double(), 0.0)  # (rows outside [q_start, q_end) are not measured)
    judge("w4-padded-left", p, out)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("w", [63, 300])
def test_window(dbg, w, dtype, fam):
    from flash_attention_cute_amd import flash_attn_window_func

    p = dense_problem((1, 4, 2, 600, 600), 128, dtype, fam, True, w)
    out = flash_attn_window_func(*dv(p.q, p.k, p.v), w, causal=True)
    assert dbg.last_path() == "w4"
    judge(f"w4-window{w}", p, out)


def rotate(x, cos, sin, dt):
    """Rotate-half RoPE of x [B, H, S, D] with cos / sin [B, S, D], in ``dt``."""
    x, cos, sin = x.to(dt), cos.to(dt)[:, None], sin.to(dt)[:, None]
    half = x.size(-1) // 2
    return x * cos + torch.cat((-x[..., half:], x[..., :half]), dim=-1) * sin


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_rope(dbg, dtype, fam):
    """flash_attn_rope_func on keys rotated by apply_rope. The reference rotates the unrotated 16-bit q and k in
    float64 and rounds nothing; the honest model rotates in fp32 and rounds q and k once (fa_fwd_kernels.hpp rope8,
    csrc/fa_rope.hip)."""
    from flash_attention_cute_amd import apply_rope, flash_attn_rope_func
    from test_rope import tables

    b, hq, hkv, s, d = 2, 4, 2, 300, 128
    p = problem(fam, dtype, b, hq, hkv, s, s, d, crc("rope", NAMES[dtype], fam), [0] * b, [s] * b, True)
    cos, sin = tables(b, s, d, dtype, 5)
    ref = A.model(rotate(p.q, cos, sin, torch.float64), rotate(p.k, cos, sin, torch.float64), p.v, p.lo, p.hi, p.scale)
    honest = A.model(rotate(p.q, cos, sin, torch.float32).to(dtype), rotate(p.k, cos, sin, torch.float32).to(dtype), p.v,
                     p.lo, p.hi, p.scale, dtype)[0]
    p.__dict__["ref"] = ref
    qd, kd, vd, cd, sd = dv(p.q, p.k, p.v, cos, sin)
    out = flash_attn_rope_func(qd, apply_rope(kd, cd, sd), vd, cd, sd, causal=True)
    assert dbg.last_path() == "w4"
    judge("w4-rope", p, out, honest)


# ---- split-KV decode, dense ---------------------------------------------------------------
DECODE = {  # form -> (shape, causal, set_dec_fuse, path, fused)
    "unsplit": ((4, 32, 8, 1, 257), False, None, "decode", None),
    "fused": ((1, 32, 8, 1, 16384), False, None, "decode_split", True),
    "combine": ((1, 32, 8, 1, 16384), False, 0, "decode_split", False),
    "causal3": ((1, 8, 2, 3, 7000), True, None, "decode_split", None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", list(DECODE))
def test_dense_decode(dbg, form, dtype, fam):
    from flash_attention_cute_amd import flash_attn_func

    shape, causal, fuse, path, fused = DECODE[form]
    p = dense_problem(shape, 128, dtype, fam, causal)
    try:
        dbg.set_dec_fuse(fuse)
        out = flash_attn_func(*dv(p.q, p.k, p.v), causal=causal)
        labels = dbg.last_path(), dbg.last_dec_fused()
        torch.cuda.synchronize()
    finally:
        dbg.set_dec_fuse(None)
    assert labels[0] == path and (fused is None or labels[1] == fused), labels
    judge(f"{path}-{form}", p, out)


# ---- paged decode -------------------------------------------------------------------------
PAGE = 64
PAGED_LENS = (37, 1000, 2049, 4000)


def to_pool(p, lens, page, seed, shared_prefix=0):
    """The problem's dense keys (the e4m3 bytes of an FP8 problem) scattered into poisoned pools through a shuffled
    table: every row that holds no key is NaN (0x7F in an e4m3 pool), every unused table entry -1. shared_prefix:
    the first rows of every sequence's table name sequence 0's pages. Returns (k pool, v pool, table, lengths)."""
    ksrc, vsrc = (p.k, p.v) if p.k8 is None else (p.k8, p.v8)
    b, hkv, cap, d = ksrc.shape
    max_pages = (cap + page - 1) // page
    ids = torch.randperm(b * max_pages + 3, generator=torch.Generator().manual_seed(seed)).tolist()
    table = torch.full((b, max_pages), -1, dtype=torch.int32)

    def pool():
        if p.k8 is not None:
            return torch.full((len(ids), hkv, page, d), 0x7F, dtype=torch.uint8).view(FP8)
        return torch.full((len(ids), hkv, page, d), float("nan"), dtype=p.dtype)

    kc, vc = pool(), pool()
    n_ids = len(ids)
    for i, n in enumerate(lens):
        for j in range((n + page - 1) // page):
            if i > 0 and (j + 1) * page <= shared_prefix:
                table[i, j] = table[0, j]
                continue
            pg, n0 = ids.pop(), j * page
            rows = min(n, n0 + page) - n0
            table[i, j] = pg
            kc[pg, :, :rows] = ksrc[i, :, n0:n0 + rows]
            vc[pg, :, :rows] = vsrc[i, :, n0:n0 + rows]
    assert kc.size(0) == n_ids
    return kc, vc, table, torch.tensor(lens, dtype=torch.int32)


@functools.lru_cache(maxsize=2)
def paged_problem(dtype, fam, fp8, w, sinks):
    b, n = len(PAGED_LENS), 4032
    return problem(fam, dtype, b, 32, 8, 1, n, 128, crc("paged", NAMES[dtype], fam, fp8), [0] * b, list(PAGED_LENS), False,
                   w, fp8=fp8, sinks=sinks)


def paged_kw(p):
    kw = {}
    if p.kscale is not None:
        kw.update(k_descale=p.kscale.to(DEV), v_descale=p.vscale.to(DEV))
    if p.sinks is not None:
        kw["sinks"] = p.sinks.to(DEV)
    return kw


# kind -> (window_left, sinks, split launch: lengths up to 4000 split; a window of 500 keys does not)
PAGED_KINDS = {"plain": (-1, False, True), "window500": (500, False, False), "sinks": (-1, True, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", list(PAGED_KINDS))
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_paged_decode(dbg, fp8, kind, dtype, fam):
    """flash_attn_paged_func, page 64 through a shuffled table: both pools (the FP8 one with descales that are NOT
    powers of two, so how the descale is folded counts), plain, with window_left 500, with sinks."""
    from flash_attention_cute_amd import flash_attn_paged_func

    w, sinks, split = PAGED_KINDS[kind]
    p = paged_problem(dtype, fam, fp8, w, sinks)
    pool = to_pool(p, PAGED_LENS, PAGE, crc("pool", fp8, kind))
    out = flash_attn_paged_func(*dv(p.q, *pool), window_left=w, **paged_kw(p))
    path = dbg.last_path()
    torch.cuda.synchronize()
    assert path == ("decode_paged_fp8" if fp8 else "decode_paged") + ("_split" if split else ""), path
    judge(f"{path}-{kind}", p, out)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_paged_decode_lse(dbg, fp8, dtype, fam):
    """return_lse=True: O as above, and the LSE against the fp32 model's error on the same data."""
    from flash_attention_cute_amd import flash_attn_paged_func

    p = paged_problem(dtype, fam, fp8, -1, False)
    pool = to_pool(p, PAGED_LENS, PAGE, crc("pool", fp8, "lse"))
    out, lse = flash_attn_paged_func(*dv(p.q, *pool), return_lse=True, **paged_kw(p))
    path = dbg.last_path()
    torch.cuda.synchronize()
    assert path == ("decode_paged_fp8_split" if fp8 else "decode_paged_split"), path
    judge(f"{path}-lse", p, out)
    judge_lse(f"{path}-lse", p, lse)


# ---- paged prefill-sized blocks and the ragged step -----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_paged_prefill(dbg, dtype, fam):
    """flash_attn_paged_func with Sq 300 over lengths (449, 300): the paged fa_fwd_w4, causal."""
    from flash_attention_cute_amd import flash_attn_paged_func

    lens = (449, 300)
    p = problem(fam, dtype, 2, 8, 2, 300, 512, 128, crc("pp", NAMES[dtype], fam), [0, 0], list(lens), True)
    out = flash_attn_paged_func(*dv(p.q, *to_pool(p, lens, PAGE, 21)), causal=True)
    assert dbg.last_path() == "w4" and dbg.last_prefill_paged()
    judge("w4-paged-prefill", p, out)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_paged_varlen(dbg, dtype, fam):
    """flash_attn_paged_varlen_func: chunks (128, 37, 1) over lengths (700, 449, 64), causal."""
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    sqs, lens = (128, 37, 1), (700, 449, 64)
    p = problem(fam, dtype, 3, 8, 2, max(sqs), 704, 128, crc("pv", NAMES[dtype], fam), [0] * 3, list(lens), True,
                qs=[0] * 3, qe=list(sqs))
    q = torch.cat([p.q[i, :, :s].transpose(0, 1) for i, s in enumerate(sqs)]).contiguous()
    cu = torch.tensor([0, 128, 165, 166], dtype=torch.int32)
    kc, vc, table, sl = to_pool(p, lens, PAGE, 22)
    out = flash_attn_paged_varlen_func(*dv(q, kc, vc, cu), max(sqs), *dv(table, sl), causal=True)
    assert dbg.last_path() == "w4" and dbg.last_prefill_paged()
    out = out.cpu().double()
    unpack = torch.zeros(p.q.shape, dtype=torch.float64)
    for i, s in enumerate(sqs):
        unpack[i, :, :s] = out[int(cu[i]):int(cu[i + 1])].transpose(0, 1)
    judge("w4-paged-varlen", p, unpack)


# ---- merges -------------------------------------------------------------------------------
def merge_model(outs, lses, dtype=None):
    """The merge of flash_attn_merge_states in float64, or (dtype) in fp32 rounded once: (out, lse)."""
    dt = torch.float64 if dtype is None else torch.float32
    l = lses.to(dt)
    mx = l.max(dim=0).values
    w = torch.exp(l - mx.masked_fill(mx == A.NEG_INF, 0))
    sw = w.sum(dim=0)
    o = (w[..., None] * outs.to(dt)).sum(dim=0) / sw.masked_fill(sw == 0, 1)[..., None]
    if dtype is not None:
        o = o.to(dtype)
    return o.double(), (mx + torch.log(sw)).double()


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_shared_prefix(dbg, dtype, fam):
    """flash_attn_paged_shared_prefix_func, B 8, prefix 512, suffixes 33 .. 300: three launches and a merge. Its
    honest model has one step more than the single-launch paths': the prefix and suffix partials are rounded to the
    io dtype before the merge, as the function documents (flash_attention.py: ``outs`` is allocated in q's dtype)."""
    from flash_attention_cute_amd import flash_attn_paged_shared_prefix_func

    b, prefix = 8, 512
    lens = [prefix + s for s in (33, 64, 100, 129, 200, 255, 256, 300)]
    p = problem(fam, dtype, b, 32, 8, 1, 832, 128, crc("sp", NAMES[dtype], fam), [0] * b, lens, False, prefix=prefix)
    zero, pre, end = (torch.tensor(x, dtype=torch.int32) for x in ([0] * b, [prefix] * b, lens))
    parts = [A.model(p.q, p.k, p.v, *A.span(s, e, 1, False), p.scale, dtype) for s, e in ((zero, pre), (pre, end))]
    honest, _ = merge_model(torch.stack([o for o, _ in parts]), torch.stack([l for _, l in parts]), dtype)
    out, lse = flash_attn_paged_shared_prefix_func(*dv(p.q, *to_pool(p, lens, PAGE, 23, shared_prefix=prefix)), prefix,
                                                   return_lse=True)
    assert dbg.last_path() in ("decode_paged", "decode_paged_split")
    judge("shared-prefix", p, out, honest)
    judge_lse("shared-prefix", p, lse)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [2, 16])
def test_merge_states(dbg, n, dtype, fam):
    """flash_attn_merge_states on 16-bit partials and fp32 LSEs: a float64 merge of the same inputs is the
    reference, that merge in fp32 rounded once the honest model. The families here: partials ``randn`` (+ 2:
    offset), LSEs ``randn`` (sharp: 5 randn, so one part holds most of a row)."""
    from flash_attention_cute_amd import flash_attn_merge_states

    g = torch.Generator().manual_seed(crc("merge", n, NAMES[dtype], fam))
    outs = (torch.randn(n, 2, 8, 8, 128, generator=g) + (2.0 if fam == "offset" else 0.0)).to(dtype)
    lses = torch.randn(n, 2, 8, 8, generator=g) * (5.0 if fam == "sharp" else 1.0)
    ref, ref_lse = merge_model(outs, lses)
    p = Problem(fam, dtype, outs[0], None, None, torch.zeros(2, 8, dtype=torch.long), torch.ones(2, 8, dtype=torch.long))
    assert ref.numel() >= MIN_ELEMENTS
    p.__dict__["ref"] = (ref, ref_lse)
    out, lse = flash_attn_merge_states(*dv(outs, lses), return_lse=True)
    torch.cuda.synchronize()
    judge(f"merge-n{n}", p, out, merge_model(outs, lses, dtype)[0])
    err = A.lse_error(lse.cpu(), ref_lse)
    base = A.lse_error(merge_model(outs, lses, torch.float32)[1], ref_lse)
    print(f"ACCURACY_LSE merge-n{n} {fam} {NAMES[dtype]} max_abs_err={err:.3e} fp32_model={base:.3e} ratio={err / base:.2f}")
    assert err <= 4 * base
