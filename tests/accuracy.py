"""What an attention kernel's arithmetic should cost: a float64 reference, a model of the honest kernel, planted
defects, and three error metrics. CPU torch only; nothing here imports the kernels (tests/test_accuracy_budget.py
is the user; tests/test_edge_weight.py takes ``span`` and ``attend`` from here).

The honest kernel (flash_attention_cute_amd/csrc/fa_fwd_kernels.hpp, header): fp32 scores, P = exp(s - m) rounded
to nearest even to the io dtype before P.V, the row sum of the fp32 P, fp32 accumulation of P.V, the output O / l
rounded once. ``model`` restates it in three forms a kernel may legitimately take:

* "row"   -- the whole row at once (this is ``attend(..., emul=dtype)``);
* "tiled" -- 32-key tiles with a running max that is only raised when a tile's max outgrows it by more than
  ``kRescaleThr = 8`` log2 units (the deferred rescale of fa_fwd_kernels.hpp), all in fp32;
* "split" -- the keys cut into 3 ranges, each an fp32 partial (O / l and a log2-domain lse), merged in fp32 as
  ``decode_merge`` (fa_decode.hpp) does, rounded once.

``defect`` plants one arithmetic fault in that model (``DEFECTS``). With ``dtype=None`` the same function is the
float64 reference. GQA, per-row key ranges (``span``: bottom-right causal, ``window_left``, per-sequence key
ranges), one sink logit per q-head that joins the denominator only, FP8 pools as widened bytes with a scale on
the logits and one on the output, and the natural-log LSE are all arguments of the one function.
"""
from __future__ import annotations

import math

import torch

F16, BF16 = torch.float16, torch.bfloat16
NAMES = {F16: "f16", BF16: "bf16"}
EPS = {F16: 2.0 ** -11, BF16: 2.0 ** -8}  # the unit roundoff of the io dtype
TILE = 32  # keys per tile of the "tiled" form and of the "o16" defect
RESCALE_THR = 8.0 * math.log(2.0)  # kRescaleThr (8 log2 units) in natural-log units
SPLITS = 3
DEFECTS = ("trunc", "o16", "exp", "drop", "partials")
NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------
# the mask as key ranges and the plain reference on them (used by tests/test_edge_weight.py as they are)
# ------------------------------------------------------------------------------------------------
def span(ks, ke, sq, causal, w=-1, qs=None, qe=None):
    """Query row m of sequence b sees the buffer rows [lo[b, m], hi[b, m]) (lo == hi == 0: none). Keys
    [ks, ke), queries [qs, qe) of Sq (the sequence's LAST positions), bottom-right causal, window w >= 0:
    key n visible iff n >= m + L - Sq_b - w (the semantics of include/fa_gfx950.h)."""
    ks, ke = ks.long()[:, None], ke.long()[:, None]
    qs = torch.zeros_like(ks) if qs is None else qs.long()[:, None]
    qe = torch.full_like(ks, sq) if qe is None else qe.long()[:, None]
    m = torch.arange(sq)[None] - qs
    n_k, n_q = ke - ks, qe - qs
    diag = n_k - n_q
    hi = ks + (torch.minimum(n_k, m + diag + 1) if causal else n_k.expand(-1, sq))
    lo = ks + ((m + diag - w).clamp(min=0) if w >= 0 else torch.zeros_like(m))
    live = (m >= 0) & (m < n_q) & (hi > lo)
    return torch.where(live, lo, 0), torch.where(live, hi, 0)


def attend(q, k, v, lo, hi, scale, emul=None):
    """softmax(scale q k^T) v with row (b, *, m) over buffer rows [lo[b, m], hi[b, m]) (none: 0). float64, or
    (``emul`` a dtype) the honest kernel's arithmetic: fp32 scores, P rounded to the io dtype before P.V, an
    fp32 row sum, the output rounded. Returns (out [B, Hq, Sq, D] float64, P [B, Hq, Sq, N])."""
    b, hq, sq, d = q.shape
    hkv, n = k.size(1), k.size(2)
    g = hq // hkv
    dt = torch.float64 if emul is None else torch.float32
    s = torch.matmul(q.reshape(b, hkv, g * sq, d).to(dt), k.to(dt).transpose(-1, -2)) * scale
    pos = torch.arange(n)
    mask = ((pos >= lo[:, :, None]) & (pos < hi[:, :, None]))[:, None].repeat(1, 1, g, 1)  # [B, 1, g * Sq, N]
    s = s.masked_fill(~mask, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))
    l = p.sum(-1, keepdim=True)
    pv = p.to(emul).to(dt) if emul is not None else p
    o = torch.where(l > 0, torch.matmul(pv, v.to(dt)) / l.clamp(min=1e-30), torch.zeros((), dtype=dt))
    if emul is not None:
        o = o.to(emul)
    return o.double().reshape(b, hq, sq, d), (p / l.clamp(min=1e-30)).reshape(b, hq, sq, n)


# ------------------------------------------------------------------------------------------------
# the model: reference (dtype None), honest forms, planted defects
# ------------------------------------------------------------------------------------------------
def toward_zero(p, dtype):
    """p >= 0 (fp32) converted to ``dtype`` by truncation instead of round-to-nearest-even."""
    h = p.to(dtype)
    bits = h.view(torch.int16) - (h.float() > p).to(torch.int16)  # (positive: one ulp down is one bit pattern down)
    return bits.view(dtype)


def _finite(m):
    return torch.where(torch.isfinite(m), m, torch.zeros_like(m))


def _to_p(p, dtype, dt, defect):
    """P as the P.V product reads it."""
    if dtype is None:
        return p
    return (toward_zero(p, dtype) if defect == "trunc" else p.to(dtype)).to(dt)


def _add_sink(m, l, o, sink):
    """The sink logit joins the denominator (and the max) once, where the final row is produced."""
    if sink is None:
        return m, l, o
    m_f = torch.maximum(m, sink)
    a = torch.exp(m - _finite(m_f))  # (a row without keys: m and its sink are -inf, and both terms are 0)
    return m_f, l * a + torch.exp(sink - _finite(m_f)), o * a[:, None]


def _row(s, vv, dtype, defect, gen):
    """One pass over the whole row: (m, l, P.V unnormalised)."""
    dt = s.dtype
    m = s.amax(-1)
    p = torch.exp(s - _finite(m)[:, None])
    if defect == "exp":  # an exponential off by one unit roundoff of the io dtype, either way
        sign = torch.randint(0, 2, p.shape, generator=gen).to(dt) * 2 - 1
        p = p * (1 + EPS[dtype] * sign)
    return m, p.sum(-1), torch.matmul(_to_p(p, dtype, dt, defect), vv)


def _tiled(s, vv, dtype, defect, t_lo, t_hi):
    """TILE-key tiles with the running max and the deferred rescale; "o16": O kept in the io dtype between tiles."""
    dt = s.dtype
    r = s.size(0)
    m = torch.full((r,), NEG_INF, dtype=dt)
    l = torch.zeros(r, dtype=dt)
    o = torch.zeros(r, vv.size(1), dtype=dt)
    for t0 in range(t_lo // TILE * TILE, t_hi, TILE):
        st = s[:, t0:t0 + TILE]
        mx = st.amax(-1)
        grow = mx > m + RESCALE_THR  # (a row's first visible key: m is -inf)
        m_new = torch.where(grow, torch.maximum(m, mx), m)
        alpha = torch.where(grow & torch.isfinite(m), torch.exp(_finite(m) - _finite(m_new)), torch.ones_like(m))
        m = m_new
        p = torch.exp(st - _finite(m)[:, None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[:, None] + torch.matmul(_to_p(p, dtype, dt, defect), vv[t0:t0 + TILE])
        if defect == "o16":
            o = o.to(dtype).to(dt)
    return m, l, o


def _problem(qr, kk, vv, lo, hi, sc, sink, dtype, variant, defect, gen):
    """Rows qr [R, D] over keys kk / vv [N, D], row r over [lo[r], hi[r]): (O / l [R, D], natural lse [R]), in
    float64 (dtype None) or fp32, not yet rounded."""
    dt = torch.float64 if dtype is None else torch.float32
    n = kk.size(0)
    pos = torch.arange(n)
    mask = (pos >= lo[:, None]) & (pos < hi[:, None])
    if defect == "drop":  # one interior key per row, on no tile boundary: n % 32 == 13, another tile for every row
        first = lo + (13 - lo) % TILE
        count = ((hi - 1 - first + TILE - 1) // TILE).clamp(min=1)  # candidates first, first + 32, .. below hi - 1
        pick = first + TILE * ((torch.arange(lo.numel()) * 7) % count)
        mask &= ~((pos == pick[:, None]) & (pick < hi - 1)[:, None])
    s = (torch.matmul(qr.to(dt), kk.to(dt).T) * sc).masked_fill(~mask, NEG_INF)
    vv = vv.to(dt)
    live = hi > lo
    t_lo, t_hi = (int(lo[live].min()), int(hi[live].max())) if live.any() else (0, 0)
    if variant == "split" or defect == "partials":
        cuts = [t_lo + (t_hi - t_lo) * i // SPLITS // TILE * TILE for i in range(SPLITS)] + [t_hi]
        cuts[0] = t_lo
        parts = []
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            inside = (pos >= c0) & (pos < c1)
            m, l, o = _row(s.masked_fill(~inside, NEG_INF), vv, dtype, None, gen)
            o = o / l.clamp(min=1e-30)[:, None]
            if defect == "partials":
                o = o.to(dtype).to(dt)
            lse2 = torch.where(l > 0, _finite(m) * math.log2(math.e) + torch.log2(l.clamp(min=1e-30)), NEG_INF)
            parts.append((o, lse2))
        lse2 = torch.stack([p[1] for p in parts])  # the merge of fa_decode.hpp decode_merge, in the log2 domain
        top = lse2.amax(0)
        if sink is not None:
            top = torch.maximum(top, sink * math.log2(math.e))
        w = torch.exp2(lse2 - _finite(top))
        sw = w.sum(0)
        o = (w[:, :, None] * torch.stack([p[0] for p in parts])).sum(0)
        if sink is not None:
            sw = sw + torch.exp2(sink * math.log2(math.e) - top) * (w.sum(0) > 0)
        out = o / sw.clamp(min=1e-30)[:, None]
        lse = torch.where(sw > 0, (_finite(top) + torch.log2(sw.clamp(min=1e-30))) * math.log(2.0), NEG_INF)
        return out * live[:, None], lse
    if variant == "tiled" or defect == "o16":
        m, l, o = _tiled(s, vv, dtype, defect, t_lo, t_hi)
    else:
        m, l, o = _row(s, vv, dtype, defect, gen)
    m, l, o = _add_sink(m, l, o, None if sink is None else torch.where(live, sink, NEG_INF))
    out = torch.where((l > 0)[:, None], o / l.clamp(min=1e-30)[:, None], torch.zeros((), dtype=dt))
    return out, torch.where(l > 0, _finite(m) + torch.log(l.clamp(min=1e-30)), NEG_INF)


def model(q, k, v, lo, hi, scale, dtype=None, variant="row", defect=None, sinks=None, kscale=None, vscale=None):
    """Attention of q [B, Hq, Sq, D] over k / v [B | 1, Hkv, N, D], row (b, *, m) over the buffer rows
    [lo[b, m], hi[b, m]). ``dtype`` None: the float64 reference; else the honest kernel's arithmetic in that io
    dtype, in the form ``variant`` ("row", "tiled", "split"), with the fault ``defect`` (one of DEFECTS) planted.
    sinks [Hq]: one logit per q-head in final-logit units, in the denominator only. kscale / vscale [B, Hkv] (an
    FP8 pool, k / v its widened bytes): the logits are ``scale * kscale * q . k``, the output ``vscale * P . v / l``,
    both applied in the working precision before the one rounding. Computed one (b, kv-head) at a time, so the
    scores never exceed g * Sq * N elements. Returns (out [B, Hq, Sq, D] float64, lse [B, Hq, Sq] float64: the
    natural-log sum over the visible keys (and the sink), -inf for a row that sees none)."""
    b, hq, sq, d = q.shape
    hkv = k.size(1)
    g = hq // hkv
    dt = torch.float64 if dtype is None else torch.float32
    gen = torch.Generator().manual_seed(12345)
    out = torch.zeros(b, hq, sq, d, dtype=torch.float64)
    lse = torch.full((b, hq, sq), NEG_INF, dtype=torch.float64)
    for i in range(b):
        ik = i if k.size(0) > 1 else 0
        for h in range(hkv):
            heads = slice(h * g, (h + 1) * g)
            sc = scale * (1.0 if kscale is None else float(kscale[i, h]))
            sink = None if sinks is None else sinks[heads].to(dt).repeat_interleave(sq)
            o, l = _problem(q[i, heads].reshape(g * sq, d), k[ik, h], v[ik, h], lo[i].repeat(g), hi[i].repeat(g), sc,
                            sink, dtype, variant, defect, gen)
            if vscale is not None:
                o = o * vscale[i, h].to(dt)
            if dtype is not None:
                o = o.to(dtype)
            out[i, heads] = o.double().reshape(g, sq, d)
            lse[i, heads] = l.double().reshape(g, sq)
    return out, lse


def lse_fp32(q, k, lo, hi, scale, kscale=None):
    """The fp32 model the kernels' LSE is measured against: fp32 scores, ``torch.logsumexp`` in float32."""
    b, hq, sq, d = q.shape
    hkv, n = k.size(1), k.size(2)
    g = hq // hkv
    pos = torch.arange(n)
    lse = torch.full((b, hq, sq), NEG_INF, dtype=torch.float32)
    for i in range(b):
        mask = ((pos >= lo[i][:, None]) & (pos < hi[i][:, None])).repeat(g, 1)
        for h in range(hkv):
            sc = scale * (1.0 if kscale is None else float(kscale[i, h]))
            s = torch.matmul(q[i, h * g:(h + 1) * g].reshape(g * sq, d).float(), k[i if k.size(0) > 1 else 0, h].float().T) * sc
            lse[i, h * g:(h + 1) * g] = torch.logsumexp(s.masked_fill(~mask, NEG_INF), dim=-1).reshape(g, sq)
    return lse.double()


# ------------------------------------------------------------------------------------------------
# the metrics
# ------------------------------------------------------------------------------------------------
def measure(got, ref, lo, hi):
    """(rms, bias, emax) of ``got`` against ``ref`` ([B, Hq, Sq, D]) over the rows that see at least one key:
    rms = sqrt(mean((got - ref)^2)), bias = mean(got - ref) / mean(|ref|), emax = max |got - ref|."""
    live = (hi > lo)[:, None].expand(-1, got.size(1), -1)
    err = (got.double() - ref.double())[live]
    return err.pow(2).mean().sqrt().item(), (err.mean() / ref.double()[live].abs().mean()).item(), err.abs().max().item()


def lse_error(lse, ref):
    """max |lse - ref| over the rows with a visible key; -inf must sit exactly where the reference has it."""
    empty = ref == NEG_INF
    assert torch.equal(lse.double() == NEG_INF, empty), "-inf rows differ"
    return (lse.double()[~empty] - ref[~empty]).abs().max().item() if (~empty).any() else 0.0


# ------------------------------------------------------------------------------------------------
# the input families
# ------------------------------------------------------------------------------------------------
FAMILIES = ("centered", "sharp", "offset")


def family(name, b, bk, hq, hkv, sq, n, d, dtype, seed):
    """q [B, Hq, Sq, D], k / v [Bk, Hkv, N, D], rounded to the io dtype. centered: all ``randn`` (a diffuse softmax,
    small outputs: a lost key or sloppy accumulation shows). sharp: q = 5 ``randn`` (logits of sigma ~5, a few keys
    hold most of a row). offset: v = ``randn`` + 2 (every output positive; for the bias metric only)."""
    assert name in FAMILIES, name
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, hq, sq, d, generator=g) * (5.0 if name == "sharp" else 1.0)
    k = torch.randn(bk, hkv, n, d, generator=g)
    v = torch.randn(bk, hkv, n, d, generator=g) + (2.0 if name == "offset" else 0.0)
    return q.to(dtype), k.to(dtype), v.to(dtype)
