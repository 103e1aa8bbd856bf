"""Head geometry -- the table of (Hq, Hkv, Sq) shapes and the row-naming checker of tests/test_head_geometry.py.

The decode kernel family (csrc/fa_decode.hpp) serves a (batch, kv-head) unit of ``rows = g * Sq <= 64`` rows
(g = Hq / Hkv) in one or two 32-row blocks; row ``rg`` is q-head ``hkv * g + rg / Sq`` at position ``rg % Sq``. The
q load, the O / LSE stores, the sink lookup and the combine kernel each repeat that decomposition. With g and Sq
powers of two a swap of the two, a ``/`` for a ``%`` or a row block assumed to start on a head boundary still gives
the right answer, so the table below holds the shapes where they do not: odd g, odd Hkv, Sq that is no divisor of 32.

``check_heads`` applies the project's tolerance (tests/test_gpu_parity.py ``TOL``, as ``test_padded.check_padded``
applies it: |out - ref| <= atol + rtol |ref| per element, then the mean error) per (b, hq, pos) row and, on failure,
names the reference row of the same batch entry that each failing output row is nearest to.
"""
from __future__ import annotations

import torch

F16, BF16 = torch.float16, torch.bfloat16

# (Hq, Hkv, Sq, lengths of the B = 3 sequences, what the row is there for). rows = Hq / Hkv * Sq. The lengths are
# drawn from {0, a value < Sq, 31, 33, 65, 256} (capacity 256): causal rows without a visible key occur for every
# Sq > 1, and each geometry meets a sequence of more than one 32-key tile.
GEOMETRY = [
    (7, 1, 1, (256, 0, 33), "MQA, g = 7"),
    (28, 4, 1, (31, 65, 0), "Qwen2-7B: g = 7, Hkv = 4"),
    (9, 3, 1, (33, 256, 31), "g = 3, Hkv = 3"),
    (10, 2, 1, (0, 65, 256), "g = 5"),
    (24, 2, 1, (65, 31, 33), "g = 12"),
    (40, 5, 1, (256, 33, 0), "Hkv = 5 (g = 8)"),
    (33, 1, 1, (31, 256, 65), "33 rows: the second row block holds one row"),
    (64, 1, 1, (0, 33, 256), "64 rows: two full blocks on the paged kernels"),
    (14, 2, 3, (2, 256, 33), "g = 7, Sq = 3: 21 rows"),
    (6, 2, 11, (65, 5, 0), "33 rows: the one row of the second block is head 2's last position"),
    (10, 2, 7, (31, 256, 3), "g = 5, Sq = 7: 35 rows, the block boundary inside head 4"),
    (7, 1, 9, (4, 33, 256), "63 rows: row 32 is head 3, position 5"),
    (3, 1, 21, (256, 10, 65), "g = 3, Sq = 21: 63 rows, the boundary inside head 1"),
    (12, 1, 5, (65, 2, 0), "g = 12, Sq = 5: 60 rows, the boundary inside head 6"),
    (5, 5, 13, (33, 6, 256), "MHA, Hkv = 5: 13 rows per unit"),
    (2, 1, 32, (16, 256, 31), "64 rows: two full blocks, exactly one head each"),
]
PAST_LIMIT = (7, 1, 10)  # 70 rows: one geometry just past the decode rule (g * Sq <= 64)
CAPACITY = 256
PAGES, DIMS = (32, 64, 256), (64, 72, 128)
SPLIT = ((7, 1, 1), (33, 1, 1), (7, 1, 9), (10, 2, 7))  # the geometries of the split cases
SPLIT_LENS, SPLIT_CAPACITY = (2048, 33), 2048  # B = 2: decode_plan gives 4 splits (64 tiles, 2 .. 8 units)
MAX_ROWS, BLOCK_ROWS = 64, 32  # csrc/fa_launch.h kDecMaxRows; the rows of one row block


def rows_of(hq, hkv, sq):
    return hq // hkv * sq


def geo_id(geo):
    return "%d-%d-%d" % tuple(geo[:3])


def index_of(hq, hkv, sq):
    return [g[:3] for g in GEOMETRY].index((hq, hkv, sq))


def case_of(gi):
    """The page size, head dim, dtype and pool layout of table row ``gi``: page sizes 32 / 64 / 256 and head dims
    64 / 72 / 128 rotate over the table (so that each page size meets each head dim), fp16 and bf16 alternate and
    both pool layouts occur with both."""
    return PAGES[gi % 3], DIMS[(gi + gi // 3) % 3], (F16, BF16)[gi % 2], ("phsd", "pshd")[(gi // 2) % 2]


def head_of_row(rg, sq):
    """The kernel's decomposition of a unit's row index: (q-head within the kv group, position)."""
    return rg // sq, rg % sq


def _excess(row, cand, atol, rtol):
    """How far ``row`` [D] lies outside the bound around each candidate row of ``cand`` [..., D] (<= 0: inside)."""
    return ((row - cand).abs() - (atol + rtol * cand.abs())).amax(dim=-1)


def name_row(row, ref_b, atol, rtol):
    """(hq', pos', excess) of the reference row of one batch entry [Hq, Sq, D] that ``row`` is nearest to."""
    ex = _excess(row, ref_b, atol, rtol)
    flat = int(ex.argmin())
    return flat // ref_b.size(1), flat % ref_b.size(1), ex.flatten()[flat].item()


def check_heads(out, ref, dtype, mean=True, tol=None, report=4):
    """``test_padded.check_padded`` per (b, hq, pos) row of out / ref [B, Hq, Sq, D]: every element within
    tests/test_gpu_parity.py TOL[dtype] (``tol``: another (atol, rtol, mean_tol) the project already uses), the mean
    error within its third entry (``mean=False``: the elementwise bound alone, as test_shared_prefix.check_bound).
    A failure names, for the first ``report`` failing rows, the reference row of the same batch entry that the
    output row holds (within the bound) or is nearest to."""
    from tests.test_gpu_parity import TOL

    atol, rtol, mean_tol = TOL[dtype] if tol is None else tol
    got, ref = out.detach().float().cpu(), ref.detach().float().cpu()
    assert got.dim() == 4 and got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "the output holds a NaN or an infinity"
    err = (got - ref).abs()
    bad = ((err - (atol + rtol * ref.abs())) > 0).any(dim=-1)  # [B, Hq, Sq]
    if bad.any():
        lines = []
        for b, h, p in bad.nonzero()[:report].tolist():
            h2, p2, ex = name_row(got[b, h, p], ref[b], atol, rtol)
            what = "is all zero and " if not got[b, h, p].any() else ""
            if ex <= 0:
                lines.append(f"b {b} head {h} pos {p} {what}holds head {h2} pos {p2}")
            else:
                lines.append(f"b {b} head {h} pos {p} {what}matches no reference row (nearest: head {h2} pos {p2}, "
                             f"{ex:.3e} outside the bound)")
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} (b, hq, pos) rows exceed {atol:g} + {rtol:g} |ref| "
                             f"(max err {err.max().item():.3e}): " + "; ".join(lines))
    if mean:
        assert err.mean().item() <= mean_tol, f"mean err {err.mean().item():.3e} exceeds {mean_tol:g}"


def packed_as_heads(t):
    """A packed [total, Hq, D] tensor as one batch entry [1, Hq, total, D] for ``check_heads``."""
    return t.transpose(0, 1)[None]


def center_sinks(q, k, lens, seed, scale=None, kd=None):
    """Sinks that carry weight on every head: the construction of test_paged_sink.make_sinks (float64 scores of the
    case, ``test_paged_sink.scores``) with the level taken from the case itself -- a distinct finite sink per
    q-head, spread over +-1.5 around the median log-sum-exp of the case's rows, and head 2 at -inf (no sink). A
    row's output is scaled by sigmoid(lse - sink), so a sink taken from another head moves it by tens of percent."""
    from test_paged_sink import scores

    lse = torch.cat([torch.logsumexp(s, dim=-1).flatten() for s in scores(q, k, lens, scale, kd) if s.size(-1)])
    hq = q.size(1)
    order = torch.randperm(hq, generator=torch.Generator().manual_seed(seed))
    sinks = (lse.median() + torch.linspace(-1.5, 1.5, hq, dtype=torch.float64)[order]).float()
    sinks[2] = float("-inf")
    return sinks
