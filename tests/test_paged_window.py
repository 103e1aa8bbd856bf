"""Sliding-window decode over the paged KV cache, 16-bit and FP8 (include/fa_gfx950_paged_window.h).

``flash_attn_paged_func(..., window_left=W)`` and ``flash_attn_with_kvcache(..., window_left=W)``: per sequence,
with L the clamped length and the queries its last Sq positions, key n is visible to query m iff
``n >= m + L - Sq - W`` (and ``n <= m + L - Sq`` with causal) -- ``fa_fwd_gfx950_window``'s mask, bottom-right
aligned per sequence. The oracle is ``tests/test_padded.py::oracle_padded`` with ``window_left`` on the dense
keys (the packed-varlen oracle, itself pinned to the reference's golden vectors), within
tests/test_gpu_parity.py TOL, the 16-bit kernels' own tolerance.

Pinned beside the values: a window that masks nothing gives the unwindowed launch's bits; a window whose start
falls on a tile edge gives the padded decode's bits on that key range; and the pages wholly below the tile of
``lo0 = max(0, L - Sq - W)`` and their table entries are never read -- the GPU cases overwrite them with NaN and
bad ids. Pools are test_paged.make_paged's: shuffled tables, every unused row NaN, every unused entry -1.
"""
from __future__ import annotations

import functools
import warnings

import pytest
import torch

from test_fp8_kvcache import FP8, NAN_BYTE, make_fp8_paged, pow2_descales
from test_kvcache import make_cache, new_tokens, rope_tables
from test_padded import check_padded, oracle_padded
from test_paged import KINDS, make_paged

F16, BF16 = torch.float16, torch.bfloat16
DEV = "cuda:0"


def win_oracle(q, k, v, sl, causal, w):
    return oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, q.size(-1) ** -0.5, causal, window_left=w)


def quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


# ------------------------------------------------------------------------------------------- CPU
CPU_LENS, CPU_GEO = (96, 0, 33, 1, 64), (4, 2, 32, 96, 64)  # lens; Hq, Hkv, page, capacity, D


@pytest.mark.parametrize("w", [0, 5, 40, 200])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq", [1, 3])
@pytest.mark.parametrize("layout", ["phsd", "pshd"])
def test_paged_window_cpu_default_matches_oracle(w, causal, sq, layout):
    from flash_attention_cute_amd import flash_attn_paged_func

    hq, hkv, page, cap, d = CPU_GEO
    q, k, v, kc, vc, table, sl = make_paged(CPU_LENS, hq, hkv, sq, page, cap, d, F16, 3, layout)
    out = quiet(flash_attn_paged_func, q.float(), kc.float(), vc.float(), table, sl, causal=causal, window_left=w)
    assert torch.isfinite(out).all() and (out[1] == 0).all()  # (a sequence without keys)
    torch.testing.assert_close(out, win_oracle(q, k, v, sl, causal, w).float(), atol=3e-3, rtol=3e-3)
    if w == 200:  # at least every length: the unwindowed result
        plain = quiet(flash_attn_paged_func, q.float(), kc.float(), vc.float(), table, sl, causal=causal)
        torch.testing.assert_close(out, plain, atol=1e-6, rtol=1e-6)


def test_paged_window_cpu_default_skips_the_pages_below_the_window():
    """The CPU default does not gather the pages the kernel never reads: NaN in them, any id in their entries."""
    from flash_attention_cute_amd import flash_attn_paged_func

    hq, hkv, page, cap, d = CPU_GEO
    q, k, v, kc, vc, table, sl = make_paged(CPU_LENS, hq, hkv, 3, page, cap, d, F16, 3)
    for b, n in enumerate(CPU_LENS):
        for j in range(max(0, n - 3 - 5) // page):
            kc[table[b, j]], vc[table[b, j]] = float("nan"), float("nan")
            table[b, j] = 2 ** 31 - 1
    out = quiet(flash_attn_paged_func, q.float(), kc.float(), vc.float(), table, sl, causal=True, window_left=5)
    torch.testing.assert_close(out, win_oracle(q, k, v, sl, True, 5).float(), atol=3e-3, rtol=3e-3)


@pytest.mark.parametrize("w", [0, 5, 40, 200])
@pytest.mark.parametrize("sq", [1, 3])
@pytest.mark.parametrize("dense", [False, True], ids=["paged", "dense"])
def test_with_kvcache_window_cpu_matches_oracle(w, sq, dense):
    """Append Sq new tokens, then the windowed attention over the advanced lengths (no RoPE: the oracle is
    the windowed one on the cache the append left behind)."""
    from flash_attention_cute_amd import flash_attn_with_kvcache
    from flash_attention_cute_amd.flash_attention import _gather_pages

    lens, hq, hkv, page, cap, d = (60, 0, 33, 90), 4, 2, 32, 96, 64
    kc, vc, table, sl = make_cache(lens, sq, hkv, page, cap, d, F16, 7, dense=dense)
    kc, vc = kc.float(), vc.float()
    kn, vn, q = new_tokens(4, hkv, sq, d, F16, 1), new_tokens(4, hkv, sq, d, F16, 2), new_tokens(4, hq, sq, d, F16, 3)
    out, new = quiet(flash_attn_with_kvcache, q.float(), kc, vc, kn.float(), vn.float(), cache_seqlens=sl,
                     block_table=table, causal=True, return_seqlens=True, window_left=w)
    assert new.tolist() == [n + sq for n in lens]
    kd, vd = (kc, vc) if dense else (_gather_pages(kc, table), _gather_pages(vc, table))
    torch.testing.assert_close(out, win_oracle(q, kd.half(), vd.half(), new, True, w).float(), atol=3e-3, rtol=3e-3)


def test_window_ops_registration():
    import flash_attention_cute_amd as m

    sch = str(torch.ops.flash_attention.paged_window_forward.default._schema)
    assert sch == ("flash_attention::paged_window_forward(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, "
                   "Tensor cache_seqlens, SymInt window_left, float softmax_scale=None, bool causal=False) -> Tensor")
    sch = str(torch.ops.flash_attention.paged_window_forward_fp8.default._schema)
    assert sch == ("flash_attention::paged_window_forward_fp8(Tensor q, Tensor k_cache, Tensor v_cache, "
                   "Tensor block_table, Tensor cache_seqlens, SymInt window_left, Tensor? k_descale=None, "
                   "Tensor? v_descale=None, float softmax_scale=None, bool causal=False) -> Tensor")
    assert "window" not in str(torch.ops.flash_attention.paged_forward.default._schema)
    assert "window" not in str(torch.ops.flash_attention.paged_forward_fp8.default._schema)
    for name in ("flash_attention_paged_window_forward", "flash_attention_paged_window_forward_fp8"):
        assert name in m.__all__
    q, _, _, kc, vc, table, lens = make_paged((40, 7), 4, 2, 2, 32, 64, 32, torch.float32, 1)
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)
    quiet(torch.library.opcheck, torch.ops.flash_attention.paged_window_forward.default,
          (q, kc, vc, table, lens, 9, 0.125, True), test_utils=("test_schema", "test_faketensor"))


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


def launch(q, kc, vc, table, sl, causal, w, fuse=None, **kw):
    """One paged launch on the device: (output on the host, path, fused)."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    _debug.set_knobs()
    _debug.set_dec_fuse(fuse)
    try:
        out = flash_attn_paged_func(*dv(q, kc, vc, table, sl), causal=causal, window_left=w,
                                    **{n: t.to(DEV) for n, t in kw.items()})
        path, fused = _debug.last_path(), _debug.last_dec_fused()
        torch.cuda.synchronize()
    finally:
        _debug.set_dec_fuse(None)
    return out.cpu(), path, fused


# 1. oracle parity, Sq == 1. Base geometry of test_paged (B 3, Hq 8, Hkv 2, capacity 256); every length triple with
# every window; page size, D, dtype and pool layout cycle so that each value meets each window and each triple.
LENS1 = [(0, 1, 31), (32, 33, 256), (64, 65, 200)]
WINDOWS1 = [0, 1, 31, 32, 33, 100]
PAGES, DIMS = (32, 64, 256), (64, 128, 72)
CASES1 = [(li, w, PAGES[(li + wi) % 3], DIMS[(li + 2 * wi + wi // 3) % 3], (F16, BF16)[(li + wi) % 2],
           ("phsd", "pshd")[(wi + wi // 2) % 2]) for li in range(3) for wi, w in enumerate(WINDOWS1)]
IDS1 = [f"L{li}-w{w}-p{p}-d{d}-{'f16' if t == F16 else 'bf16'}-{lay}" for li, w, p, d, t, lay in CASES1]


@functools.lru_cache(maxsize=None)
def run1(ci):
    li, w, page, d, dtype, layout = CASES1[ci]
    q, k, v, kc, vc, table, sl = make_paged(LENS1[li], 8, 2, 1, page, 256, d, dtype, 500 + ci, layout)
    out, path, _ = launch(q, kc, vc, table, sl, False, w)
    return out, path, win_oracle(q, k, v, sl, False, w), (q, kc, vc, table, sl)


def test_case_list_covers_the_geometry():
    for col, vals in ((2, PAGES), (3, DIMS), (4, (F16, BF16)), (5, ("phsd", "pshd"))):
        assert {c[col] for c in CASES1} == set(vals)
        for li in range(len(LENS1)):
            assert {c[col] for c in CASES1 if c[0] == li} == set(vals)
    for w in WINDOWS1:  # every window meets every page size and head dim
        assert {c[2] for c in CASES1 if c[1] == w} == set(PAGES) and {c[3] for c in CASES1 if c[1] == w} == set(DIMS)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES1)), ids=IDS1)
def test_window_decode_matches_the_oracle(ops, ci):
    li, w, _, _, dtype, _ = CASES1[ci]
    out, path, ref, _ = run1(ci)
    assert path == "decode_paged"
    check_padded(out, ref, dtype)
    for i, n in enumerate(LENS1[li]):
        if n == 0:
            assert (out[i] == 0).all()


# 2. rows whose windows start in different tiles. lo0 = L - Sq - W; the first two sequences have lo0 % 32 = 20 and
# 30 (lo0 = 52, 94), so with Sq 5 / 16 (and Sq 3 at 30) row 0's bound and the last row's lie in different tiles:
# the later rows see an all-masked tile before their first visible key. The third sequence has L < Sq.
ROWS2 = {"sq3_g4": (8, 2, 3, 40, 2), "sq5_g8": (16, 2, 5, 40, 4), "sq16_g4": (8, 2, 16, 40, 7)}  # Hq, Hkv, Sq, W, short L
CASES2 = [(name, causal, (32, 64, 256)[i % 3], (128, 72, 64)[i % 3], (F16, BF16)[i % 2], ("phsd", "pshd")[i % 2])
          for i, (name, causal) in enumerate((n, c) for n in ROWS2 for c in (True, False))]
IDS2 = [f"{n}-{'causal' if c else 'full'}-p{p}-d{d}-{'f16' if t == F16 else 'bf16'}" for n, c, p, d, t, _ in CASES2]


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES2)), ids=IDS2)
def test_rows_whose_windows_start_in_different_tiles(ops, ci):
    name, causal, page, d, dtype, layout = CASES2[ci]
    hq, hkv, sq, w, short = ROWS2[name]
    lens = (52 + sq + w, 94 + sq + w, short)
    assert [(n - sq - w) % 32 for n in lens[:2]] == [20, 30] and short < sq
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, 256, d, dtype, 600 + ci, layout)
    out, path, _ = launch(q, kc, vc, table, sl, causal, w)
    assert path == "decode_paged" and torch.isfinite(out.float()).all()
    check_padded(out, win_oracle(q, k, v, sl, causal, w), dtype)


# 3. split: capacity 4096, window 2047: the plan is made for 65 tiles (4 units -> 4 splits), the longer sequence's
# tiles [64, 128) and the shorter one's [7, 72) are shared among them
SPLIT = dict(lens=(4096, 2300), hq=8, hkv=2, page=64, cap=4096, d=128, dtype=BF16, w=2047)


@functools.lru_cache(maxsize=None)
def split_inputs(fp8=False):
    s = SPLIT
    if fp8:
        kd, vd = pow2_descales(2, s["hkv"]), pow2_descales(2, s["hkv"], 2)
        return make_fp8_paged(s["lens"], s["hq"], s["hkv"], 1, s["page"], s["cap"], s["d"], s["dtype"], 77, "phsd", kd,
                              vd) + (kd, vd)
    return make_paged(s["lens"], s["hq"], s["hkv"], 1, s["page"], s["cap"], s["d"], s["dtype"], 77)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", [None, 0], ids=["fused", "unfused"])
def test_window_split_decode(ops, fuse):
    q, k, v, kc, vc, table, sl = split_inputs()
    out, path, fused = launch(q, kc, vc, table, sl, False, SPLIT["w"], fuse)
    assert path == "decode_paged_split" and fused == (fuse is None)
    check_padded(out, win_oracle(q, k, v, sl, False, SPLIT["w"]), SPLIT["dtype"])
    again, _, _ = launch(q, kc, vc, table, sl, False, SPLIT["w"], fuse)
    assert torch.equal(out, again)


# 4. windows that mask nothing are the unwindowed launch, bit for bit
NOOP = [("unsplit", 64, 128, F16, (64, 65, 200)), ("split", 64, 128, BF16, (2048, 33)),
        ("split_unfused", 32, 72, F16, (32, 1999)), ("sq3_causal", 64, 72, BF16, (64, 65, 256)),
        ("g8_sq5", 256, 64, F16, (256, 4, 33))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", NOOP, ids=[c[0] for c in NOOP])
def test_noop_windows_are_bit_identical(ops, case):
    kind, page, d, dtype, lens = case
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    fuse = 0 if kind == "split_unfused" else None
    args = make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 700, "pshd")
    q, _, _, kc, vc, table, sl = args
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    _debug.set_dec_fuse(fuse)
    plain = flash_attn_paged_func(*dv(q, kc, vc, table, sl), causal=causal)  # (the call without the keyword)
    plain_path = _debug.last_path()
    torch.cuda.synchronize()
    assert plain_path == ("decode_paged_split" if kind.startswith("split") else "decode_paged")
    for w in (-1, max(lens), cap, 2 ** 40):
        out, path, _ = launch(q, kc, vc, table, sl, causal, w, fuse)
        assert path == plain_path and torch.equal(out, plain.cpu()), w


# 5. the exact case: a window start on a tile edge is the padded decode on that key range -- same tiles, same
# order, nothing masked below
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,d,page", [(F16, 128, 32), (BF16, 64, 64), (F16, 72, 256)])
def test_tile_aligned_window_equals_padded_decode_on_the_key_range(ops, dtype, d, page):
    from flash_attention_cute_amd import _debug, flash_attn_padded_func

    lens, w = (200, 72, 136), 39
    assert all((n - 1 - w) % 32 == 0 for n in lens)
    q, k, v, kc, vc, table, sl = make_paged(lens, 8, 2, 1, page, 256, d, dtype, 800)
    out, path, _ = launch(q, kc, vc, table, sl, False, w)
    dense = flash_attn_padded_func(*dv(q, k, v, sl - 1 - w, sl))
    assert _debug.last_path() == "decode" and path == "decode_paged"
    assert torch.equal(out, dense.cpu())


# 6. freed pages are never read
def free_pages_below_the_window(kc, vc, table, lens, sq, w, page, bad, poison):
    """Overwrite every page wholly below tile t_first_b with `poison` and its entry with `bad`; also the pool's
    first and last page unless live (a clamped bad id would otherwise read finite data). Returns the count."""
    kc, vc, table = kc.clone(), vc.clone(), table.clone()

    def fill(pg):  # (through byte views for an fp8 pool: it has no fill / index_put)
        for c in (kc, vc):
            (c.view(torch.uint8) if c.dtype == FP8 else c)[pg].fill_(poison)

    freed = 0
    for b, n in enumerate(lens):
        t_first = max(0, n - sq - w) // 32
        for j in range(t_first * 32 // page):
            fill(int(table[b, j]))
            table[b, j] = bad
            freed += 1
    live = {int(table[b, j]) for b, n in enumerate(lens) for j in range((n + page - 1) // page) if table[b, j] != bad}
    for pg in (0, kc.size(0) - 1):
        if pg not in live:
            fill(pg)
    return kc, vc, table, freed


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [2 ** 31 - 1, -1])
@pytest.mark.parametrize("ci", [13, 14], ids=[IDS1[13], IDS1[14]])
def test_freed_pages_and_their_entries_are_never_read(ops, ci, bad):
    li, w, page, _, _, _ = CASES1[ci]
    out, _, _, (q, kc, vc, table, sl) = run1(ci)
    lens = LENS1[li]
    assert max(n - 1 - w for n in lens) >= 64 and page < 256
    kc2, vc2, table2, freed = free_pages_below_the_window(kc, vc, table, lens, 1, w, page, bad, float("nan"))
    assert freed >= 2
    got, _, _ = launch(q, kc2, vc2, table2, sl, False, w)
    assert torch.isfinite(got.float()).all() and torch.equal(got, out)


# 7. FP8: parity, split, no-op windows and freed pages on an e4m3 pool with per-(batch, kv-head) descales. The
# reference is the 16-bit windowed oracle on the dequantized cache (powers of two: exact), at the 16-bit tolerance.
def fp8_win_oracle(q, k8, v8, sl, kd, vd, causal, w):
    dt = q.dtype
    return win_oracle(q, k8.to(dt) * kd[:, :, None, None].to(dt), v8.to(dt) * vd[:, :, None, None].to(dt), sl, causal, w)


@pytest.mark.gpu
@pytest.mark.parametrize("d,dtype,page,lens,w", [(128, BF16, 32, (64, 65, 200), 31), (64, F16, 64, (32, 33, 256), 100)])
def test_fp8_window_decode_parity_noop_and_freed_pages(ops, d, dtype, page, lens, w):
    kd, vd = pow2_descales(3, 2), pow2_descales(3, 2, 2)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, 8, 2, 1, page, 256, d, dtype, 900, "pshd", kd, vd)
    ds = dict(k_descale=kd, v_descale=vd)
    out, path, _ = launch(q, kc8, vc8, table, sl, False, w, **ds)
    assert path == "decode_paged_fp8"
    check_padded(out, fp8_win_oracle(q, k8, v8, sl, kd, vd, False, w), dtype)
    # no-op windows: the unwindowed FP8 launch's bits
    plain, _, _ = launch(q, kc8, vc8, table, sl, False, -1, **ds)
    assert torch.equal(launch(q, kc8, vc8, table, sl, False, 256, **ds)[0], plain)
    # freed pages: NaN bytes and a bad id
    kc2, vc2, table2, freed = free_pages_below_the_window(kc8, vc8, table, lens, 1, w, page, 2 ** 31 - 1, NAN_BYTE)
    assert freed >= 2
    got, _, _ = launch(q, kc2, vc2, table2, sl, False, w, **ds)
    assert torch.isfinite(got.float()).all() and torch.equal(got, out)


@pytest.mark.gpu
def test_fp8_window_split_decode(ops):
    q, k8, v8, kc8, vc8, table, sl, kd, vd = split_inputs(True)
    out, path, fused = launch(q, kc8, vc8, table, sl, False, SPLIT["w"], k_descale=kd, v_descale=vd)
    assert path == "decode_paged_fp8_split" and fused
    check_padded(out, fp8_win_oracle(q, k8, v8, sl, kd, vd, False, SPLIT["w"]), SPLIT["dtype"])


# 8. flash_attn_with_kvcache(window_left=W)
@pytest.mark.gpu
def test_with_kvcache_window_paged_equals_the_composed_step(ops, device):
    fam = ops
    lens, hq, hkv, page, cap, d, w = (70, 0, 33, 127), 8, 2, 32, 128, 128, 40
    kc, vc, table, sl = dv(*make_cache(lens, 1, hkv, page, cap, d, BF16, 21))
    kn, vn, q = dv(new_tokens(4, hkv, 1, d, BF16, 1), new_tokens(4, hkv, 1, d, BF16, 2), new_tokens(4, hq, 1, d, BF16, 3))
    cos, sin = dv(*rope_tables(cap, d, BF16))
    kc2, vc2 = kc.clone(), vc.clone()
    out, new = fam.flash_attn_with_kvcache(q, kc, vc, kn, vn, cos, sin, cache_seqlens=sl, block_table=table, causal=True,
                                           return_seqlens=True, window_left=w)
    new2, q_rot = torch.ops.flash_attention.kvcache_append(kc2, vc2, kn, vn, sl, table, q, cos, sin)
    ref = fam.flash_attn_paged_func(q_rot, kc2, vc2, table, new2, causal=True, window_left=w)
    torch.cuda.synchronize()
    assert torch.equal(new, new2) and torch.equal(kc.view(torch.int16), kc2.view(torch.int16))
    assert torch.equal(out, ref)
    assert not torch.equal(out, fam.flash_attn_paged_func(q_rot, kc2, vc2, table, new2, causal=True))  # (it windows)


@pytest.mark.gpu
@pytest.mark.parametrize("sq", [1, 3])
def test_with_kvcache_window_on_a_dense_cache(ops, device, sq):
    from flash_attention_cute_amd import _debug

    fam = ops
    lens, hq, hkv, cap, d, w = (70, 0, 33, 100), 8, 2, 128, 128, 40
    kc, vc, _, sl = make_cache(lens, sq, hkv, 32, cap, d, F16, 22, dense=True)
    kn, vn, q = new_tokens(4, hkv, sq, d, F16, 1), new_tokens(4, hkv, sq, d, F16, 2), new_tokens(4, hq, sq, d, F16, 3)
    kg, vg = dv(kc, vc)
    out, new = fam.flash_attn_with_kvcache(*dv(q), kg, vg, *dv(kn, vn), cache_seqlens=sl.to(DEV), causal=True,
                                           return_seqlens=True, window_left=w)
    path = _debug.last_path()
    torch.cuda.synchronize()
    if sq == 1:
        assert path in ("decode", "decode_split")
    assert new.tolist() == [n + sq for n in lens]
    check_padded(out, win_oracle(q, kg.cpu(), vg.cpu(), new.cpu(), True, w), F16)


@pytest.mark.gpu
def test_with_kvcache_window_on_a_dense_fp8_cache(ops, device):
    from flash_attention_cute_amd import _debug

    fam = ops
    lens, hq, hkv, cap, d, w = (70, 0, 33, 100), 8, 2, 128, 128, 40
    kd, vd = pow2_descales(4, hkv), pow2_descales(4, hkv, 2)
    k16, v16, _, sl = make_cache(lens, 0, hkv, 32, cap, d, BF16, 23, dense=True)
    k8 = (k16.float() / kd[:, :, None, None]).clamp(-448, 448).to(FP8)
    v8 = (v16.float() / vd[:, :, None, None]).clamp(-448, 448).to(FP8)
    q = new_tokens(4, hq, 1, d, BF16, 3)
    out = fam.flash_attn_with_kvcache(*dv(q, k8, v8), cache_seqlens=sl.to(DEV), causal=True, window_left=w,
                                      k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    assert _debug.last_path() == "decode_paged_fp8"
    check_padded(out, fp8_win_oracle(q, k8, v8, sl, kd, vd, True, w), BF16)


# 9. graph capture
@pytest.mark.gpu
def test_window_decode_graph_capture(ops, device):
    """A windowed paged step captures into a graph (no host synchronisation); the replay follows lengths
    advanced in place across a tile edge (95 -> 96 -> 97: the window's first tile and the last tile both move)."""
    fam = ops
    b, hq, hkv, page, cap, d, w = 4, 8, 2, 32, 256, 128, 63
    lens = [95, 160, 31, 255]
    q, _, _, kc, vc, table, sl = dv(*make_paged([cap] * b, hq, hkv, 1, page, cap, d, BF16, 31))
    sl.copy_(torch.tensor(lens, dtype=torch.int32))
    eager = fam.flash_attn_paged_func(q, kc, vc, table, sl, window_left=w)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fam.flash_attn_paged_func(q, kc, vc, table, sl, window_left=w)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    for _ in range(2):
        sl.add_(1)
        g.replay()
        torch.cuda.synchronize()
        fresh = fam.flash_attn_paged_func(q, kc, vc, table, sl, window_left=w)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all() and torch.equal(out, fresh)
    assert not torch.equal(out, eager)


# 10. the copying path passes the window on
@pytest.mark.gpu
def test_copying_path_with_a_window(ops, device):
    from flash_attention_cute_amd import _debug

    lens, page, cap, d, w = (300, 40, 512), 64, 512, 128, 100
    q, k, v, kc, vc, table, sl = make_paged(lens, 8, 2, 40, page, cap, d, F16, 29, "pshd")  # g * Sq = 160 rows
    out, path, _ = launch(q, kc, vc, table, sl, True, w)
    assert path == "w4"
    check_padded(out, win_oracle(q, k, v, sl, True, w), F16)
