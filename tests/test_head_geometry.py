"""Odd head geometry on every attention path: GQA with g = 3, 5, 6, 7, 12, MQA, Hkv = 3 and 5, and query blocks
whose 32-row block boundary falls inside a head (tests/head_geometry.py has the table and what each row is for).

Every other case table under tests/ uses Hkv = 2 with Hq in {2, 4, 8, 16}: every divisor of the row mapping a power
of two, where a swap of g and Sq, a ``/`` for a ``%`` or a row block assumed to start on a head boundary cannot be
seen. The "paged == padded, bit for bit" yardsticks cannot see such a bug either (both sides share the mapping code),
so every case here is held to an independent reference -- the packed-varlen oracle (``test_padded.oracle_padded``),
the float64 references of test_paged_lse / test_paged_sink, ``test_kvcache.expected_append`` -- through
``head_geometry.check_heads``: the project's tolerance (tests/test_gpu_parity.py TOL, fp16 2e-3 + 2e-3 |ref|, bf16
1.6e-2 + 1.6e-2 |ref|, as ``test_padded.check_padded`` applies it) per (b, hq, pos) row, with a failure that names
the reference row the output row holds ("head 3 pos 5 holds head 5 pos 3"). The LSE bound is test_paged_lse's 2^-12
absolute. No tolerance is new. The CPU tests of the checker itself (a swap of two heads, of two positions, heads
regrouped) are how the file shows that it bites.

Inputs are the project's generators (``make_paged`` and friends): independent random draws per head, shuffled tables,
NaN in every unused pool row and -1 in every unused table entry.
"""
from __future__ import annotations

import ctypes
import functools
import warnings

import pytest
import torch

from head_geometry import (BF16, BLOCK_ROWS, CAPACITY, F16, GEOMETRY, MAX_ROWS, PAST_LIMIT, SPLIT, SPLIT_CAPACITY,
                           SPLIT_LENS, case_of, center_sinks, check_heads, geo_id, head_of_row, index_of,
                           packed_as_heads, rows_of)
from oracle import fa_oracle as O
from oracle import fa_oracle_c as OC
from test_fp8_kvcache import expected_fp8_append, fp8_oracle, make_fp8_cache, make_fp8_paged, norm_bytes
from test_kvcache import PATTERN, bits, expected_append, make_cache, new_tokens, rope_tables, targets
from test_padded import oracle_padded
from test_paged import make_paged
from test_paged_lse import check_lse, lse_oracle, make_states, merge_oracle
from test_paged_sink import descales, sink_oracle
from test_paged_window import fp8_win_oracle, win_oracle
from test_shared_prefix import GROUP_ROWS, make_shared, share_prefix

DEV = "cuda:0"
I32 = torch.int32
GEO_IDS = [geo_id(g) for g in GEOMETRY]
CPU_TOL = (3e-3, 3e-3, None)  # test_paged.test_paged_op_cpu_default_matches_oracle: the CPU defaults' bar
NAMES = {F16: "f16", BF16: "bf16"}


def quiet(fn, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


def dv(*ts):
    return tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in ts)


def paged_oracle(q, k, v, sl, causal):
    """The packed-varlen oracle on each sequence's first ``sl[b]`` keys of the dense K / V [B, Hkv, cap, D]."""
    return oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, q.size(-1) ** -0.5, causal)


def dense_oracle(q, k, v, causal, w=-1):
    """The dense oracle (oracle/fa_oracle.c) with the rows that see no key 0, as the kernels define them."""
    ref = OC.forward(q, k, v, q.size(-1) ** -0.5, causal, window_left=w).float()
    masked = torch.from_numpy(O.fully_masked_rows(q.size(2), k.size(2), causal))
    ref[:, :, masked] = 0
    return ref


# ============================================================================================ 1. the checker (CPU)
def checker_case(hq=7, hkv=1, sq=9, d=64, dtype=F16):
    """A reference as the kernels' outputs are: independent draws per (b, hq, pos), rounded to dtype."""
    return torch.randn(3, hq, sq, d, generator=torch.Generator().manual_seed(hq * 100 + sq)).to(dtype)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_checker_accepts_the_reference_and_an_output_inside_the_bound(dtype):
    from tests.test_gpu_parity import TOL

    ref = checker_case(dtype=dtype)
    check_heads(ref, ref, dtype)
    atol, rtol, mean_tol = TOL[dtype]
    near = ref.float() + 0.9 * mean_tol * torch.sign(torch.randn(ref.shape, generator=torch.Generator().manual_seed(1)))
    check_heads(near, ref, dtype)  # (the mean bound is the tighter of the two here)
    with pytest.raises(AssertionError, match="mean err"):
        check_heads(ref.float() + 0.9 * atol, ref, dtype)
    check_heads(ref.float() + 0.9 * atol, ref, dtype, mean=False)
    with pytest.raises(AssertionError, match="NaN"):
        bad = ref.clone()
        bad[1, 2, 3, 4] = float("nan")
        check_heads(bad, ref, dtype)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_checker_names_two_swapped_heads(dtype):
    ref = checker_case(dtype=dtype)
    out = ref.clone()
    out[:, 3], out[:, 5] = ref[:, 5], ref[:, 3]
    with pytest.raises(AssertionError) as e:
        check_heads(out, ref, dtype, report=100)
    msg = str(e.value)
    assert "54 of 189 (b, hq, pos) rows" in msg  # 3 sequences x 2 heads x 9 positions
    for b in range(3):
        assert f"b {b} head 3 pos 5 holds head 5 pos 5" in msg and f"b {b} head 5 pos 0 holds head 3 pos 0" in msg
    assert "matches no reference row" not in msg


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_checker_names_two_swapped_positions(dtype):
    ref = checker_case(dtype=dtype)
    out = ref.clone()
    out[:, :, 2], out[:, :, 7] = ref[:, :, 7], ref[:, :, 2]
    with pytest.raises(AssertionError) as e:
        check_heads(out, ref, dtype, report=100)
    msg = str(e.value)
    assert "42 of 189" in msg and "b 0 head 0 pos 2 holds head 0 pos 7" in msg
    assert "b 2 head 6 pos 7 holds head 6 pos 2" in msg


def test_checker_names_g_and_sq_swapped_in_the_row_decomposition():
    """Row rg read as (rg % g, rg / g) instead of (rg / Sq, rg % Sq): the bug that a power-of-two table with g == Sq
    (or the q-head pack, Sq == 1) cannot see. Row 32 of the 7-1-9 geometry is head 3 position 5; the swapped
    decomposition puts head 4 position 4 there."""
    hq, hkv, sq = 7, 1, 9
    ref = checker_case(hq, hkv, sq)
    g = hq // hkv
    out = torch.empty_like(ref)
    for rg in range(g * sq):
        h, p = head_of_row(rg, sq)
        out[:, h, p] = ref[:, rg % g, rg // g]
    assert head_of_row(32, sq) == (3, 5)
    with pytest.raises(AssertionError, match="b 0 head 3 pos 5 holds head 4 pos 4"):
        check_heads(out, ref, F16, report=100)


def test_checker_names_heads_regrouped_modulo_hkv():
    """q-heads grouped as hq % Hkv instead of hq // g, twice. As a permutation of the rows (the packed [Hkv][g] rows
    read as [g][Hkv]) the checker names every moved head; as the attention itself computed against the wrong
    kv-head it reports rows that match NO reference row, on exactly the heads whose kv-head changed."""
    hq, hkv, sq, d, n = 9, 3, 2, 64, 40
    g = hq // hkv
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(2, hq, sq, d, generator=gen).to(F16)
    k, v = (torch.randn(2, hkv, n, d, generator=gen).to(F16) for _ in range(2))
    ref = dense_oracle(q, k, v, True)
    perm = [(h % hkv) * g + h // hkv for h in range(hq)]
    with pytest.raises(AssertionError) as e:
        check_heads(ref[:, perm], ref, F16, report=100)
    msg = str(e.value)
    moved = [h for h in range(hq) if perm[h] != h]
    assert moved == [1, 2, 3, 5, 6, 7] and f"{2 * len(moved) * sq} of {2 * hq * sq}" in msg
    for h in moved:
        assert f"b 1 head {h} pos 1 holds head {perm[h]} pos 1" in msg
    wrong_kv = [h % hkv for h in range(hq)]
    wrong = dense_oracle(q, k[:, wrong_kv], v[:, wrong_kv], True)  # (MHA over the wrongly chosen kv-heads)
    with pytest.raises(AssertionError) as e:
        check_heads(wrong, ref, F16, report=100)
    msg = str(e.value)
    changed = [h for h in range(hq) if wrong_kv[h] != h // g]
    assert f"{2 * len(changed) * sq} of {2 * hq * sq}" in msg and " holds head" not in msg
    for h in changed:
        assert f"b 0 head {h} pos 0 matches no reference row" in msg


# ============================================================================================ 2. the table
def test_case_list_covers_the_geometry():
    geos = [g[:3] for g in GEOMETRY]
    assert len(set(geos)) == len(geos) == 16
    gs = {hq // hkv for hq, hkv, _ in geos}
    assert all(hq % hkv == 0 for hq, hkv, _ in geos)
    assert {3, 5, 7} <= gs and gs & {6, 12}
    assert {1, 3, 5} <= {hkv for _, hkv, _ in geos}
    assert all(rows_of(*g) <= MAX_ROWS for g in geos) and rows_of(*PAST_LIMIT) == 70
    # a row-block boundary strictly inside a head: row 32 exists and is not some head's position 0
    inside = [g for g in geos if rows_of(*g) > BLOCK_ROWS and head_of_row(BLOCK_ROWS, g[2])[1] != 0]
    assert {(7, 1, 9), (6, 2, 11), (10, 2, 7)} <= set(inside)
    assert head_of_row(32, 9) == (3, 5) and head_of_row(32, 11) == (2, 10) and head_of_row(32, 7) == (4, 4)
    assert any(rows_of(*g) == BLOCK_ROWS + 1 for g in geos)  # a second block of exactly one row
    assert sum(rows_of(*g) == MAX_ROWS for g in geos) >= 2    # exactly 64 rows
    assert (2, 1, 32) in geos and head_of_row(32, 32) == (1, 0)  # ... once with the boundary ON a head boundary
    # sizes: B = 3, capacity 256, lengths from {0, a value < Sq, 31, 33, 65, 256}; every geometry with Sq > 1 has a
    # causal row without a visible key and every geometry a sequence of more than one 32-key tile
    seen = set()
    for (hq, hkv, sq, lens, _), gi in zip(GEOMETRY, range(16)):
        assert len(lens) == 3 and max(lens) > 32 and max(lens) <= CAPACITY
        assert all(n in (0, 31, 33, 65, 256) or n < sq for n in lens), lens
        assert sq == 1 or any(n < sq for n in lens)
        seen |= {n if n in (0, 31, 33, 65, 256) else "short" for n in lens}
        page, d, dtype, layout = case_of(gi)
        assert CAPACITY % page == 0
    assert seen == {0, 31, 33, 65, 256, "short"}
    combos = [case_of(gi) for gi in range(16)]
    assert {(p, d) for p, d, _, _ in combos} == {(p, d) for p in (32, 64, 256) for d in (64, 72, 128)}
    assert {(t, lay) for _, _, t, lay in combos} == {(t, lay) for t in (F16, BF16) for lay in ("phsd", "pshd")}
    assert all(g in geos for g in SPLIT)


# ============================================================================================ shared GPU pieces
@pytest.fixture
def gpu(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    _debug.set_dec_fuse(None)
    yield fam
    _debug.set_knobs()
    _debug.set_dec_fuse(None)


MODES = {"unsplit": None, "split": None, "split_unfused": 0}  # mode -> _debug.set_dec_fuse
# (table row, mode): every row unsplit; the split geometries with the fused merge and with the combine launch
PAGED_CASES = [(gi, "unsplit") for gi in range(len(GEOMETRY))] + \
              [(index_of(*g), m) for g in SPLIT for m in ("split", "split_unfused")]
PAGED_IDS = [f"{GEO_IDS[gi]}-{m}" for gi, m in PAGED_CASES]


def shape_of(gi, mode):
    """(lengths, capacity, causal) of a table row in a mode: Sq > 1 is causal (each position its own diagonal)."""
    hq, hkv, sq, lens, _ = GEOMETRY[gi]
    if mode == "unsplit":
        return lens, CAPACITY, sq > 1
    return SPLIT_LENS, SPLIT_CAPACITY, sq > 1


@functools.lru_cache(maxsize=None)
def paged_inputs(gi, mode="unsplit"):
    """make_paged's (q, k, v, k_cache, v_cache, table, lens) of a table row (never modified)."""
    hq, hkv, sq, _, _ = GEOMETRY[gi]
    page, d, dtype, layout = case_of(gi)
    lens, cap, _ = shape_of(gi, mode)
    return make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 7000 + gi, layout)


@functools.lru_cache(maxsize=None)
def fp8_inputs(gi, mode="unsplit"):
    """make_fp8_paged's (q, K8, V8, pools, table, lens) and descales != 1, distinct per (batch, kv-head)
    (test_paged_sink.descales). The FP8 entry needs D % 16 == 0: a row whose head dim is 72 runs at 128."""
    hq, hkv, sq, _, _ = GEOMETRY[gi]
    page, d, dtype, layout = case_of(gi)
    d = 128 if d == 72 else d
    lens, cap, _ = shape_of(gi, mode)
    kd, vd = descales(len(lens), hkv), descales(len(lens), hkv, 2)
    return make_fp8_paged(lens, hq, hkv, sq, page, cap, d, dtype, 7100 + gi, layout, kd, vd) + (kd, vd)


def run_paged(args, causal, w=-1, fuse=None, lse=False, **kw):
    """One flash_attn_paged_func launch: (result on the host, last_path, last_dec_fused)."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    _debug.set_knobs()
    _debug.set_dec_fuse(fuse)
    try:
        res = flash_attn_paged_func(*dv(*args), causal=causal, window_left=w, return_lse=lse,
                                    **{n: t.to(DEV) for n, t in kw.items()})
        path, fused = _debug.last_path(), _debug.last_dec_fused()
        torch.cuda.synchronize()
    finally:
        _debug.set_dec_fuse(None)
    return (tuple(t.cpu() for t in res) if lse else res.cpu()), path, fused


def want_path(mode, fp8=False):
    return ("decode_paged_fp8" if fp8 else "decode_paged") + ("" if mode == "unsplit" else "_split")


def assert_path(path, fused, mode, fp8=False):
    assert path == want_path(mode, fp8), path
    if mode != "unsplit":
        assert fused == (mode == "split")


@functools.lru_cache(maxsize=None)
def paged_result(gi, mode):
    """The plain paged launch of a case, shared by the oracle, bit-equality and LSE tests."""
    q, _, _, kc, vc, table, sl = paged_inputs(gi, mode)
    return run_paged((q, kc, vc, table, sl), shape_of(gi, mode)[2], fuse=MODES[mode])


def assert_empty_sequences_are_zero(out, lens):
    for i, n in enumerate(lens):
        if n == 0:
            assert (out[i] == 0).all()


# ============================================================================================ 3. the decode family
DENSE_SK = (33, 65, 256, 7)  # keys of the dense cases, rotated over the table; 7 < Sq: causal rows without a key
DENSE_CASES = [(gi, c) for gi, g in enumerate(GEOMETRY) for c in ((False, True) if g[2] > 1 else (False,))]


@pytest.mark.gpu
@pytest.mark.parametrize("gi,causal", DENSE_CASES,
                         ids=[f"{GEO_IDS[gi]}-{'causal' if c else 'full'}" for gi, c in DENSE_CASES])
def test_dense_decode(gpu, gi, causal):
    """flash_attn_func: Sq == 1 runs as the q-head pack, Sq > 1 unpacked -- both on the decode kernel."""
    from flash_attention_cute_amd import _debug, flash_attn_func
    from tests.test_gpu_parity import make

    hq, hkv, sq, _, _ = GEOMETRY[gi]
    _, d, dtype, _ = case_of(gi)
    q, k, v = make(3, hq, hkv, sq, DENSE_SK[gi % 4], d, dtype, 7200 + gi)
    out = flash_attn_func(*dv(q, k, v), causal=causal)
    assert _debug.last_path() == "decode"
    torch.cuda.synchronize()
    check_heads(out, dense_oracle(q, k, v, causal and sq > 1), dtype)  # (the pack forces non-causal)


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(GEOMETRY)), ids=GEO_IDS)
def test_padded_decode_with_key_ranges(gpu, gi):
    """flash_attn_padded_func over a dense cache with each sequence's own key range [ks, ke)."""
    from flash_attention_cute_amd import _debug, flash_attn_padded_func

    _, _, sq, lens, _ = GEOMETRY[gi]
    q, k, v, _, _, _, _ = paged_inputs(gi)
    ks = torch.tensor([0, 5, 40], dtype=I32)
    ke = torch.tensor([min(s + n, CAPACITY) for s, n in zip(ks.tolist(), lens)], dtype=I32)
    causal = sq > 1
    out = flash_attn_padded_func(*dv(q, k, v, ks, ke), causal=causal)
    assert _debug.last_path() == "decode"
    torch.cuda.synchronize()
    check_heads(out, oracle_padded(q, k, v, ks, ke, None, None, q.size(-1) ** -0.5, causal), case_of(gi)[2])
    assert_empty_sequences_are_zero(out, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("gi,mode", PAGED_CASES, ids=PAGED_IDS)
def test_paged_decode(gpu, gi, mode):
    """flash_attn_paged_func on a 16-bit pool: the oracle, and the bits of the padded decode on the dense cache."""
    from flash_attention_cute_amd import _debug, flash_attn_padded_func

    q, k, v, _, _, _, sl = paged_inputs(gi, mode)
    lens, _, causal = shape_of(gi, mode)
    out, path, fused = paged_result(gi, mode)
    assert_path(path, fused, mode)
    check_heads(out, paged_oracle(q, k, v, sl, causal), case_of(gi)[2])
    assert_empty_sequences_are_zero(out, lens)
    _debug.set_dec_fuse(MODES[mode])
    dense = flash_attn_padded_func(*dv(q, k, v, torch.zeros_like(sl), sl), causal=causal)
    assert _debug.last_path() == ("decode" if mode == "unsplit" else "decode_split")
    assert torch.equal(out, dense.cpu())


FP8_CASES = [((7, 1, 1), "unsplit"), ((40, 5, 1), "unsplit"), ((6, 2, 11), "unsplit"), ((33, 1, 1), "split")]


@pytest.mark.gpu
@pytest.mark.parametrize("geo,mode", FP8_CASES, ids=[f"{geo_id(g)}-{m}" for g, m in FP8_CASES])
def test_fp8_paged_decode(gpu, geo, mode):
    """Hkv = 1, Hkv = 5, two row blocks (33 rows) and a split launch, descales != 1 per (batch, kv-head)."""
    gi = index_of(*geo)
    q, k8, v8, kc8, vc8, table, sl, kd, vd = fp8_inputs(gi, mode)
    lens, _, causal = shape_of(gi, mode)
    out, path, fused = run_paged((q, kc8, vc8, table, sl), causal, fuse=MODES[mode], k_descale=kd, v_descale=vd)
    assert_path(path, fused, mode, fp8=True)
    check_heads(out, fp8_oracle(q, k8, v8, sl, kd, vd, causal), case_of(gi)[2])
    assert_empty_sequences_are_zero(out, lens)


WINDOW_GEOS = ((7, 1, 9), (6, 2, 11), (10, 2, 7))  # the block boundary falls inside a head


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("w", [0, 31, 40])
@pytest.mark.parametrize("geo", WINDOW_GEOS, ids=[geo_id(g) for g in WINDOW_GEOS])
def test_window_decode(gpu, geo, w, fp8):
    """A sliding window with Sq = 7 .. 11: the windows of one head's positions start in different 32-key tiles, and
    each row's lower bound comes from ITS position (rg % Sq)."""
    gi = index_of(*geo)
    dtype = case_of(gi)[2]
    if fp8:
        q, k8, v8, kc8, vc8, table, sl, kd, vd = fp8_inputs(gi)
        out, path, _ = run_paged((q, kc8, vc8, table, sl), True, w, k_descale=kd, v_descale=vd)
        ref = fp8_win_oracle(q, k8, v8, sl, kd, vd, True, w)
    else:
        q, k, v, kc, vc, table, sl = paged_inputs(gi)
        out, path, _ = run_paged((q, kc, vc, table, sl), True, w)
        ref = win_oracle(q, k, v, sl, True, w)
    assert path == want_path("unsplit", fp8)
    check_heads(out, ref, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("gi,mode", PAGED_CASES, ids=PAGED_IDS)
def test_lse_decode(gpu, gi, mode):
    """return_lse=True: the LSE [B, Hq, Sq] within test_paged_lse's 2^-12 of float64, O the bits of the plain call."""
    q, k, v, kc, vc, table, sl = paged_inputs(gi, mode)
    lens, _, causal = shape_of(gi, mode)
    (out, lse), path, fused = run_paged((q, kc, vc, table, sl), causal, fuse=MODES[mode], lse=True)
    assert_path(path, fused, mode)
    assert lse.dtype == torch.float32 and lse.shape == q.shape[:3]
    assert torch.equal(out, paged_result(gi, mode)[0])
    check_lse(lse, lse_oracle(q, k, lens, q.size(-1) ** -0.5, causal), f"{GEO_IDS[gi]}-{mode}")
    check_heads(out, paged_oracle(q, k, v, sl, causal), case_of(gi)[2])


SINK_GEOS = ((7, 1, 1), (28, 4, 1), (33, 1, 1), (7, 1, 9), (12, 1, 5))
SINK_WINDOW = {"unsplit": 40, "split": 1023, "split_unfused": 1023}  # (a window of 1024 keys still plans 2 splits)


@functools.lru_cache(maxsize=None)
def sink_inputs(geo, mode, fp8):
    """The table row's head dim and page size; lengths and capacity of the mode (the split lengths for ANY of the
    sink geometries: 12-1-5 and 28-4-1 are no rows of head_geometry.SPLIT)."""
    gi = index_of(*geo)
    hq, hkv, sq = geo
    page, d, dtype, layout = case_of(gi)
    lens, cap = (GEOMETRY[gi][3], CAPACITY) if mode == "unsplit" else (SPLIT_LENS, SPLIT_CAPACITY)
    if fp8:
        d = 128 if d == 72 else d
        kd, vd = descales(len(lens), hkv), descales(len(lens), hkv, 2)
        return make_fp8_paged(lens, hq, hkv, sq, page, cap, d, dtype, 7300 + gi, layout, kd, vd) + (kd, vd), lens, dtype
    return make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 7300 + gi, layout), lens, dtype


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("window", [False, True], ids=["full", "window"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geo", SINK_GEOS, ids=[geo_id(g) for g in SINK_GEOS])
def test_sink_decode(gpu, geo, mode, window, fp8):
    """sinks=: a distinct finite sink per q-head that carries weight, head 2 at -inf. The sink is looked up per ROW
    (q-head hkv * g + rg / Sq), in the kernel's epilogue or, in a split launch, in the merge."""
    args, lens, dtype = sink_inputs(geo, mode, fp8)
    causal, w = geo[2] > 1, (SINK_WINDOW[mode] if window else -1)
    if fp8:
        q, k8, v8, kc, vc, table, sl, kd, vd = args
        k, v, ds = k8.float(), v8.float(), dict(k_descale=kd, v_descale=vd)
    else:
        q, k, v, kc, vc, table, sl = args
        kd = vd = None
        ds = {}
    sinks = center_sinks(q, k, lens, 11, kd=kd)
    out, path, fused = run_paged((q, kc, vc, table, sl), causal, w, MODES[mode], sinks=sinks, **ds)
    assert_path(path, fused, mode, fp8)
    ref = sink_oracle(q, k, v, lens, sinks, causal, w, kd=kd, vd=vd)
    check_heads(out, ref, dtype)
    assert_empty_sequences_are_zero(out, lens)
    if mode == "unsplit" and not window:
        # the case bites: the same softmax with every head's sink taken from its neighbour misses the bound
        with pytest.raises(AssertionError, match="matches no reference row"):
            check_heads(sink_oracle(q, k, v, lens, sinks.roll(1), causal, w, kd=kd, vd=vd), ref, dtype)
        plain, _, _ = run_paged((q, kc, vc, table, sl), causal, w, MODES[mode], **ds)
        assert torch.equal(out[:, 2], plain[:, 2]) and not torch.equal(out[:, 3:], plain[:, 3:])  # (head 2: no sink)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["bhsd", "bshd"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("hq,sq,d,dtype", [(3, 21, 64, F16), (7, 9, 128, BF16), (7, 1, 72, F16), (3, 5, 128, BF16)],
                         ids=["h3-s21-d64-f16", "h7-s9-d128-bf16", "h7-s1-d72-f16", "h3-s5-d128-bf16"])
def test_merge_states(gpu, hq, sq, d, dtype, n, layout):
    """flash_attn_merge_states (4 rows per workgroup over the flattened (head, position) rows) with 3 and 7 heads."""
    from flash_attention_cute_amd import flash_attn_merge_states

    outs, lses = make_states(n, 3, hq, sq, d, dtype, 7400 + hq + n)
    if layout == "bshd":  # a transposed view: head stride D, seq stride H * D
        d_outs = outs.transpose(2, 3).contiguous().to(DEV).transpose(2, 3)
        d_lses = lses.transpose(2, 3).contiguous().to(DEV).transpose(2, 3)
    else:
        d_outs, d_lses = outs.to(DEV), lses.to(DEV)
    o, l = flash_attn_merge_states(d_outs, d_lses, return_lse=True)
    torch.cuda.synchronize()
    ro, rl = merge_oracle(outs, lses)
    check_heads(o, ro, dtype)
    check_lse(l, rl, f"merge-h{hq}-s{sq}-n{n}-{layout}")


# (Hq, Hkv, B, page, D, dtype, layout): c = max(1, 32 // g) sequences per group
SHARED = [
    (7, 1, 9, 32, 64, F16, "phsd"),      # g 7: c = 4 (28 of the 32 rows), two groups and a tail of one
    (9, 3, 11, 64, 128, BF16, "pshd"),   # g 3: c = 10 and a tail of one
    (10, 2, 7, 32, 72, BF16, "phsd"),    # g 5: c = 6 and a tail of one
    (33, 1, 3, 64, 128, F16, "pshd"),    # g 33: c = 1, every sequence its own group
]
SHARED_SUFFIXES = (0, 1, 33, 100)


def poisoned_prefix_entries(table, sl, c, n_pre, page):
    """Out-of-range ids in the prefix entries of every row but each group's first, and in every entry past a
    sequence's last page, as test_shared_prefix.test_shared_prefix_entries_that_are_never_read does."""
    bad = table.clone()
    for i in range(table.size(0)):
        if i % c:
            bad[i, :n_pre] = 2 ** 31 - 1 - i
        bad[i, (int(sl[i]) + page - 1) // page:] = -(2 ** 31) + i
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv,b,page,d,dtype,layout", SHARED,
                         ids=[f"{c[0]}-{c[1]}-b{c[2]}-p{c[3]}-d{c[4]}-{NAMES[c[5]]}" for c in SHARED])
def test_shared_prefix(gpu, hq, hkv, b, page, d, dtype, layout):
    """flash_attn_paged_shared_prefix_func groups c = max(1, 32 // g) sequences into one batch row of c positions
    (an as_strided view of q): c = 4, 10, 6, 1. Against the oracle on the full keys within the bound
    test_shared_prefix.py uses for this call (TOL, elementwise), the merged LSE within 2^-12."""
    from flash_attention_cute_amd import flash_attn_paged_shared_prefix_func as shared

    prefix = 2 * page
    q, k, v, kc, vc, table, sl, c = make_shared(b, hq, hkv, page, prefix, SHARED_SUFFIXES, d, dtype, 7500 + hq, layout)
    assert c == max(1, GROUP_ROWS // (hq // hkv)) == {7: 4, 3: 10, 5: 6, 33: 1}[hq // hkv]
    assert b % c == (0 if c == 1 else 1) and b // c >= 1  # full groups and (c > 1) a tail of one
    bad = poisoned_prefix_entries(table, sl, c, prefix // page, page)
    assert c == 1 or not torch.equal(bad[:, :prefix // page], table[:, :prefix // page])
    out, lse = shared(*dv(q, kc, vc, bad, sl), prefix, return_lse=True)
    torch.cuda.synchronize()
    check_heads(out, paged_oracle(q, k, v, sl, False), dtype, mean=False)
    check_lse(lse, lse_oracle(q, k, sl.tolist(), d ** -0.5, False), f"shared-{hq}-{hkv}")
    assert torch.equal(shared(*dv(q, kc, vc, bad, sl), prefix), out)  # without the lse: the same bits


@pytest.mark.gpu
def test_shared_prefix_fp8(gpu):
    """g = 7 on an FP8 pool: the descales of a group come from its first row (kd[lo:hi:c])."""
    from flash_attention_cute_amd import flash_attn_paged_shared_prefix_func as shared

    hq, hkv, b, page, d, prefix = 7, 1, 9, 64, 128, 128
    c = GROUP_ROWS // (hq // hkv)
    lens = [prefix + SHARED_SUFFIXES[i % 4] for i in range(b)]
    cap = (max(lens) + page - 1) // page * page
    # rows of a group must share their descales: one pair per GROUP, distinct between groups and != 1
    kd = descales(3, hkv).repeat_interleave(c, dim=0)[:b].contiguous()
    vd = descales(3, hkv, 2).repeat_interleave(c, dim=0)[:b].contiguous()
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, 1, page, cap, d, BF16, 7550, kd=kd, vd=vd)
    share_prefix(k8, v8, kc8, vc8, table, prefix, page, c)
    bad = poisoned_prefix_entries(table, sl, c, prefix // page, page)
    out, lse = shared(*dv(q, kc8, vc8, bad, sl), prefix, k_descale=kd.to(DEV), v_descale=vd.to(DEV), return_lse=True)
    torch.cuda.synchronize()
    check_heads(out, fp8_oracle(q, k8, v8, sl, kd, vd, False), BF16, mean=False)
    check_lse(lse, lse_oracle(q, k8.float(), lens, d ** -0.5, False, kd), "shared-fp8")


# ---------------------------------------------------------------------------- one row past the limit: 70 rows
def past_limit_inputs(page, d=64, fp8=False):
    hq, hkv, sq = PAST_LIMIT
    lens = (65, 4, 256)
    if fp8:
        kd, vd = descales(3, hkv), descales(3, hkv, 2)
        return make_fp8_paged(lens, hq, hkv, sq, page, CAPACITY, d, F16, 7600, "phsd", kd, vd) + (kd, vd)
    return make_paged(lens, hq, hkv, sq, page, CAPACITY, d, F16, 7600)


def test_past_the_limit_sinks_lse_and_shared_prefix_raise_as_documented():
    """7-1-10 is 70 rows: the calls that exist for decode shapes only say so before anything is launched."""
    from flash_attention_cute_amd import flash_attn_paged_func, flash_attn_paged_shared_prefix_func

    assert rows_of(*PAST_LIMIT) == MAX_ROWS + 6
    q, _, _, kc, vc, table, sl = past_limit_inputs(64)
    with pytest.raises(NotImplementedError, match="decode shapes"):
        flash_attn_paged_func(q, kc, vc, table, sl, causal=True, sinks=torch.zeros(7))
    with pytest.raises(NotImplementedError, match="decode shapes"):
        flash_attn_paged_func(q, kc, vc, table, sl, causal=True, return_lse=True)
    with pytest.raises(ValueError, match="decode steps"):  # Sq > 1: no shared-prefix call, at any row count
        flash_attn_paged_shared_prefix_func(q, kc, vc, table, sl, 64)
    q3 = paged_inputs(index_of(14, 2, 3))[0]
    with pytest.raises(ValueError, match="decode steps"):
        flash_attn_paged_shared_prefix_func(q3, kc, vc, table, sl, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("page", [64, 32])
def test_past_the_limit_takes_the_prefill_route(gpu, page):
    """70 rows on the uniform ops: the dense op and the paged op (in place with 64-key pages, the copying path with
    32-key pages) run the prefill kernel; an FP8 pool takes the copying path."""
    from flash_attention_cute_amd import _debug, flash_attn_func, flash_attn_paged_func

    q, k, v, kc, vc, table, sl = past_limit_inputs(page)
    out = flash_attn_paged_func(*dv(q, kc, vc, table, sl), causal=True)
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged() == (page == 64)
    torch.cuda.synchronize()
    check_heads(out, paged_oracle(q, k, v, sl, True), F16)
    dense = flash_attn_func(*dv(q, k, v), causal=True)
    assert _debug.last_path() == "w4"
    check_heads(dense, dense_oracle(q, k, v, True), F16)
    q8, k8, v8, kc8, vc8, table8, sl8, kd, vd = past_limit_inputs(page, fp8=True)
    out8 = flash_attn_paged_func(*dv(q8, kc8, vc8, table8, sl8), causal=True, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    assert _debug.last_path() == "w4"
    check_heads(out8, fp8_oracle(q8, k8, v8, sl8, kd, vd, True), F16)


@pytest.mark.gpu
def test_fp8_with_head_dim_72_raises(gpu):
    """The FP8 entry reads the pool in place and needs D % 16 == 0: D 72 is rejected by the library, not padded."""
    from flash_attention_cute_amd import flash_attn_paged_func

    q, _, _, kc8, vc8, table, sl, kd, vd = past_limit_inputs(64, d=72, fp8=True)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        flash_attn_paged_func(*dv(q[:, :, :1].contiguous(), kc8, vc8, table, sl), k_descale=kd.to(DEV),
                              v_descale=vd.to(DEV))


# ============================================================================================ 4. the write side
APPEND_GEOS = ((7, 1), (9, 3), (40, 5))
APPEND_LENS = (31, 30, 64)  # page 32: one token lands on the last row of a page / on the first row of the next one;
#                             three tokens cross the edge after 1 (31, 32, 33) and after 2 (30, 31, 32) of them
APPEND_CAP, APPEND_PAGE = 128, 32


def append_shape(hq):
    """(D, dtype, pool layout) per geometry: D 128 / 72 / 64."""
    return {7: (128, F16, "phsd"), 9: (72, BF16, "pshd"), 40: (64, F16, "pshd")}[hq]


@pytest.mark.gpu
@pytest.mark.parametrize("sn", [1, 3])
@pytest.mark.parametrize("hq,hkv", APPEND_GEOS, ids=[f"{a}-{b}" for a, b in APPEND_GEOS])
def test_append_16bit(gpu, hq, hkv, sn):
    """flash_attn_kvcache_append with RoPE, q rotated as well: the pools against test_kvcache.expected_append bit for
    bit (every row that is not written keeps its poison), q against the rotation at the last positions."""
    from flash_attention_cute_amd import apply_rope

    d, dtype, layout = append_shape(hq)
    kc, vc, table, sl = make_cache(APPEND_LENS, sn, hkv, APPEND_PAGE, APPEND_CAP, d, dtype, 7700 + hq + sn, layout)
    k, v, q = (new_tokens(3, h, sn, d, dtype, 7710 + i).to(DEV) for i, h in enumerate((hkv, hkv, hq)))
    cos, sin = dv(*rope_tables(APPEND_CAP, d, dtype))
    kc, vc = dv(kc, vc)
    before = bits(kc).clone()
    ek, ev = expected_append(kc, vc, k, v, APPEND_LENS, table, cos, sin, apply_rope)
    new, q_rot = torch.ops.flash_attention.kvcache_append(kc, vc, k, v, *dv(sl, table), q, cos, sin)
    torch.cuda.synchronize()
    assert new.tolist() == [n + sn for n in APPEND_LENS]
    assert torch.equal(bits(kc), bits(ek)) and torch.equal(bits(vc), bits(ev))
    written = (bits(kc) != before).any(dim=-1)  # [pages, Hkv, page] rows
    assert int(written.sum()) == 3 * sn * hkv  # exactly the new tokens' rows, on every kv-head
    assert len(targets(APPEND_LENS, sn, table, APPEND_PAGE, APPEND_CAP, kc.size(0))) == 3 * sn
    qpos = torch.tensor([[n + i for i in range(sn)] for n in APPEND_LENS], device=DEV)
    assert torch.equal(q_rot, apply_rope(q, cos[qpos], sin[qpos]))


@pytest.mark.gpu
@pytest.mark.parametrize("sn", [1, 3])
@pytest.mark.parametrize("hq,hkv", APPEND_GEOS, ids=[f"{a}-{b}" for a, b in APPEND_GEOS])
def test_append_fp8(gpu, hq, hkv, sn):
    """The quantizing append: the byte pools against test_fp8_kvcache.expected_fp8_append (0x7F in every row that is
    not written), descales != 1 per (batch, kv-head); q_rot is the 16-bit rotation."""
    from flash_attention_cute_amd import apply_rope

    d, dtype, layout = append_shape(hq)
    d = 128 if d == 72 else d  # (an fp8 cache needs D % 16 == 0)
    kc8, vc8, table, sl = make_fp8_cache(APPEND_LENS, sn, hkv, APPEND_PAGE, APPEND_CAP, d, 7800 + hq + sn, layout)
    kd, vd = descales(3, hkv), descales(3, hkv, 2)
    k, v, q = (new_tokens(3, h, sn, d, dtype, 7810 + i).to(DEV) for i, h in enumerate((hkv, hkv, hq)))
    cos, sin = dv(*rope_tables(APPEND_CAP, d, dtype))
    gk, gv = dv(kc8, vc8)
    ek, ev = expected_fp8_append(gk, gv, k, v, APPEND_LENS, table, cos, sin, apply_rope, kd, vd)
    new, q_rot = torch.ops.flash_attention.kvcache_append_fp8(gk, gv, k, v, *dv(sl, table), q, cos, sin, *dv(kd, vd))
    torch.cuda.synchronize()
    assert new.tolist() == [n + sn for n in APPEND_LENS]
    assert torch.equal(norm_bytes(gk.cpu()), norm_bytes(ek.cpu())), "K pool"
    assert torch.equal(norm_bytes(gv.cpu()), norm_bytes(ev.cpu())), "V pool"
    written = (gk.cpu().view(torch.uint8) != kc8.view(torch.uint8)).any(dim=-1)
    assert int(written.sum()) == 3 * sn * hkv  # exactly the new tokens' rows (no e4m3 byte written is 0x7F)
    qpos = torch.tensor([[n + i for i in range(sn)] for n in APPEND_LENS], device=DEV)
    assert q_rot.dtype == dtype and torch.equal(q_rot, apply_rope(q, cos[qpos], sin[qpos]))


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv", [(7, 1), (9, 3)], ids=["7-1", "9-3"])
def test_with_kvcache_step(gpu, hq, hkv):
    """One flash_attn_with_kvcache step of 3 tokens, causal: the composed append + paged call bit for bit, and the
    oracle on the cache after the append."""
    fam = gpu
    sq, lens = 3, (31, 0, 62)
    d, dtype, layout = append_shape(hq)
    kc, vc, table, sl = dv(*make_cache(lens, sq, hkv, APPEND_PAGE, APPEND_CAP, d, dtype, 7900 + hq, layout))
    k, v, q = (new_tokens(3, h, sq, d, dtype, 7910 + i).to(DEV) for i, h in enumerate((hkv, hkv, hq)))
    cos, sin = dv(*rope_tables(APPEND_CAP, d, dtype))
    kc2, vc2 = kc.clone(), vc.clone()
    out, new = fam.flash_attn_with_kvcache(q, kc, vc, k, v, cos, sin, cache_seqlens=sl, block_table=table, causal=True,
                                           return_seqlens=True)
    new2, q_rot = torch.ops.flash_attention.kvcache_append(kc2, vc2, k, v, sl, table, q, cos, sin)
    ref = fam.flash_attn_paged_func(q_rot, kc2, vc2, table, new2, causal=True)
    torch.cuda.synchronize()
    assert new.tolist() == [n + sq for n in lens] and torch.equal(new, new2)
    assert torch.equal(bits(kc), bits(kc2)) and torch.equal(bits(vc), bits(vc2))
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)
    kd, vd = fam._gather_pages(kc, table).cpu(), fam._gather_pages(vc, table).cpu()
    check_heads(out, paged_oracle(q_rot.cpu(), kd, vd, new.cpu(), True), dtype)


RAGGED_NEWS = (1, 40, 0, 70)
RAGGED_LENS = (63, 30, 100, 0)  # 63 + 1 ends on a page edge; 30 + 40 and 0 + 70 cross it (page 64)


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv,d,dtype", [(7, 1, 128, BF16), (10, 2, 64, F16)], ids=["7-1", "10-2"])
def test_ragged_append_and_step(gpu, hq, hkv, d, dtype):
    """flash_attn_kvcache_append_varlen against per-sequence appends (bit for bit, q rotated), and
    flash_attn_varlen_with_kvcache against the composed step (bit for bit) and the oracle per sequence."""
    from flash_attention_cute_amd import _debug
    from test_paged_varlen import cu_of, packed_rows, per_sequence_append, ragged_cache

    fam = gpu
    page, cap, total = 64, 256, sum(RAGGED_NEWS)
    kc, vc, table, sl = dv(*ragged_cache(RAGGED_LENS, RAGGED_NEWS, hkv, page, cap, d, dtype, 8000 + hq))
    cu = cu_of(RAGGED_NEWS).to(DEV)
    k, v, q = (packed_rows(total, h, d, dtype, 8010 + i).to(DEV) for i, h in enumerate((hkv, hkv, hq)))
    cos, sin = dv(*rope_tables(cap, d, dtype))
    kc_ref, vc_ref, new_ref, q_ref = per_sequence_append(kc, vc, k, v, cu, sl, table, cos, sin, q, cu)
    kc2, vc2 = kc.clone(), vc.clone()
    new2, q_rot = fam.flash_attn_kvcache_append_varlen(kc2, vc2, k, v, cu, sl, table, cos, sin, q, cu)
    torch.cuda.synchronize()
    assert new2.tolist() == [a + b for a, b in zip(RAGGED_LENS, RAGGED_NEWS)] and torch.equal(new2, new_ref)
    assert torch.equal(bits(kc2), bits(kc_ref)) and torch.equal(bits(vc2), bits(vc_ref))
    assert torch.equal(bits(q_rot), bits(q_ref))
    assert int((bits(kc2) != bits(kc)).any(dim=-1).sum()) == total * hkv  # the new tokens' rows and no other
    assert (kc2.cpu() == PATTERN).all(dim=-1).any()
    # the step
    out, new = fam.flash_attn_varlen_with_kvcache(q, kc, vc, cu, max(RAGGED_NEWS), k, v, rotary_cos=cos, rotary_sin=sin,
                                                  cache_seqlens=sl, block_table=table, causal=True, return_seqlens=True)
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
    ref = fam.flash_attn_paged_varlen_func(q_rot, kc2, vc2, cu, max(RAGGED_NEWS), table, new2, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(new, new2) and torch.equal(bits(kc), bits(kc2)) and torch.equal(bits(vc), bits(vc2))
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)
    kd, vd, qr = fam._gather_pages(kc, table).cpu(), fam._gather_pages(vc, table).cpu(), q_rot.cpu()
    want, r = torch.zeros_like(qr), cu.tolist()
    for b, n in enumerate(new.tolist()):
        if RAGGED_NEWS[b]:
            one = paged_oracle(qr[r[b]:r[b + 1]].transpose(0, 1)[None], kd[b:b + 1], vd[b:b + 1],
                               torch.tensor([n], dtype=I32), True)
            want[r[b]:r[b + 1]] = one[0].transpose(0, 1)
    check_heads(packed_as_heads(out), packed_as_heads(want), dtype)


# ============================================================================================ 5. the prefill family
# (Hq, Hkv, Sq, Sk, D, dtype): Sq = Sk = 300 is two 256-row q-tiles with a ragged last one, at g = 7, 7, 3, 5, 12, 1;
# one Sq < Sk and one Sq > Sk (causal rows without a visible key)
PREFILL = [(7, 1, 300, 300, 128, F16), (28, 4, 300, 300, 64, BF16), (9, 3, 300, 300, 128, BF16),
           (10, 2, 300, 300, 64, F16), (24, 2, 300, 300, 128, F16), (5, 5, 300, 300, 64, BF16),
           (7, 1, 100, 333, 64, BF16), (10, 2, 333, 100, 128, F16)]


def prefill_inputs(hq, hkv, sq, sk, d, dtype):
    from tests.test_gpu_parity import make

    return make(1, hq, hkv, sq, sk, d, dtype, 8100 + hq + hkv + sq)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("hq,hkv,sq,sk,d,dtype", PREFILL, ids=["-".join(map(str, p[:5])) + "-" + NAMES[p[5]] for p in PREFILL])
def test_dense_prefill(gpu, hq, hkv, sq, sk, d, dtype, causal):
    """flash_attn_func on the prefill kernel at the default grid, and with 8 workgroups: a workgroup then walks
    several (head, q-tile) blocks and the block count (7 heads x 2 tiles) is no multiple of the grid."""
    from flash_attention_cute_amd import _debug, flash_attn_func

    q, k, v = prefill_inputs(hq, hkv, sq, sk, d, dtype)
    out = flash_attn_func(*dv(q, k, v), causal=causal)
    assert _debug.last_path() == "w4"
    with _debug.knobs(w4_grid=8):
        walked = flash_attn_func(*dv(q, k, v), causal=causal)
        assert _debug.last_path() == "w4"
    torch.cuda.synchronize()
    ref = dense_oracle(q, k, v, causal)
    check_heads(out, ref, dtype)
    check_heads(walked, ref, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv", [(7, 1), (12, 2), (24, 2)], ids=["7-1", "12-2", "24-2"])
def test_forced_prefill_layouts(gpu, hq, hkv):
    """Zigzag, key-split and head-packed causal blocks forced on: g = 12 head-packs (three q-head quads per
    kv-head) and is bit-identical to the plain layout, as tests/test_gpu_parity.py::test_head_packed_blocks claims;
    g = 7 and g = 6 are no multiple of 4 and must report that the head-pack did not run."""
    import flash_attention_cute_amd as m
    from flash_attention_cute_amd import _debug

    dtype = BF16 if hq == 12 else F16
    q, k, v = prefill_inputs(hq, hkv, 300, 300, 128, dtype)
    args = dv(q, k, v)
    ref = dense_oracle(q, k, v, True)
    quads = hq // hkv % 4 == 0

    def run(split=0, zigzag=0, head_pack=0):
        _debug.set_split(split)
        _debug.set_zigzag(zigzag)
        _debug.set_head_pack(head_pack)
        out = m.flash_attn_func(*args, causal=True)
        assert _debug.last_path() == "w4"
        return out, _debug.last_layout(), _debug.last_head_pack()

    m.split_errors(reset=True)
    try:
        plain, layout, _ = run()
        assert layout == "plain"
        zigzag, layout, _ = run(zigzag=2)
        assert layout == "zigzag"
        split, layout, head_packed = run(split=2)
        assert layout == "split" and not head_packed
        packed, layout, head_packed = run(head_pack=2)
        assert head_packed == quads and layout == ("headpack" if quads else "plain")
        torch.cuda.synchronize()
    finally:
        _debug.set_split()
        _debug.set_zigzag()
        _debug.set_head_pack()
    assert m.split_errors() == 0
    assert torch.equal(packed, plain)
    for out in (plain, zigzag, split):
        check_heads(out, ref, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["varlen", "window", "rope", "padded"])
def test_other_prefill_entries(gpu, entry):
    """flash_attn_varlen_func (28-4), flash_attn_window_func (7-1, W 40), flash_attn_rope_func (28-4) and
    flash_attn_padded_func with query ranges (7-1), causal."""
    from flash_attention_cute_amd import (_debug, flash_attn_padded_func, flash_attn_rope_func, flash_attn_varlen_func,
                                          flash_attn_window_func)
    from test_padded import make_batch, ranges
    from test_rope import oracle_rope, tables
    from test_varlen import pack

    if entry == "varlen":
        q, k, v, cu_q, cu_k, mq, mk = pack((28, 4, 128, [(300, 300), (0, 0), (45, 130), (1, 70)]), BF16, 8200)
        out = flash_attn_varlen_func(*dv(q, k, v, cu_q, cu_k), mq, mk, causal=True)
        ref = OC.forward_varlen(q, k, v, cu_q, cu_k, 128 ** -0.5, True).float()
        out, ref, dtype = packed_as_heads(out), packed_as_heads(ref), BF16
    elif entry == "window":
        q, k, v = prefill_inputs(7, 1, 300, 300, 128, F16)
        dtype = F16
        out = flash_attn_window_func(*dv(q, k, v), 40, causal=True)
        ref = dense_oracle(q, k, v, True, w=40)
    elif entry == "rope":
        q, k, v = make_batch(2, 28, 4, 300, 300, 64, F16, 8201, "bshd")  # HF projection views
        cos, sin = tables(2, 300, 64, F16, 8202)
        out = flash_attn_rope_func(*dv(q, k, v, cos, sin), causal=True)
        ref, dtype = dense_oracle(oracle_rope(q, cos, sin), k.contiguous(), v.contiguous(), True), F16
    else:
        b, sq, sk = 3, 300, 333
        q, k, v = make_batch(b, 7, 1, sq, sk, 128, BF16, 8203, "bshd")
        ks, ke, qs, qe = ranges(b, sq, sk, 8203, "mixed")
        out = flash_attn_padded_func(*dv(q, k, v, ks, ke, qs, qe), causal=True)
        ref, dtype = oracle_padded(q, k, v, ks, ke, qs, qe, 128 ** -0.5, True), BF16
    assert _debug.last_path() == "w4"
    torch.cuda.synchronize()
    check_heads(out, ref, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq", [40, 300])
@pytest.mark.parametrize("hq,hkv,page,d,dtype", [(7, 1, 64, 128, F16), (10, 2, 128, 64, BF16)], ids=["7-1-p64", "10-2-p128"])
def test_paged_prefill(gpu, hq, hkv, page, d, dtype, sq, causal):
    """flash_attn_paged_func with Sq = 40 (280 / 200 rows per kv-head) and Sq = 300 reads the pool in place:
    test_paged_prefill.check_case (the path labels, the bits of the padded op on the gathered keys, check_padded),
    then the oracle row by row."""
    from test_paged_prefill import check_case, oracle

    args = make_paged((0, 37, 300, 449), hq, hkv, sq, page, 512, d, dtype, 8300 + hq + sq, ("phsd", "pshd")[hkv - 1])
    out = check_case(args, causal, dtype)
    q, k, v, _, _, _, sl = args
    check_heads(out, oracle(q, k, v, sl, causal), dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("hq,hkv,page,d,dtype", [(7, 1, 64, 128, F16), (10, 2, 128, 64, BF16)], ids=["7-1-p64", "10-2-p128"])
def test_ragged_paged_step(gpu, hq, hkv, page, d, dtype, causal):
    """flash_attn_paged_varlen_func on the (Sq_b, L_b) pairs of test_paged_varlen.test_other_head_dims_and_groups:
    test_paged_varlen.check_case (the bits of flash_attn_varlen_func on the gathered keys, check_padded, the path
    labels), then the oracle row by row."""
    from test_paged_varlen import Ragged, check_case

    c = Ragged(((300, 700), (0, 100), (1, 1), (257, 300), (65, 64), (40, 768)), hq, hkv, page, 768, d, dtype, 8400 + hq)
    out = check_case(c, causal)
    check_heads(packed_as_heads(out), packed_as_heads(c.oracle(causal)), dtype)


# ============================================================================================ 6. CPU cases
CPU_GEOS = ((7, 1, 1), (9, 3, 1), (33, 1, 1), (10, 2, 7), (7, 1, 9), (3, 1, 21))


def cpu_inputs(geo, fp8=False):
    """A table row on the host at D 64 (the CPU defaults compute in fp32 on fp32 copies of the 16-bit inputs)."""
    gi = index_of(*geo)
    hq, hkv, sq, lens, _ = GEOMETRY[gi]
    page, _, _, layout = case_of(gi)
    if fp8:
        kd, vd = descales(3, hkv), descales(3, hkv, 2)
        return make_fp8_paged(lens, hq, hkv, sq, page, CAPACITY, 64, F16, 8500 + gi, layout, kd, vd) + (kd, vd), lens
    return make_paged(lens, hq, hkv, sq, page, CAPACITY, 64, F16, 8500 + gi, layout), lens


@pytest.mark.parametrize("geo", CPU_GEOS, ids=[geo_id(g) for g in CPU_GEOS])
def test_cpu_defaults_paged_window_and_lse(geo):
    """flash_attn_paged_func's CPU default (``_paged_reference``), plain, windowed and with the LSE, against the
    oracles within the bar test_paged.test_paged_op_cpu_default_matches_oracle sets (3e-3 + 3e-3 |ref|); the LSE
    within test_paged_lse.test_lse_op_cpu_default_matches_float64's 1e-4."""
    from flash_attention_cute_amd import flash_attn_paged_func

    (q, k, v, kc, vc, table, sl), lens = cpu_inputs(geo)
    causal = geo[2] > 1
    f = (q.float(), kc.float(), vc.float(), table, sl)
    out, lse = quiet(flash_attn_paged_func, *f, causal=causal, return_lse=True)
    check_heads(out, paged_oracle(q, k, v, sl, causal), F16, mean=False, tol=CPU_TOL)
    want = lse_oracle(q, k, lens, 64 ** -0.5, causal)
    assert torch.equal(lse == float("-inf"), want == float("-inf"))
    torch.testing.assert_close(lse.double()[want != float("-inf")], want[want != float("-inf")], atol=1e-4, rtol=0)
    for w in (0, 31, 40):
        out = quiet(flash_attn_paged_func, *f, causal=causal, window_left=w)
        check_heads(out, win_oracle(q, k, v, sl, causal, w), F16, mean=False, tol=CPU_TOL)


@pytest.mark.parametrize("geo", CPU_GEOS, ids=[geo_id(g) for g in CPU_GEOS])
def test_cpu_defaults_fp8_and_sinks(geo):
    """The FP8 default (descales folded per (batch, kv-head), repeat_interleave(g)) at the same 3e-3 bar, and
    ``_sdpa_with_sink`` against the float64 softmax within test_paged_sink.test_sink_cpu_default_matches_float64's
    1e-5 + 1e-5 |ref| (16-bit) and, on an FP8 pool whose default returns fp16, check_padded's fp16 bar."""
    from flash_attention_cute_amd import flash_attn_paged_func

    causal = geo[2] > 1
    (q, k8, v8, kc8, vc8, table, sl, kd, vd), lens = cpu_inputs(geo, fp8=True)
    out = quiet(flash_attn_paged_func, q, kc8, vc8, table, sl, causal=causal, k_descale=kd, v_descale=vd)
    check_heads(out, fp8_oracle(q, k8, v8, sl, kd, vd, causal), F16, mean=False, tol=CPU_TOL)
    sinks = center_sinks(q, k8.float(), lens, 3, kd=kd)
    for w in (-1, 31):
        out = quiet(flash_attn_paged_func, q, kc8, vc8, table, sl, causal=causal, k_descale=kd, v_descale=vd,
                    window_left=w, sinks=sinks)
        check_heads(out, sink_oracle(q, k8.float(), v8.float(), lens, sinks, causal, w, kd=kd, vd=vd), F16)
    (q, k, v, kc, vc, table, sl), lens = cpu_inputs(geo)
    sinks = center_sinks(q, k, lens, 4)
    for w in (-1, 40):
        out = quiet(flash_attn_paged_func, q.float(), kc.float(), vc.float(), table, sl, causal=causal, window_left=w,
                    sinks=sinks)
        ref = sink_oracle(q, k, v, lens, sinks, causal, w)
        check_heads(out, ref, F16, mean=False, tol=(1e-5, 1e-5, None))
        with pytest.raises(AssertionError):  # (a sink from the neighbouring head misses even the 16-bit bar)
            check_heads(sink_oracle(q, k, v, lens, sinks.roll(1), causal, w), ref, F16)


@pytest.mark.parametrize("hq,hkv,b,page,d,dtype,layout", SHARED,
                         ids=[f"{c[0]}-{c[1]}-b{c[2]}" for c in SHARED])
def test_cpu_default_shared_prefix(hq, hkv, b, page, d, dtype, layout):
    """The host arithmetic of flash_attn_paged_shared_prefix_func (the group list, the as_strided views of q, the
    outputs and the LSE, each group's first table row) at c = 4, 10, 6, 1 through the CPU defaults, with the
    entries it must not read poisoned: 3e-3 against the oracle as test_shared_prefix's CPU test, 1e-4 on the LSE."""
    from flash_attention_cute_amd import flash_attn_paged_shared_prefix_func as shared

    prefix = 2 * page
    q, k, v, kc, vc, table, sl, c = make_shared(b, hq, hkv, page, prefix, SHARED_SUFFIXES, 64, F16, 8600 + hq, layout)
    bad = poisoned_prefix_entries(table, sl, c, prefix // page, page)
    out, lse = quiet(shared, q.float(), kc.float(), vc.float(), bad, sl, prefix, return_lse=True)
    check_heads(out, paged_oracle(q, k, v, sl, False), F16, mean=False, tol=CPU_TOL)
    torch.testing.assert_close(lse.double(), lse_oracle(q, k, sl.tolist(), 64 ** -0.5, False), atol=1e-4, rtol=0)


# --------------------------------------------------------------------------------------------- the C-ABI (ctypes)
@pytest.fixture(scope="module")
def lib():
    from test_paged_abi import LIB

    assert LIB.exists(), "libfa_gfx950.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    i64, ptr, i32 = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    for stem in ("fa_fwd_gfx950_paged", "fa_fwd_gfx950_paged_fp8"):
        getattr(lib, stem + "_workspace_size").argtypes = [ptr, i32, i32]
        getattr(lib, stem + "_workspace_size").restype = i64
    for stem in ("fa_fwd_gfx950_paged_window", "fa_fwd_gfx950_paged_window_fp8", "fa_fwd_gfx950_paged_lse",
                 "fa_fwd_gfx950_paged_lse_fp8", "fa_fwd_gfx950_paged_sink", "fa_fwd_gfx950_paged_sink_fp8"):
        getattr(lib, stem + "_check").argtypes = [ptr, i32, i32, i64]
        getattr(lib, stem + "_workspace_size").argtypes = [ptr, i32, i32, i64]
        getattr(lib, stem + "_workspace_size").restype = i64
    return lib


def abi_descriptions(hq, hkv, sq, d=128, b=3, max_pages=8, page_size=32):
    """(entry stem, params, takes a window) of one geometry as the torch binding describes it: the plain entries
    with the Sq == 1 q-head pack, the LSE and sink entries without it."""
    from test_fp8_abi import fp8_params
    from test_lse_abi import lse_params
    from test_paged_abi import paged_params
    from test_sink_abi import sink_params

    kw = dict(b=b, hq=hq, hkv=hkv, sq=sq, d=d, max_pages=max_pages, page_size=page_size)
    pack = sq == 1
    return [("fa_fwd_gfx950_paged", paged_params(pack=pack, **kw), False),
            ("fa_fwd_gfx950_paged_fp8", fp8_params(pack=pack, **kw), False),
            ("fa_fwd_gfx950_paged_window", paged_params(pack=pack, **kw), True),
            ("fa_fwd_gfx950_paged_window_fp8", fp8_params(pack=pack, **kw), True),
            ("fa_fwd_gfx950_paged_lse", lse_params(False, **kw), True),
            ("fa_fwd_gfx950_paged_lse_fp8", lse_params(True, **kw), True),
            ("fa_fwd_gfx950_paged_sink", sink_params(False, **kw), True),
            ("fa_fwd_gfx950_paged_sink_fp8", sink_params(True, **kw), True)]


def abi_call(lib, stem, p, suffix, causal, window):
    fn = getattr(lib, stem + suffix)
    return fn(ctypes.byref(p), 1, causal, -1) if window else fn(ctypes.byref(p), 1, causal)


@pytest.mark.parametrize("gi", range(len(GEOMETRY)), ids=GEO_IDS)
def test_abi_checks_and_workspace_sizes_accept_every_geometry(lib, gi):
    from test_abi import FA_OK, check, decode_params

    hq, hkv, sq, _, _ = GEOMETRY[gi]
    causal = int(sq > 1)
    for stem, p, window in abi_descriptions(hq, hkv, sq):
        assert abi_call(lib, stem, p, "_check", causal, window) == FA_OK, (stem, lib.fa_last_error())
        assert abi_call(lib, stem, p, "_workspace_size", causal, window) >= 0, (stem, lib.fa_last_error())
    assert check(lib, decode_params(b=3, hq=hq, hkv=hkv, sk=CAPACITY, sq=sq, pack=sq == 1), dtype=1, causal=causal)[0] == FA_OK
    # the appends of a step with this geometry: Sq new tokens per sequence, q rotated
    from test_fp8_abi import kv_fp8_params
    from test_kvcache_abi import kv_params

    kw = dict(b=3, hq=hq, hkv=hkv, sn=sq, sq=sq, max_pages=8, page_size=32)
    assert lib.fa_kvcache_append_gfx950_check(ctypes.byref(kv_params(**kw)), 1) == FA_OK, lib.fa_last_error()
    assert lib.fa_kvcache_append_fp8_gfx950_check(ctypes.byref(kv_fp8_params(**kw)), 1) == FA_OK, lib.fa_last_error()


def test_abi_reports_the_decode_rule_for_70_rows(lib):
    """The paged decode entries serve g * Sq <= 64 only: FA_ERR_UNSUPPORTED naming the rule, workspace size -1; the
    dense entry takes the shape (its prefill kernel)."""
    from test_abi import FA_ERR_UNSUPPORTED, FA_OK, check, decode_params

    hq, hkv, sq = PAST_LIMIT
    for stem, p, window in abi_descriptions(hq, hkv, sq):
        assert abi_call(lib, stem, p, "_check", 1, window) == FA_ERR_UNSUPPORTED, stem
        err = lib.fa_last_error().decode()
        assert "head_q_per_group * seqlen_q" in err, (stem, err)
        assert abi_call(lib, stem, p, "_workspace_size", 1, window) == -1, stem
    assert check(lib, decode_params(b=3, hq=hq, hkv=hkv, sk=CAPACITY, sq=sq, pack=False), dtype=1, causal=1)[0] == FA_OK


@pytest.mark.parametrize("geo", [(7, 1, 9), (10, 2, 7), (33, 1, 1)], ids=["7-1-9", "10-2-7", "33-1-1"])
def test_abi_workspace_holds_the_plans_slots(lib, geo):
    """decode_ws_bytes is at least what the plan's units x n_split x 32 partial rows need (an fp32 row of the head-dim
    tile and one fp32 each; test_fp8_abi.fp8_plan_workspace restates decode_plan): units counts the row BLOCKS,
    ceil(rows / 32) per (batch, kv-head), with 63, 35 and 33 rows."""
    from test_fp8_abi import fp8_plan_workspace

    hq, hkv, sq = geo
    rows = rows_of(*geo)
    for d in (64, 128):
        for stem, p, window in abi_descriptions(hq, hkv, sq, d=d, b=2, max_pages=SPLIT_CAPACITY // 64, page_size=64):
            target = 256 if "fp8" in stem else 160
            need = fp8_plan_workspace(2, hkv, rows, SPLIT_CAPACITY, d, target=target)
            assert need == 2 * hkv * 2 * 4 * 32 * ((64 if d <= 64 else 128) * 4 + 4)  # 2 blocks per unit, 4 splits
            got = abi_call(lib, stem, p, "_workspace_size", int(sq > 1), window)
            assert got >= need, (stem, d, got, need)


def test_abi_fp8_rejects_head_dim_72(lib):
    from test_abi import FA_ERR_INVALID_ARGUMENT

    for stem, p, window in abi_descriptions(7, 1, 9, d=72):
        if "fp8" in stem:
            assert abi_call(lib, stem, p, "_check", 1, window) == FA_ERR_INVALID_ARGUMENT
            assert b"multiple of 16" in lib.fa_last_error()
