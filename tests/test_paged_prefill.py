"""Paged prefill -- prefill-sized query blocks read the paged KV cache in place.

``flash_attn_paged_func`` / ``flash_attn_with_kvcache`` with ``Hq / Hkv * Sq > 64`` on a 16-bit pool whose
page size is a multiple of 64 run the paged variant of fa_fwd_w4 (C-ABI ``fa_fwd_gfx950_paged_prefill``,
include/fa_gfx950_paged_prefill.h): the same kernel body with a tile's descriptors pointed through the block
table, so the output is that of ``flash_attn_padded_func`` on the gathered dense keys BIT FOR BIT -- the
contract every GPU test here checks first, before the packed-varlen oracle (``test_padded.oracle_padded``)
within tests/test_gpu_parity.py TOL and the path labels (``last_path() == "w4"``, the kernel it is, with
``last_prefill_paged()``).

As in tests/test_paged.py every case scatters its keys through a SHUFFLED table into a pool whose unused rows
and unreferenced pages hold NaN, with -1 in every unused table entry: a row or an entry the kernel must not
read shows up as a NaN or a different bit.
"""
from __future__ import annotations

import functools

import pytest
import torch

from test_padded import check_padded, oracle_padded
from test_paged import make_paged

F16, BF16 = torch.float16, torch.bfloat16
DEV = "cuda:0"


def dv(*ts):
    return tuple(t.to(DEV) for t in ts)


def oracle(q, k, v, sl, causal, w=-1):
    return oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, q.size(-1) ** -0.5, causal, window_left=w)


@pytest.fixture
def fam(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    yield fam
    _debug.set_knobs()


def paged(q, kc, vc, table, sl, causal, w=-1):
    """One paged launch on the device: (output on the host, last_path, last_prefill_paged)."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    out = flash_attn_paged_func(*dv(q, kc, vc, table, sl), causal=causal, window_left=w)
    labels = _debug.last_path(), _debug.last_prefill_paged()
    torch.cuda.synchronize()
    return (out.cpu(), *labels)


def padded(q, k, v, sl, causal, w=-1):
    """The contract's right-hand side: the padded op on the dense keys (what the copying path computes)."""
    from flash_attention_cute_amd import _debug, flash_attn_padded_func

    out = flash_attn_padded_func(*dv(q, k, v, torch.zeros_like(sl), sl), causal=causal, window_left=w)
    assert _debug.last_path() == "w4" and not _debug.last_prefill_paged()  # (any other prefill launch resets it)
    torch.cuda.synchronize()
    return out.cpu()


def check_case(args, causal, dtype, w=-1):
    """The three checks of every case; returns the paged output."""
    q, k, v, kc, vc, table, sl = args
    out, path, in_place = paged(q, kc, vc, table, sl, causal, w)
    assert path == "w4" and in_place
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, padded(q, k, v, sl, causal, w))
    check_padded(out, oracle(q, k, v, sl, causal, w), dtype)
    return out


# 1. the base grid: B 7, Hq 8, Hkv 2, Sq 40 (160 rows per kv-head), D 128, capacity 512. Lengths: no keys, fewer
# keys than Sq, a page edge, one key past it, a tile tail, a full table. (page, dtype, layout) cycle so that every
# value meets both mask modes.
BASE_LENS = (0, 37, 64, 65, 300, 449, 512)
BASE = [(64, F16, "phsd"), (128, BF16, "pshd"), (256, F16, "pshd"), (64, BF16, "pshd"), (128, F16, "phsd"),
        (256, BF16, "phsd")]


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("page,dtype,layout", BASE, ids=[f"p{p}-{'f16' if t == F16 else 'bf16'}-{lay}" for p, t, lay in BASE])
def test_base_grid(fam, page, dtype, layout, causal):
    args = make_paged(BASE_LENS, 8, 2, 40, page, 512, 128, dtype, 900 + page, layout)
    out = check_case(args, causal, dtype)
    assert (out[0] == 0).all()  # no keys: 0 rows, no table entry read
    if causal:
        assert (out[1][:, :3] == 0).all()  # 37 keys under 40 queries: the first three rows see none


# 2. two q-tiles: Sq 300 is a full 256-row block and a partial one; lengths straddle Sq
@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("hq,d,dtype", [(2, 64, F16), (8, 96, BF16), (2, 96, F16), (8, 64, BF16)],
                         ids=["g1-d64", "g4-d96", "g1-d96", "g4-d64"])
def test_two_q_tiles(fam, hq, d, dtype, causal):
    args = make_paged((0, 100, 300, 301, 700), hq, 2, 300, 128, 768, d, dtype, 910 + hq + d)
    check_case(args, causal, dtype)


# 3. many rounds per workgroup: 6 sequences x 2 heads x 2 q-tiles = 24 blocks on 8 workgroups, so a workgroup's
# consecutive blocks belong to different sequences -- the next block's first K tile, staged under the drain, goes
# through ANOTHER table row and length. 7. two launches give the same bits.
ROUNDS_LENS = (700, 64, 301, 0, 129, 512)


@functools.lru_cache(maxsize=None)
def rounds_args():
    return make_paged(ROUNDS_LENS, 2, 2, 300, 64, 768, 128, BF16, 920)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_many_rounds_per_workgroup_and_determinism(fam, causal):
    from flash_attention_cute_amd import _debug

    args = rounds_args()
    q, k, v, kc, vc, table, sl = args
    plain = check_case(args, causal, BF16)
    with _debug.knobs(w4_grid=8):
        walked, path, in_place = paged(q, kc, vc, table, sl, causal)
        again, _, _ = paged(q, kc, vc, table, sl, causal)
    assert path == "w4" and in_place
    assert torch.equal(walked, plain) and torch.equal(again, walked)


# 4. the window. Every block starts its lookups at its own first tile: the pages wholly below the lowest key any
# row of the sequence sees, and their table entries, may hold anything.
def free_pages_below(kc, vc, table, lens, sq, w, page, bad):
    kc, vc, table = kc.clone(), vc.clone(), table.clone()
    freed = 0
    for b, n in enumerate(lens):
        first_key = max(0, n - sq - w) // 64 * 64
        for j in range(first_key // page):
            kc[int(table[b, j])], vc[int(table[b, j])] = float("nan"), float("nan")
            table[b, j] = bad
            freed += 1
    return kc, vc, table, freed


WIN_LENS = (0, 37, 300, 449, 640, 768)
WIN = [(0, 40, 64, True), (63, 300, 128, False), (64, 40, 128, True), (100, 300, 64, True), (100, 40, 64, False),
       (0, 300, 128, False), (63, 40, 64, False), (64, 300, 64, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,sq,page,causal", WIN, ids=[f"w{w}-sq{s}-p{p}-{'causal' if c else 'full'}" for w, s, p, c in WIN])
def test_window_and_freed_pages(fam, w, sq, page, causal):
    args = make_paged(WIN_LENS, 8, 2, sq, page, 768, 128, F16, 930 + w + sq + page, "pshd")
    q, k, v, kc, vc, table, sl = args
    out = check_case(args, causal, F16, w)
    freed_any = 0
    for bad in (-1, 2 ** 31 - 1):
        kc2, vc2, table2, freed = free_pages_below(kc, vc, table, WIN_LENS, sq, w, page, bad)
        freed_any += freed
        got, path, in_place = paged(q, kc2, vc2, table2, sl, causal, w)
        assert path == "w4" and in_place
        assert torch.isfinite(got.float()).all() and torch.equal(got, out)
    if sq == 40:
        assert freed_any >= 2  # (the case does free pages)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq,page", [(40, 128), (300, 64)])
def test_window_that_covers_the_capacity_is_the_unwindowed_call(fam, sq, page, causal):
    args = make_paged(WIN_LENS, 8, 2, sq, page, 768, 128, BF16, 940 + sq)
    q, k, v, kc, vc, table, sl = args
    plain = check_case(args, causal, BF16)
    for w in (768, 2 ** 40):
        out, path, in_place = paged(q, kc, vc, table, sl, causal, w)
        assert path == "w4" and in_place and torch.equal(out, plain), w


# 5. prefix sharing: two sequences reference the same physical pages for a common prompt
@pytest.mark.gpu
def test_prefix_sharing(fam):
    page, cap, d = 64, 256, 128
    q, k, v, kc, vc, table, sl = make_paged((200, 130, 64), 8, 2, 40, page, cap, d, BF16, 11)
    k[1, :, :128], v[1, :, :128] = k[0, :, :128], v[0, :, :128]  # the common prefix: two pages
    for j in range(2):
        kc[table[1, j]], vc[table[1, j]] = kc[table[0, j]], vc[table[0, j]]
    shared = table.clone()
    shared[1, :2] = table[0, :2]
    kc_s, vc_s = kc.clone(), vc.clone()
    for j in range(2):  # the second copy is no longer referenced: poison it
        kc_s[table[1, j]], vc_s[table[1, j]] = float("nan"), float("nan")
    own = check_case((q, k, v, kc, vc, table, sl), True, BF16)
    got, path, in_place = paged(q, kc_s, vc_s, shared, sl, True)
    assert path == "w4" and in_place
    assert torch.isfinite(got.float()).all() and torch.equal(got, own)


# 6. graph capture: one chunk step, replayed on new q, lengths and table contents
@pytest.mark.gpu
def test_chunk_step_graph_capture(fam):
    from flash_attention_cute_amd import _debug

    b, hq, hkv, sq, page, cap, d = 4, 8, 2, 40, 64, 512, 128
    lens = [40 + (137 * i) % (cap - 40) for i in range(b)]
    q, _, _, kc, vc, table, sl = dv(*make_paged(lens, hq, hkv, sq, page, cap, d, BF16, 17))
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)  # (the replay below re-deals every page)
    fam.flash_attn_paged_func(q, kc, vc, table, sl, causal=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fam.flash_attn_paged_func(q, kc, vc, table, sl, causal=True)
    gen = torch.Generator().manual_seed(3)
    q.copy_(torch.randn(q.shape, generator=gen).to(BF16))
    sl.copy_(torch.tensor([cap - n + 40 for n in lens], dtype=torch.int32))
    table.copy_(torch.randperm(kc.size(0), generator=gen)[:table.numel()].reshape(table.shape).to(torch.int32))
    g.replay()
    torch.cuda.synchronize()
    eager = fam.flash_attn_paged_func(q, kc, vc, table, sl, causal=True)
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.equal(out, eager)


# 8. no gather: the in-place call allocates its output (and nothing of the cache's size)
@pytest.mark.gpu
def test_no_gathered_copy_of_the_cache_is_allocated(fam):
    b, hq, hkv, sq, page, cap, d = 4, 8, 2, 40, 64, 2048, 128
    q, _, _, kc, vc, table, sl = dv(*make_paged((2048, 1000, 65, 0), hq, hkv, sq, page, cap, d, BF16, 950))
    fam.flash_attn_paged_func(q, kc, vc, table, sl, causal=True)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fam.flash_attn_paged_func(q, kc, vc, table, sl, causal=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    one_gathered_k = b * hkv * cap * d * 2
    print(f"peak rise {rise} bytes; one gathered K {one_gathered_k} bytes; output {out.numel() * 2} bytes")
    assert rise < one_gathered_k


# 9. routing: what runs in place, and what still copies (with the bits of the padded op either way)
@pytest.mark.gpu
@pytest.mark.parametrize("page,dtype", [(64, F16), (128, BF16), (256, F16), (64, BF16)])
def test_routing_in_place(fam, page, dtype):
    args = make_paged((300, 40, 512), 8, 2, 40, page, 768, 64, dtype, 960 + page)
    check_case(args, True, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("page", [32, 96])
def test_routing_other_page_sizes_keep_the_copying_path(fam, page):
    q, k, v, kc, vc, table, sl = make_paged((300, 40, 480), 8, 2, 40, page, 480, 64, F16, 970 + page)
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)  # (the gather reads whole pages; clamped unused entries too)
    out, path, in_place = paged(q, kc, vc, table, sl, True)
    assert path == "w4" and not in_place
    assert torch.equal(out, padded(q, k, v, sl, True))


@pytest.mark.gpu
def test_routing_padded_head_dim_keeps_the_copying_path(fam):
    q, k, v, kc, vc, table, sl = make_paged((300, 40, 512), 8, 2, 40, 64, 512, 68, F16, 975)
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)
    out, path, in_place = paged(q, kc, vc, table, sl, True)
    assert path == "w4" and not in_place
    assert torch.equal(out, padded(q, k, v, sl, True))


@pytest.mark.gpu
def test_routing_fp8_pool_keeps_the_copying_path(fam):
    from flash_attention_cute_amd import _debug, flash_attn_padded_func, flash_attn_paged_func

    fp8 = torch.float8_e4m3fn
    q, k, v, kc, vc, table, sl = make_paged((300, 40, 512), 8, 2, 40, 64, 512, 128, BF16, 980)
    k8, v8 = k.clamp(-448, 448).to(fp8), v.clamp(-448, 448).to(fp8)
    kc8, vc8 = kc.nan_to_num(0.0).clamp(-448, 448).to(fp8), vc.nan_to_num(0.0).clamp(-448, 448).to(fp8)
    out = flash_attn_paged_func(*dv(q, kc8, vc8, table, sl), causal=True)
    assert _debug.last_path() == "w4" and not _debug.last_prefill_paged()
    ref = flash_attn_padded_func(*dv(q, k8.to(BF16), v8.to(BF16), torch.zeros_like(sl), sl), causal=True)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


# 10. flash_attn_with_kvcache: a chunk append followed by attention over the cache it just extended
@pytest.mark.gpu
def test_with_kvcache_chunk_step_runs_in_place(fam):
    from flash_attention_cute_amd import _debug
    from test_kvcache import make_cache, new_tokens, rope_tables

    lens, hq, hkv, sn, page, cap, d = (70, 0, 33, 200), 8, 2, 40, 64, 256, 128
    kc, vc, table, sl = dv(*make_cache(lens, sn, hkv, page, cap, d, BF16, 21))
    kn, vn, q = dv(new_tokens(4, hkv, sn, d, BF16, 1), new_tokens(4, hkv, sn, d, BF16, 2),
                   new_tokens(4, hq, sn, d, BF16, 3))
    cos, sin = dv(*rope_tables(cap, d, BF16))
    kc2, vc2 = kc.clone(), vc.clone()
    out, new = fam.flash_attn_with_kvcache(q, kc, vc, kn, vn, cos, sin, cache_seqlens=sl, block_table=table,
                                           causal=True, return_seqlens=True)
    assert _debug.last_path() == "w4" and _debug.last_prefill_paged()
    new2, q_rot = torch.ops.flash_attention.kvcache_append(kc2, vc2, kn, vn, sl, table, q, cos, sin)
    ref = fam.flash_attn_paged_func(q_rot, kc2, vc2, table, new2, causal=True)
    torch.cuda.synchronize()
    assert new.tolist() == [n + sn for n in lens] and torch.equal(new, new2)
    assert torch.equal(kc.view(torch.int16), kc2.view(torch.int16))
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)
