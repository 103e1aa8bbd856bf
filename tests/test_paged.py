"""Paged KV-cache decode -- block-table attention on the split-KV decode kernel.

No reference counterpart (the reference has no KV cache). ``flash_attn_paged_func`` (C-ABI
``fa_fwd_gfx950_paged``, include/fa_gfx950_paged.h) reads a pool of fixed-size pages
[num_pages, Hkv, page_size, D] in place through a per-sequence block table, the layout of vLLM-style
engines and flash-attn's ``flash_attn_with_kvcache(..., block_table=...)``.

Semantics pinned here: sequence b is the dense operator on its ``cache_seqlens[b]`` keys, gathered
through its table row, with the queries its last Sq positions (bottom-right causal per sequence, rows
that see no key 0). Two yardsticks: the padded decode on the gathered dense cache, which the paged
launch must equal BIT FOR BIT (same split plan, same arithmetic in the same order), and the packed-varlen
oracle on the gathered rows (``tests/test_padded.py::oracle_padded``) within tests/test_gpu_parity.py TOL
(fp16 2e-3 + 2e-3|ref|, bf16 1.6e-2 + 1.6e-2|ref|), so the feature does not rest on the padded path
alone.

Every GPU case scatters a dense random K / V into the pool through a SHUFFLED, non-monotonic table,
poisons every unused pool row with NaN (the tail of each last page, all unreferenced pages) and sets
every unused table entry to -1: a row or an entry the kernel must not read shows up as a NaN or a
different bit.
"""
from __future__ import annotations

import functools
import warnings

import pytest
import torch

from test_padded import check_padded, oracle_padded

F16, BF16 = torch.float16, torch.bfloat16


def make_paged(lens, hq, hkv, sq, page_size, cap, d, dtype, seed, layout="phsd", unused=-1, spare_pages=3):
    """q [B, Hq, Sq, D], a dense K / V [B, Hkv, cap, D], and the same keys scattered into a NaN-poisoned
    pool through a shuffled table. layout "phsd": pool [P, Hkv, page, D] contiguous; "pshd": flash-attn's
    [P, page, Hkv, D], passed as its transposed view."""
    g = torch.Generator().manual_seed(seed)
    b, max_pages = len(lens), cap // page_size
    q = torch.randn(b, hq, sq, d, generator=g).to(dtype)
    k = torch.randn(b, hkv, cap, d, generator=g).to(dtype)
    v = torch.randn(b, hkv, cap, d, generator=g).to(dtype)
    num_pages = b * max_pages + spare_pages
    ids = torch.randperm(num_pages, generator=g).tolist()  # shuffled: neither sorted nor per-sequence runs
    table = torch.full((b, max_pages), unused, dtype=torch.int32)

    def pool():
        if layout == "pshd":
            return torch.full((num_pages, page_size, hkv, d), float("nan"), dtype=dtype).transpose(1, 2)
        return torch.full((num_pages, hkv, page_size, d), float("nan"), dtype=dtype)

    kc, vc = pool(), pool()
    for i, n in enumerate(lens):
        for j in range((n + page_size - 1) // page_size):
            page, n0 = ids.pop(), j * page_size
            rows = min(n, n0 + page_size) - n0
            table[i, j] = page
            kc[page, :, :rows] = k[i, :, n0:n0 + rows]
            vc[page, :, :rows] = v[i, :, n0:n0 + rows]
    return q, k, v, kc, vc, table, torch.tensor(lens, dtype=torch.int32)


# ------------------------------------------------------------------------------------------- CPU
def test_paged_op_registration():
    import flash_attention_cute_amd  # noqa: F401

    sch = str(torch.ops.flash_attention.paged_forward.default._schema)
    assert sch == ("flash_attention::paged_forward(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, "
                   "Tensor cache_seqlens, float softmax_scale=None, bool causal=False) -> Tensor")
    q, _, _, kc, vc, table, lens = make_paged((40, 7), 4, 2, 2, 32, 64, 32, torch.float32, 1)
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.library.opcheck(torch.ops.flash_attention.paged_forward.default,
                              (q, kc, vc, table, lens, 0.125, True), test_utils=("test_schema", "test_faketensor"))


def test_paged_func_is_exported_like_the_other_extras():
    import flash_attention
    import flash_attention.flash_attention as ref_mod
    import flash_attention_cute_amd as m

    assert m.flash_attn_paged_func is flash_attention.flash_attn_paged_func is ref_mod.flash_attn_paged_func
    assert "flash_attn_paged_func" in m.__all__ and "flash_attention_paged_forward" in m.__all__


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq", [1, 3])
@pytest.mark.parametrize("layout", ["phsd", "pshd"])
def test_paged_op_cpu_default_matches_oracle(causal, sq, layout):
    """The CPU default gathers each sequence's pages and runs SDPA with the kernel's semantics; the NaN
    poison in every unused pool row and the -1 in every unused table entry must not reach it."""
    from flash_attention_cute_amd import flash_attn_paged_func

    lens, hq, hkv, page, cap, d = (96, 0, 33, 1, 64), 4, 2, 32, 96, 64
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, F16, 3, layout)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = flash_attn_paged_func(q.float(), kc.float(), vc.float(), table, sl, causal=causal)
    assert torch.isfinite(out).all()
    ref = oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, causal).float()
    torch.testing.assert_close(out, ref, atol=3e-3, rtol=3e-3)
    assert (out[1] == 0).all()  # a sequence without keys


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def ops(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam
    from flash_attention_cute_amd import flash_attn_padded_func, flash_attn_paged_func

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    _debug.set_dec_fuse(None)
    yield flash_attn_paged_func, flash_attn_padded_func, _debug
    _debug.set_dec_fuse(None)


# kind -> (B, Hq, Hkv, Sq, capacity, causal). "split": decode_plan gives 4 splits (64 tiles, 4 units).
KINDS = {
    "unsplit": (3, 8, 2, 1, 256, False),
    "split": (2, 8, 2, 1, 2048, False),
    "split_unfused": (2, 8, 2, 1, 2048, False),  # _debug.set_dec_fuse(0): the separate combine launch
    "sq3_causal": (3, 8, 2, 3, 256, True),       # unpacked GQA, g = 4, 12 rows
    "g8_sq5": (3, 16, 2, 5, 256, True),          # 40 rows: two row blocks
}
# (kind, page_size, D, dtype, pool layout, lengths). Over the list: every page size with every kind, D 64 /
# 128 / 72 (a D tile not filled), both dtypes, both stride orders, and lengths 0, 1, 31, 32, 33, exactly
# one page, one key past a page and full capacity for every page size.
CASES = [
    ("unsplit", 32, 128, F16, "phsd", (0, 1, 31)),
    ("unsplit", 32, 64, BF16, "pshd", (32, 33, 256)),
    ("unsplit", 64, 72, F16, "pshd", (64, 65, 33)),
    ("unsplit", 64, 128, BF16, "phsd", (31, 256, 0)),
    ("unsplit", 256, 64, F16, "phsd", (256, 1, 32)),
    ("unsplit", 256, 72, BF16, "pshd", (33, 0, 255)),
    ("split", 32, 128, BF16, "phsd", (2048, 33)),
    ("split", 64, 64, F16, "pshd", (65, 2047)),
    ("split", 256, 128, F16, "pshd", (257, 2048)),
    ("split", 256, 72, BF16, "phsd", (256, 0)),
    ("split_unfused", 32, 72, F16, "phsd", (32, 1999)),
    ("split_unfused", 64, 128, BF16, "pshd", (2048, 1)),
    ("split_unfused", 256, 64, F16, "phsd", (257, 31)),
    ("sq3_causal", 32, 128, F16, "pshd", (0, 1, 33)),
    ("sq3_causal", 64, 72, BF16, "phsd", (64, 65, 256)),
    ("sq3_causal", 256, 64, BF16, "pshd", (2, 256, 32)),
    ("g8_sq5", 32, 64, F16, "phsd", (31, 32, 256)),
    ("g8_sq5", 64, 128, BF16, "pshd", (5, 65, 0)),
    ("g8_sq5", 256, 72, F16, "phsd", (256, 4, 33)),
]
CASE_IDS = [f"{k}-p{p}-d{d}-{'f16' if t == F16 else 'bf16'}-{lay}" for k, p, d, t, lay, _ in CASES]


@functools.lru_cache(maxsize=None)
def run_case(ci, unused=-1):
    """One paged launch, the padded launch on the gathered dense cache and the oracle, computed once per
    case and shared by the tests below (never modified)."""
    from flash_attention_cute_amd import _debug, flash_attn_padded_func, flash_attn_paged_func

    kind, page, d, dtype, layout, lens = CASES[ci]
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    assert len(lens) == b
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 100 + ci, layout, unused)
    dev = torch.device("cuda:0")
    dv = lambda t: t.to(dev)  # noqa: E731
    _debug.set_knobs()
    _debug.set_dec_fuse(0 if kind == "split_unfused" else None)
    try:
        out = flash_attn_paged_func(dv(q), dv(kc), dv(vc), dv(table), dv(sl), causal=causal)
        path, fused = _debug.last_path(), _debug.last_dec_fused()
        dense = flash_attn_padded_func(dv(q), dv(k), dv(v), dv(torch.zeros_like(sl)), dv(sl), causal=causal)
        dense_path = _debug.last_path()
        torch.cuda.synchronize()
    finally:
        _debug.set_dec_fuse(None)
    ref = oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, causal)
    return out.cpu(), dense.cpu(), ref, path, fused, dense_path


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_paged_equals_padded_decode_on_the_gathered_cache_bit_for_bit(ops, ci):
    kind, _, _, _, _, lens = CASES[ci]
    out, dense, _, path, fused, dense_path = run_case(ci)
    split = kind.startswith("split")
    assert path == ("decode_paged_split" if split else "decode_paged")
    assert dense_path == ("decode_split" if split else "decode")
    if split:
        assert fused == (kind == "split")
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, dense)
    for i, n in enumerate(lens):
        if n == 0:
            assert (out[i] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_paged_matches_the_oracle(ops, ci):
    out, _, ref, _, _, _ = run_case(ci)
    check_padded(out, ref, CASES[ci][3])


@pytest.mark.gpu
@pytest.mark.parametrize("ci", [1, 8, 15], ids=[CASE_IDS[i] for i in (1, 8, 15)])
def test_unused_table_entries_are_never_read(ops, ci):
    """Entries of pages past ceil(len / page_size) hold 2**31 - 1 instead of -1: the same bits."""
    assert torch.equal(run_case(ci, 2 ** 31 - 1)[0], run_case(ci)[0])


@pytest.mark.gpu
def test_bad_page_ids_are_clamped_into_the_pool(ops, device):
    """A USED entry outside [0, num_pages) addresses the pool's first / last page, never memory outside
    it (the policy of the padded entry's range clamping): the result is that of the clamped table."""
    paged, _, _ = ops
    q, _, _, kc, vc, table, sl = make_paged((64, 64), 8, 2, 1, 32, 64, 128, F16, 5, spare_pages=0)
    kc, vc = kc.nan_to_num(0.5), vc.nan_to_num(0.25)  # (every page is read here)
    bad = table.clone()
    bad[0, 1], bad[1, 0] = 2 ** 31 - 1, -7
    dv = lambda t: t.to(device)  # noqa: E731
    out = paged(dv(q), dv(kc), dv(vc), dv(bad), dv(sl))
    ref = paged(dv(q), dv(kc), dv(vc), dv(bad.clamp(0, kc.size(0) - 1)), dv(sl))
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)


@pytest.mark.gpu
def test_prefix_sharing(ops, device):
    """Two sequences whose tables reference the SAME physical pages for their first pages (a shared
    prompt): the result equals the unshared layout's."""
    paged, _, _ = ops
    page, cap, d = 64, 256, 128
    q, k, v, kc, vc, table, sl = make_paged((200, 130, 64), 8, 2, 1, page, cap, d, BF16, 11)
    k[1, :, :128], v[1, :, :128] = k[0, :, :128], v[0, :, :128]  # the common prefix: two pages
    for j in range(2):
        kc[table[1, j]], vc[table[1, j]] = kc[table[0, j]], vc[table[0, j]]
    shared = table.clone()
    shared[1, :2] = table[0, :2]
    kc_s, vc_s = kc.clone(), vc.clone()
    for j in range(2):  # the second copy is no longer referenced: poison it
        kc_s[table[1, j]], vc_s[table[1, j]] = float("nan"), float("nan")
    dv = lambda t: t.to(device)  # noqa: E731
    a = paged(dv(q), dv(kc), dv(vc), dv(table), dv(sl))
    s = paged(dv(q), dv(kc_s), dv(vc_s), dv(shared), dv(sl))
    assert torch.isfinite(s.float()).all() and torch.equal(a, s)
    check_padded(s, oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, False), BF16)


@pytest.mark.gpu
def test_pool_beyond_2_31_elements(ops, device):
    """Pages past element 2^31 of the pool (the page term of the address is 64-bit): an uninitialised
    pool of which only the last pages are written and referenced gives the bits of a small pool."""
    paged, _, _ = ops
    hkv, page, d, lens = 1, 256, 128, (1000, 257)
    first = 2 ** 31 // (hkv * page * d) + 1  # the first page that lies wholly past element 2^31
    free, _ = torch.cuda.mem_get_info(device)
    if free < 12 * 2 ** 30:
        pytest.skip("needs about 12 GiB of free device memory")
    q, _, _, kc, vc, table, sl = make_paged(lens, 8, hkv, 1, page, 1024, d, BF16, 23, spare_pages=0)
    small = paged(q.to(device), kc.to(device), vc.to(device), table.to(device), sl.to(device))
    n = kc.size(0)
    big_k = torch.empty(first + n, hkv, page, d, dtype=BF16, device=device)
    big_v = torch.empty_like(big_k)
    assert big_k.numel() > 2 ** 31
    big_k[first:], big_v[first:] = kc.to(device), vc.to(device)
    far = torch.where(table >= 0, table + first, table)
    out = paged(q.to(device), big_k, big_v, far.to(device), sl.to(device))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.equal(out, small)


@pytest.mark.gpu
def test_paged_decode_graph_capture(ops, device):
    """The paged decode step makes no host synchronisation: it captures into a HIP graph, and the
    replay follows new q, lengths and table contents."""
    paged, _, _debug = ops
    b, hq, hkv, page, cap, d = 16, 32, 8, 128, 2048, 128
    lens = [1 + (137 * i) % cap for i in range(b)]
    q, _, _, kc, vc, table, sl = (t.to(device) for t in make_paged(lens, hq, hkv, 1, page, cap, d, BF16, 17))
    kc, vc = kc.nan_to_num(0.0), vc.nan_to_num(0.0)  # (the replay below re-deals every page)
    paged(q, kc, vc, table, sl)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = paged(q, kc, vc, table, sl)
    gen = torch.Generator().manual_seed(3)
    q.copy_(torch.randn(q.shape, generator=gen).to(BF16))
    sl.copy_(torch.tensor([cap - n + 1 for n in lens], dtype=torch.int32))
    table.copy_(torch.randperm(kc.size(0), generator=gen)[:table.numel()].reshape(table.shape).to(torch.int32))
    g.replay()
    torch.cuda.synchronize()
    ref = paged(q, kc, vc, table, sl)
    assert _debug.last_path().startswith("decode_paged")
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)


@pytest.mark.gpu
def test_copying_fallback_for_larger_query_blocks(ops, device):
    """g * Sq = 160 rows is no decode shape: the op gathers the table's pages into a dense cache and runs
    the padded entry on the prefill kernel -- the bits of flash_attn_padded_func on the gathered cache."""
    paged, padded, _debug = ops
    lens, page, cap, d = (300, 40, 512), 64, 512, 128
    q, k, v, kc, vc, table, sl = (t.to(device) for t in make_paged(lens, 8, 2, 40, page, cap, d, F16, 29, "pshd"))
    out = paged(q, kc, vc, table, sl, causal=True)
    assert _debug.last_path() == "w4"
    ref = padded(q, k, v, torch.zeros_like(sl), sl, causal=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref)
    check_padded(out, oracle_padded(q.cpu(), k.cpu(), v.cpu(), torch.zeros_like(sl).cpu(), sl.cpu(), None, None,
                                    d ** -0.5, True), F16)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", [8, 12], ids=[CASE_IDS[i] for i in (8, 12)])
def test_paged_decode_is_deterministic(ops, device, ci):
    """Two launches of the same case (fused merge: whichever split arrives last merges in split order;
    separate combine) give the same bits."""
    paged, _, _debug = ops
    kind, page, d, dtype, layout, lens = CASES[ci]
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    q, _, _, kc, vc, table, sl = (t.to(device) for t in make_paged(lens, hq, hkv, sq, page, cap, d, dtype, 100 + ci,
                                                                   layout))
    _debug.set_dec_fuse(0 if kind == "split_unfused" else None)
    a = paged(q, kc, vc, table, sl, causal=causal)
    b2 = paged(q, kc, vc, table, sl, causal=causal)
    torch.cuda.synchronize()
    assert torch.equal(a, b2) and torch.equal(a.cpu(), run_case(ci)[0])
