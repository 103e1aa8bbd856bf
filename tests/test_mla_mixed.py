"""Sparse MLA decode and append on the mixed FP8 latent row of DeepSeek-V3.2 (include/fa_gfx950_mla_mixed.h): a
``torch.uint8`` cache [num_pages, page_size, 656] through ``flash_attn_mla_decode_func(indices=)``,
``flash_attn_mla_append`` and ``flash_attn_mla_with_kvcache``.

The reference is float64 on the CPU over the dequantised rows (e4m3 * scale per 128-column tile, RoPE bf16), gathered
per list as tests/test_mla_sparse.py does. The kernel's arithmetic is the bf16 sparse kernel's plus one more fp32
factor inside the bf16 rounding of P, so the bounds are that test's, unchanged. Tile j of token n is multiplied by
(0.25, 1, 2, 0.5)[j] * (0.5 + (n % 4) / 2) before quantising: another tile's or another key's scale misses the bound.
The pool is byte 0xFF (NaN as e4m3, fp32 and bf16) outside live rows, the table -1 outside live entries."""
from __future__ import annotations

import ctypes
import functools
import warnings

import pytest
import torch

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK
from test_mla_decode import BF16, LSE_TOL, SCALE, TOL, check, lib  # noqa: F401
from test_mla_fp8 import FP8, SENTINEL, norm_bytes
from test_mla_sparse import LENS, make_lists, sparse_params

FLT_MIN = torch.finfo(torch.float32).tiny


def dequant(rows):
    """float64 [..., 576] of mixed rows (uint8 [..., 656])"""
    scale = rows[..., 512:528].contiguous().view(torch.float32).double()
    nope = rows[..., :512].contiguous().view(FP8).double().unflatten(-1, (4, 128)) * scale[..., None]
    return torch.cat([nope.flatten(-2), rows[..., 528:].contiguous().view(BF16).double()], -1)


@functools.lru_cache(maxsize=None)
def make_mixed(lens, hq, sq, page, seed=0):
    """q [B, Hq, Sq, 576] bf16, the dense dequantised latent (float64 [B, cap, 576]), its mixed rows scattered into a
    0xFF pool [P, page, 656] through a shuffled table (-1 in unused entries), the table and the lengths."""
    from flash_attention_cute_amd.flash_attention import pack_mla_mixed_rows

    g = torch.Generator().manual_seed(seed)
    b, max_pages = len(lens), (max(max(lens), 1) + page - 1) // page
    q = torch.randn(b, hq, sq, 576, generator=g).to(BF16)
    kv = torch.randn(b, max_pages * page, 576, generator=g)
    kv[..., :512] *= torch.tensor([0.25, 1, 2, 0.5]).repeat_interleave(128)
    kv[..., :512] *= (0.5 + (torch.arange(max_pages * page) % 4) / 2)[:, None]
    rows = pack_mla_mixed_rows(kv[..., :512].to(BF16), kv[..., 512:].to(BF16))
    ids = torch.randperm(b * max_pages + 3, generator=g).tolist()
    pool = torch.full((b * max_pages + 3, page, 656), 0xFF, dtype=torch.uint8)
    table = torch.full((b, max_pages), -1, dtype=torch.int32)
    for i, n in enumerate(lens):
        for j in range((n + page - 1) // page):
            live = min(n - j * page, page)
            table[i, j] = ids.pop()
            pool[table[i, j], :live] = rows[i, j * page:j * page + live]
    return q, dequant(rows), pool, table, torch.tensor(lens, dtype=torch.int32)


def reference(q, deq, idx, lens, causal):
    """tests/test_mla_sparse.py's sparse_reference over the dequantised latent"""
    b, hq, sq, _ = q.shape
    out = torch.zeros(b, hq, sq, 512, dtype=torch.float64)
    lse = torch.full((b, hq, sq), float("-inf"), dtype=torch.float64)
    for i, n in enumerate(lens):
        for pos in range(sq):
            lim = min(n - 1, pos + n - sq) if causal else n - 1
            ids = idx[i, pos].long()
            k = deq[i, ids[(ids >= 0) & (ids <= lim)]]
            if len(k):
                s = q[i, :, pos].double() @ k.t() * SCALE
                lse[i, :, pos] = torch.logsumexp(s, -1)
                out[i, :, pos] = torch.exp(s - lse[i, :, pos, None]) @ k[:, :512]
    return out, lse


@functools.lru_cache(maxsize=None)
def case_reference(lens, hq, sq, page, topk, causal):
    q, deq, *_ = make_mixed(lens, hq, sq, page)
    return reference(q, deq, make_lists(lens, sq, topk), lens, causal)


# ------------------------------------------------------------------------------------------- GPU
CASES = [(16, 1, 32, 32, False), (40, 1, 32, 64, False), (128, 1, 64, 96, False), (24, 3, 32, 96, True),
         (16, 1, 96, 64, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("hq,sq,page,topk,causal", CASES, ids=[f"{c[0]}x{c[1]}-p{c[2]}-k{c[3]}" for c in CASES])
def test_mla_mixed_sparse_matches_float64(hq, sq, page, topk, causal, num_splits):
    """Half a block with one tile; a partial second block (3 splits of 2 tiles leave one empty); two head groups on
    one list; one list per position under the causal limit; a page size that is no power of two. The lists are
    tests/test_mla_sparse.py's: entries that are no key inside a live tile, a duplicate, a skipped tile."""
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    q, _, pool, table, sl = (t.cuda() for t in make_mixed(LENS, hq, sq, page))
    idx = make_lists(LENS, sq, topk).cuda()
    out, lse = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, return_lse=True,
                                          num_splits=num_splits, indices=idx)
    assert out.shape == (len(LENS), hq, sq, 512) and out.dtype == BF16
    assert lse.shape == (len(LENS), hq, sq) and lse.dtype == torch.float32
    check(out, lse, *case_reference(LENS, hq, sq, page, topk, causal), BF16,
          f"mla mixed {hq}x{sq} page {page} topk {topk} splits {num_splits}")
    assert (out[0] == 0).all() and (lse[0] == float("-inf")).all()  # a sequence without keys
    plain = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, num_splits=num_splits, indices=idx)
    assert torch.equal(plain, out)


def append_case(sn=3):
    """tests/test_mla_fp8.py's append_case on 656-byte rows: starting lengths (0, 30, 63, capacity - 2) on page 32 (a
    page edge, the capacity), one table entry outside the pool, a sentinel pool; token (0, 0) has a tile of zeros."""
    g = torch.Generator().manual_seed(sn)
    page, max_pages, num_pages = 32, 4, 19
    lens = (0, 30, 63, max_pages * page - 2)
    table = torch.randperm(num_pages, generator=g)[:16].reshape(4, max_pages).to(torch.int32)
    table[1, 1] = num_pages + 5
    pool = torch.full((num_pages, page, 656), SENTINEL, dtype=torch.uint8)
    c_kv, k_pe = torch.randn(4, sn, 512, generator=g).to(BF16), torch.randn(4, sn, 64, generator=g).to(BF16)
    c_kv[0, 0, 128:256] = 0
    return pool, c_kv, k_pe, torch.tensor(lens, dtype=torch.int32), table


def append_loop(pool, c_kv, k_pe, lens, table):
    """The append by a plain loop with the drop rules: (expected pool, new lengths)."""
    from flash_attention_cute_amd.flash_attention import pack_mla_mixed_rows

    exp, (num_pages, page, _), cap = pool.clone(), pool.shape, table.size(1) * pool.size(1)
    rows = pack_mla_mixed_rows(c_kv, k_pe)
    for b, n0 in enumerate(lens):
        for i in range(rows.size(1)):
            n = n0 + i
            pid = int(table[b, n // page]) if n < cap else -1
            if 0 <= pid < num_pages:
                exp[pid, n % page] = rows[b, i]
    return exp, [min(n + rows.size(1), cap) for n in lens]


def same_rows(a, b):
    """byte equality of mixed pools, the e4m3 part as tests/test_mla_fp8.py's norm_bytes compares it"""
    a, b = a.cpu(), b.cpu()
    return torch.equal(norm_bytes(a[..., :512].view(FP8)), norm_bytes(b[..., :512].view(FP8))) and \
        torch.equal(a[..., 512:], b[..., 512:])


@pytest.mark.gpu
def test_mla_mixed_append_writes_exactly_the_loops_bytes():
    from flash_attention_cute_amd import flash_attn_mla_append

    pool, c_kv, k_pe, sl, table = append_case()
    exp, exp_lens = append_loop(pool, c_kv, k_pe, sl.tolist(), table)
    assert (exp[table[1, 0], 30:] != SENTINEL).any() and (exp[:, 0] == SENTINEL).all(-1).sum() > 0  # (the case bites)
    pool_g = pool.cuda()
    new = flash_attn_mla_append(pool_g.unsqueeze(2), c_kv.cuda(), k_pe.cuda(), sl.cuda(), table.cuda())
    assert same_rows(pool_g, exp)  # the whole pool: dropped tokens (page outside the pool, past capacity) wrote nothing
    assert new.tolist() == exp_lens and new.dtype == torch.int32
    row = pool_g[table[0, 0], 0].cpu()  # the tile of zeros
    assert row[516:520].view(torch.float32).item() == FLT_MIN and (row[128:256] == 0).all()


@pytest.mark.gpu
def test_mla_mixed_with_kvcache_step_matches_float64():
    """One step from an empty 0xFF cache: 40 tokens a sequence (a page edge), then the sparse decode over them."""
    from flash_attention_cute_amd import flash_attn_mla_with_kvcache

    g = torch.Generator().manual_seed(5)
    lens, hq, topk = (40, 40), 16, 64
    q = torch.randn(2, hq, 1, 576, generator=g).to(BF16)
    c_kv, k_pe = (torch.randn(2, 40, n, generator=g).to(BF16) for n in (512, 64))
    pool = torch.full((5, 32, 656), 0xFF, dtype=torch.uint8, device="cuda")
    table, idx = torch.tensor([[3, 0], [1, 4]], dtype=torch.int32), make_lists(lens, 1, topk)
    out, lse, new = flash_attn_mla_with_kvcache(q.cuda(), pool, c_kv.cuda(), k_pe.cuda(),
                                                torch.zeros(2, dtype=torch.int32).cuda(), table.cuda(), SCALE,
                                                return_lse=True, return_seqlens=True, indices=idx.cuda())
    exp, _ = append_loop(torch.zeros(5, 32, 656, dtype=torch.uint8), c_kv, k_pe, [0, 0], table)
    deq = dequant(exp[table.long()].flatten(1, 2))  # [B, cap, 576]
    assert new.tolist() == list(lens)
    check(out, lse, *reference(q, deq, idx, lens, True), BF16, "mla mixed with_kvcache")


# ------------------------------------------------------------------------------------------- CPU
def test_mla_mixed_op_schemas_fakes_and_opcheck():
    import flash_attention_cute_amd as m
    from flash_attention_cute_amd.flash_attention import pack_mla_mixed_rows

    ops = torch.ops.flash_attention
    for name in ("flash_attention_mla_sparse_decode_forward_mixed", "flash_attention_mla_append_mixed"):
        assert name in m.__all__ and callable(getattr(m, name))
    assert str(ops.mla_sparse_decode_forward_mixed.default._schema) == (
        "flash_attention::mla_sparse_decode_forward_mixed(Tensor q, Tensor kv_cache, Tensor block_table, "
        "Tensor cache_seqlens, Tensor indices, float softmax_scale, bool causal=True, SymInt num_splits=0) "
        "-> (Tensor, Tensor)")
    assert str(ops.mla_append_mixed.default._schema) == (
        "flash_attention::mla_append_mixed(Tensor(a0!) kv_cache, Tensor c_kv, Tensor k_pe, Tensor cache_seqlens, "
        "Tensor block_table) -> Tensor")
    q, _, pool, table, sl = make_mixed((40, 7), 4, 2, 32)
    idx = make_lists((40, 7), 2, 32)
    with torch._subclasses.FakeTensorMode() as mode:
        o, lse = ops.mla_sparse_decode_forward_mixed(*(mode.from_tensor(t) for t in (q, pool, table, sl, idx)), SCALE)
    assert o.shape == (2, 4, 2, 512) and o.dtype == BF16 and lse.shape == (2, 4, 2) and lse.dtype == torch.float32
    c_kv, k_pe = torch.randn(2, 3, 512).to(BF16), torch.randn(2, 3, 64).to(BF16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        both = ("test_schema", "test_faketensor")
        torch.library.opcheck(ops.mla_sparse_decode_forward_mixed.default, (q, pool, table, sl, idx, SCALE, True),
                              test_utils=both)
        torch.library.opcheck(ops.mla_append_mixed.default, (pool.clone(), c_kv, k_pe, sl, table), test_utils=both)
    # the write formula: vLLM's scale, and a row within half an e4m3 step (2^-4 of the tile's scale * 448 at most)
    rows = pack_mla_mixed_rows(c_kv, k_pe)
    amax = c_kv.float().unflatten(-1, (4, 128)).abs().amax(-1)
    assert torch.equal(rows[..., 512:528].contiguous().view(torch.float32), amax / 448)
    err = (dequant(rows) - torch.cat([c_kv, k_pe], -1).double()).unflatten(-1, (9, 64)).abs().amax(-1)
    assert (err[..., :8] <= amax.double().repeat_interleave(2, -1) * 2.0 ** -4).all() and (err[..., 8] == 0).all()


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_mla_mixed_cpu_default_matches_float64(causal):
    lens, hq, sq, topk = (100, 0, 33, 1), 4, 3, 96
    q, deq, pool, table, sl = make_mixed(lens, hq, sq, 32)
    idx = make_lists(lens, sq, topk)
    with pytest.warns(UserWarning, match="fallback to pytorch"):
        out, lse = torch.ops.flash_attention.mla_sparse_decode_forward_mixed(q.float(), pool, table, sl, idx, SCALE,
                                                                             causal)
    ref, ref_lse = reference(q, deq, idx, lens, causal)
    assert torch.isfinite(out).all()  # (the 0xFF pool: nothing invisible was read)
    torch.testing.assert_close(out.double(), ref, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(lse.double(), ref_lse, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(q=torch.zeros(1, 4, 1, 576, dtype=torch.float16)), ValueError), (dict(kv_descale=1.0), ValueError),
    (dict(kv_cache=torch.zeros(2, 32, 656, dtype=torch.int8)), ValueError),
    (dict(kv_cache=torch.zeros(2, 32, 640, dtype=torch.uint8)), ValueError), (dict(indices=None), NotImplementedError)],
    ids=["f16-q", "kv_descale", "int8-656", "width-640", "dense"])
def test_mla_mixed_wrapper_errors(kwargs, exc):
    from flash_attention_cute_amd import flash_attn_mla_append, flash_attn_mla_decode_func

    args = dict(q=torch.zeros(1, 4, 1, 576, dtype=BF16), kv_cache=torch.zeros(2, 32, 656, dtype=torch.uint8),
                block_table=torch.zeros(1, 2, dtype=torch.int32), cache_seqlens=torch.ones(1, dtype=torch.int32),
                softmax_scale=SCALE, indices=torch.zeros(1, 1, 32, dtype=torch.int32))
    args.update(kwargs)
    with pytest.raises(exc):
        flash_attn_mla_decode_func(**args)
    if exc is ValueError:  # the append's: c_kv / k_pe of q's dtype
        with pytest.raises(ValueError):
            flash_attn_mla_append(args["kv_cache"], torch.zeros(1, 1, 512, dtype=args["q"].dtype),
                                  torch.zeros(1, 1, 64, dtype=args["q"].dtype), args["cache_seqlens"],
                                  args["block_table"], args.get("kv_descale"))


class FaMlaAppendParams(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in ("kv_ptr", "c_kv", "k_pe", "block_table", "seqlens_k", "seqlens_out",
                                                 "kv_descale")] +
                [(n, ctypes.c_int64) for n in (
                    "kv_descale_stride", "batch_size", "seqlen_new", "ckv_batch_stride", "ckv_seqlen_stride",
                    "kpe_batch_stride", "kpe_seqlen_stride", "kv_page_stride", "kv_row_stride", "num_pages",
                    "page_size", "max_pages", "block_table_stride")] + [("cache_dtype", ctypes.c_int32)])


@pytest.mark.parametrize("kw,code", [({}, FA_OK), (dict(indices=None), FA_ERR_INVALID_ARGUMENT),
                                     (dict(topk=48), FA_ERR_INVALID_ARGUMENT),
                                     (dict(kv_row_stride=664), FA_ERR_INVALID_ARGUMENT),
                                     (dict(page_size=48), FA_ERR_INVALID_ARGUMENT)],
                         ids=["ok", "indices-null", "topk-48", "row-stride-664", "page-48"])
def test_mla_mixed_check_codes_and_workspace(lib, kw, code):  # noqa: F811
    """Host-only: the checks read no device memory, the launch entries return the same code before any launch, and
    the plan (so the workspace) is the 16-bit sparse entry's."""
    lib.fa_mla_sparse_mixed_decode_gfx950_ws_bytes.restype = lib.fa_mla_sparse_decode_gfx950_ws_bytes.restype = \
        ctypes.c_int64
    p = sparse_params(**{"kv_row_stride": 656, "kv_page_stride": 32 * 656, **kw})
    assert lib.fa_mla_sparse_mixed_decode_gfx950_check(ctypes.byref(p), 1) == code
    a = FaMlaAppendParams(0x200000, 0x100000, 0x300000, 0x500000, 0x600000, 0, 0, 0, 2, 3, 3 * 512, 512, 3 * 64, 64,
                          p.base.kv_page_stride, p.base.kv_row_stride, 8, p.base.page_size, 4, 4, 9)
    append_code = code if "kv_row_stride" in kw else FA_OK  # (the list and the tile are the decode's)
    assert lib.fa_mla_append_mixed_gfx950_check(ctypes.byref(a), 1) == append_code
    if code != FA_OK:
        assert lib.fa_mla_sparse_mixed_decode_gfx950(ctypes.byref(p), 1, None, 0, None) == code
        assert lib.fa_mla_sparse_mixed_decode_gfx950_ws_bytes(ctypes.byref(p)) == -1
        assert append_code == FA_OK or lib.fa_mla_append_mixed_gfx950(ctypes.byref(a), 1, None) == code
        return
    assert lib.fa_mla_mixed_version() == 1
    assert lib.fa_mla_sparse_mixed_decode_gfx950_check(ctypes.byref(p), 0) == FA_ERR_UNSUPPORTED  # fp16 q
    assert lib.fa_mla_append_mixed_gfx950_check(ctypes.byref(a), 0) == FA_ERR_UNSUPPORTED
    for shape in (dict(), dict(b=2, hq=24, sq=3, num_splits=3), dict(b=32, hq=128), dict(num_splits=1)):
        m, s = sparse_params(kv_row_stride=656, kv_page_stride=32 * 656, **shape), sparse_params(**shape)
        assert lib.fa_mla_sparse_mixed_decode_gfx950_ws_bytes(ctypes.byref(m)) == \
            lib.fa_mla_sparse_decode_gfx950_ws_bytes(ctypes.byref(s)) >= 0
