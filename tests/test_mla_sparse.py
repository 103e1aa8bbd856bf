"""Sparse MLA decode over top-k token indices of the paged latent cache (``flash_attn_mla_decode_func(indices=)``,
include/fa_gfx950_mla_sparse.h).

The reference is float64 on the CPU over the same 16-bit inputs: per (b, pos) the entries with 0 <= idx <= lim are
gathered from the dense latent (a duplicate is a repeated row), softmax(SCALE q k^T) k[:, :512] and the logsumexp.
Bounds are tests/test_mla_decode.py's (the arithmetic is that kernel's). The pool is NaN outside live rows and the
table -1 outside live entries, so any read for an entry that is not a key shows as a non-finite output."""
from __future__ import annotations

import ctypes
import functools
import warnings

import pytest
import torch

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_OK
from test_mla_decode import (BF16, F16, LENS32, LIB, LSE_TOL, SCALE, TOL, FaMlaParams, check, make_latent,  # noqa: F401
                             mla_params, reference as dense_reference)

LENS = (0, 1, 31, 33, 64, 100, 417)
INT_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def make_lists(lens, sq, topk, seed=0):
    """int32 [B, Sq, topk]: per list a shuffled sample of [0, len) without replacement, laid into every tile but
    one (all -1: a skipped tile with live tiles behind it, when there are two tiles or more); then -1, len and
    2^31 - 1 planted inside the first live tile and one duplicate; -1 padding to topk."""
    g = torch.Generator().manual_seed(seed)
    nt = topk // 32
    slots = torch.tensor([i for i in range(topk) if nt < 2 or i // 32 != nt - 2])
    idx = torch.full((len(lens), sq, topk), -1, dtype=torch.int32)
    for b, n in enumerate(lens):
        for pos in range(sq):
            k = min(n, len(slots) - 4)
            row = idx[b, pos]
            row[slots[:k]] = torch.randperm(n, generator=g)[:k].to(torch.int32)
            row[slots[1]], row[slots[2]], row[slots[3]] = -1, n, INT_MAX
            row[slots[5]] = row[slots[4]]
    return idx


@functools.lru_cache(maxsize=None)
def sparse_reference(lens, hq, sq, page, dtype, topk, causal, seed=0):
    q, kv, *_ = make_latent(lens, hq, sq, page, dtype, seed)
    idx = make_lists(lens, sq, topk, seed)
    out = torch.zeros(len(lens), hq, sq, 512, dtype=torch.float64)
    lse = torch.full((len(lens), hq, sq), float("-inf"), dtype=torch.float64)
    for b, n in enumerate(lens):
        for pos in range(sq):
            lim = min(n - 1, pos + n - sq) if causal else n - 1
            ids = idx[b, pos].long()
            k = kv[b, ids[(ids >= 0) & (ids <= lim)]].double()
            if len(k):
                s = q[b, :, pos].double() @ k.t() * SCALE
                lse[b, :, pos] = torch.logsumexp(s, -1)
                out[b, :, pos] = torch.exp(s - lse[b, :, pos, None]) @ k[:, :512]
    return out, lse


# ------------------------------------------------------------------------------------------- GPU
CASES = [(BF16, 16, 1, 32, 32, False), (F16, 40, 1, 32, 64, False), (BF16, 128, 1, 64, 96, False),
         (F16, 24, 3, 32, 96, True), (BF16, 24, 3, 64, 96, True), (F16, 16, 1, 96, 64, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("dtype,hq,sq,page,topk,causal", CASES,
                         ids=[f"{'f16' if c[0] is F16 else 'bf16'}-{c[1]}x{c[2]}-p{c[3]}-k{c[4]}" for c in CASES])
def test_mla_sparse_matches_float64(dtype, hq, sq, page, topk, causal, num_splits):
    """Half a block with one tile; a partial second block (3 splits of 2 tiles leave one empty); two head groups
    on one list; one list per position under the causal limit (Sq > a length included); a page size that is no
    power of two (the translation divides instead of shifting). Every list has entries
    that are no key inside a live tile, a duplicate and, from two tiles on, a skipped tile before a live one."""
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    q, _, pool, table, sl = (t.cuda() for t in make_latent(LENS, hq, sq, page, dtype))
    idx = make_lists(LENS, sq, topk).cuda()
    ref, ref_lse = sparse_reference(LENS, hq, sq, page, dtype, topk, causal)
    out, lse = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, return_lse=True,
                                          num_splits=num_splits, indices=idx)
    assert out.shape == (len(LENS), hq, sq, 512) and out.dtype == dtype
    assert lse.shape == (len(LENS), hq, sq) and lse.dtype == torch.float32
    check(out, lse, ref, ref_lse, dtype, f"mla sparse {dtype} {hq}x{sq} page {page} topk {topk} splits {num_splits}")
    assert (out[0] == 0).all() and (lse[0] == float("-inf")).all()  # a sequence without keys
    plain = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, num_splits=num_splits, indices=idx)
    assert torch.equal(plain, out)


@pytest.mark.gpu
def test_mla_sparse_full_list_is_the_dense_function():
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    hq, dtype, topk = 16, BF16, 448
    q, _, pool, table, sl = (t.cuda() for t in make_latent(LENS32, hq, 1, 32, dtype))
    idx = torch.arange(topk, dtype=torch.int32).repeat(len(LENS32), 1, 1)
    idx[idx >= torch.tensor(LENS32)[:, None, None]] = -1
    out, lse = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=False, return_lse=True,
                                          indices=idx.cuda())
    check(out, lse, *dense_reference(LENS32, hq, 1, 32, dtype, False), dtype, "mla sparse, full lists")


@pytest.mark.gpu
def test_mla_sparse_pool_beyond_4gib():
    """One 4.5 GiB pool; the live pages lie on both sides of byte 2^32 (page 58254 of 73728 bytes straddles it)."""
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    page, hq, dtype, n = 64, 16, BF16, 300
    num_pages = (9 << 29) // (page * 1152)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(1, hq, 1, 576, generator=g).to(dtype)
    kv = torch.randn(5 * page, 576, generator=g).to(dtype)
    ids = [58253, 1, 58254, num_pages - 1, 58255]
    pool = torch.empty(num_pages * page * 1152, dtype=torch.uint8, device="cuda").fill_(0xFF).view(dtype)
    pool = pool.view(num_pages, page, 576)
    pool[ids] = kv.view(5, page, 576).cuda()
    pool[ids[-1], n - 4 * page:] = float("nan")
    idx = torch.full((1, 1, 64), -1, dtype=torch.int32)
    idx[0, 0, :40] = torch.randperm(n, generator=g)[:40].to(torch.int32)
    k = kv[idx[0, 0, :40].long()].double()
    s = q[0, :, 0].double() @ k.t() * SCALE
    ref_lse = torch.logsumexp(s, -1)
    ref = torch.exp(s - ref_lse[:, None]) @ k[:, :512]
    out, lse = flash_attn_mla_decode_func(q.cuda(), pool, torch.tensor([ids], dtype=torch.int32).cuda(),
                                          torch.tensor([n], dtype=torch.int32).cuda(), SCALE, causal=False,
                                          return_lse=True, indices=idx.cuda())
    check(out, lse, ref[None, :, None], ref_lse[None, :, None], dtype, "mla sparse, pool beyond 4 GiB")


# ------------------------------------------------------------------------------------------- CPU
def test_mla_sparse_op_schema_fake_and_opcheck():
    import flash_attention_cute_amd as m

    assert "flash_attention_mla_sparse_decode_forward" in m.__all__
    assert str(torch.ops.flash_attention.mla_sparse_decode_forward.default._schema) == (
        "flash_attention::mla_sparse_decode_forward(Tensor q, Tensor kv_cache, Tensor block_table, "
        "Tensor cache_seqlens, Tensor indices, float softmax_scale, bool causal=True, SymInt num_splits=0) "
        "-> (Tensor, Tensor)")
    q, _, pool, table, sl = make_latent((40, 7), 4, 2, 32, BF16)
    idx = make_lists((40, 7), 2, 32)
    with torch._subclasses.FakeTensorMode() as mode:
        o, lse = torch.ops.flash_attention.mla_sparse_decode_forward(
            *(mode.from_tensor(t) for t in (q, pool, table, sl, idx)), SCALE)
    assert o.shape == (2, 4, 2, 512) and o.dtype == BF16 and lse.shape == (2, 4, 2) and lse.dtype == torch.float32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.library.opcheck(torch.ops.flash_attention.mla_sparse_decode_forward.default,
                              (q.float(), pool.float(), table, sl, idx, SCALE, True),
                              test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_mla_sparse_cpu_default_matches_float64(causal):
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    lens, hq, sq, topk = (100, 0, 33, 1), 4, 3, 96
    q, _, pool, table, sl = make_latent(lens, hq, sq, 32, F16)
    with pytest.warns(UserWarning, match="fallback to pytorch"):
        out, lse = flash_attn_mla_decode_func(q.float(), pool.float(), table, sl, SCALE, causal=causal,
                                              return_lse=True, indices=make_lists(lens, sq, topk))
    ref, ref_lse = sparse_reference(lens, hq, sq, 32, F16, topk, causal)
    assert out.shape == ref.shape and torch.isfinite(out).all()  # (the NaN pool: nothing invisible was read)
    torch.testing.assert_close(out.double(), ref, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(lse.double(), ref_lse, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(kv_cache=torch.zeros(2, 32, 576).to(torch.float8_e4m3fn)), NotImplementedError),
    (dict(kv_descale=1.0), NotImplementedError), (dict(indices=torch.zeros(1, 1, 48, dtype=torch.int32)), ValueError),
    (dict(indices=torch.zeros(1, 1, 32, dtype=torch.int64)), ValueError),
    (dict(indices=torch.zeros(2, 1, 32, dtype=torch.int32)), ValueError),
    (dict(indices=torch.zeros(1, 32, dtype=torch.int32)), ValueError)],
    ids=["fp8-cache", "kv_descale", "topk-48", "int64", "leading-shape", "rank"])
def test_mla_sparse_wrapper_errors(kwargs, exc):
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    args = dict(q=torch.zeros(1, 4, 1, 576, dtype=F16), kv_cache=torch.zeros(2, 32, 576, dtype=F16),
                block_table=torch.zeros(1, 2, dtype=torch.int32), cache_seqlens=torch.ones(1, dtype=torch.int32),
                softmax_scale=SCALE, indices=torch.zeros(1, 1, 32, dtype=torch.int32))
    with pytest.raises(exc):
        flash_attn_mla_decode_func(**{**args, **kwargs})


class FaMlaSparseParams(ctypes.Structure):
    _fields_ = [("base", FaMlaParams), ("indices", ctypes.c_void_p), ("topk", ctypes.c_int64),
                ("indices_batch_stride", ctypes.c_int64), ("indices_seqlen_stride", ctypes.c_int64)]


def sparse_params(indices=0x700000, topk=2048, **kw):
    base = mla_params(**kw)
    return FaMlaSparseParams(base, indices, topk, base.seqlen_q * topk, topk)


@pytest.mark.parametrize("kw,code", [({}, FA_OK), (dict(indices=None), FA_ERR_INVALID_ARGUMENT),
                                     (dict(topk=48), FA_ERR_INVALID_ARGUMENT), (dict(topk=0), FA_ERR_INVALID_ARGUMENT),
                                     (dict(indices=0x700002), FA_ERR_INVALID_ARGUMENT),
                                     (dict(page_size=48), FA_ERR_INVALID_ARGUMENT)],
                         ids=["ok", "indices-null", "topk-48", "topk-0", "indices-misaligned", "base-page-48"])
def test_mla_sparse_check_codes_and_workspace(kw, code):
    """Host-only: the check reads no device memory, and the launch entry returns the same code before any launch."""
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(str(LIB))
    lib.fa_mla_sparse_decode_gfx950_ws_bytes.restype = ctypes.c_int64
    p = sparse_params(**kw)
    assert lib.fa_mla_sparse_decode_gfx950_check(ctypes.byref(p), 1) == code
    if code != FA_OK:
        assert lib.fa_mla_sparse_decode_gfx950(ctypes.byref(p), 1, None, 0, None) == code
        assert lib.fa_mla_sparse_decode_gfx950_ws_bytes(ctypes.byref(p)) == -1
        return
    assert lib.fa_mla_sparse_version() == 1 and lib.fa_mla_sparse_decode_gfx950_check(None, 1) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_mla_sparse_decode_gfx950_ws_bytes(ctypes.byref(sparse_params(num_splits=1))) == 0
    assert lib.fa_mla_sparse_decode_gfx950_ws_bytes(ctypes.byref(sparse_params(b=2, hq=24, sq=3, num_splits=3))) == \
        2 * 3 * 24 * 3 * (512 * 4 + 4)


# (shape, topk -> workspace bytes) as the library answered before the three entries shared one plan: the dense
# rule over B * Sq * head groups and the list's topk / 32 tiles, a split at least 2 tiles. Rows: the 2-tile minimum
# deciding (topk 256: 4 splits of 2 tiles, where the dense entry's 8-tile minimum would not split; topk 160: 5 tiles,
# 2 splits) and forbidding a split (topk 64, 32); the workgroup target deciding (B 32, B 64); the head-group boundary
# Hq = 64 / 65; positions, which multiply the workgroups and not the head groups; a forced split count above the
# 256 cap, and one below.
SPARSE_WS_BYTES = [({}, 2048, 1050624), ({}, 256, 131328), ({}, 160, 65664), ({}, 64, 0), ({}, 32, 0),
                   (dict(b=64), 256, 8404992), (dict(hq=64), 2048, 4202496), (dict(hq=65), 2048, 4268160),
                   (dict(hq=16, sq=4), 2048, 4202496), (dict(hq=128, sq=2), 256, 2101248),
                   (dict(b=32, hq=128), 2048, 33619968), (dict(b=32, hq=16, sq=2), 2048, 8404992),
                   (dict(num_splits=300), 2048, 8404992), (dict(b=2, hq=24, sq=3, num_splits=3), 2048, 886464)]


@pytest.mark.parametrize("kw,topk,ws_bytes", SPARSE_WS_BYTES, ids=[
    ",".join(f"{k}={v}" for k, v in {**kw, "topk": topk}.items()) for kw, topk, _ in SPARSE_WS_BYTES])
def test_mla_sparse_ws_bytes_table(kw, topk, ws_bytes):
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(str(LIB))
    lib.fa_mla_sparse_decode_gfx950_ws_bytes.restype = ctypes.c_int64
    assert lib.fa_mla_sparse_decode_gfx950_ws_bytes(ctypes.byref(sparse_params(topk=topk, **kw))) == ws_bytes
