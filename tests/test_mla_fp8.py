"""The FP8 (e4m3) latent cache of the MLA decode and the latent cache's write side (include/fa_gfx950_mla_fp8.h):
``flash_attn_mla_decode_func`` over a ``torch.float8_e4m3fn`` pool, ``flash_attn_mla_append`` (16-bit and
quantizing) and ``flash_attn_mla_with_kvcache``.

The reference is float64 on the CPU over ``bytes.float() * descale``. The kernel widens the bytes exactly and then
does the 16-bit MLA kernel's arithmetic, so the tolerances are tests/test_mla_decode.py's, unchanged. Every unused
page and every row past a length holds the e4m3 NaN byte, every unused table entry -1: every output must be
finite. The append is held to byte equality of the WHOLE pool against a plain loop."""
from __future__ import annotations

import ctypes
import functools
import warnings

import pytest
import torch

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK
from test_mla_decode import (BF16, F16, LENS32, LENS64, SCALE, WS_BYTES, FaMlaParams, check, lib,  # noqa: F401
                             mla_params)

FP8, NAN_BYTE, SENTINEL = torch.float8_e4m3fn, 0x7F, 0x5A


def descales(b):
    return 0.037 * torch.arange(1, b + 1, dtype=torch.float32)  # neither 1 nor a power of two


@functools.lru_cache(maxsize=None)
def make_pool8(lens, hq, sq, page, dtype, seed=0, zero=None, spare=0):
    """q [B, Hq, Sq, 576], the dense dequantised latent (float64 [B, cap, 576]), its bytes scattered into a
    NaN-byte pool [P, page, 576] through a shuffled table (-1 in unused entries; `spare` more pages per
    sequence are allotted for appends), the table, the lengths and the per-sequence descales."""
    from flash_attention_cute_amd.flash_attention import quantize_e4m3

    g = torch.Generator().manual_seed(seed)
    b, max_pages = len(lens), (max(max(lens), 1) + page - 1) // page + spare
    q = torch.randn(b, hq, sq, 576, generator=g).to(dtype)
    kv = torch.randn(b, max_pages * page, 576, generator=g).to(dtype)
    if zero:
        kv[..., slice(512, 576) if zero == "rope" else slice(0, 512)] = 0
    ds = descales(b)
    kv8 = quantize_e4m3(kv, ds[:, None, None])
    ids = torch.randperm(b * max_pages + 3, generator=g).tolist()
    pool = torch.full((b * max_pages + 3, page, 576), NAN_BYTE, dtype=torch.uint8)
    table = torch.full((b, max_pages), -1, dtype=torch.int32)
    for i, n in enumerate(lens):
        for j in range((n + page - 1) // page + spare):
            rows = max(min(n - j * page, page), 0)
            table[i, j] = ids.pop()
            pool[table[i, j], :rows] = kv8.view(torch.uint8)[i, j * page:j * page + rows]
    return q, kv8.double() * ds.double()[:, None, None], pool.view(FP8), table, torch.tensor(lens, dtype=torch.int32), ds


def reference(q, deq, lens, causal):
    """float64: s = scale q kv^T over all 576 columns, bottom-right causal mask, softmax, times kv[:, :512]"""
    b, hq, sq, _ = q.shape
    out = torch.zeros(b, hq, sq, 512, dtype=torch.float64)
    lse = torch.full((b, hq, sq), float("-inf"), dtype=torch.float64)
    for i, n in enumerate(lens):
        k = deq[i, :n]
        s = q[i].double() @ k.t() * SCALE
        if causal:
            s = s.masked_fill(torch.arange(n)[None, :] > torch.arange(sq)[:, None] + n - sq, float("-inf"))
        lse[i] = torch.logsumexp(s, -1) if n else lse[i]
        out[i] = torch.exp(s - lse[i].masked_fill(lse[i].isinf(), 0)[..., None]) @ k[:, :512]
    return out, lse


def append_loop(pool, c_kv, k_pe, lens, table, ds):
    """The append by a plain loop with the drop rules: (expected pool, new lengths)."""
    from flash_attention_cute_amd.flash_attention import quantize_e4m3

    exp, (num_pages, page, _), cap = pool.clone(), pool.shape, table.size(1) * pool.size(1)
    rows = torch.cat([c_kv, k_pe], -1)
    for b, n0 in enumerate(lens):
        for i in range(rows.size(1)):
            n, pid = max(n0, 0) + i, -1
            if n < cap:
                pid = int(table[b, n // page])
            if 0 <= pid < num_pages:
                if pool.dtype == FP8:
                    exp.view(torch.uint8)[pid, n % page] = quantize_e4m3(rows[b, i], ds[b]).view(torch.uint8)
                else:
                    exp[pid, n % page] = rows[b, i]
    return exp, [min(max(n, 0) + rows.size(1), cap) for n in lens]


def norm_bytes(t):
    """The bytes of a pool, for e4m3 with -0 folded onto +0 and both NaN bytes onto one."""
    u = t.contiguous().view(torch.uint8).clone().cpu()
    if t.dtype == FP8:
        u[u == 0x80] = 0
        u[u == 0xFF] = NAN_BYTE
    return u


def append_case(cache_dtype, sn, dtype=BF16):
    """Starting lengths (0, 30, 63, capacity - 2) on page 32: writes cross a page edge and run off the capacity; one
    table entry is outside the pool; the pool holds a sentinel byte pattern."""
    g = torch.Generator().manual_seed(sn)
    page, max_pages, num_pages = 32, 4, 19
    lens = (0, 30, 63, max_pages * page - 2)
    table = torch.randperm(num_pages, generator=g)[:16].reshape(4, max_pages).to(torch.int32)
    table[1, 1] = num_pages + 5
    pool = torch.full((num_pages, page, 576 * (1 if cache_dtype == FP8 else 2)), SENTINEL, dtype=torch.uint8)
    c_kv, k_pe = torch.randn(4, sn, 512, generator=g).to(dtype), torch.randn(4, sn, 64, generator=g).to(dtype)
    return pool.view(cache_dtype), c_kv, k_pe, torch.tensor(lens, dtype=torch.int32), table, descales(4)


# ------------------------------------------------------------------------------------------- GPU
CASES = [(BF16, 16, 1, LENS32, 32, True), (F16, 40, 1, LENS32, 32, True), (BF16, 128, 1, LENS64, 64, False),
         (F16, 16, 2, LENS32, 32, True), (BF16, 24, 3, LENS32, 32, True), (F16, 24, 3, LENS64, 64, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("dtype,hq,sq,lens,page,causal", CASES,
                         ids=[f"{'f16' if c[0] is F16 else 'bf16'}-{c[1]}x{c[2]}-p{c[4]}" for c in CASES])
def test_mla_fp8_decode_matches_float64(dtype, hq, sq, lens, page, causal, num_splits):
    """Half a block, a partial second block, two row groups, positions inside a block and a block boundary inside a
    head (Sq above a length included); lengths that leave a pair of tiles half empty, an odd and an even tile
    count, shuffled pages. 3 splits leave length 100 (4 tiles) an empty split."""
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    q, deq, pool, table, sl, ds = make_pool8(lens, hq, sq, page, dtype)
    ref, ref_lse = reference(q, deq, lens, causal)
    q, pool, table, sl, ds = (t.cuda() for t in (q, pool, table, sl, ds))
    out, lse = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, return_lse=True,
                                          num_splits=num_splits, kv_descale=ds)
    assert out.shape == (len(lens), hq, sq, 512) and out.dtype == dtype and lse.dtype == torch.float32
    check(out, lse, ref, ref_lse, dtype, f"mla fp8 {dtype} {hq}x{sq} page {page} splits {num_splits}")
    assert (out[0] == 0).all() and (lse[0] == float("-inf")).all()  # a sequence without keys
    plain = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, num_splits=num_splits, kv_descale=ds)
    assert torch.equal(plain, out)
    one = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, num_splits=num_splits, kv_descale=0.05)
    scalar = torch.full((1,), 0.05, device="cuda")  # broadcast to [B] with stride 0
    assert torch.equal(flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, num_splits=num_splits,
                                                  kv_descale=scalar), one)


@pytest.mark.gpu
@pytest.mark.parametrize("zero", ["rope", "nope"])
def test_mla_fp8_decode_score_and_value_columns(zero):
    """Latent columns 512..575 zero: the RoPE columns enter the score and nothing else. Columns 0..511 zero: no
    RoPE column leaks into the output (it is 0) while the LSE is still the reference's."""
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    lens, hq, sq, dtype = (100, 33), 40, 2, F16
    q, deq, pool, table, sl, ds = make_pool8(lens, hq, sq, 32, dtype, 1, zero)
    out, lse = flash_attn_mla_decode_func(q.cuda(), pool.cuda(), table.cuda(), sl.cuda(), SCALE, return_lse=True,
                                          kv_descale=ds.cuda())
    check(out, lse, *reference(q, deq, lens, True), dtype, f"mla fp8 zero {zero}")
    if zero == "nope":
        assert (out == 0).all()


@pytest.mark.gpu
def test_mla_fp8_decode_plan_splits_a_long_sequence():
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    lens, hq, dtype = (4129,), 16, BF16
    q, deq, pool, table, sl, ds = make_pool8(lens, hq, 1, 32, dtype)
    out, lse = flash_attn_mla_decode_func(q.cuda(), pool.cuda(), table.cuda(), sl.cuda(), SCALE, return_lse=True,
                                          kv_descale=ds.cuda())  # num_splits=0: the plan's
    check(out, lse, *reference(q, deq, lens, True), dtype, "mla fp8 plan-split 4129 keys")


@pytest.mark.gpu
@pytest.mark.parametrize("sn", [1, 3, 40])
@pytest.mark.parametrize("cache_dtype", [BF16, FP8], ids=["bf16", "fp8"])
def test_mla_append_writes_exactly_the_loops_bytes(cache_dtype, sn):
    from flash_attention_cute_amd import flash_attn_mla_append

    pool, c_kv, k_pe, sl, table, ds = append_case(cache_dtype, sn)
    exp, exp_lens = append_loop(pool, c_kv, k_pe, sl.tolist(), table, ds)
    pool_g, sl_g = pool.cuda(), sl.cuda()
    new = flash_attn_mla_append(pool_g, c_kv.cuda(), k_pe.cuda(), sl_g, table.cuda(),
                                ds.cuda() if cache_dtype == FP8 else None)
    assert torch.equal(norm_bytes(pool_g), norm_bytes(exp))  # the whole pool: nothing else was written
    assert new.tolist() == exp_lens and new.dtype == torch.int32 and torch.equal(sl_g.cpu(), sl)


@pytest.mark.gpu
def test_mla_with_kvcache_three_steps_on_an_fp8_pool():
    from flash_attention_cute_amd import flash_attn_mla_append, flash_attn_mla_decode_func, flash_attn_mla_with_kvcache
    from flash_attention_cute_amd.flash_attention import quantize_e4m3

    lens, hq, sq, dtype = [31, 64, 0], 16, 2, BF16
    q0, deq, pool, table, sl, ds = make_pool8(tuple(lens), hq, sq, 32, dtype, 2, None, 1)
    pool, table, sl, ds_g = pool.cuda(), table.cuda(), sl.cuda(), ds.cuda()
    deq, g = deq.clone(), torch.Generator().manual_seed(3)
    for step in range(3):
        q = torch.randn(3, hq, sq, 576, generator=g).to(dtype)
        c_kv, k_pe = torch.randn(3, sq, 512, generator=g).to(dtype), torch.randn(3, sq, 64, generator=g).to(dtype)
        for b in range(3):  # the expected dequantised history
            row8 = quantize_e4m3(torch.cat([c_kv[b], k_pe[b]], -1), ds[b])
            deq[b, lens[b]:lens[b] + sq] = row8.double() * ds[b].double()
        if step == 2:
            pool2 = pool.clone()
            n2 = flash_attn_mla_append(pool2, c_kv.cuda(), k_pe.cuda(), sl, table, ds_g)
            two = flash_attn_mla_decode_func(q.cuda(), pool2, table, n2, SCALE, return_lse=True, kv_descale=ds_g)
        out, lse, new = flash_attn_mla_with_kvcache(q.cuda(), pool, c_kv.cuda(), k_pe.cuda(), sl, table, SCALE,
                                                    kv_descale=ds_g, return_lse=True, return_seqlens=True)
        lens = [n + sq for n in lens]
        assert new.tolist() == lens
        check(out, lse, *reference(q, deq, lens, True), dtype, f"mla fp8 with_kvcache step {step}")
        sl = new
    assert torch.equal(out, two[0]) and torch.equal(lse, two[1]) and torch.equal(norm_bytes(pool), norm_bytes(pool2))


# ------------------------------------------------------------------------------------------- CPU
def test_mla_fp8_op_schemas_fakes_and_opcheck():
    import flash_attention_cute_amd as m

    for name in ("flash_attn_mla_append", "flash_attn_mla_with_kvcache", "flash_attention_mla_decode_forward_fp8",
                 "flash_attention_mla_append", "flash_attention_mla_append_fp8"):
        assert name in m.__all__ and callable(getattr(m, name))
    ops = torch.ops.flash_attention
    assert str(ops.mla_decode_forward_fp8.default._schema) == (
        "flash_attention::mla_decode_forward_fp8(Tensor q, Tensor kv_cache, Tensor block_table, Tensor cache_seqlens, "
        "Tensor? kv_descale, float softmax_scale, bool causal=True, SymInt num_splits=0) -> (Tensor, Tensor)")
    assert str(ops.mla_append.default._schema) == (
        "flash_attention::mla_append(Tensor(a0!) kv_cache, Tensor c_kv, Tensor k_pe, Tensor cache_seqlens, "
        "Tensor block_table) -> Tensor")
    assert str(ops.mla_append_fp8.default._schema) == (
        "flash_attention::mla_append_fp8(Tensor(a0!) kv_cache, Tensor c_kv, Tensor k_pe, Tensor cache_seqlens, "
        "Tensor block_table, Tensor? kv_descale=None) -> Tensor")
    q, _, pool, table, sl, ds = make_pool8((40, 7), 4, 2, 32, BF16)
    with torch._subclasses.FakeTensorMode() as mode:
        o, lse = ops.mla_decode_forward_fp8(*(mode.from_tensor(t) for t in (q, pool, table, sl, ds)), SCALE)
    assert o.shape == (2, 4, 2, 512) and o.dtype == BF16 and lse.shape == (2, 4, 2) and lse.dtype == torch.float32
    c_kv, k_pe = torch.randn(2, 3, 512).to(BF16), torch.randn(2, 3, 64).to(BF16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clean = torch.where(pool.view(torch.uint8) == NAN_BYTE, 0, pool.view(torch.uint8)).view(FP8)
        # (torch's "test_schema" compares inputs with allclose, which float8 tensors do not have on the CPU: the
        # schema strings above pin what the FP8 ops mutate)
        fake = ("test_faketensor",)
        torch.library.opcheck(ops.mla_decode_forward_fp8.default, (q, clean, table, sl, ds, SCALE, True), test_utils=fake)
        torch.library.opcheck(ops.mla_append_fp8.default, (clean.clone(), c_kv, k_pe, sl, table, ds), test_utils=fake)
        torch.library.opcheck(ops.mla_append.default, (torch.zeros(5, 32, 576, dtype=BF16), c_kv, k_pe, sl, table),
                              test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_mla_fp8_cpu_default_matches_float64(causal):
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    lens, hq, sq = (100, 0, 33, 1), 4, 3
    q, deq, pool, table, sl, ds = make_pool8(lens, hq, sq, 32, F16)
    with pytest.warns(UserWarning, match="fallback to pytorch"):
        out, lse = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, return_lse=True, kv_descale=ds)
    ref, ref_lse = reference(q, deq, lens, causal)
    assert out.dtype == F16 and torch.isfinite(out).all()
    torch.testing.assert_close(out.double(), ref, atol=2e-3, rtol=2e-3)  # (one rounding to fp16)
    torch.testing.assert_close(lse.double(), ref_lse, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("sn", [1, 40])
@pytest.mark.parametrize("cache_dtype", [BF16, FP8], ids=["bf16", "fp8"])
def test_mla_append_cpu_default_matches_the_loop(cache_dtype, sn):
    from flash_attention_cute_amd import flash_attn_mla_append

    pool, c_kv, k_pe, sl, table, ds = append_case(cache_dtype, sn)
    exp, exp_lens = append_loop(pool, c_kv, k_pe, sl.tolist(), table, ds)
    new = flash_attn_mla_append(pool, c_kv, k_pe, sl, table, ds if cache_dtype == FP8 else None)
    assert torch.equal(norm_bytes(pool), norm_bytes(exp)) and new.tolist() == exp_lens


@pytest.mark.parametrize("kwargs", [
    dict(kv_cache=torch.zeros(2, 32, 576, dtype=torch.uint8).view(torch.float8_e5m2)),
    dict(kv_descale=0.5), dict(kv_cache=torch.zeros(2, 48, 576, dtype=torch.uint8).view(FP8)),
    dict(q=torch.zeros(1, 4, 1, 576), kv_cache=torch.zeros(2, 32, 576, dtype=torch.uint8).view(FP8))],
    ids=["e5m2-pool", "descale-16bit-pool", "page-48", "fp32-q"])
def test_mla_fp8_wrapper_errors(kwargs):
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    args = dict(q=torch.zeros(1, 4, 1, 576, dtype=F16), kv_cache=torch.zeros(2, 32, 576, dtype=F16),
                block_table=torch.zeros(1, 2, dtype=torch.int32), cache_seqlens=torch.ones(1, dtype=torch.int32),
                softmax_scale=SCALE)
    with pytest.raises(ValueError):
        flash_attn_mla_decode_func(**{**args, **kwargs})


class FaMlaFp8Params(ctypes.Structure):
    _fields_ = [("base", FaMlaParams), ("kv_descale", ctypes.c_void_p), ("kv_descale_stride", ctypes.c_int64)]


@pytest.mark.parametrize("kw,descale_stride,code", [
    ({}, 1, FA_OK), ({}, 0, FA_OK), (dict(q_ptr=None), 1, FA_ERR_INVALID_ARGUMENT),
    (dict(kv_ptr=None), 1, FA_ERR_INVALID_ARGUMENT), (dict(seqlens_k=None), 1, FA_ERR_INVALID_ARGUMENT),
    (dict(kv_row_stride=580), 1, FA_ERR_INVALID_ARGUMENT), (dict(kv_row_stride=584), 1, FA_ERR_INVALID_ARGUMENT),
    ({}, -1, FA_ERR_INVALID_ARGUMENT), (dict(headdim_qk=512), 1, FA_ERR_UNSUPPORTED),
    (dict(headdim_v=576), 1, FA_ERR_UNSUPPORTED)],
    ids=["ok", "ok-scalar", "q-null", "kv-null", "lens-null", "row-stride-580", "row-stride-584", "descale-stride",
         "dqk-512", "dv-576"])
def test_mla_fp8_check_codes(lib, kw, descale_stride, code):  # noqa: F811
    """Host-only: the check reads no device memory, and the launch entry returns the same code before any launch."""
    lib.fa_mla_decode_fp8_gfx950_ws_bytes.restype = ctypes.c_int64
    p = FaMlaFp8Params(mla_params(**kw), 0x700000, descale_stride)
    assert lib.fa_mla_decode_fp8_gfx950_check(ctypes.byref(p), 1) == code
    if code != FA_OK:
        assert lib.fa_mla_decode_fp8_gfx950(ctypes.byref(p), 1, None, 0, None) == code
        assert lib.fa_mla_decode_fp8_gfx950_ws_bytes(ctypes.byref(p)) == -1
    else:  # the 16-bit call's plan and workspace
        assert lib.fa_mla_decode_fp8_gfx950_ws_bytes(ctypes.byref(p)) == \
            lib.fa_mla_decode_gfx950_ws_bytes(ctypes.byref(p.base)) > 0
    assert lib.fa_mla_decode_fp8_gfx950_check(None, 1) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_mla_fp8_version() == 1


def test_mla_fp8_ws_bytes_is_the_dense_entrys(lib):  # noqa: F811
    """One plan: on every row of the dense entry's table the FP8 entry asks for the same workspace."""
    lib.fa_mla_decode_fp8_gfx950_ws_bytes.restype = ctypes.c_int64
    for kw, ws_bytes in WS_BYTES:
        p = FaMlaFp8Params(mla_params(**kw), 0x700000, 1)
        assert lib.fa_mla_decode_fp8_gfx950_ws_bytes(ctypes.byref(p)) == ws_bytes == \
            lib.fa_mla_decode_gfx950_ws_bytes(ctypes.byref(p.base)), kw
