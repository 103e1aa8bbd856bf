"""MLA decode over a paged latent KV cache (``flash_attn_mla_decode_func``, include/fa_gfx950_mla.h): 576 score
columns, the first 512 of the same rows are the value, one latent stream per sequence shared by every q-head.

The reference is float64 on the CPU over the same 16-bit inputs. Tolerances are the project's: the output bound
of tests/test_gpu_parity.py (fp32 scores, P rounded to T, one output rounding -- the longer dot product only adds
fp32 accumulation error) and 2^-12 absolute on the LSE (tests/test_paged_lse.py), -inf exactly where the
reference has it. The pool is NaN in every unused page and in every row past a length, the table -1 in every
unused entry: every output must be finite."""
from __future__ import annotations

import ctypes
import functools
import warnings
from pathlib import Path

import pytest
import torch

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK

F16, BF16 = torch.float16, torch.bfloat16
TOL = {F16: 2e-3, BF16: 1.6e-2}  # |out - ref| <= tol + tol |ref| (tests/test_gpu_parity.py)
LSE_TOL = 2.0 ** -12
SCALE = 192 ** -0.5  # DeepSeek's: (128 nope + 64 rope) ** -0.5
LENS32, LENS64 = (0, 1, 31, 33, 64, 100, 417), (0, 64, 191)
LIB = Path(__file__).resolve().parent.parent / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"


@functools.lru_cache(maxsize=None)
def make_latent(lens, hq, sq, page, dtype, seed=0, zero=None):
    """q [B, Hq, Sq, 576], the dense latent [B, cap, 576], and the same rows scattered into a NaN-poisoned pool
    [P, page, 576] through a shuffled table (-1 in unused entries). zero: "rope" / "nope" zeroes those columns."""
    g = torch.Generator().manual_seed(seed)
    b, max_pages = len(lens), (max(max(lens), 1) + page - 1) // page
    q = torch.randn(b, hq, sq, 576, generator=g).to(dtype)
    kv = torch.randn(b, max_pages * page, 576, generator=g).to(dtype)
    if zero == "rope":
        kv[..., 512:] = 0
    if zero == "nope":
        kv[..., :512] = 0
    ids = torch.randperm(b * max_pages + 3, generator=g).tolist()
    pool = torch.full((b * max_pages + 3, page, 576), float("nan"), dtype=dtype)
    table = torch.full((b, max_pages), -1, dtype=torch.int32)
    for i, n in enumerate(lens):
        for j in range((n + page - 1) // page):
            rows = min(n - j * page, page)
            table[i, j] = ids.pop()
            pool[table[i, j], :rows] = kv[i, j * page:j * page + rows]
    return q, kv, pool, table, torch.tensor(lens, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def reference(lens, hq, sq, page, dtype, causal, seed=0, zero=None):
    """float64: s = scale q kv^T over all 576 columns, bottom-right causal mask, softmax, times kv[:, :512]"""
    q, kv, *_ = make_latent(lens, hq, sq, page, dtype, seed, zero)
    out = torch.zeros(len(lens), hq, sq, 512, dtype=torch.float64)
    lse = torch.full((len(lens), hq, sq), float("-inf"), dtype=torch.float64)
    for b, n in enumerate(lens):
        k = kv[b, :n].double()
        s = q[b].double() @ k.t() * SCALE
        if causal:
            s = s.masked_fill(torch.arange(n)[None, :] > torch.arange(sq)[:, None] + n - sq, float("-inf"))
        lse[b] = torch.logsumexp(s, -1) if n else lse[b]
        out[b] = torch.exp(s - lse[b].masked_fill(lse[b].isinf(), 0)[..., None]) @ k[:, :512]
    return out, lse


def check(out, lse, ref, ref_lse, dtype, what):
    assert torch.isfinite(out).all(), what
    err = ((out.double().cpu() - ref).abs() / (1 + ref.abs())).max().item()
    inf = ref_lse.isinf()
    assert (lse.cpu()[inf] == float("-inf")).all() and torch.isfinite(lse.cpu()[~inf]).all(), what
    lerr = (lse.double().cpu() - ref_lse)[~inf].abs().max().item() if (~inf).any() else 0.0
    print(f"{what}: max |out - ref| / (1 + |ref|) = {err:.3e} (bound {TOL[dtype]:.1e}), max |lse - ref| = {lerr:.3e}")
    assert err <= TOL[dtype] and lerr <= LSE_TOL, what


# ------------------------------------------------------------------------------------------- GPU
CASES = [(BF16, 16, 1, LENS32, 32, True), (F16, 40, 1, LENS32, 32, True), (BF16, 128, 1, LENS64, 64, False),
         (F16, 128, 1, LENS32, 32, True), (F16, 16, 2, LENS32, 32, True), (BF16, 24, 3, LENS32, 32, True),
         (F16, 24, 3, LENS64, 64, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("dtype,hq,sq,lens,page,causal", CASES,
                         ids=[f"{'f16' if c[0] is F16 else 'bf16'}-{c[1]}x{c[2]}-p{c[4]}" for c in CASES])
def test_mla_decode_matches_float64(dtype, hq, sq, lens, page, causal, num_splits):
    """Half a block, a partial second block, two row groups, positions inside a block and a block boundary inside
    a head (a row's limit per position, Sq > a length included); lengths: empty, a tile's first row, a tile edge
    on either side, an exact page, several shuffled pages. 3 splits leave length 100 (4 tiles) an empty split."""
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    q, _, pool, table, sl = (t.cuda() for t in make_latent(lens, hq, sq, page, dtype))
    ref, ref_lse = reference(lens, hq, sq, page, dtype, causal)
    out, lse = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, return_lse=True,
                                          num_splits=num_splits)
    assert out.shape == (len(lens), hq, sq, 512) and out.dtype == dtype and lse.dtype == torch.float32
    check(out, lse, ref, ref_lse, dtype, f"mla {dtype} {hq}x{sq} page {page} splits {num_splits}")
    assert (out[0] == 0).all()  # a sequence without keys
    plain = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=causal, num_splits=num_splits)
    assert torch.equal(plain, out)
    # a 4-D pool with a singleton head axis in either position is the same view
    for pool4 in (pool.unsqueeze(1), pool.unsqueeze(2)):
        assert torch.equal(flash_attn_mla_decode_func(q, pool4, table, sl, SCALE, causal=causal,
                                                      num_splits=num_splits), out)


@pytest.mark.gpu
def test_mla_decode_plan_splits_a_long_sequence():
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    lens, hq, dtype = (4129,), 16, BF16
    q, _, pool, table, sl = (t.cuda() for t in make_latent(lens, hq, 1, 32, dtype))
    out, lse = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, return_lse=True)  # num_splits=0: the plan's
    check(out, lse, *reference(lens, hq, 1, 32, dtype, True), dtype, "mla plan-split 4129 keys")


@pytest.mark.gpu
@pytest.mark.parametrize("zero", ["rope", "nope"])
def test_mla_decode_score_and_value_columns(zero):
    """Latent columns 512..575 zero: the RoPE columns enter the score and nothing else. Columns 0..511 zero: no
    RoPE column leaks into the output (it is 0) while the LSE is still the reference's."""
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    lens, hq, sq, dtype = (100, 33), 40, 2, F16
    q, _, pool, table, sl = (t.cuda() for t in make_latent(lens, hq, sq, 32, dtype, 1, zero))
    ref, ref_lse = reference(lens, hq, sq, 32, dtype, True, 1, zero)
    out, lse = flash_attn_mla_decode_func(q, pool, table, sl, SCALE, return_lse=True)
    check(out, lse, ref, ref_lse, dtype, f"mla zero {zero}")
    if zero == "nope":
        assert (out == 0).all()


@pytest.mark.gpu
def test_mla_decode_non_contiguous_q_is_bit_identical():
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    q, _, pool, table, sl = (t.cuda() for t in make_latent(LENS64, 24, 3, 64, BF16))
    qt = q.transpose(1, 2).contiguous().transpose(1, 2)  # a [B, Sq, Hq, 576] buffer viewed as [B, Hq, Sq, 576]
    assert not qt.is_contiguous()
    for ns in (1, 3):
        assert torch.equal(flash_attn_mla_decode_func(qt, pool, table, sl, SCALE, num_splits=ns),
                           flash_attn_mla_decode_func(q, pool, table, sl, SCALE, num_splits=ns))


# ------------------------------------------------------------------------------------------- CPU
def test_mla_op_schema_fake_and_opcheck():
    import flash_attention_cute_amd as m

    assert "flash_attn_mla_decode_func" in m.__all__ and "flash_attention_mla_decode_forward" in m.__all__
    assert str(torch.ops.flash_attention.mla_decode_forward.default._schema) == (
        "flash_attention::mla_decode_forward(Tensor q, Tensor kv_cache, Tensor block_table, Tensor cache_seqlens, "
        "float softmax_scale, bool causal=True, SymInt num_splits=0) -> (Tensor, Tensor)")
    q, _, pool, table, sl = make_latent((40, 7), 4, 2, 32, BF16)
    with torch._subclasses.FakeTensorMode() as mode:
        o, lse = torch.ops.flash_attention.mla_decode_forward(mode.from_tensor(q), mode.from_tensor(pool),
                                                              mode.from_tensor(table), mode.from_tensor(sl), SCALE)
    assert o.shape == (2, 4, 2, 512) and o.dtype == BF16 and lse.shape == (2, 4, 2) and lse.dtype == torch.float32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.library.opcheck(torch.ops.flash_attention.mla_decode_forward.default,
                              (q.float(), pool.float().nan_to_num(0.0), table, sl, SCALE, True),
                              test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_mla_cpu_default_matches_float64(causal):
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    lens, hq, sq = (100, 0, 33, 1), 4, 3
    q, _, pool, table, sl = make_latent(lens, hq, sq, 32, F16)
    with pytest.warns(UserWarning, match="fallback to pytorch"):
        out, lse = flash_attn_mla_decode_func(q.float(), pool.float(), table, sl, SCALE, causal=causal,
                                              return_lse=True)
    ref, ref_lse = reference(lens, hq, sq, 32, F16, causal)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    torch.testing.assert_close(out.double(), ref, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(lse.double(), ref_lse, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(softmax_scale=None), TypeError), (dict(q=torch.zeros(1, 4, 1, 512, dtype=F16)), NotImplementedError),
    (dict(head_dim_v=256), NotImplementedError), (dict(kv_cache=torch.zeros(2, 32, 576, dtype=BF16)), ValueError)],
    ids=["no-scale", "q-width", "head_dim_v", "dtype"])
def test_mla_wrapper_errors(kwargs, exc):
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    args = dict(q=torch.zeros(1, 4, 1, 576, dtype=F16), kv_cache=torch.zeros(2, 32, 576, dtype=F16),
                block_table=torch.zeros(1, 2, dtype=torch.int32), cache_seqlens=torch.ones(1, dtype=torch.int32),
                softmax_scale=SCALE)
    with pytest.raises(exc):
        flash_attn_mla_decode_func(**{**args, **kwargs})
    with pytest.raises(TypeError):  # softmax_scale has no default
        flash_attn_mla_decode_func(args["q"], args["kv_cache"], args["block_table"], args["cache_seqlens"])


class FaMlaParams(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in ("q_ptr", "kv_ptr", "o_ptr", "lse_ptr", "block_table", "seqlens_k")] +
                [(n, ctypes.c_int64) for n in (
                    "batch_size", "num_heads_q", "seqlen_q", "headdim_qk", "headdim_v", "q_batch_stride",
                    "q_head_stride", "q_seqlen_stride", "o_batch_stride", "o_head_stride", "o_seqlen_stride",
                    "lse_batch_stride", "lse_head_stride", "lse_seqlen_stride", "kv_page_stride", "kv_row_stride",
                    "num_pages", "page_size", "max_pages", "block_table_stride", "num_splits")] +
                [("softmax_scale", ctypes.c_float), ("causal", ctypes.c_int32)])


def mla_params(b=1, hq=16, sq=1, page=32, max_pages=130, **kw):
    p = FaMlaParams(0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, b, hq, sq, 576, 512,
                    hq * sq * 576, sq * 576, 576, hq * sq * 512, sq * 512, 512, hq * sq, sq, 1, page * 576, 576,
                    b * max_pages, page, max_pages, max_pages, 0, 0.1, 1)
    for key, val in kw.items():
        setattr(p, key, val)
    return p


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(str(LIB))
    lib.fa_mla_decode_gfx950_ws_bytes.restype = ctypes.c_int64
    return lib


@pytest.mark.parametrize("kw,code", [
    ({}, FA_OK), (dict(q_ptr=None), FA_ERR_INVALID_ARGUMENT), (dict(kv_ptr=None), FA_ERR_INVALID_ARGUMENT),
    (dict(block_table=None), FA_ERR_INVALID_ARGUMENT), (dict(seqlens_k=None), FA_ERR_INVALID_ARGUMENT),
    (dict(page_size=48), FA_ERR_INVALID_ARGUMENT), (dict(kv_row_stride=580), FA_ERR_INVALID_ARGUMENT),
    (dict(headdim_qk=512), FA_ERR_UNSUPPORTED), (dict(headdim_v=576), FA_ERR_UNSUPPORTED),
    (dict(batch_size=-1), FA_ERR_INVALID_ARGUMENT)],
    ids=["ok", "q-null", "kv-null", "table-null", "lens-null", "page-48", "row-stride-580", "dqk-512", "dv-576",
         "batch-negative"])
def test_mla_check_codes(lib, kw, code):
    """Host-only: the check reads no device memory, and the launch entry returns the same code before any launch."""
    p = mla_params(**kw)
    assert lib.fa_mla_decode_gfx950_check(ctypes.byref(p), 1) == code
    if code != FA_OK:
        assert lib.fa_mla_decode_gfx950(ctypes.byref(p), 1, None, 0, None) == code
        assert lib.fa_mla_decode_gfx950_ws_bytes(ctypes.byref(p)) == -1
    assert lib.fa_mla_decode_gfx950_check(None, 1) == FA_ERR_INVALID_ARGUMENT


def test_mla_plan_splits_one_long_sequence_and_honours_num_splits(lib):
    """B = 1 with 4129 keys (130 pages of 32): the plan picks more than one split; the workspace is the plan's
    fp32 partials (512 columns and one lse per row and split)."""
    assert lib.fa_mla_decode_gfx950_ws_bytes(ctypes.byref(mla_params())) > 0
    assert lib.fa_mla_decode_gfx950_ws_bytes(ctypes.byref(mla_params(max_pages=4))) == 0
    assert lib.fa_mla_decode_gfx950_ws_bytes(ctypes.byref(mla_params(num_splits=1))) == 0
    assert lib.fa_mla_decode_gfx950_ws_bytes(ctypes.byref(mla_params(b=2, hq=24, sq=3, num_splits=3))) == \
        2 * 3 * 72 * (512 * 4 + 4)


# (shape -> workspace bytes) as the library answered before the three entries shared one plan: the split rule (256
# workgroups over B * row groups, a split at least 8 tiles of the table's capacity, at most 256) times 2052 bytes per
# (batch, split, row). Rows: the 8-tile minimum on either side (15 / 16 tiles) and deciding (130 tiles); the
# row-group boundary Hq * Sq = 64 / 65, by heads and by positions; the workgroup target deciding at B 32; a batch
# that needs no split; a forced split count above the 256 cap, and one below; a page of 96; an empty batch.
WS_BYTES = [({}, 525312), (dict(max_pages=4), 0), (dict(max_pages=15), 0), (dict(max_pages=16), 65664),
            (dict(hq=64), 2101248), (dict(hq=65), 2134080), (dict(hq=16, sq=4), 2101248), (dict(hq=13, sq=5), 2134080),
            (dict(b=32, hq=128, max_pages=64), 33619968), (dict(b=32, hq=16, page=64, max_pages=63), 8404992),
            (dict(b=4096, hq=1, max_pages=4096), 0), (dict(num_splits=300), 8404992),
            (dict(b=2, hq=24, sq=3, num_splits=3), 886464), (dict(page=96, max_pages=7), 65664),
            (dict(b=0, num_pages=1, num_splits=3), 0)]


@pytest.mark.parametrize("kw,ws_bytes", WS_BYTES, ids=[",".join(f"{k}={v}" for k, v in kw.items()) or "default"
                                                       for kw, _ in WS_BYTES])
def test_mla_ws_bytes_table(lib, kw, ws_bytes):
    assert lib.fa_mla_decode_gfx950_ws_bytes(ctypes.byref(mla_params(**kw))) == ws_bytes
