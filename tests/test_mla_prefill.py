"""MLA prefill attention (include/fa_gfx950_mla_prefill.h, flash_attn_mla_prefill_func): 192 key / 128 value columns
over packed sequences, against a float64 reference over the same 16-bit inputs.

Tolerances are tests/test_mla_decode.py's (from test_gpu_parity.py and test_paged_lse.py): |out - ref| <= tol (1 +
|ref|) with tol 2e-3 (fp16) / 1.6e-2 (bf16), 2^-12 absolute on the LSE, -inf exactly where the reference has it.
"""
from __future__ import annotations

import ctypes
import functools
import warnings
from pathlib import Path

import pytest
import torch

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK

F16, BF16 = torch.float16, torch.bfloat16
TOL = {F16: 2e-3, BF16: 1.6e-2}
LSE_TOL = 2.0 ** -12
SCALE = 0.1147  # (not 192 ** -0.5: with YaRN the scale is the model's)
LIB = Path(__file__).resolve().parent.parent / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
# (Sq_b, Sk_b): no queries; one row; a partial block; Sq < Sk across a 64-key tile edge; either side of the 128- and
# 256-row blocks; more queries than keys (causal: the first 50 rows see nothing); no keys
SEQS = ((0, 40), (1, 1), (31, 31), (64, 200), (129, 129), (257, 300), (70, 20), (33, 0))
SMALL = tuple(s for s in SEQS if s[0] <= 128)  # max_seqlen_q 70: the 128-row variant
CHUNK = ((100, 300),)


@functools.lru_cache(maxsize=None)
def make_inputs(seqs, hq, hkv, dtype, zero=None):
    """q [total_q, Hq, 192], k [total_k, Hkv, 192], v [total_k, Hkv, 128], cu_seqlens_q, cu_seqlens_k."""
    g = torch.Generator().manual_seed(len(seqs) + hq)
    tq, tk = sum(s[0] for s in seqs), sum(s[1] for s in seqs)
    q, k = torch.randn(tq, hq, 192, generator=g).to(dtype), torch.randn(tk, hkv, 192, generator=g).to(dtype)
    v = torch.randn(tk, hkv, 128, generator=g).to(dtype)
    if zero == "rope":
        k[..., 128:] = 0
    if zero == "v":
        v.zero_()
    cu = [torch.tensor([0] + [s[i] for s in seqs]).cumsum(0).to(torch.int32) for i in (0, 1)]
    return q, k, v, cu[0], cu[1]


@functools.lru_cache(maxsize=None)
def reference(seqs, hq, hkv, dtype, causal, zero=None):
    """float64: per sequence s = scale q k^T over all 192 columns, bottom-right causal mask, softmax, times v"""
    q, k, v, cq, ck = make_inputs(seqs, hq, hkv, dtype, zero)
    out = torch.zeros(q.size(0), hq, 128, dtype=torch.float64)
    lse = torch.full((hq, q.size(0)), float("-inf"), dtype=torch.float64)
    for b, (sq, sk) in enumerate(seqs):
        if sq == 0 or sk == 0:
            continue
        qs, ks = slice(cq[b], cq[b] + sq), slice(ck[b], ck[b] + sk)
        kb, vb = (t[ks].double().repeat_interleave(hq // hkv, 1) for t in (k, v))
        s = torch.einsum("mhd,nhd->hmn", q[qs].double(), kb) * SCALE
        if causal:
            s = s.masked_fill(torch.arange(sk)[None, :] > torch.arange(sq)[:, None] + sk - sq, float("-inf"))
        lse[:, qs] = torch.logsumexp(s, -1)
        out[qs] = torch.einsum("hmn,nhd->mhd", torch.exp(s - lse[:, qs].masked_fill(lse[:, qs].isinf(), 0)[..., None]), vb)
    return out, lse


def check(out, lse, ref, ref_lse, dtype, what):
    assert torch.isfinite(out).all(), what
    err = ((out.double().cpu() - ref).abs() / (1 + ref.abs())).max().item()
    inf = ref_lse.isinf()
    assert (lse.cpu()[inf] == float("-inf")).all() and torch.isfinite(lse.cpu()[~inf]).all(), what
    lerr = (lse.double().cpu() - ref_lse)[~inf].abs().max().item()
    print(f"{what}: max |out - ref| / (1 + |ref|) = {err:.3e} (bound {TOL[dtype]:.1e}), max |lse - ref| = {lerr:.3e}")
    assert err <= TOL[dtype] and lerr <= LSE_TOL, what


def run(seqs, hq, hkv, dtype, causal, zero=None, **kw):
    from flash_attention_cute_amd import flash_attn_mla_prefill_func

    q, k, v, cq, ck = (t.cuda() for t in make_inputs(seqs, hq, hkv, dtype, zero))
    args = dict(q=q, k=k, v=v, cu_seqlens_q=cq, cu_seqlens_k=ck, max_seqlen_q=max(s[0] for s in seqs),
                max_seqlen_k=max(s[1] for s in seqs), softmax_scale=SCALE, causal=causal, return_lse=True)
    return flash_attn_mla_prefill_func(**{**args, **(kw.pop("edit")(args) if "edit" in kw else {}), **kw})


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("seqs", [SEQS, SMALL], ids=["rows256", "rows128"])
@pytest.mark.parametrize("hq,hkv", [(2, 2), (4, 2)], ids=["mha", "gqa"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_mla_prefill_matches_float64(dtype, causal, hq, hkv, seqs):
    out, lse = run(seqs, hq, hkv, dtype, causal)
    assert out.shape == (sum(s[0] for s in seqs), hq, 128) and out.dtype == dtype
    assert lse.shape == (hq, out.size(0)) and lse.dtype == torch.float32
    check(out, lse, *reference(seqs, hq, hkv, dtype, causal), dtype, f"mla prefill {dtype} causal {causal} {hq}/{hkv}")
    assert torch.equal(run(seqs, hq, hkv, dtype, causal, return_lse=False), out)


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_mla_prefill_reads_nothing_outside_a_sequence(causal):
    """The (0, 40) sequence has keys and no queries: its 40 rows are NaN; k / v are 64 NaN rows longer than the last
    sequence's end. A tile that overhangs a sequence's end must read zeros, so the result is the clean run's bits."""
    def poison(args):
        k, v = (torch.cat([t, t.new_full((64, *t.shape[1:]), float("nan"))]) for t in (args["k"], args["v"]))
        k[:40], v[:40] = float("nan"), float("nan")
        return dict(k=k, v=v)

    clean, dirty = run(SEQS, 4, 2, BF16, causal), run(SEQS, 4, 2, BF16, causal, edit=poison)
    assert torch.isfinite(dirty[0]).all()
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[1], clean[1])


@pytest.mark.gpu
def test_mla_prefill_split_key_and_strided_views_are_bit_identical():
    def concatenated(args):  # one RoPE stream (head 0's) for every head, expanded and concatenated
        k = args["k"]
        return dict(k=torch.cat([k[..., :128], k[:, :1, 128:].expand(-1, k.size(1), -1)], -1))

    def split(args):  # the same key as k_pe= with a singleton head axis
        return dict(k=args["k"][..., :128].contiguous(), k_pe=args["k"][:, :1, 128:].contiguous())

    def views(args):  # v: the upper half of a [total_k, Hkv, 256] buffer; q: a transposed [Hq, total_q, 192]
        buf = torch.cat([torch.full_like(args["v"], float("nan")), args["v"]], -1)
        return dict(v=buf[..., 128:], q=args["q"].transpose(0, 1).contiguous().transpose(0, 1))

    cat, two = run(SEQS, 4, 2, F16, True, edit=concatenated), run(SEQS, 4, 2, F16, True, edit=split)
    assert torch.equal(two[0], cat[0]) and torch.equal(two[1], cat[1])
    plain, viewed = run(SEQS, 4, 2, F16, True), run(SEQS, 4, 2, F16, True, edit=views)
    assert torch.equal(viewed[0], plain[0]) and torch.equal(viewed[1], plain[1])


@pytest.mark.gpu
@pytest.mark.parametrize("zero", ["rope", "v"])
def test_mla_prefill_column_ranges(zero):
    """rope columns of k zeroed: the reference's result with them zeroed (they enter the score); v zero: out == 0
    while the LSE still matches (no key column reaches the output)."""
    out, lse = run(SEQS, 4, 2, BF16, True, zero=zero)
    check(out, lse, *reference(SEQS, 4, 2, BF16, True, zero), BF16, f"mla prefill zero {zero}")
    assert zero != "v" or (out == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_mla_prefill_chunks_merge_to_the_single_causal_call(dtype):
    """300 keys, the last 100 queries: causal over keys 200..299 plus non-causal over keys 0..199, merged."""
    from flash_attention_cute_amd import flash_attn_merge_states

    cu = lambda n: torch.tensor([0, n], dtype=torch.int32, device="cuda")  # noqa: E731
    new = run(CHUNK, 4, 2, dtype, True, edit=lambda a: dict(k=a["k"][200:], v=a["v"][200:], cu_seqlens_k=cu(100)))
    ctx = run(CHUNK, 4, 2, dtype, False, edit=lambda a: dict(k=a["k"][:200], v=a["v"][:200], cu_seqlens_k=cu(200)))
    out, lse = flash_attn_merge_states([new[0], ctx[0]], [new[1], ctx[1]], return_lse=True)
    check(out, lse, *reference(CHUNK, 4, 2, dtype, True), dtype, f"mla prefill chunked {dtype}")


# ------------------------------------------------------------------------------------------- CPU
def test_mla_prefill_op_schema_fake_and_opcheck():
    import flash_attention_cute_amd as m

    assert "flash_attn_mla_prefill_func" in m.__all__ and "flash_attention_mla_prefill_forward" in m.__all__
    assert str(torch.ops.flash_attention.mla_prefill_forward.default._schema) == (
        "flash_attention::mla_prefill_forward(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, "
        "SymInt max_seqlen_q, float softmax_scale, bool causal=True, Tensor? k_pe=None) -> (Tensor, Tensor)")
    q, k, v, cq, ck = make_inputs(SMALL, 4, 2, BF16)
    with torch._subclasses.FakeTensorMode() as mode:
        o, lse = torch.ops.flash_attention.mla_prefill_forward(*(mode.from_tensor(t) for t in (q, k, v, cq, ck)), 70, SCALE)
    assert o.shape == (q.size(0), 4, 128) and o.dtype == BF16 and lse.shape == (4, q.size(0)) and lse.dtype == torch.float32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.library.opcheck(torch.ops.flash_attention.mla_prefill_forward.default,
                              (q.float(), k[..., :128].float(), v.float(), cq, ck, 70, SCALE, True, k[:, :1, 128:].float()),
                              test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_mla_prefill_cpu_default_matches_float64(causal):
    from flash_attention_cute_amd import flash_attn_mla_prefill_func

    q, k, v, cq, ck = make_inputs(SEQS, 4, 2, F16)
    with pytest.warns(UserWarning, match="fallback to pytorch"):
        out, lse = flash_attn_mla_prefill_func(q.float(), k.float(), v.float(), cq, ck, 257, 300, SCALE, causal=causal,
                                               return_lse=True)
    ref, ref_lse = reference(SEQS, 4, 2, F16, causal)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    torch.testing.assert_close(out.double(), ref, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(lse.double(), ref_lse, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("kwargs,exc", [
    (dict(softmax_scale=None), TypeError), (dict(q=torch.zeros(3, 4, 128, dtype=F16), k=torch.zeros(5, 2, 128, dtype=F16)),
                                            NotImplementedError),
    (dict(v=torch.zeros(5, 2, 192, dtype=F16)), NotImplementedError), (dict(q=torch.zeros(3, 192, dtype=F16)), ValueError),
    (dict(v=torch.zeros(5, 2, 128, dtype=BF16)), ValueError), (dict(q=torch.zeros(3, 3, 192, dtype=F16)), ValueError),
    (dict(k=torch.zeros(5, 2, 128, dtype=F16)), ValueError)],
    ids=["no-scale", "qk-width", "v-width", "rank", "dtype", "heads", "k-width-without-k_pe"])
def test_mla_prefill_wrapper_errors(kwargs, exc):
    from flash_attention_cute_amd import flash_attn_mla_prefill_func

    cu = torch.tensor([0, 3], dtype=torch.int32)
    args = dict(q=torch.zeros(3, 4, 192, dtype=F16), k=torch.zeros(5, 2, 192, dtype=F16),
                v=torch.zeros(5, 2, 128, dtype=F16), cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=3,
                max_seqlen_k=3, softmax_scale=SCALE)
    with pytest.raises(exc):
        flash_attn_mla_prefill_func(**{**args, **kwargs})


class FaMlaPrefillParams(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_void_p) for n in ("q_ptr", "k_nope_ptr", "k_rope_ptr", "v_ptr", "o_ptr", "lse_ptr",
                                                "cu_seqlens_q", "cu_seqlens_k")] +
                [(n, ctypes.c_int64) for n in (
                    "batch_size", "total_q", "total_k", "max_seqlen_q", "num_heads_q", "num_heads_kv", "headdim_qk",
                    "headdim_v", "q_row_stride", "q_head_stride", "k_nope_row_stride", "k_nope_head_stride",
                    "k_rope_row_stride", "k_rope_head_stride", "v_row_stride", "v_head_stride", "o_row_stride",
                    "o_head_stride", "lse_head_stride", "lse_row_stride")] +
                [("softmax_scale", ctypes.c_float), ("causal", ctypes.c_int32)])


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    return lib


def test_mla_prefill_header_functions_are_exported(lib):
    header = (LIB.parent.parent.parent / "include" / "fa_gfx950_mla_prefill.h").read_text()
    for name in ("fa_mla_prefill_gfx950", "fa_mla_prefill_gfx950_check", "fa_mla_prefill_version"):
        assert f"{name}(" in header and hasattr(lib, name)
    assert lib.fa_mla_prefill_version() == 1


@pytest.mark.parametrize("kw,code,field", [
    ({}, FA_OK, ""), (dict(headdim_qk=128), FA_ERR_UNSUPPORTED, "headdim_qk"),
    (dict(headdim_v=192), FA_ERR_UNSUPPORTED, "headdim_v"),
    (dict(k_rope_ptr=0x200108), FA_ERR_INVALID_ARGUMENT, "k_rope_ptr"),
    (dict(v_ptr=0x300004), FA_ERR_INVALID_ARGUMENT, "v_ptr"),
    (dict(v_row_stride=4 * 256 + 4), FA_ERR_INVALID_ARGUMENT, "v_row_stride"),
    (dict(k_rope_row_stride=32), FA_ERR_INVALID_ARGUMENT, "k_rope_row_stride"),
    (dict(num_heads_q=6), FA_ERR_INVALID_ARGUMENT, "num_heads_kv"),
    (dict(cu_seqlens_k=None), FA_ERR_INVALID_ARGUMENT, "cu_seqlens_k"),
    (dict(softmax_scale=float("inf")), FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    (dict(softmax_scale=float("nan")), FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    (dict(softmax_scale=0.0), FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    (dict(softmax_scale=-0.1), FA_ERR_INVALID_ARGUMENT, "softmax_scale")],
    ids=["ok", "dqk-128", "dv-192", "rope-base-8", "v-base-4", "stride-not-8", "rope-stride-narrow", "heads-6-over-4",
         "cu-null", "scale-inf", "scale-nan", "scale-0", "scale-negative"])
def test_mla_prefill_check_codes(lib, kw, code, field):
    """Host-only: the check reads no device memory, and the launch entry returns the same code before any launch.
    The good block is the split key: a RoPE stream [total_k, 1, 64] (head stride 0), v the half of a 256-wide buffer."""
    p = FaMlaPrefillParams(0x100000, 0x200000, 0x200100, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000,
                           2, 100, 300, 64, 8, 4, 192, 128, 8 * 192, 192, 4 * 128, 128, 64, 0, 4 * 256, 256, 8 * 128, 128,
                           100, 1, 0.1, 1)
    for key, val in kw.items():
        setattr(p, key, val)
    assert lib.fa_mla_prefill_gfx950_check(ctypes.byref(p), 1) == code
    if code != FA_OK:
        assert field in lib.fa_last_error().decode()
        assert lib.fa_mla_prefill_gfx950(ctypes.byref(p), 1, None) == code
    assert lib.fa_mla_prefill_gfx950_check(None, 1) == FA_ERR_INVALID_ARGUMENT
