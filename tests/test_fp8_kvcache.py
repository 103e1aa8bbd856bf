"""FP8 (OCP e4m3, ``torch.float8_e4m3fn``) KV cache: the quantizing in-place append and the paged decode
that reads the 8-bit pool in place (include/fa_gfx950_fp8.h). No reference counterpart.

Read: ``out = v_descale[b,h] * softmax((softmax_scale * k_descale[b,h]) * q . T(K8)^T) . T(V8)`` with T the
exact widening of a byte to the query dtype. Every e4m3 value is exact in fp16 and bf16, so after the
widening the arithmetic is the 16-bit decode kernel's: the yardstick is ``oracle_padded`` on ``K8.to(T)``,
``V8.to(T)`` with the scales folded, within the project's own bar (tests/test_gpu_parity.py TOL: fp16
2e-3 + 2e-3|ref|, bf16 1.6e-2 + 1.6e-2|ref|) -- a derived tolerance, not a new one. Per-(b, h) descales are
distinct powers of two, so folding them into the oracle's K / V inputs is exact; one case per dtype uses
the non-power-of-two pair (0.37, 1.9), folded into the oracle's softmax_scale and onto its result.

Write: ``byte = e4m3_rne(clamp(fp32(x) / descale[b,h], -448, 448))``, x the rotated key already rounded to
the input dtype (V: the input). Compared as BYTES over the WHOLE pool (0x00 and 0x80 count as equal: the
kernels are built with -fno-signed-zeros), so any other row touched shows.

Every pool byte that holds no key is 0x7F (e4m3 NaN), every unused table entry -1, every table shuffled.
"""
from __future__ import annotations

import functools
import warnings

import pytest
import torch

from test_kvcache import expected_append, new_tokens, rope_tables, targets
from test_padded import check_padded, oracle_padded
from test_paged import KINDS, make_paged

F16, BF16 = torch.float16, torch.bfloat16
FP8 = torch.float8_e4m3fn
NAN_BYTE = 0x7F


def pow2_descales(b, hkv, shift=0):
    """Distinct powers of two 2^-3 .. 2^2 per (b, h) (cyclic beyond six), fp32 [B, Hkv]."""
    e = (torch.arange(b * hkv).reshape(b, hkv) + shift) % 6 - 3
    return torch.pow(2.0, e.float())


def quant(x, descale):
    """The write formula on the host."""
    return (x.float() / descale).clamp(-448.0, 448.0).to(FP8)


def norm_bytes(t):
    """The bytes of an fp8 tensor with -0 folded onto +0."""
    u = t.contiguous().view(torch.uint8).clone()
    u[u == 0x80] = 0
    return u


def empty_pool(num_pages, hkv, page, d, layout):
    shape = (num_pages, page, hkv, d) if layout == "pshd" else (num_pages, hkv, page, d)
    pool = torch.full(shape, NAN_BYTE, dtype=torch.uint8).view(FP8)
    return pool.transpose(1, 2) if layout == "pshd" else pool


def make_fp8_paged(lens, hq, hkv, sq, page, cap, d, dtype, seed, layout="phsd", kd=None, vd=None):
    """test_paged.make_paged's q, dense keys and shuffled table, the keys quantized per (b, h) and scattered
    into 0x7F-poisoned byte pools. Returns q, the dense quantized K8 / V8 [B, Hkv, cap, D], the pools, the
    table and the lengths."""
    q, k, v, kc, _, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, dtype, seed, layout)
    b = len(lens)
    kd = torch.ones(b, hkv) if kd is None else kd
    vd = torch.ones(b, hkv) if vd is None else vd
    k8, v8 = quant(k, kd[:, :, None, None]), quant(v, vd[:, :, None, None])
    kc8, vc8 = (empty_pool(kc.size(0), hkv, page, d, layout) for _ in range(2))
    for i, n in enumerate(lens):
        for j in range((n + page - 1) // page):
            pg, n0 = int(table[i, j]), j * page
            rows = min(n, n0 + page) - n0
            kc8[pg, :, :rows] = k8[i, :, n0:n0 + rows]
            vc8[pg, :, :rows] = v8[i, :, n0:n0 + rows]
    return q, k8, v8, kc8, vc8, table, sl


def fp8_oracle(q, k8, v8, sl, kd, vd, causal, scale=None, pow2=True):
    """oracle_padded on the widened bytes with the scales folded: into K / V when they are powers of two
    (exact), else (uniform scalars) into softmax_scale and onto the result."""
    dtype, d = q.dtype, q.size(-1)
    scale = d ** -0.5 if scale is None else scale
    zero = torch.zeros_like(sl)
    if pow2:
        return oracle_padded(q, k8.to(dtype) * kd[:, :, None, None].to(dtype), v8.to(dtype) * vd[:, :, None, None].to(dtype),
                             zero, sl, None, None, scale, causal).float()
    return oracle_padded(q, k8.to(dtype), v8.to(dtype), zero, sl, None, None, scale * float(kd), causal).float() * float(vd)


# ------------------------------------------------------------------------------------------- CPU
def test_fp8_op_registration():
    import flash_attention_cute_amd  # noqa: F401

    sch = str(torch.ops.flash_attention.paged_forward_fp8.default._schema)
    assert sch == ("flash_attention::paged_forward_fp8(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, "
                   "Tensor cache_seqlens, Tensor? k_descale=None, Tensor? v_descale=None, float softmax_scale=None, "
                   "bool causal=False) -> Tensor")
    sch = str(torch.ops.flash_attention.kvcache_append_fp8.default._schema)
    assert sch == ("flash_attention::kvcache_append_fp8(Tensor(a0!) k_cache, Tensor(a1!) v_cache, Tensor? k, Tensor? v, "
                   "Tensor cache_seqlens, Tensor? block_table=None, Tensor? q=None, Tensor? rotary_cos=None, "
                   "Tensor? rotary_sin=None, Tensor? k_descale=None, Tensor? v_descale=None) -> (Tensor, Tensor)")
    # the 16-bit ops' schemas did not move
    assert "descale" not in str(torch.ops.flash_attention.paged_forward.default._schema)
    assert "descale" not in str(torch.ops.flash_attention.kvcache_append.default._schema)
    kd, vd = pow2_descales(2, 2), pow2_descales(2, 2, 1)
    q, _, _, kc8, vc8, table, sl = make_fp8_paged((40, 7), 4, 2, 2, 32, 64, 32, F16, 1, kd=kd, vd=vd)
    kc8, vc8 = (torch.where(c.view(torch.uint8) == NAN_BYTE, 0, c.view(torch.uint8)).view(FP8) for c in (kc8, vc8))
    k, v, qn = (new_tokens(2, h, 2, 32, F16, 2 + i) for i, h in enumerate((2, 2, 4)))
    cos, sin = rope_tables(64, 32, F16)
    read, append = torch.ops.flash_attention.paged_forward_fp8.default, torch.ops.flash_attention.kvcache_append_fp8.default
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.library.opcheck(read, (q, kc8, vc8, table, sl, kd, vd, 0.125, True), test_utils=("test_faketensor",))
        schema_holds(read, (q, kc8, vc8, table, sl, kd, vd, 0.125, True), mutated=())
        for args in ((kc8, vc8, k, v, sl, table, qn, cos, sin, kd, vd), (kc8, vc8, k, v, sl, table),
                     (kc8, vc8, None, None, sl, table, qn, cos, sin)):
            torch.library.opcheck(append, args, test_utils=("test_faketensor",))
            schema_holds(append, args, mutated=(0, 1) if args[2] is not None else ())


def schema_holds(op, args, mutated):
    """opcheck's "test_schema" by hand: torch's SchemaCheckMode compares every input with torch.allclose,
    which is not implemented for float8 tensors on the CPU, so it cannot run on these ops. The same
    properties on byte views: exactly the arguments the schema marks as written change, the others keep
    their bits, and no output aliases an input."""
    for i, a in enumerate(op._schema.arguments):
        assert (a.alias_info is not None and a.alias_info.is_write) == (i in (0, 1) and "append" in op._schema.name)
    args = [a.clone() if isinstance(a, torch.Tensor) else a for a in args]
    as_bytes = lambda t: t.contiguous().view(torch.uint8).clone()  # noqa: E731
    before = [as_bytes(a) if isinstance(a, torch.Tensor) else None for a in args]
    out = op(*args)
    for i, (a, b0) in enumerate(zip(args, before)):
        if b0 is not None:
            assert torch.equal(as_bytes(a), b0) == (i not in mutated), (op._schema.name, i)
    ptrs = {a.untyped_storage().data_ptr() for a in args if isinstance(a, torch.Tensor)}
    for o in (out if isinstance(out, tuple) else (out,)):
        assert o.numel() == 0 or o.untyped_storage().data_ptr() not in ptrs


def test_fp8_ops_are_exported_like_the_other_extras():
    import flash_attention
    import flash_attention.flash_attention as ref_mod
    import flash_attention_cute_amd as m

    for name in ("flash_attention_paged_forward_fp8", "flash_attention_kvcache_append_fp8"):
        assert getattr(m, name) is getattr(flash_attention, name) is getattr(ref_mod, name)
        assert name in m.__all__


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("sq", [1, 3])
@pytest.mark.parametrize("layout", ["phsd", "pshd"])
def test_fp8_read_cpu_default_matches_oracle(causal, sq, layout):
    from flash_attention_cute_amd import flash_attn_paged_func

    lens, hq, hkv, page, cap, d = (96, 0, 33, 1, 64), 4, 2, 32, 96, 64
    kd, vd = pow2_descales(len(lens), hkv), pow2_descales(len(lens), hkv, 2)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, sq, page, cap, d, F16, 3, layout, kd, vd)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = flash_attn_paged_func(q, kc8, vc8, table, sl, causal=causal, k_descale=kd, v_descale=vd)
    assert out.dtype == F16 and torch.isfinite(out).all()
    ref = fp8_oracle(q, k8, v8, sl, kd, vd, causal)
    torch.testing.assert_close(out.float(), ref, atol=3e-3, rtol=3e-3)
    assert (out[1] == 0).all()  # a sequence without keys


def special_values(x, descale):
    """Plant saturating inputs (|x| > 448 descale) and exact RNE ties (17/16 -> 16/16, 19/16 -> 20/16 of a
    power of two) in the first elements of every row; descale broadcasts as [B, H, 1]."""
    x = x.clone()
    s = descale.to(x.dtype)
    x[..., 0] = (17 / 16) * s
    x[..., 1] = (19 / 16) * s
    x[..., 2] = 1000.0 * s
    x[..., 3] = -1000.0 * s
    x[..., 4] = -(17 / 16) * 4 * s
    x[..., 5] = 448.0 * s
    return x


def make_fp8_cache(lens, sn, hkv, page, cap, d, seed, layout="phsd", dense=False):
    """Byte pools (0x7F everywhere: every row is compared) and the shuffled table of the lengths after the
    append; dense: [B, Hkv, cap, D] and no table."""
    sl = torch.tensor(lens, dtype=torch.int32)
    if dense:
        kc, vc = (torch.full((len(lens), hkv, cap, d), NAN_BYTE, dtype=torch.uint8).view(FP8) for _ in range(2))
        return kc, vc, None, sl
    after = tuple(min(max(n, 0) + sn, cap) for n in lens)
    _, _, _, kc, _, table, _ = make_paged(after, hkv, hkv, 1, page, cap, d, F16, seed, layout)
    kc8, vc8 = (empty_pool(kc.size(0), hkv, page, d, layout) for _ in range(2))
    return kc8, vc8, table, sl


def expected_fp8_append(kc8, vc8, k_new, v_new, lens, table, cos, sin, apply_rope, kd, vd):
    """The hand-written loop: test_kvcache.expected_append on 16-bit scratch pools gives the rotated,
    rounded keys and their places; the rows it wrote are quantized with their sequence's descales."""
    num_pages, _, page, _ = kc8.shape
    cap = page * (table.size(1) if table is not None else 1)
    z = torch.zeros(kc8.shape, dtype=k_new.dtype, device=k_new.device)
    ek16, ev16 = expected_append(z, z.clone(), k_new, v_new, lens, table, cos, sin, apply_rope)
    ek, ev = kc8.clone(), vc8.clone()
    for b, _, pg, row in targets(lens, k_new.size(2), table, page, cap, num_pages):
        ek[pg, :, row] = quant(ek16[pg, :, row], kd[b].to(k_new.device)[:, None])
        ev[pg, :, row] = quant(ev16[pg, :, row], vd[b].to(k_new.device)[:, None])
    return ek, ev


APPEND_KINDS = {  # name -> (lens, dense, table edit)
    "plain": ((0, 31, 60), False, None),
    "bad_page_id": ((0, 31, 60), False, "bad"),
    "at_capacity": ((62, 64, 0), False, None),
    "dense": ((0, 31, 62), True, None),
}


def append_case(kind, rope, dtype, d, sn, layout, seed, pow2=True):
    lens, dense, edit = APPEND_KINDS[kind]
    b, hkv, page, cap = len(lens), 2, 32, 64
    kc8, vc8, table, sl = make_fp8_cache(lens, sn, hkv, page, cap, d, seed, layout, dense)
    if edit == "bad":  # the page the first new token of sequences 1 and 2 lands in: outside the pool
        table[1, lens[1] // page] = -1
        table[2, lens[2] // page] = 2 ** 31 - 1
    kd = pow2_descales(b, hkv) if pow2 else torch.full((b, hkv), 0.37)
    vd = pow2_descales(b, hkv, 3) if pow2 else torch.full((b, hkv), 1.9)
    k = special_values(new_tokens(b, hkv, sn, d, dtype, seed + 1), kd[:, :, None])
    v = special_values(new_tokens(b, hkv, sn, d, dtype, seed + 2), vd[:, :, None])
    cos, sin = rope_tables(cap, d, dtype) if rope else (None, None)
    return kc8, vc8, table, sl, k, v, cos, sin, kd, vd


@pytest.mark.parametrize("rope", [False, True], ids=["norope", "rope"])
@pytest.mark.parametrize("kind", list(APPEND_KINDS))
def test_fp8_append_cpu_default_equals_the_hand_written_loop(kind, rope):
    from flash_attention_cute_amd import flash_attn_kvcache_append
    from flash_attention_cute_amd.flash_attention import _rope_reference

    kc8, vc8, table, sl, k, v, cos, sin, kd, vd = append_case(kind, rope, F16, 32, 3, "phsd", 11)
    ek, ev = expected_fp8_append(kc8, vc8, k, v, sl.tolist(), table, cos, sin, _rope_reference, kd, vd)
    new = flash_attn_kvcache_append(kc8, vc8, k, v, sl, table, cos, sin, k_descale=kd, v_descale=vd)
    cap = 64
    assert new.tolist() == [min(n + 3, cap) for n in sl.tolist()]
    assert torch.equal(norm_bytes(kc8), norm_bytes(ek)) and torch.equal(norm_bytes(vc8), norm_bytes(ev))
    # the planted values: ties to even and saturation, in V (never rotated) of a written row
    t = targets(sl.tolist(), 3, table, 32, cap, kc8.size(0))
    assert t
    b, _, pg, row = t[0]
    got = vc8[pg, :, row].float()
    assert got[:, :6].tolist() == [[1.0, 1.25, 448.0, -448.0, -4.0, 448.0]] * 2
    if kind != "plain":  # something was dropped: fewer rows written than tokens
        assert len(t) < 3 * len(sl)


def test_fp8_wrapper_errors():
    from flash_attention_cute_amd import flash_attn_kvcache_append, flash_attn_paged_func, flash_attn_with_kvcache

    q, _, _, kc8, vc8, table, sl = make_fp8_paged((40, 7), 4, 2, 1, 32, 64, 32, F16, 1)
    k16 = torch.zeros(kc8.shape, dtype=F16)
    for other in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        bad = kc8.view(torch.uint8).view(other)
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            flash_attn_paged_func(q, bad, bad, table, sl)
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            flash_attn_kvcache_append(bad, bad, None, None, sl, table)
    with pytest.raises(ValueError, match="same data type"):
        flash_attn_paged_func(q, kc8, k16, table, sl)
    with pytest.raises(ValueError, match="same data type"):
        flash_attn_with_kvcache(q, k16, vc8, cache_seqlens=sl, block_table=table)
    with pytest.raises(ValueError, match="descale"):
        flash_attn_paged_func(q, k16, k16, table, sl, k_descale=0.5)
    with pytest.raises(ValueError, match="descale"):
        flash_attn_kvcache_append(k16, k16, None, None, sl, table, v_descale=torch.ones(2, 2))
    with pytest.raises(ValueError, match="k_descale"):
        flash_attn_paged_func(q, kc8, vc8, table, sl, k_descale=torch.ones(2, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"v_descale must be \[batch, kv heads\]"):
        flash_attn_paged_func(q, kc8, vc8, table, sl, v_descale=torch.ones(3, 5))
    dense = torch.zeros(2, 2, 48, 32, dtype=torch.uint8).view(FP8)  # 48 keys: no multiple of 32
    with pytest.raises(ValueError, match="multiple of 32"):
        flash_attn_with_kvcache(q, dense, dense, cache_seqlens=sl)
    # a Python float is accepted and expanded
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = flash_attn_paged_func(q, kc8, vc8, table, sl, k_descale=0.5, v_descale=2.0)
        b = flash_attn_paged_func(q, kc8, vc8, table, sl, k_descale=torch.full((2, 2), 0.5), v_descale=torch.full((2, 2), 2.0))
    assert torch.equal(a, b)


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


# (kind, page_size, D, dtype, pool layout, lengths, descales): test_paged's kinds; every page size with every
# kind, D 64 / 96 (a tile not filled) / 128, both dtypes, both stride orders, lengths 0, 1, 31, 32, 33, exactly
# one page, one key past a page and full capacity. descales "pow2": distinct powers of two per (b, h);
# "uniform": the scalars (0.37, 1.9).
CASES = [
    ("unsplit", 32, 128, F16, "phsd", (0, 1, 31), "pow2"),
    ("unsplit", 32, 64, BF16, "pshd", (32, 33, 256), "pow2"),
    ("unsplit", 64, 96, F16, "pshd", (64, 65, 33), "uniform"),
    ("unsplit", 64, 128, BF16, "phsd", (31, 256, 0), "uniform"),
    ("unsplit", 256, 64, F16, "phsd", (256, 1, 32), "pow2"),
    ("unsplit", 256, 96, BF16, "pshd", (33, 0, 255), "pow2"),
    ("split", 32, 128, BF16, "phsd", (2048, 33), "pow2"),
    ("split", 64, 64, F16, "pshd", (65, 2047), "pow2"),
    ("split", 256, 128, F16, "pshd", (257, 2048), "pow2"),
    ("split", 256, 96, BF16, "phsd", (256, 0), "pow2"),
    ("split_unfused", 32, 96, F16, "phsd", (32, 1999), "pow2"),
    ("split_unfused", 64, 128, BF16, "pshd", (2048, 1), "pow2"),
    ("split_unfused", 256, 64, F16, "phsd", (257, 31), "pow2"),
    ("sq3_causal", 32, 128, F16, "pshd", (0, 1, 33), "pow2"),
    ("sq3_causal", 64, 96, BF16, "phsd", (64, 65, 256), "pow2"),
    ("sq3_causal", 256, 64, BF16, "pshd", (2, 256, 32), "pow2"),
    ("g8_sq5", 32, 64, F16, "phsd", (31, 32, 256), "pow2"),
    ("g8_sq5", 64, 128, BF16, "pshd", (5, 65, 0), "pow2"),
    ("g8_sq5", 256, 96, F16, "phsd", (256, 4, 33), "pow2"),
]
CASE_IDS = [f"{k}-p{p}-d{d}-{'f16' if t == F16 else 'bf16'}-{lay}-{ds}" for k, p, d, t, lay, _, ds in CASES]


@functools.lru_cache(maxsize=None)
def run_case(ci):
    """One FP8 paged launch and its oracle, computed once per case (never modified)."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    kind, page, d, dtype, layout, lens, ds = CASES[ci]
    b, hq, hkv, sq, cap, causal = KINDS[kind]
    pow2 = ds == "pow2"
    kd = pow2_descales(b, hkv) if pow2 else torch.full((b, hkv), 0.37)
    vd = pow2_descales(b, hkv, 2) if pow2 else torch.full((b, hkv), 1.9)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, sq, page, cap, d, dtype, 300 + ci, layout, kd, vd)
    dev = torch.device("cuda:0")
    _debug.set_knobs()
    _debug.set_dec_fuse(0 if kind == "split_unfused" else None)
    try:
        out = flash_attn_paged_func(q.to(dev), kc8.to(dev), vc8.to(dev), table.to(dev), sl.to(dev), causal=causal,
                                    k_descale=kd.to(dev), v_descale=vd.to(dev))
        path, fused = _debug.last_path(), _debug.last_dec_fused()
        torch.cuda.synchronize()
    finally:
        _debug.set_dec_fuse(None)
    ref = fp8_oracle(q, k8, v8, sl, kd if pow2 else 0.37, vd if pow2 else 1.9, causal, pow2=pow2)
    return out.cpu(), ref, path, fused


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_fp8_paged_decode_matches_the_oracle(ops, ci):
    kind, _, _, dtype, _, lens, _ = CASES[ci]
    out, ref, path, fused = run_case(ci)
    split = kind.startswith("split")
    assert path == ("decode_paged_fp8_split" if split else "decode_paged_fp8")
    if split:
        assert fused == (kind == "split")
    assert out.dtype == dtype and torch.isfinite(out.float()).all()
    for i, n in enumerate(lens):
        if n == 0:
            assert (out[i] == 0).all()
    check_padded(out, ref, dtype)


@pytest.mark.gpu
def test_fp8_paged_large_query_block_takes_the_copying_path(ops, device):
    """g * Sq = 4 * 17 = 68 rows: past the decode rule, the pages are gathered, widened and scaled for the
    padded entry (K is rounded once more: power-of-two descales keep that exact)."""
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    lens, hq, hkv, sq, page, cap, d = (100, 17, 64), 8, 2, 17, 32, 128, 64
    kd, vd = pow2_descales(3, hkv), pow2_descales(3, hkv, 1)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, sq, page, cap, d, F16, 401, "phsd", kd, vd)
    out = flash_attn_paged_func(*(t.to(device) for t in (q, kc8, vc8, table, sl)), causal=True,
                                k_descale=kd.to(device), v_descale=vd.to(device))
    assert not _debug.last_path().startswith("decode_paged")
    check_padded(out, fp8_oracle(q, k8, v8, sl, kd, vd, True), F16)


@pytest.mark.gpu
def test_fp8_paged_stride0_descale_and_float_descale(ops, device):
    from flash_attention_cute_amd import flash_attn_paged_func

    lens, hq, hkv, page, cap, d = (70, 33, 1), 8, 2, 32, 128, 128
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, hq, hkv, 1, page, cap, d, BF16, 402, "pshd",
                                                     torch.full((3, hkv), 0.5), torch.full((3, hkv), 4.0))
    args = [t.to(device) for t in (q, kc8, vc8, table, sl)]
    kd = torch.full((1, 1), 0.5, device=device).expand(3, hkv)
    vd = torch.full((1, 1), 4.0, device=device).expand(3, hkv)
    assert kd.stride() == (0, 0)
    out = flash_attn_paged_func(*args, k_descale=kd, v_descale=vd)
    check_padded(out, fp8_oracle(q, k8, v8, sl, torch.full((3, hkv), 0.5), torch.full((3, hkv), 4.0), False), BF16)
    assert torch.equal(out, flash_attn_paged_func(*args, k_descale=0.5, v_descale=4.0))
    # None is 1.0
    ones = torch.ones(3, hkv, device=device)
    assert torch.equal(flash_attn_paged_func(*args), flash_attn_paged_func(*args, k_descale=ones, v_descale=ones))


APPEND_GPU = [  # (kind, rope, dtype, D, Sn, layout, pow2)
    ("plain", True, F16, 128, 3, "phsd", True),
    ("plain", False, BF16, 64, 1, "pshd", True),
    ("plain", True, BF16, 96, 3, "pshd", False),
    ("plain", False, F16, 96, 1, "phsd", False),
    ("bad_page_id", True, BF16, 128, 3, "phsd", True),
    ("bad_page_id", False, F16, 64, 1, "pshd", True),
    ("at_capacity", True, F16, 64, 3, "pshd", True),
    ("at_capacity", False, BF16, 128, 3, "phsd", True),
    ("dense", True, BF16, 64, 3, "phsd", True),
    ("dense", False, F16, 128, 1, "phsd", True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", APPEND_GPU, ids=[f"{c[0]}-{'rope' if c[1] else 'norope'}-{'f16' if c[2] == F16 else 'bf16'}"
                                                  f"-d{c[3]}-sn{c[4]}-{c[5]}-{'pow2' if c[6] else 'np2'}" for c in APPEND_GPU])
def test_fp8_append_writes_the_formula_bit_for_bit(ops, device, case):
    from flash_attention_cute_amd import apply_rope

    kind, rope, dtype, d, sn, layout, pow2 = case
    kc8, vc8, table, sl, k, v, cos, sin, kd, vd = append_case(kind, rope, dtype, d, sn, layout, 500 + d + sn, pow2)
    dv = lambda t: None if t is None else t.to(device)  # noqa: E731
    gk, gv = dv(kc8), dv(vc8)
    ek, ev = expected_fp8_append(gk, gv, dv(k), dv(v), sl.tolist(), table, dv(cos), dv(sin), apply_rope, kd, vd)
    hq = 4
    q = new_tokens(len(sl), hq, 2, d, dtype, 7) if rope else None
    new, q_rot = torch.ops.flash_attention.kvcache_append_fp8(gk, gv, dv(k), dv(v), dv(sl), dv(table), dv(q), dv(cos),
                                                              dv(sin), dv(kd), dv(vd))
    torch.cuda.synchronize()
    cap = 64
    assert new.tolist() == [min(n + sn, cap) for n in sl.tolist()]
    assert torch.equal(norm_bytes(gk.cpu()), norm_bytes(ek.cpu())), "K pool"
    assert torch.equal(norm_bytes(gv.cpu()), norm_bytes(ev.cpu())), "V pool"
    if rope:  # q_rot is the 16-bit append's, bit for bit
        k16 = torch.zeros(kc8.shape, dtype=dtype, device=device)
        _, q16 = torch.ops.flash_attention.kvcache_append(k16, k16.clone(), dv(k), dv(v), dv(sl), dv(table), dv(q),
                                                          dv(cos), dv(sin))
        assert q_rot.dtype == dtype and torch.equal(q_rot.view(torch.int16), q16.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True], ids=["paged", "dense"])
def test_fp8_four_decode_steps_end_to_end(ops, device, dense):
    from flash_attention_cute_amd import flash_attn_with_kvcache

    b, hq, hkv, d, page, cap, dtype, lens, steps = 3, 8, 2, 128, 32, 128, BF16, (0, 31, 60), 4
    kd, vd = pow2_descales(b, hkv), pow2_descales(b, hkv, 1)
    kc8, vc8, table, sl = make_fp8_cache(lens, steps, hkv, page, cap, d, 600, dense=dense)
    cos, sin = rope_tables(cap, d, dtype)
    # history before the first step: quantized random keys, written through the op itself would hide a bug
    # shared by append and reference, so they are placed by hand
    g = torch.Generator().manual_seed(601)
    hist_k = quant(torch.randn(b, hkv, cap, d, generator=g).to(dtype), kd[:, :, None, None])
    hist_v = quant(torch.randn(b, hkv, cap, d, generator=g).to(dtype), vd[:, :, None, None])
    for i, n in enumerate(lens):
        for n_ in range(n):
            pg, row = (i, n_) if dense else (int(table[i, n_ // page]), n_ % page)
            kc8[pg, :, row], vc8[pg, :, row] = hist_k[i, :, n_], hist_v[i, :, n_]
    toks = [[new_tokens(b, h, 1, d, dtype, 610 + 3 * s + i) for i, h in enumerate((hq, hkv, hkv))] for s in range(steps)]
    # the reference loop starts from the same history
    ref_outs = []
    k8, v8, cur = hist_k.clone(), hist_v.clone(), list(lens)
    for i, n in enumerate(lens):
        k8[i, :, n:], v8[i, :, n:] = 0, 0
    from flash_attention_cute_amd import apply_rope
    for s in range(steps):
        q, k, v = toks[s]
        pos = torch.tensor([[n] for n in cur], device=device)
        k_rot = apply_rope(k.to(device), cos.to(device)[pos], sin.to(device)[pos]).cpu()
        q_rot = apply_rope(q.to(device), cos.to(device)[pos], sin.to(device)[pos]).cpu()
        for i, n in enumerate(cur):
            k8[i, :, n] = quant(k_rot[i, :, 0], kd[i][:, None])
            v8[i, :, n] = quant(v[i, :, 0], vd[i][:, None])
        cur = [n + 1 for n in cur]
        ref_outs.append(fp8_oracle(q_rot, k8, v8, torch.tensor(cur, dtype=torch.int32), kd, vd, True))
    dv = lambda t: None if t is None else t.to(device)  # noqa: E731
    gk, gv, gsl, gt = dv(kc8), dv(vc8), dv(sl), dv(table)
    for s in range(steps):
        q, k, v = (dv(t) for t in toks[s])
        out, new = flash_attn_with_kvcache(q, gk, gv, k, v, dv(cos), dv(sin), cache_seqlens=gsl, block_table=gt,
                                           causal=True, return_seqlens=True, k_descale=dv(kd), v_descale=dv(vd))
        gsl = new
        check_padded(out, ref_outs[s], dtype)
    assert gsl.tolist() == [n + steps for n in lens]


@pytest.mark.gpu
def test_fp8_serving_step_graph_capture(ops, device):
    """append + attend + cache_seqlens.copy_(new_seqlens) on an FP8 cache captured once and replayed twice
    with advancing lengths: the pool, the lengths and the outputs of two eager steps from the same start."""
    from flash_attention_cute_amd import flash_attn_with_kvcache

    b, hq, hkv, d, page, cap, dtype, lens, steps = 3, 8, 2, 128, 32, 128, BF16, (30, 31, 63), 2
    kd, vd = pow2_descales(b, hkv).to(device), pow2_descales(b, hkv, 1).to(device)
    kc0, vc0, table, sl0 = make_fp8_cache(lens, steps, hkv, page, cap, d, 700)
    g = torch.Generator().manual_seed(701)
    for c in (kc0, vc0):  # finite history everywhere (the rows below the lengths are read)
        c.view(torch.uint8).copy_(torch.randint(0, 0x78, c.shape, generator=g, dtype=torch.uint8))
    kc0, vc0, table, sl0 = (t.to(device) for t in (kc0, vc0, table, sl0))
    cos, sin = (t.to(device) for t in rope_tables(cap, d, dtype))
    toks = [[new_tokens(b, h, 1, d, dtype, 710 + 3 * s + i).to(device) for i, h in enumerate((hq, hkv, hkv))]
            for s in range(steps)]

    def step(q, k, v, kc, vc, sl):
        out, new = flash_attn_with_kvcache(q, kc, vc, k, v, cos, sin, cache_seqlens=sl, block_table=table,
                                           return_seqlens=True, k_descale=kd, v_descale=vd)
        sl.copy_(new)
        return out

    kc_e, vc_e, sl_e = kc0.clone(), vc0.clone(), sl0.clone()
    eager = [step(q, k, v, kc_e, vc_e, sl_e).clone() for q, k, v in toks]  # (also the warm-up)
    torch.cuda.synchronize()
    kc, vc, sl = kc0.clone(), vc0.clone(), sl0.clone()
    q, k, v = (t.clone() for t in toks[0])
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = step(q, k, v, kc, vc, sl)
    assert torch.equal(kc.view(torch.uint8), kc0.view(torch.uint8)) and sl.tolist() == list(lens)  # captured, not run
    for s in range(steps):
        for dst, src in zip((q, k, v), toks[s]):
            dst.copy_(src)
        gr.replay()
        assert torch.equal(out, eager[s])
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert sl.tolist() == sl_e.tolist() == [n + steps for n in lens]
    assert torch.equal(kc.view(torch.uint8), kc_e.view(torch.uint8))
    assert torch.equal(vc.view(torch.uint8), vc_e.view(torch.uint8))
