"""The ragged step's three public calls without a GPU: the schemas of the two new ops, their fakes, the exports,
and the CPU defaults against the float oracle / a hand-written loop at small shapes."""
from __future__ import annotations

import warnings

import pytest
import torch

from test_kvcache import rope_tables
from test_paged_varlen import Ragged, cu_of, packed_rows, per_sequence_append, ragged_cache

F16, BF16 = torch.float16, torch.bfloat16
NEW = ("flash_attn_paged_varlen_func", "flash_attn_kvcache_append_varlen", "flash_attn_varlen_with_kvcache")


def test_op_schemas():
    import flash_attention_cute_amd  # noqa: F401

    sch = str(torch.ops.flash_attention.paged_varlen_forward.default._schema)
    assert sch == ("flash_attention::paged_varlen_forward(Tensor q, Tensor k_cache, Tensor v_cache, Tensor cu_seqlens_q, "
                   "SymInt max_seqlen_q, Tensor block_table, Tensor cache_seqlens, float softmax_scale=None, "
                   "bool causal=False, SymInt window_left=-1) -> Tensor")
    sch = str(torch.ops.flash_attention.kvcache_append_varlen.default._schema)
    assert sch == ("flash_attention::kvcache_append_varlen(Tensor(a0!) k_cache, Tensor(a1!) v_cache, Tensor k, Tensor v, "
                   "Tensor cu_seqlens_new, Tensor cache_seqlens, Tensor block_table, Tensor? rotary_cos=None, "
                   "Tensor? rotary_sin=None, Tensor? q=None, Tensor? cu_seqlens_q=None) -> (Tensor, Tensor)")


def test_fakes_and_opcheck():
    import flash_attention_cute_amd  # noqa: F401

    c = Ragged(((0, 30), (3, 49), (5, 0), (7, 5)), 4, 2, 64, 128, 16, torch.float32, 1)
    kc, vc = c.kc.nan_to_num(0.0), c.vc.nan_to_num(0.0)
    kc2, vc2, table, sl = ragged_cache((3, 60, 0), (4, 10, 0), 2, 64, 128, 16, torch.float32, 2)
    cu, cuq = cu_of((4, 10, 0)), cu_of((1, 12, 3))
    k, v, q = packed_rows(14, 2, 16, torch.float32, 3), packed_rows(14, 2, 16, torch.float32, 4), packed_rows(16, 4, 16, torch.float32, 5)
    cos, sin = rope_tables(128, 16, torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.library.opcheck(torch.ops.flash_attention.paged_varlen_forward.default,
                              (c.q, kc, vc, c.cu_q, c.max_q, c.table, c.sl, 0.25, True, 3),
                              test_utils=("test_schema", "test_faketensor"))
        for args in ((kc2, vc2, k, v, cu, sl, table, cos, sin, q, cuq), (kc2, vc2, k, v, cu, sl, table)):
            torch.library.opcheck(torch.ops.flash_attention.kvcache_append_varlen.default, args,
                                  test_utils=("test_schema", "test_faketensor"))


def test_new_functions_are_exported_like_the_other_extras():
    import flash_attention
    import flash_attention.flash_attention as ref_mod
    import flash_attention_cute_amd as m

    for name in NEW:
        assert getattr(m, name) is getattr(flash_attention, name) is getattr(ref_mod, name)
        assert name in m.__all__
    for name in ("flash_attention_paged_varlen_forward", "flash_attention_kvcache_append_varlen"):
        assert name in m.__all__ and callable(getattr(m, name))
    assert "256-row block" in m.flash_attn_paged_varlen_func.__doc__.replace("\n   ", "")  # the decode warning
    assert "flash_attn_paged_func" in m.flash_attn_paged_varlen_func.__doc__


# CPU default of the attention against the float oracle: an empty range, Sq_b > L_b (causal: leading rows 0), no
# keys, a sequence that fills its table; with and without a window; both pool layouts
PAIRS = ((0, 30), (1, 49), (5, 0), (7, 5), (20, 128), (9, 65))


@pytest.mark.parametrize("w", [-1, 0, 3, 70])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype,layout", [(F16, "phsd"), (BF16, "pshd")], ids=["f16", "bf16-pshd"])
def test_cpu_default_attention_matches_the_oracle(dtype, layout, causal, w):
    from flash_attention_cute_amd import flash_attn_paged_varlen_func
    from test_padded import check_padded

    c = Ragged(PAIRS, 4, 2, 64, 128, 32, dtype, 11, layout)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = flash_attn_paged_varlen_func(c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl, causal=causal, window_left=w)
    check_padded(out, c.oracle(causal, w), dtype)  # (finite: no NaN row of the pool, no unused entry was read)
    r = c.cu_q.tolist()
    assert (out[r[2]:r[3]] == 0).all()
    if causal:
        assert (out[r[3]:r[3] + 2] == 0).all() and not (out[r[3] + 2] == 0).all()  # 5 keys under 7 queries


def test_cpu_default_clamps_a_bad_cu_seqlens_q():
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    c = Ragged(PAIRS, 4, 2, 64, 128, 32, F16, 12)
    total = c.q.size(0)
    bad = c.cu_q.clone()
    bad[0], bad[-1] = -7, total + 50  # clamped to 0 and total_q: the same ranges
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = flash_attn_paged_varlen_func(c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl, causal=True)
        got = flash_attn_paged_varlen_func(c.q, c.kc, c.vc, bad, c.max_q, c.table, c.sl, causal=True)
    assert torch.equal(got, want)


def test_cpu_default_refuses_what_the_kernel_does_not_read():
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = Ragged(((4, 64), (7, 96)), 4, 2, 32, 96, 32, F16, 13)
        with pytest.raises(NotImplementedError, match="flash_attn_paged_func"):
            flash_attn_paged_varlen_func(c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl)
        c = Ragged(((4, 64), (7, 100)), 4, 2, 64, 128, 32, F16, 14)
        k8 = c.kc.nan_to_num(0.0).to(torch.float8_e4m3fn)
        with pytest.raises(NotImplementedError, match="FP8"):
            flash_attn_paged_varlen_func(c.q, k8, k8, c.cu_q, c.max_q, c.table, c.sl)
        c = Ragged(((4, 64), (7, 100)), 4, 2, 64, 128, 20, F16, 15)
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            flash_attn_paged_varlen_func(c.q, c.kc, c.vc, c.cu_q, c.max_q, c.table, c.sl)


def test_max_seqlen_q_is_verified_on_request(monkeypatch):
    from flash_attention_cute_amd import flash_attn_paged_varlen_func

    c = Ragged(PAIRS, 4, 2, 64, 128, 32, F16, 16)
    monkeypatch.setenv("FA_CHECK_VARLEN", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flash_attn_paged_varlen_func(c.q, c.kc, c.vc, c.cu_q, 20, c.table, c.sl)
        with pytest.raises(ValueError, match="max_seqlen_q=19"):
            flash_attn_paged_varlen_func(c.q, c.kc, c.vc, c.cu_q, 19, c.table, c.sl)


# CPU default of the append against the existing op called once per sequence (B = 1): ragged counts, a page edge,
# an overflow, bad page ids, a sequence shorter than its Sq_b
@pytest.mark.parametrize("scenario", ["plain", "bad_page", "overflow"])
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
def test_cpu_default_append_matches_per_sequence_appends(scenario, rope):
    from flash_attention_cute_amd import flash_attn_kvcache_append_varlen

    hq, hkv, page, cap, d, dt = 4, 2, 32, 128, 16, torch.float32
    lens = (0, 31, 95, 120) if scenario == "overflow" else (0, 31, 95, 60)
    news, sqs = (5, 3, 0, 20), (9, 3, 2, 1)  # 9 queries over 5 keys: positions max(5 - 9 + i, 0)
    kc, vc, table, sl = ragged_cache(lens, news, hkv, page, cap, d, dt, 21)
    if scenario == "bad_page":
        table[1, 1] = -1          # sequence 1's tokens at positions 32, 33 (31 is written)
        table[3, 2] = 2 ** 31 - 1  # sequence 3's tokens at 64 .. 79 (60 .. 63 are written)
    cu, cuq = cu_of(news), cu_of(sqs)
    k, v, q = packed_rows(28, hkv, d, dt, 22), packed_rows(28, hkv, d, dt, 23), packed_rows(15, hq, d, dt, 24)
    cos, sin = rope_tables(cap, d, dt) if rope else (None, None)
    kr, vr, nr, qr = per_sequence_append(kc, vc, k, v, cu, sl, table, cos, sin, q if rope else None, cuq if rope else None)
    kc0 = kc.clone()
    got = flash_attn_kvcache_append_varlen(kc, vc, k, v, cu, sl, table, cos, sin, q if rope else None, cuq if rope else None)
    new, q_rot = got if rope else (got, None)
    assert new.tolist() == [min(n + m, cap) for n, m in zip(lens, news)] and torch.equal(new, nr)
    assert torch.equal(kc, kr) and torch.equal(vc, vr)
    written = int((kc != kc0).any(dim=-1).sum())
    assert written == {"plain": 28, "bad_page": 28 - 2 - 16, "overflow": 28 - 12}[scenario] * hkv
    if rope:
        assert torch.equal(q_rot, qr)


def test_step_is_the_append_followed_by_the_attention():
    from flash_attention_cute_amd import (flash_attn_kvcache_append_varlen, flash_attn_paged_varlen_func,
                                          flash_attn_varlen_with_kvcache)

    hq, hkv, page, cap, d, dt = 4, 2, 64, 128, 16, F16
    lens, news = (0, 31, 95, 60), (5, 3, 0, 20)
    kc, vc, table, sl = ragged_cache(lens, news, hkv, page, cap, d, dt, 31)
    cu = cu_of(news)
    k, v, q = packed_rows(28, hkv, d, dt, 32), packed_rows(28, hkv, d, dt, 33), packed_rows(28, hq, d, dt, 34)
    cos, sin = rope_tables(cap, d, dt)
    kc2, vc2 = kc.clone(), vc.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, new = flash_attn_varlen_with_kvcache(q, kc, vc, cu, 20, k, v, rotary_cos=cos, rotary_sin=sin, cache_seqlens=sl,
                                                  block_table=table, causal=True, return_seqlens=True)
        new2, q_rot = flash_attn_kvcache_append_varlen(kc2, vc2, k, v, cu, sl, table, cos, sin, q, cu)
        ref = flash_attn_paged_varlen_func(q_rot, kc2, vc2, cu, 20, table, new2, causal=True)
        # without tables: the append alone, q as it is
        kc3, vc3 = kc2.clone(), vc2.clone()
        out3 = flash_attn_varlen_with_kvcache(q, kc3, vc3, cu, 20, cache_seqlens=new2, block_table=table, causal=True)
        ref3 = flash_attn_paged_varlen_func(q, kc2, vc2, cu, 20, table, new2, causal=True)
    assert new.tolist() == [5, 34, 95, 80] and torch.equal(new, new2)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2) and torch.equal(out, ref)
    assert torch.equal(out3, ref3) and torch.equal(kc3, kc2)
    with pytest.raises(ValueError, match="block_table"):
        flash_attn_varlen_with_kvcache(q, kc, vc, cu, 20, cache_seqlens=sl)
