"""In-place KV-cache append with fused RoPE, and ``flash_attn_with_kvcache``.

No reference counterpart (the reference has no KV cache). ``flash_attn_kvcache_append`` (C-ABI
``fa_kvcache_append_gfx950``, include/fa_gfx950_kvcache.h) writes the new keys / values of a decode or
prefill step into the page pool that ``flash_attn_paged_func`` reads (or a dense cache), rotating k -- and
q -- at the tokens' positions on the way, in one launch.

The yardstick is made of ops that existed before: the expected pool is the initial pool with the rows
``(block_table[b][n // page], n % page)`` overwritten by ``apply_rope`` of the new keys (cos / sin
gathered in torch) and by the new values. Pools are compared WHOLE and as bits (``view(int16)``,
``torch.equal``): the right rows hold the right bits and no other row changed. Every pool row that
holds no key carries a fixed non-NaN bit pattern, every unused table entry -1.
"""
from __future__ import annotations

import warnings

import pytest
import torch

from test_padded import check_padded, oracle_padded
from test_paged import make_paged

F16, BF16 = torch.float16, torch.bfloat16
PATTERN = 0.40625  # exact in fp16 and bf16: the fixed bit pattern of rows that hold no key
LENS = (0, 31, 95)


def rope_tables(max_pos, d, dtype, seed=0):
    """Full-width rotate-half tables [max_pos, D] (both halves equal, as HF builds them), rounded to dtype."""
    g = torch.Generator().manual_seed(1000 + seed)
    ang = torch.rand(max_pos, d // 2, generator=g) * 6.283
    ang = torch.cat((ang, ang), dim=-1)
    return ang.cos().to(dtype), ang.sin().to(dtype)


def bits(t):
    return t.view(torch.int16)


def make_cache(lens, sn, hkv, page, cap, d, dtype, seed, layout="phsd", unused=-1, dense=False):
    """A cache that holds ``lens`` keys per sequence with room for ``sn`` more: the pool and the shuffled
    table of test_paged.make_paged for the lengths after the append, rows without a key set to PATTERN.
    dense: [B, Hkv, cap, D] and no table. Returns (k_cache, v_cache, table or None, lens int32)."""
    sl = torch.tensor(lens, dtype=torch.int32)
    if dense:
        g = torch.Generator().manual_seed(seed)
        kc = torch.randn(len(lens), hkv, cap, d, generator=g).to(dtype)
        vc = torch.randn(len(lens), hkv, cap, d, generator=g).to(dtype)
        for i, n in enumerate(lens):
            kc[i, :, n:] = PATTERN
            vc[i, :, n:] = PATTERN
        return kc, vc, None, sl
    after = tuple(min(max(n, 0) + sn, cap) for n in lens)
    _, _, _, kc, vc, table, _ = make_paged(after, hkv, hkv, 1, page, cap, d, dtype, seed, layout, unused)
    for c in (kc, vc):
        c[c.isnan()] = PATTERN
    return kc, vc, table, sl


def targets(lens, sn, table, page, cap, num_pages):
    """(b, i, page, row) of every new token that is written: the rule of the header, on the host."""
    out = []
    for b, n0 in enumerate(lens):
        n0 = min(max(n0, 0), cap)
        for i in range(sn):
            n = n0 + i
            if n >= cap:
                continue
            pg = b if table is None else int(table[b, n // page])
            if 0 <= pg < num_pages:
                out.append((b, i, pg, n % page))
    return out


def expected_append(kc, vc, k_new, v_new, lens, table, cos, sin, apply_rope):
    """The yardstick: clones of the pools with the written rows replaced by apply_rope(k_new) / v_new (on
    the tensors' device; ``table`` and ``lens`` are host lists / tensors)."""
    num_pages, _, page, _ = kc.shape
    cap = page * (table.size(1) if table is not None else 1)
    sn = k_new.size(2)
    ek, ev = kc.clone(), vc.clone()
    if cos is not None:
        pos = torch.tensor([[min(max(n, 0), cap) + i for i in range(sn)] for n in lens]).clamp(max=cos.size(0) - 1)
        pos = pos.to(k_new.device)
        k_new = apply_rope(k_new, cos[pos], sin[pos])
    t = targets(lens, sn, table, page, cap, num_pages)
    if t:
        bs, is_, pg, row = (torch.tensor(x, device=kc.device) for x in zip(*t))
        ek[pg, :, row] = k_new[bs, :, is_]
        ev[pg, :, row] = v_new[bs, :, is_]
    return ek, ev


def new_tokens(b, h, s, d, dtype, seed, hf=False):
    g = torch.Generator().manual_seed(seed)
    if hf:  # an HF projection view: [B, S, H, D] transposed
        return torch.randn(b, s, h, d, generator=g).to(dtype).transpose(1, 2)
    return torch.randn(b, h, s, d, generator=g).to(dtype)


# ------------------------------------------------------------------------------------------- CPU
def test_kvcache_op_registration():
    import flash_attention_cute_amd  # noqa: F401

    sch = str(torch.ops.flash_attention.kvcache_append.default._schema)
    assert sch == ("flash_attention::kvcache_append(Tensor(a0!) k_cache, Tensor(a1!) v_cache, Tensor? k, Tensor? v, "
                   "Tensor cache_seqlens, Tensor? block_table=None, Tensor? q=None, Tensor? rotary_cos=None, "
                   "Tensor? rotary_sin=None) -> (Tensor, Tensor)")
    kc, vc, table, sl = make_cache((5, 40), 2, 2, 32, 64, 16, torch.float32, 1)
    k, v, q = new_tokens(2, 2, 2, 16, torch.float32, 2), new_tokens(2, 2, 2, 16, torch.float32, 3), \
        new_tokens(2, 4, 2, 16, torch.float32, 4)
    cos, sin = rope_tables(64, 16, torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for args in ((kc, vc, k, v, sl, table, q, cos, sin), (kc, vc, k, v, sl, table),
                     (kc, vc, None, None, sl, table, q, cos, sin)):
            torch.library.opcheck(torch.ops.flash_attention.kvcache_append.default, args,
                                  test_utils=("test_schema", "test_faketensor"))


def test_kvcache_funcs_are_exported_like_the_other_extras():
    import flash_attention
    import flash_attention.flash_attention as ref_mod
    import flash_attention_cute_amd as m

    for name in ("flash_attn_kvcache_append", "flash_attn_with_kvcache", "flash_attention_kvcache_append"):
        assert getattr(m, name) is getattr(flash_attention, name) is getattr(ref_mod, name)
        assert name in m.__all__


@pytest.mark.parametrize("scenario", ["plain", "bad_page", "at_capacity", "dense"])
def test_kvcache_op_cpu_default_matches_a_hand_written_loop(scenario):
    """The CPU default against a loop over (sequence, token, head) that writes one row at a time."""
    from flash_attention_cute_amd import flash_attention_kvcache_append

    hkv, hq, sn, page, cap, d, dt = 2, 4, 3, 32, 128, 16, torch.float32
    lens = (0, 31, 127) if scenario == "at_capacity" else LENS
    page = cap if scenario == "dense" else page  # a dense cache is one page of Smax rows per sequence
    kc, vc, table, sl = make_cache(lens, sn, hkv, page, cap, d, dt, 5, dense=scenario == "dense")
    if scenario == "bad_page":
        table[1, 1] = -1  # sequence 1's tokens at positions 32, 33
        table[2, 2] = 2 ** 31 - 1  # sequence 2's tokens at 95 (page 2); 96, 97 are page 3
    k, v, q = new_tokens(3, hkv, sn, d, dt, 6), new_tokens(3, hkv, sn, d, dt, 7), new_tokens(3, hq, sn, d, dt, 8)
    cos, sin = rope_tables(120, d, dt)  # shorter than the capacity: positions 120.. use row 119
    ek, ev = kc.clone(), vc.clone()
    num_pages, half = kc.size(0), d // 2
    written = 0
    for b, n0 in enumerate(lens):
        for i in range(sn):
            n = n0 + i
            if n >= cap:
                continue
            pg = b if table is None else int(table[b, n // page])
            if pg < 0 or pg >= num_pages:
                continue
            written += 1
            c, s = cos[min(n, 119)], sin[min(n, 119)]
            for h in range(hkv):
                x = k[b, h, i]
                ek[pg, h, n % page] = x * c + torch.cat((-x[half:], x[:half])) * s
                ev[pg, h, n % page] = v[b, h, i]
    assert written == {"plain": 9, "bad_page": 6, "at_capacity": 7, "dense": 9}[scenario]
    new, q_rot = flash_attention_kvcache_append(kc, vc, k, v, sl, table, q, cos, sin)
    assert torch.equal(kc, ek) and torch.equal(vc, ev)
    assert new.dtype == torch.int32 and new.tolist() == [min(n + sn, cap) for n in lens]
    for b, e in enumerate(new.tolist()):
        for i in range(sn):
            p = min(max(e - sn + i, 0), 119)
            x = q[b, :, i]
            want = x * cos[p] + torch.cat((-x[:, half:], x[:, :half]), dim=-1) * sin[p]
            assert torch.equal(q_rot[b, :, i], want)
    assert sl.tolist() == list(lens)  # the input lengths are not modified


def test_with_kvcache_cpu_matches_the_composed_step():
    from flash_attention_cute_amd import flash_attn_kvcache_append, flash_attn_paged_func, flash_attn_with_kvcache
    from flash_attention_cute_amd.flash_attention import _rope_reference

    hkv, hq, page, cap, d, dt, lens = 2, 4, 32, 64, 16, torch.float32, (31, 40)
    kc, vc, table, sl = make_cache(lens, 1, hkv, page, cap, d, dt, 9)
    k, v, q = new_tokens(2, hkv, 1, d, dt, 1), new_tokens(2, hkv, 1, d, dt, 2), new_tokens(2, hq, 1, d, dt, 3)
    cos, sin = rope_tables(cap, d, dt)
    kc2, vc2 = kc.clone(), vc.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, new = flash_attn_with_kvcache(q, kc, vc, k, v, cos, sin, cache_seqlens=sl, block_table=table,
                                           return_seqlens=True)
        new2 = flash_attn_kvcache_append(kc2, vc2, k, v, sl, table, cos, sin)
        pos = sl.long()[:, None]
        ref = flash_attn_paged_func(_rope_reference(q, cos[pos], sin[pos]), kc2, vc2, table, new2)
    assert torch.equal(new, new2) and new.tolist() == [32, 41]
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2) and torch.equal(out, ref)
    with pytest.raises(ValueError, match="cache_seqlens"):
        flash_attn_with_kvcache(q, kc, vc, k, v)


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def ops(device):
    from flash_attention_cute_amd import _debug, apply_rope
    from flash_attention_cute_amd import flash_attention as fam
    from flash_attention_cute_amd import (flash_attention_kvcache_append, flash_attn_kvcache_append,
                                          flash_attn_padded_func, flash_attn_paged_func, flash_attn_with_kvcache)

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    _debug.set_dec_fuse(None)

    class Ops:
        append = staticmethod(flash_attn_kvcache_append)
        op = staticmethod(flash_attention_kvcache_append)
        with_kvcache = staticmethod(flash_attn_with_kvcache)
        paged = staticmethod(flash_attn_paged_func)
        padded = staticmethod(flash_attn_padded_func)
        rope = staticmethod(apply_rope)
        gather = staticmethod(fam._gather_pages)

    return Ops


# (dtype, D, rope, pool layout, page, Sn, input). cap 128, lens (0, 31, 95): Sn 40 crosses a page boundary
# for every sequence (for len 31 it ends inside the second page) and runs past the capacity for len 95.
# D 72 takes the element path; "hf": k / v are [B, Sn, H, D].transpose(1, 2) views; "dense": no table,
# Smax = 100 (not a multiple of 32); "odd": the pool is a view at a 2-byte-aligned offset of a wider buffer.
APPEND_CASES = [
    (F16, 128, True, "phsd", 32, 1, "plain"),
    (BF16, 128, True, "pshd", 64, 3, "plain"),
    (F16, 128, True, "pshd", 64, 40, "plain"),
    (BF16, 128, True, "phsd", 32, 40, "hf"),
    (F16, 64, True, "pshd", 32, 40, "plain"),
    (BF16, 64, True, "phsd", 64, 1, "hf"),
    (F16, 72, True, "phsd", 32, 3, "plain"),
    (BF16, 72, True, "pshd", 64, 40, "hf"),
    (BF16, 128, False, "phsd", 32, 40, "plain"),
    (F16, 128, False, "pshd", 64, 1, "hf"),
    (BF16, 128, True, "phsd", 100, 3, "dense"),
    (F16, 64, True, "phsd", 100, 40, "dense"),
    (F16, 72, False, "phsd", 100, 1, "dense"),
    (BF16, 128, True, "phsd", 32, 3, "odd"),
]
APPEND_IDS = [f"{'f16' if t == F16 else 'bf16'}-d{d}-{'rope' if r else 'norope'}-{lay}-p{p}-sn{sn}-{inp}"
              for t, d, r, lay, p, sn, inp in APPEND_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("case", APPEND_CASES, ids=APPEND_IDS)
def test_append_is_bit_exact_and_touches_no_other_row(ops, device, case):
    dtype, d, rope, layout, page, sn, inp = case
    hkv, dense = 2, inp == "dense"
    cap = page if dense else 128
    kc, vc, table, sl = make_cache(LENS, sn, hkv, page, cap, d, dtype, 40 + sn + d, layout, dense=dense)
    k = new_tokens(3, hkv, sn, d, dtype, 50, hf=inp == "hf").to(device)
    v = new_tokens(3, hkv, sn, d, dtype, 51, hf=inp == "hf").to(device)
    if inp == "hf":
        assert k.stride(1) == d and k.stride(2) == hkv * d  # heads inside a token's row
    cos, sin = (t.to(device) for t in rope_tables(cap, d, dtype)) if rope else (None, None)
    kc, vc = kc.to(device), vc.to(device)
    if inp == "odd":  # the same pool one element into a wider buffer: 2-byte aligned, row stride D + 2
        wide = [torch.full((*c.shape[:3], d + 2), 1.5, dtype=dtype, device=device) for c in (kc, vc)]
        for w, c in zip(wide, (kc, vc)):
            w[..., 1:d + 1] = c
        kc, vc = (w[..., 1:d + 1] for w in wide)
        assert kc.data_ptr() % 4 == 2
    ek, ev = expected_append(kc, vc, k, v, LENS, table, cos, sin, ops.rope)
    ptr = kc.data_ptr()
    new = ops.append(kc, vc, k, v, sl.to(device), None if dense else table.to(device), cos, sin)
    torch.cuda.synchronize()
    assert kc.data_ptr() == ptr
    assert torch.equal(bits(kc), bits(ek)) and torch.equal(bits(vc), bits(ev))
    assert not torch.equal(bits(kc), bits(make_cache(LENS, sn, hkv, page, cap, d, dtype, 40 + sn + d, layout,
                                                     dense=dense)[0].to(device)))  # (something was written)
    assert new.dtype == torch.int32 and new.device == kc.device
    assert new.tolist() == [min(n + sn, cap) for n in LENS]
    if inp == "odd":  # the margins of the wider buffer are untouched
        for w in wide:
            assert (w[..., 0] == 1.5).all() and (w[..., d + 1] == 1.5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,d,s,with_k", [(F16, 128, 1, True), (BF16, 128, 3, True), (F16, 72, 3, True),
                                              (BF16, 64, 1, False), (F16, 128, 3, False)],
                         ids=["f16-d128-s1", "bf16-d128-s3", "f16-d72-s3", "bf16-d64-s1-no_k", "f16-d128-s3-no_k"])
def test_q_is_rotated_at_the_last_positions(ops, device, dtype, d, s, with_k):
    hkv, hq, page, cap = 2, 8, 32, 128
    sn = s if with_k else 0
    kc, vc, table, sl = (t.to(device) for t in make_cache(LENS, sn, hkv, page, cap, d, dtype, 60 + s))
    k, v = (new_tokens(3, hkv, s, d, dtype, 61 + i).to(device) for i in range(2)) if with_k else (None, None)
    q = new_tokens(3, hq, s, d, dtype, 63, hf=True).to(device)
    cos, sin = (t.to(device) for t in rope_tables(cap, d, dtype))
    before = bits(kc).clone()
    new, q_rot = ops.op(kc, vc, k, v, sl, table, q, cos, sin)
    qpos = torch.tensor([[max(n + sn - s + i, 0) for i in range(s)] for n in LENS], device=device)
    assert torch.equal(q_rot, ops.rope(q, cos[qpos], sin[qpos]))
    assert q_rot.is_contiguous() and new.tolist() == [n + sn for n in LENS]
    if not with_k:
        assert torch.equal(bits(kc), before)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [-1, 2 ** 31 - 1])
def test_a_bad_page_id_drops_the_row_and_never_redirects_it(ops, device, bad):
    dtype, d, hkv, page, cap, sn = BF16, 128, 2, 32, 128, 3
    kc, vc, table, sl = make_cache(LENS, sn, hkv, page, cap, d, dtype, 70)
    table[1, 1] = bad  # sequence 1 (len 31): token 0 lands in page 0, tokens 1, 2 in this page
    k, v = (new_tokens(3, hkv, sn, d, dtype, 71 + i).to(device) for i in range(2))
    cos, sin = (t.to(device) for t in rope_tables(cap, d, dtype))
    kc, vc = kc.to(device), vc.to(device)
    assert len(targets(LENS, sn, table, page, cap, kc.size(0))) == 7
    ek, ev = expected_append(kc, vc, k, v, LENS, table, cos, sin, ops.rope)
    new = ops.append(kc, vc, k, v, sl.to(device), table.to(device), cos, sin)
    assert torch.equal(bits(kc), bits(ek)) and torch.equal(bits(vc), bits(ev))
    assert new.tolist() == [n + sn for n in LENS]  # the lengths advance: the table is the caller's


@pytest.mark.gpu
def test_capacity_negative_lengths_and_short_tables(ops, device):
    """Tokens past the capacity are dropped and the length stops there; a negative length counts as 0; a
    rotary table shorter than the position uses its last row."""
    dtype, d, hkv, page, cap, sn = F16, 64, 2, 32, 128, 5
    lens = (126, -7, 128, 60)
    kc, vc, table, sl = make_cache(lens, sn, hkv, page, cap, d, dtype, 80)
    k, v = (new_tokens(4, hkv, sn, d, dtype, 81 + i).to(device) for i in range(2))
    q = new_tokens(4, 4, 2, d, dtype, 83).to(device)
    cos, sin = (t.to(device) for t in rope_tables(62, d, dtype))  # positions 62.. use row 61
    kc, vc = kc.to(device), vc.to(device)
    assert len(targets(lens, sn, table, page, cap, kc.size(0))) == 2 + 5 + 0 + 5
    ek, ev = expected_append(kc, vc, k, v, lens, table, cos, sin, ops.rope)
    new, q_rot = ops.op(kc, vc, k, v, sl.to(device), table.to(device), q, cos, sin)
    assert torch.equal(bits(kc), bits(ek)) and torch.equal(bits(vc), bits(ev))
    assert new.tolist() == [128, 5, 128, 65]
    qpos = torch.tensor([[min(e - 2 + i, 61) for i in range(2)] for e in (128, 5, 128, 65)], device=device)
    assert torch.equal(q_rot, ops.rope(q, cos[qpos], sin[qpos]))


@pytest.mark.gpu
def test_unused_table_entries_are_never_read(ops, device):
    """Entries of pages no new token lands in hold 2**31 - 1 instead of -1: the same bits."""
    dtype, d, hkv, page, cap, sn = F16, 128, 2, 32, 128, 3
    pools = []
    for unused in (-1, 2 ** 31 - 1):
        kc, vc, table, sl = (t.to(device) for t in make_cache(LENS, sn, hkv, page, cap, d, dtype, 90, unused=unused))
        assert (table == unused).any()
        k, v = (new_tokens(3, hkv, sn, d, dtype, 91 + i).to(device) for i in range(2))
        cos, sin = (t.to(device) for t in rope_tables(cap, d, dtype))
        ops.append(kc, vc, k, v, sl, table, cos, sin)
        pools.append((bits(kc).clone(), bits(vc).clone()))
    assert torch.equal(pools[0][0], pools[1][0]) and torch.equal(pools[0][1], pools[1][1])


def decode_steps(ops, device, dtype, dense, steps=4):
    """`steps` successive decode steps with flash_attn_with_kvcache from lens (30, 31, 63) -- crossing the
    page boundaries at 32 and 64 -- each checked against the yardstick; returns nothing."""
    b, hq, hkv, d, page, lens = 3, 8, 2, 128, 32, (30, 31, 63)
    cap = 100 if dense else 128
    kc, vc, table, sl = make_cache(lens, steps, hkv, 100 if dense else page, cap, d, dtype, 110, dense=dense)
    if not dense:  # the pool holds the keys of the lengths AFTER the steps: blank the rows to be written
        for bb, i, pg, row in targets(lens, steps, table, page, cap, kc.size(0)):
            kc[pg, :, row] = PATTERN
            vc[pg, :, row] = PATTERN
    kc, vc, sl = kc.to(device), vc.to(device), sl.to(device)
    tb = None if dense else table.to(device)
    cos, sin = (t.to(device) for t in rope_tables(cap, d, dtype))
    cur = list(lens)
    for step in range(steps):
        q = new_tokens(b, hq, 1, d, dtype, 120 + 3 * step).to(device)
        k = new_tokens(b, hkv, 1, d, dtype, 121 + 3 * step).to(device)
        v = new_tokens(b, hkv, 1, d, dtype, 122 + 3 * step).to(device)
        ek, ev = expected_append(kc, vc, k, v, cur, table, cos, sin, ops.rope)
        out, new = ops.with_kvcache(q, kc, vc, k, v, cos, sin, cache_seqlens=sl, block_table=tb, return_seqlens=True)
        cur = [n + 1 for n in cur]
        assert new.tolist() == cur
        assert torch.equal(bits(kc), bits(ek)) and torch.equal(bits(vc), bits(ev))
        qpos = torch.tensor(cur, device=device)[:, None] - 1
        q_rot = ops.rope(q, cos[qpos], sin[qpos])
        if dense:
            ref = ops.padded(q_rot, ek, ev, torch.zeros_like(new), new)
            kd, vd = ek, ev
        else:
            ref = ops.paged(q_rot, ek, ev, tb, new)
            kd, vd = ops.gather(ek, tb), ops.gather(ev, tb)
        assert torch.isfinite(out.float()).all() and torch.equal(out, ref)
        zero = torch.zeros(b, dtype=torch.int32)
        check_padded(out, oracle_padded(q_rot.cpu(), kd.cpu(), vd.cpu(), zero, new.cpu(), None, None, d ** -0.5,
                                        False), dtype)
        sl = new


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_with_kvcache_four_decode_steps_on_a_paged_cache(ops, device, dtype):
    decode_steps(ops, device, dtype, dense=False)


@pytest.mark.gpu
def test_with_kvcache_four_decode_steps_on_a_dense_cache(ops, device):
    decode_steps(ops, device, BF16, dense=True)


@pytest.mark.gpu
def test_serving_step_graph_capture(ops, device):
    """append + attend + cache_seqlens.copy_(new_seqlens) captured once and replayed 3 times with new
    q / k / v: the pool, the lengths and the outputs of 3 eager steps from the same start."""
    b, hq, hkv, d, page, cap, dtype, lens, steps = 3, 8, 2, 128, 32, 128, BF16, (30, 31, 63), 3
    kc0, vc0, table, sl0 = (t.to(device) for t in make_cache(lens, steps, hkv, page, cap, d, dtype, 130))
    cos, sin = (t.to(device) for t in rope_tables(cap, d, dtype))
    toks = [[new_tokens(b, h, 1, d, dtype, 140 + 3 * s + i).to(device) for i, h in enumerate((hq, hkv, hkv))]
            for s in range(steps)]

    def step(q, k, v, kc, vc, sl):
        out, new = ops.with_kvcache(q, kc, vc, k, v, cos, sin, cache_seqlens=sl, block_table=table,
                                    return_seqlens=True)
        sl.copy_(new)
        return out

    kc_e, vc_e, sl_e = kc0.clone(), vc0.clone(), sl0.clone()
    eager = [step(q, k, v, kc_e, vc_e, sl_e).clone() for q, k, v in toks]  # (also the warm-up)
    torch.cuda.synchronize()
    kc, vc, sl = kc0.clone(), vc0.clone(), sl0.clone()
    q, k, v = (t.clone() for t in toks[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step(q, k, v, kc, vc, sl)
    assert torch.equal(bits(kc), bits(kc0)) and sl.tolist() == list(lens)  # captured, not run
    for s in range(steps):
        for dst, src in zip((q, k, v), toks[s]):
            dst.copy_(src)
        g.replay()
        assert torch.equal(out, eager[s])
    torch.cuda.synchronize()
    assert sl.tolist() == sl_e.tolist() == [n + steps for n in lens]
    assert torch.equal(bits(kc), bits(kc_e)) and torch.equal(bits(vc), bits(vc_e))


@pytest.mark.gpu
def test_append_into_a_pool_beyond_2_31_elements(ops, device):
    """Pages past element 2^31 of the pool (the page term of the address is 64-bit): the append into an
    uninitialised large pool of which only the last pages are referenced leaves the bits of a small pool."""
    hkv, page, d, lens, sn, cap = 1, 256, 128, (1000, 250), 8, 1024
    first = 2 ** 31 // (hkv * page * d) + 1  # the first page that lies wholly past element 2^31
    free, _ = torch.cuda.mem_get_info(device)
    if free < 12 * 2 ** 30:
        pytest.skip("needs about 12 GiB of free device memory")
    kc, vc, table, sl = (t.to(device) for t in make_cache(lens, sn, hkv, page, cap, d, BF16, 150))
    k, v = (new_tokens(2, hkv, sn, d, BF16, 151 + i).to(device) for i in range(2))
    cos, sin = (t.to(device) for t in rope_tables(cap, d, BF16))
    n = kc.size(0)
    big_k = torch.empty(first + n, hkv, page, d, dtype=BF16, device=device)
    big_v = torch.empty_like(big_k)
    assert big_k.numel() > 2 ** 31
    big_k[first:], big_v[first:] = kc, vc
    far = torch.where(table >= 0, table + first, table)
    ek, ev = expected_append(kc, vc, k, v, lens, table.cpu(), cos, sin, ops.rope)
    new_small = ops.append(kc, vc, k, v, sl, table, cos, sin)
    new = ops.append(big_k, big_v, k, v, sl, far, cos, sin)
    torch.cuda.synchronize()
    assert torch.equal(new, new_small) and new.tolist() == [1008, 258]
    assert torch.equal(bits(kc), bits(ek)) and torch.equal(bits(vc), bits(ev))
    assert torch.equal(bits(big_k[first:]), bits(ek)) and torch.equal(bits(big_v[first:]), bits(ev))
