"""Every kernel on buffers that span more than 2^31 and 2^32 bytes (tests/large_arena.py holds the arena).

Why. The kernels form the page, batch, head and part terms of an address in 64 bits and narrow the row strides
to ``int`` under host rules; every other pool in tests/ is a few MiB, so a dropped ``int64_t`` cast, a new
kernel with an ``int`` offset or a host rule off by a factor of two passes all of them bit for bit. Here the
SHAPES are the small ones of each path's own tests; only the addresses are large: every buffer of a launch is
an ``as_strided`` view of one 9 GiB uint8 allocation, at least 4 GiB into it and reaching at most 4.5 GiB from
its base, so a term kept in 32 bits reads or writes INSIDE the arena -- wrong data, never a fault.

Pools. K and V interleaved as ``[P, 2, Hkv, page, D]`` (16-bit, Hkv 2, D 128): one page pitch is 64 KiB at page 64
(id 32768 starts at 2^31 B, id 65536 at 2^32 B = 2^31 elements; P = 65536 + 16) and 32 KiB at page 32 (ids 65536 /
131072; P = 131072 + 16). An e4m3 pool views the same bytes with the same byte pitch. The ragged cases need 31 live
pages and use P = 65536 + 64. Tables mix the ids {t - 1, t} of both thresholds, 0, 1 and P - 1 with a seeded shuffle
of the ids above the last threshold (``large_arena.high_page_table``); the longest sequence walks 32767 -> 32768 ->
65535 -> 65536 in consecutive pages, so consecutive tiles -- and the prefill kernel's K and V cursors -- sit on
different sides of a threshold.

Single-term mistakes (``large_arena.MISTAKES``) and where one of them lands, arena byte offsets, from
``test_model_*`` (pool base 0x1_0000_0000, page pitch 0x1_0000; every address below lies inside the arena and holds
pattern bytes or another sequence's page, never the row that should have been read):

    page term of kc, byte offset in uint32   page 65536 row 0   right 0x2_0000_0000   wrong 0x1_0000_0000 (page 0)
    page term of kc, byte offset in int32    page 32768 row 0   right 0x1_8000_0000   wrong 0x0_8000_0000 (pattern)
    page term of kc, element offset in int32 page 65536 row 0   right 0x2_0000_0000   wrong 0x0_0000_0000 (pattern)
    page term of kc, element offset in uint32: never changes an address inside a 4.5 GiB span (2^32 elements are
        8 GiB): not claimed by any case
    batch term of q / k / v / o (dense, stride 2^31 + 128 elements), byte offset in uint32:
                                             batch 1           right base + 0x1_0000_0100   wrong base + 0x100
    head term (stride 3 * 2^28 + 8 elements), byte offset in int32: head 2 right base + 0xC000_0020, wrong
        base - 0x3FFF_FFE0 (pattern)
    part term of the merge's outs (stride 9 * 2^27 + 8 elements), element offset in int32: part 2 right
        base + 0x1_2000_0020, wrong base - 0xE000_0000 + 0x20 (pattern)
    packed row term of the ragged q (stride 2406560 elements), byte offset in uint32: row 893 wraps by 2^32
    descale batch term (fp32, stride 2^29 + 8 elements), byte offset in int32: batch 1 right base + 0x8000_0020,
        wrong base - 0x7FFF_FFE0 (pattern)
    a row stride taken as int after doubling: changes nothing below the host rules (that is what they are for);
        the rule cases of section (c) run the kernels AT the rules' limits instead

Yardsticks, in this order: float64 softmax on the rounded inputs (``oracle_padded``) under tests/test_gpu_parity.py
``TOL``; ``test_paged_lse.LSE_TOL`` for an LSE; then ``torch.equal`` with the same launch on a compact copy (the same
pages renumbered from 0, the same tensors contiguous) -- the launch plans depend on B, the head counts, Sq and the
table's CAPACITY (``decode_plan``: units and seqlen_kv = max_pages * page_size), never on num_pages or a stride, so
the two launches run the same plan; ``last_path`` is compared as well. Appends are held bit for bit to the existing
references on the compact pool. After every launch the whole arena must hold the pattern again outside the declared
outputs, under 0xFF and under 0x7B.

That the cases can fail was seen once, with two uncommitted library edits for which ``test_model_*`` shows every
address inside the arena: ``page * kps`` of ``PagedWalk::tile`` through ``uint32_t`` failed every decode case of
``test_paged_reads``, ``test_paged_lse_*``, ``test_paged_fp8_with_descales_*`` and ``test_shared_prefix_*[suffix]`` under both patterns
(non-finite output under 0xFF, up to 3.1 over the bound under 0x7B), and ``page * p.k_page_stride`` of
``fa_kvcache_append_varlen`` through ``int32_t`` failed ``test_append_varlen`` and ``test_with_kvcache_*`` on 31040
stray 8-byte granules from arena byte 0x0 on (the rows meant for page 65536 and above, 8 GiB too low). The prefill and
ragged-attention cases stayed green, as they should: they do not run the edited lines.

Outputs. The public ops allocate their own output, so every entry is ALSO run through the C ABI (ctypes, the
structures of tests/test_abi.py, test_paged_abi.py, test_fp8_abi.py, test_paged_varlen_abi.py, test_lse_abi.py) with o --
and the workspace, when the launch wants one -- as declared outputs in the arena at strides that cross 2^31 and 2^32
bytes: the dense, padded, window, rope and varlen entries, the paged decode (split and unsplit), windowed decode, FP8
decode, paged prefill and ragged prefill, the LSE launch and the merge (out and lse).

Limits of what is covered: spans stop at 4.5 GiB, so 2^32 ELEMENTS of a 16-bit pool (8 GiB from a base) stay untested,
and the fp32 arrays (LSE, descales) cross 2^31 and 2^32 BYTES, not 2^31 elements. The shared-prefix op, the appends'
rotated q and new lengths, and the with_kvcache steps write their results outside the arena (the public ops allocate
them); q, the table and the lengths of the two strided-pool rule cases are plain tensors.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from large_arena import (ARENA_BYTES, BASE_MIN, GIB, MIB, MISTAKES, PATTERNS, BigArena, Plan, high_page_table,
                         item_size, s32)
from test_fp8_kvcache import FP8, make_fp8_paged, pow2_descales
from test_kvcache import expected_append, new_tokens, rope_tables
from test_padded import check_padded, oracle_padded
from test_paged import make_paged
from test_paged_lse import check_lse, lse_oracle, make_states, merge_oracle  # (check_lse asserts LSE_TOL)
from test_paged_varlen import BASE_PAIRS, Ragged, cu_of, packed_rows, per_sequence_append

F16, BF16, I32, F32 = torch.float16, torch.bfloat16, torch.int32, torch.float32
DEV = "cuda:0"
POOL_BASE = BASE_MIN
HKV, D = 2, 128
P64, P32, P_RAGGED = 65536 + 16, 131072 + 16, 65536 + 64
PACKED_Q_STRIDE = 2406560  # elements (4.6 MiB a row): 893 * 2 * it = 2^32 + 3 MiB + 0xc40


def dv(*ts):
    return tuple(t.to(DEV) if isinstance(t, torch.Tensor) else t for t in ts)


# ------------------------------------------------------------------------------------------------
# paged cases: a compact case of the path's own tests, and the same pages at high ids of a pool in the arena
# ------------------------------------------------------------------------------------------------
class PagedCase:
    """``compact``: (q, k, v, kc, vc, table, sl) of make_paged / make_fp8_paged (k, v: the dense keys the oracle
    reads). ``ids``: per table row, the big page id of every used entry. Builds the big table, the (small id, big
    id) list of the pages to copy, and the Plan."""

    def __init__(self, name, compact, num_pages, page, layout, ids=None, thresholds=None, q_strides=None, seed=0):
        self.name, self.compact = name, compact
        self.q, self.k, self.v, self.kc, self.vc, self.table, self.sl = compact
        self.num_pages, self.page, self.layout = num_pages, page, layout
        lens = self.sl.tolist()
        used = [(min(max(n, 0), self.table.size(1) * page) + page - 1) // page for n in lens]
        if ids is None:
            ids = high_page_table(used, num_pages, thresholds, seed)
        self.big_table = torch.full_like(self.table, -1)
        pairs = {}
        for b, n in enumerate(used):
            for j in range(n):
                small, big = int(self.table[b, j]), int(ids[b][j])
                assert pairs.setdefault(small, big) == big, "one small page maps to one big page"
                self.big_table[b, j] = big
        self.pairs = sorted(pairs.items())
        assert len({b for _, b in self.pairs}) == len(self.pairs)
        self.rows_of = {}  # big id -> rows of the page that hold keys
        for b, n in enumerate(lens):
            for j in range(used[b]):
                r = min(n, (j + 1) * page) - j * page
                big = int(self.big_table[b, j])
                self.rows_of[big] = max(self.rows_of.get(big, 0), r)
        self.plan = self._plan(q_strides)

    def _plan(self, q_strides):
        plan = Plan(self.name)
        dtype, page = self.kc.dtype, self.page
        item = item_size(dtype)
        pitch = 2 * HKV * page * D * 2  # bytes per page of K and V together, at 16 bits (an e4m3 pool keeps it)
        ps = pitch // item
        strides = (ps, page * D, D, 1) if self.layout == "phsd" else (ps, D, HKV * D, 1)
        live, data = [], []
        for _, big in self.pairs:
            for h in range(HKV):
                for r in range(page):
                    live.append((big, h, r))
                    data.append(r < self.rows_of[big])
        live, data = np.array(live, np.int64), np.array(data, bool)
        shape = (self.num_pages, HKV, page, D)
        plan.add("kc", dtype, shape, strides, POOL_BASE, ("page", "head", "row"), live, data=data)
        plan.add("vc", dtype, shape, strides, POOL_BASE + pitch // 2, ("page", "head", "row"), live, data=data)
        if q_strides is None:
            plan.small("q", self.q.dtype, self.q.shape, ("batch", "head", "row")[-(self.q.dim() - 1):])
        else:
            base, st, dims = q_strides
            plan.add("q", self.q.dtype, self.q.shape, st, base, dims)
        plan.small("table", I32, self.big_table.shape, ("batch",))
        plan.small("sl", I32, self.sl.shape, ())
        plan.check_disjoint()
        return plan

    def load(self, arena, updated=False):
        """The pools (their live pages), q, the table and the lengths as views of the arena."""
        kc, vc = arena.view(self.plan.placements["kc"]), arena.view(self.plan.placements["vc"])
        for small, big in self.pairs:
            arena.load(kc[big], self.kc[small], updated=f"kc{small}" if updated else None)
            arena.load(vc[big], self.vc[small], updated=f"vc{small}" if updated else None)
        q = arena.load(arena.view(self.plan.placements["q"]), self.q)
        table = arena.load(arena.view(self.plan.placements["table"]), self.big_table)
        sl = arena.load(arena.view(self.plan.placements["sl"]), self.sl)
        return q, kc, vc, table, sl


READS = {  # name -> (lens, Hq, Sq, page, capacity, causal, window, dtype, layout, num_pages, thresholds)
    "unsplit": ((0, 37, 300, 449), 8, 1, 64, 512, False, -1, F16, "phsd", P64, (32768, 65536)),
    "split": ((1000, 37), 8, 1, 64, 1024, False, -1, BF16, "phsd", P64, (32768, 65536)),
    "split_unfused": ((37, 1000), 8, 1, 64, 1024, False, -1, F16, "phsd", P64, (32768, 65536)),
    "sq3_causal": ((0, 37, 300, 449), 8, 3, 64, 512, True, -1, BF16, "phsd", P64, (32768, 65536)),
    "g8_sq5_causal": ((449, 0, 37, 300), 16, 5, 64, 512, True, -1, F16, "phsd", P64, (32768, 65536)),
    "window": ((0, 37, 300, 449), 8, 3, 64, 512, True, 100, F16, "phsd", P64, (32768, 65536)),
    "window_full": ((449, 300, 37, 0), 8, 1, 64, 512, False, 70, BF16, "phsd", P64, (32768, 65536)),
    "pshd": ((300, 0, 449, 37), 8, 1, 64, 512, False, -1, BF16, "pshd", P64, (32768, 65536)),
    "page32": ((0, 37, 300, 200), 8, 1, 32, 320, False, -1, F16, "phsd", P32, (65536, 131072)),
    "prefill_sq40": ((0, 37, 300, 449), 8, 40, 64, 512, True, -1, F16, "phsd", P64, (32768, 65536)),
    "prefill_sq300": ((449, 300, 37, 0), 8, 300, 64, 512, False, -1, BF16, "phsd", P64, (32768, 65536)),
    "prefill_sq300_causal_pshd": ((300, 449, 0, 37), 8, 300, 64, 512, True, -1, F16, "pshd", P64, (32768, 65536)),
}
DECODE = ["unsplit", "split", "split_unfused", "sq3_causal", "g8_sq5_causal", "window", "window_full", "pshd", "page32"]
PREFILL = ["prefill_sq40", "prefill_sq300", "prefill_sq300_causal_pshd"]
LSE = ["unsplit", "split", "split_unfused", "sq3_causal"]


@functools.lru_cache(maxsize=None)
def read_case(name):
    lens, hq, sq, page, cap, causal, w, dtype, layout, num_pages, thr = READS[name]
    seed = 7000 + sorted(READS).index(name)
    compact = make_paged(lens, hq, HKV, sq, page, cap, D, dtype, seed, layout, spare_pages=0)
    return PagedCase(name, compact, num_pages, page, layout, thresholds=thr, seed=seed)


@functools.lru_cache(maxsize=None)
def read_oracle(name):
    lens, hq, sq, page, cap, causal, w, dtype, layout, num_pages, thr = READS[name]
    c = read_case(name)
    return oracle_padded(c.q, c.k, c.v, torch.zeros_like(c.sl), c.sl, None, None, D ** -0.5, causal, window_left=w)


@functools.lru_cache(maxsize=None)
def lse_case(name):
    """read_case(name) with o and lse placed in the arena as well, between the pool's live pages: o with a batch
    stride of 2^31 + 64 elements (B = 2) or 3 * 2^28 + 64 (B = 4: batch 2 past 2^31 bytes, batch 3 past 2^32 bytes
    and 2^31 elements), lse (fp32) with 2^30 + 8 or 3 * 2^27 + 8 elements: the same byte offsets."""
    lens, hq, sq, page, cap, causal, w, dtype, layout, num_pages, thr = READS[name]
    seed = 7000 + sorted(READS).index(name)
    c = PagedCase(f"lse_{name}", read_case(name).compact, num_pages, page, layout, thresholds=thr, seed=seed)
    b = len(lens)
    o_st, l_st = {2: (2 ** 31 + 64, 2 ** 30 + 8), 4: (3 * 2 ** 28 + 64, 3 * 2 ** 27 + 8)}[b]
    c.plan.add("o", dtype, (b, hq, sq, D), (o_st, sq * D, D, 1), POOL_BASE + MIB, ("batch", "head", "row"), written=True)
    c.plan.add("lse", F32, (b, hq, sq), (l_st, sq, 1), POOL_BASE + 2 * MIB, ("batch", "head"), written=True)
    c.plan.check_disjoint()
    return c


@functools.lru_cache(maxsize=None)
def fp8_case(kind):
    lens, cap = ((1000, 37), 1024) if kind == "split" else ((300, 37, 449), 512)
    b = len(lens)
    kd, vd = pow2_descales(b, HKV), pow2_descales(b, HKV, 2)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, 8, HKV, 1, 64, cap, D, BF16, 7100 + len(kind), kd=kd, vd=vd)
    c = PagedCase(f"fp8_{kind}", (q, k8, v8, kc8, vc8, table, sl), P64, 64, "phsd", thresholds=(32768, 65536),
                  seed=7100 + len(kind))
    # the descales [B, Hkv] fp32 with a batch stride of 2^29 + 8 elements (B = 3: batch 1 lies past 2^31 bytes, batch
    # 2 past 2^32 bytes) or 2^30 + 8 (B = 2). 2^31 fp32 ELEMENTS would be 8 GiB, outside any span of this arena
    for i, (nm, t) in enumerate((("kd", kd), ("vd", vd))):
        c.plan.add(nm, F32, t.shape, (2 ** 29 + 8 if b == 3 else 2 ** 30 + 8, 1), POOL_BASE + GIB // 4 + 4096 * (i + 1),
                   ("batch",))
    c.plan.add("o", BF16, q.shape, (O_BATCH_STRIDE[b], q.size(2) * D, D, 1), POOL_BASE + MIB, ("batch", "head", "row"), written=True)
    c.plan.check_disjoint()
    c.kd, c.vd = kd, vd
    return c


@functools.lru_cache(maxsize=None)
def ragged_case(packed_q):
    """test_paged_varlen's base pairs at page 64; ``packed_q``: q's packed row stride is PACKED_Q_STRIDE elements,
    so row 893 of 894 lies past 2^32 bytes (the packed row term alone crosses) and no row meets a live page."""
    r = Ragged(BASE_PAIRS, 8, HKV, 64, 512, D, F16, 7200, "phsd")
    qs = None
    if packed_q:
        qs = (POOL_BASE + MIB, (PACKED_Q_STRIDE, D, 1), ("packed", "head"))
    c = PagedCase(f"ragged{'_packed_q' if packed_q else ''}", (r.q, r.k, r.v, r.kc, r.vc, r.table, r.sl), P_RAGGED, 64,
                  "phsd", thresholds=(32768, 65536), q_strides=qs, seed=7200)
    c.plan.small("cu_q", I32, r.cu_q.shape, ())
    if packed_q:  # (o for the C-ABI case: packed like q, its rows 4 KiB behind q's)
        c.plan.add("o", F16, r.q.shape, (PACKED_Q_STRIDE, D, 1), POOL_BASE + MIB + 4096, ("packed", "head"), written=True)
    c.plan.check_disjoint()
    c.ragged = r
    return c


# ------------------------------------------------------------------------------------------------
# dense cases: tiny shapes viewed with huge pitches
# ------------------------------------------------------------------------------------------------
BATCH_STRIDE = 2 ** 31 + 128     # elements: batch 1 starts past 2^32 bytes and past 2^31 elements; a multiple of
#                                  the compact row pitch D, as the padded entry asks of a batch stride
HEAD_STRIDE = 3 * 2 ** 28 + 8    # elements: 1.5 GiB; head 2 lies past 2^31 bytes, head 3 past 2^32 bytes and 2^31
#                                  elements (2^30 elements, 2 GiB, would put the fourth head 6 GiB from the base)
PART_STRIDE = 9 * 2 ** 27 + 8    # elements of the merge's 16-bit outs: 2.25 GiB; part 1 past 2^31, part 2 past 2^32 bytes
PART_STRIDE_LSE = 9 * 2 ** 26 + 8  # fp32 elements: the same bytes

DENSE = {  # name -> (B, Hq, Hkv, Sq, Sk, causal, dtype, which stride is huge)
    "batch_prefill": (2, 8, 2, 300, 300, True, F16, "batch"),
    "batch_decode": (2, 8, 2, 1, 449, False, BF16, "batch"),
    "head_prefill": (1, 4, 4, 130, 130, True, BF16, "head"),
    "head_decode": (1, 4, 4, 1, 300, False, F16, "head"),  # (g = 1: decode_rule bounds a GROUP's q-head span)
}


@functools.lru_cache(maxsize=None)
def dense_case(name):
    b, hq, hkv, sq, sk, causal, dtype, huge = DENSE[name]
    g = torch.Generator().manual_seed(7300 + sorted(DENSE).index(name))
    q = torch.randn(b, hq, sq, D, generator=g).to(dtype)
    k = torch.randn(b, hkv, sk, D, generator=g).to(dtype)
    v = torch.randn(b, hkv, sk, D, generator=g).to(dtype)
    plan = Plan(name)
    for i, (nm, t) in enumerate((("q", q), ("k", k), ("v", v), ("o", q))):
        h, s = t.size(1), t.size(2)
        if huge == "batch":
            strides = (BATCH_STRIDE, s * D, D, 1)
        else:
            strides = (h * HEAD_STRIDE, HEAD_STRIDE, D, 1)
        plan.add(nm, dtype, t.shape, strides, BASE_MIN + (i + 1) * (32 << 20), ("batch", "head", "row"), written=nm == "o")
    plan.check_disjoint()
    return plan, (q, k, v), causal


PACKED_ROW_STRIDE = 3586008  # elements (6.8 MiB a row): row 599 of 600 lies 2^32 + 1.07e6 bytes from row 0


@functools.lru_cache(maxsize=None)
def varlen_case():
    """The batch_prefill tensors packed [total, H, D] (two sequences of 300), every packed row PACKED_ROW_STRIDE
    elements after the last: the packed row term alone crosses 2^31 and 2^32 bytes."""
    _, (q, k, v), _ = dense_case("batch_prefill")
    packed = [t.transpose(1, 2).reshape(-1, t.size(1), D).contiguous() for t in (q, k, v)]
    plan = Plan("varlen_packed")
    for i, (nm, t) in enumerate(zip("qkv", packed)):
        plan.add(nm, t.dtype, t.shape, (PACKED_ROW_STRIDE, D, 1), BASE_MIN + (i + 1) * (4 << 20), ("packed", "head"))
    plan.check_disjoint()
    return plan, packed


@functools.lru_cache(maxsize=None)
def merge_case():
    n, b, h, s, d = 3, 2, 5, 2, 128
    outs, lses = make_states(n, b, h, s, d, F16, 7400)
    plan = Plan("merge")
    plan.add("outs", F16, outs.shape, (PART_STRIDE, h * s * d, s * d, d, 1), BASE_MIN + 4096, ("part", "batch", "head", "row"))
    plan.add("lses", F32, lses.shape, (PART_STRIDE_LSE, h * s, s, 1), BASE_MIN + (64 << 20), ("part", "batch", "head"))
    plan.check_disjoint()
    return plan, outs, lses


# ------------------------------------------------------------------------------------------------
# CPU self-tests: the tests can fail, and cannot leave the arena
# ------------------------------------------------------------------------------------------------
def all_plans():
    out = [read_case(n).plan for n in READS] + [lse_case(n).plan for n in LSE]
    out += [fp8_case("unsplit").plan, fp8_case("split").plan, ragged_case(False).plan, ragged_case(True).plan]
    out += [dense_case(n)[0] for n in DENSE]
    out += [merge_case()[0], merge_out_case()[0], varlen_case()[0]] + [dense_op_case(op)[0] for op in DENSE_OPS]
    out += [o_case(n).plan for _, n in PAGED_ABI] + [shared_case(h).plan for h in ("prefix", "suffix")]
    out += [append_case(kind, rope).plan for kind in ("uniform", "varlen") for rope in (False, True)] + [append_fp8_case().plan]
    return out + rule_plans()


def rule_plans():
    """The placements of every host-rule case of section (c), under and over each limit, as the GPU tests build them."""
    from test_fp8_kvcache import FP8 as e4m3

    out = []
    for which in ("kv", "qo"):
        st = check_params_case(which)[0]
        out += [rule_plan(f"rule_{which}", check_params_tensors(which, st)),
                rule_plan(f"rule_{which}_over", check_params_tensors(which, st + 8))]
    q, k, _ = small_qkv(8, 1, 1, 300, BF16, 7810)
    out += [qspan_plan("decode", q, k, qspan_limit(8)), qspan_plan("w4", q, k, qspan_limit(8) + 8)]
    top = rule_constants()["limit"]
    zz = (top - 256) // (2 * (130 + 32)) // 8 * 8
    q, k, v = small_qkv(4, 2, 130, 130, F16, 7820)
    out += [rule_plan(f"rule_zigzag_{w}", [("q", q, st), ("k", k, None), ("v", v, None), ("o", q, st)])
            for w, st in (("zigzag", zz), ("plain", zz + 8))]
    out.append(strided_pool_plan("rule_paged_prefill", (2, HKV, 128, D), F16, top // (2 * 128) // 8 * 8))
    out.append(strided_pool_plan("rule_fp8", (4, HKV, 64, D), e4m3, rule_limit(64) // 16 * 16))
    return out


# what every case claims to catch: (tensor, dim) -> the mistakes that must move at least one live row
CLAIMS = {
    "pool": {("kc", "page"): ("byte_i32", "byte_u32", "elem_i32"), ("vc", "page"): ("byte_i32", "byte_u32", "elem_i32")},
    "fp8": {("kc", "page"): ("byte_i32", "byte_u32", "elem_i32", "elem_u32"), ("kd", "batch"): ("byte_i32", "byte_u32"),
            ("vd", "batch"): ("byte_i32", "byte_u32")},
    "packed_q": {("q", "packed"): ("byte_i32", "byte_u32")},
    "batch": {(t, "batch"): ("byte_i32", "byte_u32", "elem_i32") for t in "qkvo"},
    "head": {(t, "head"): ("byte_i32", "byte_u32", "elem_i32") for t in "qkvo"},
    "varlen_packed": {(t, "packed"): ("byte_i32", "byte_u32", "elem_i32") for t in "qkv"},
    "merge": {("outs", "part"): ("byte_i32", "byte_u32", "elem_i32"), ("lses", "part"): ("byte_i32", "byte_u32")},
}


def claims_of(plan):
    n = plan.name
    if n in DENSE:
        return CLAIMS[DENSE[n][7]]
    if n in ("merge", "varlen_packed"):
        return CLAIMS[n]
    if n == "merge_out":
        return {**CLAIMS["merge"], ("out", "batch"): ("byte_i32", "byte_u32", "elem_i32"), ("lse", "batch"): ("byte_i32", "byte_u32")}
    if n.startswith("dense_"):
        return {(t, "packed" if n == "dense_varlen" else "batch"): ("byte_i32", "byte_u32", "elem_i32") for t in "qkvo"}
    if n.startswith("rule_"):  # what a rule protects is the ROW term of the tensors at the limit
        if n.startswith("rule_qspan"):  # (the rule stops 1 MiB short of 2^31: no 32-bit term wraps on either side)
            return {}
        if n == "rule_fp8":  # (page 3 of 4 starts 3.2e9 bytes in; the second page of rule_paged_prefill starts 2 KiB
            return {(t, "page"): ("byte_i32",) for t in ("kc", "vc")}  # short of 2^31: only page + row together cross)
        big = {"rule_kv": "kv", "rule_kv_over": "kv", "rule_qo": "qo", "rule_qo_over": "qo"}.get(n, ())
        return {(t, "row"): ("byte_i32", "byte_u32") for t in big}
    out = dict(CLAIMS["fp8"] if n.startswith("fp8") else CLAIMS["pool"])
    if n.endswith("packed_q"):
        out.update(CLAIMS["packed_q"])
    if n.startswith("o_") or n.startswith("fp8"):
        out[("o", "batch")] = ("byte_i32", "byte_u32", "elem_i32")
    if n.endswith("packed_q"):
        out[("o", "packed")] = ("byte_i32", "byte_u32")
    if n.startswith("lse_"):
        out[("o", "batch")] = out[("lse", "batch")] = ("byte_i32", "byte_u32")
    return out


def test_model_every_mistake_lands_inside_the_arena_on_other_data():
    """For every live row of every case and every single-term mistake: the wrong address lies inside the arena, and
    where it differs from the right one it holds pattern bytes, a poison row or another row's (seeded random)
    data -- never the row that should have been addressed."""
    seen = 0
    for plan in all_plans():
        for key, rec in plan.mistakes().items():
            assert 0 <= rec["lo"] and rec["hi"] <= ARENA_BYTES, (plan.name, key, hex(rec["lo"]), hex(rec["hi"]))
            if rec["changed"]:
                assert rec["lands_on_itself"] == 0, (plan.name, key)
                seen += 1
    assert seen > 100


def test_model_every_case_is_moved_by_the_mistakes_it_claims():
    """A case for which no listed mistake changes an address would be a wasted case."""
    for plan in all_plans():
        got = plan.mistakes()
        for (tensor, dim), ms in claims_of(plan).items():
            for m in ms:
                assert got[(tensor, dim, m)]["changed"] > 0, (plan.name, tensor, dim, m)


def test_model_docstring_landing_addresses():
    """The landing addresses the module docstring lists."""
    got = read_case("unsplit").plan.mistakes()
    kc = read_case("unsplit").plan.placements["kc"]
    rows = {int(p): int(a) for (p, h, r), a in zip(kc.live.tolist(), kc.right().tolist()) if h == 0 and r == 0}
    assert rows[65536] == 0x2_0000_0000 and rows[32768] == 0x1_8000_0000 and rows[0] == 0x1_0000_0000
    w = dict(zip(map(tuple, kc.live.tolist()), kc.wrong("page", "byte_u32").tolist()))
    assert w[(65536, 0, 0)] == 0x1_0000_0000
    w = dict(zip(map(tuple, kc.live.tolist()), kc.wrong("page", "byte_i32").tolist()))
    assert w[(32768, 0, 0)] == 0x0_8000_0000
    w = dict(zip(map(tuple, kc.live.tolist()), kc.wrong("page", "elem_i32").tolist()))
    assert w[(65536, 0, 0)] == 0
    assert got[("kc", "page", "elem_u32")]["changed"] == 0 and got[("kc", "page", "stride2_i32")]["changed"] == 0
    assert "kc" in got[("kc", "page", "byte_u32")]["lands"]  # page 65536 wraps onto page 0, a live decoy


def test_model_tables_cross_each_threshold_between_consecutive_pages():
    for name in ("unsplit", "split", "prefill_sq300", "page32"):
        c = read_case(name)
        thr = READS[name][10]
        crossings = set()
        for row in c.big_table.tolist():
            for a, b_ in zip(row, row[1:]):
                for t in thr:
                    if a >= 0 and b_ >= 0 and (a < t) != (b_ < t):
                        crossings.add(t)
        assert crossings == set(thr), (name, crossings)
        ids = {b for _, b in c.pairs}
        assert {0, 1, c.num_pages - 1} <= ids and all(t in ids and t - 1 in ids for t in thr)


def test_model_high_page_table_and_narrowing_helpers():
    assert s32(2 ** 31) == -2 ** 31 and s32(2 ** 32 + 5) == 5 and s32(-1) == -1
    assert MISTAKES["byte_u32"](65536, 32768, 2) == 0 and MISTAKES["elem_i32"](65536, 32768, 2) == -2 ** 32
    assert MISTAKES["stride2_i32"](3, 2 ** 30, 2) == 3 * -2 ** 31
    t = high_page_table([1, 5, 8], P64, (32768, 65536), 3)
    assert t[2][:4] == [32767, 32768, 65535, 65536] and t[1][:2] == [0, P64 - 1] and t[0] == [1]
    with pytest.raises(AssertionError):
        high_page_table([30], P64, (32768, 65536), 3)  # more pages than the pool has above the last threshold


# the host rules of section (c), on the CPU: the strides the GPU cases use sit within 8 elements of each limit
def rule_limit(rows):
    """The largest stride (a multiple of 8 elements) with stride * 2 * rows + 256 <= 0x7fffffff."""
    return (rule_constants()["limit"] - 256) // (2 * rows) // 8 * 8


def test_model_rule_strides_sit_at_the_limits():
    k_, top = launch_constants(), rule_constants()["limit"]
    assert (k_["kBlockN"], k_["kQoSpanRows"]) == (64, 160)
    for rows in (k_["kBlockN"], k_["kQoSpanRows"]):
        st = rule_limit(rows)
        assert st * 2 * rows + 256 <= top < (st + 8) * 2 * rows + 256
        assert s32((rows - 1) * st * 2) == (rows - 1) * st * 2  # admitted: the tile's last row offset fits int32
        assert s32((rows - 1) * 2 * st * 2) != (rows - 1) * 2 * st * 2  # a rule off by two would admit a wrap
    st = 0x7fffffff // (2 * 128) // 8 * 8  # the paged prefill rule: page_size * stride * 2 <= 0x7fffffff
    assert 128 * st * 2 <= 0x7fffffff < 128 * (st + 8) * 2


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena(device):
    free, total = torch.cuda.mem_get_info(device)
    need = ARENA_BYTES + 2 * GIB
    if free < need:
        pytest.skip(f"the large-address arena needs {need / GIB:.1f} GiB of free device memory ({ARENA_BYTES / GIB:.0f} GiB "
                    f"+ 2 GiB), {free / GIB:.1f} GiB are free")
    print(f"LARGE_ARENA bytes={ARENA_BYTES} free_before={free} total={total}")
    a = BigArena(device)
    yield a
    del a.buf, a.words
    torch.cuda.empty_cache()


@pytest.fixture
def fam(device):
    from flash_attention_cute_amd import _debug
    from flash_attention_cute_amd import flash_attention as fam

    assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
    _debug.set_knobs()
    _debug.set_dec_fuse(None)
    yield fam
    _debug.set_knobs()
    _debug.set_dec_fuse(None)


PAT = pytest.mark.parametrize("pattern", PATTERNS, ids=["ff", "7b"])


@pytest.mark.gpu
@PAT
def test_arena_check_sees_one_stray_byte_and_one_changed_input(arena, pattern):
    """The write check itself: one byte 2 GiB below a declared output, and one changed input element, are reported;
    after the erase the arena is clean again."""
    plan = Plan("self")
    pi, po = plan.small("in", F16, (4, 8)), plan.small("out", F16, (4, 8), written=True)
    with arena.case(pattern):
        arena.load(arena.view(pi), torch.ones(4, 8, dtype=F16))
        out = arena.expect(arena.view(po), "out")
        out.fill_(2.0)
        arena.buf[po.base - 2 * GIB + 3] = 0x11
        with pytest.raises(AssertionError, match="no longer hold the pattern") as e:
            arena.settle()
        assert hex((po.base - 2 * GIB) // 8 * 8) in str(e.value)
        arena.buf[po.base - 2 * GIB + 3] = pattern
        assert arena.stray() == []
        v = arena.load(arena.view(pi), torch.ones(4, 8, dtype=F16))
        v[2, 5] = 3.0
        with pytest.raises(AssertionError, match="inputs changed"):
            arena.settle()
        assert arena.stray() == []


def compact_pools(c):
    return dv(c.q, c.kc, c.vc, c.table, c.sl)


# ---- (a) paged reads
@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("name", DECODE + PREFILL)
def test_paged_reads(arena, fam, name, pattern):
    from flash_attention_cute_amd import _debug

    lens, hq, sq, page, cap, causal, w, dtype, layout, num_pages, thr = READS[name]
    c = read_case(name)
    _debug.set_dec_fuse(0 if name == "split_unfused" else None)
    with arena.case(pattern):
        q, kc, vc, table, sl = c.load(arena)
        assert kc.stride(0) * (kc.size(0) - 1) * kc.element_size() >= 2 ** 32  # the last page starts past 2^32 bytes
        out = fam.flash_attn_paged_func(q, kc, vc, table, sl, causal=causal, window_left=w)
        path, fused, in_place = _debug.last_path(), _debug.last_dec_fused(), _debug.last_prefill_paged()
        arena.settle()
    check_padded(out, read_oracle(name), dtype)
    small = fam.flash_attn_paged_func(*compact_pools(c), causal=causal, window_left=w)
    assert (path, in_place) == (_debug.last_path(), _debug.last_prefill_paged())
    if name in PREFILL:
        assert path == "w4" and in_place
    else:
        assert path == ("decode_paged_split" if name.startswith("split") else "decode_paged")
        if name.startswith("split"):
            assert fused == (name == "split")
    assert torch.equal(out, small)
    for i, n in enumerate(lens):
        if n == 0:
            assert (out[i] == 0).all()


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("name", LSE)
def test_paged_lse_with_out_and_lse_in_the_arena(arena, fam, name, pattern):
    """The LSE launch writes o and lse through views the caller gives: both lie in the arena, at the batch strides of
    ``lse_case`` (o 2^31 + 64 elements for B = 2, 3 * 2^28 + 64 for B = 4; lse, fp32, 2^30 + 8 and 3 * 2^27 + 8)."""
    from flash_attention_cute_amd import _debug

    lens, hq, sq, page, cap, causal, w, dtype, layout, num_pages, thr = READS[name]
    c = lse_case(name)
    _debug.set_dec_fuse(0 if name == "split_unfused" else None)
    with arena.case(pattern):
        q, kc, vc, table, sl = c.load(arena)
        o = arena.expect(arena.view(c.plan.placements["o"]), "o")
        lse = arena.expect(arena.view(c.plan.placements["lse"]), "lse")
        fam._lse_into(q, kc, vc, table, sl, 0, None, None, D ** -0.5, causal, o, lse)
        path = _debug.last_path()
        got = arena.settle()
    assert path == ("decode_paged_split" if name.startswith("split") else "decode_paged")
    check_padded(got["o"], read_oracle(name), dtype)
    check_lse(got["lse"], lse_oracle(c.q, c.k, lens, D ** -0.5, causal), f"large-{name}")
    so, sl_ = fam.flash_attn_paged_func(*compact_pools(c), causal=causal, return_lse=True)
    assert torch.equal(got["o"], so) and torch.equal(got["lse"], sl_)


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("kind", ["unsplit", "split"])
def test_paged_fp8_with_descales_at_large_strides(arena, fam, kind, pattern):
    from flash_attention_cute_amd import _debug
    from test_fp8_kvcache import fp8_oracle

    c = fp8_case(kind)
    with arena.case(pattern):
        q, kc, vc, table, sl = c.load(arena)
        assert kc.dtype == FP8 and kc.stride(0) == 65536
        kd = arena.load(arena.view(c.plan.placements["kd"]), c.kd)
        vd = arena.load(arena.view(c.plan.placements["vd"]), c.vd)
        out = fam.flash_attn_paged_func(q, kc, vc, table, sl, k_descale=kd, v_descale=vd)
        path = _debug.last_path()
        arena.settle()
    assert path == ("decode_paged_fp8_split" if kind == "split" else "decode_paged_fp8")
    check_padded(out, fp8_oracle(c.q, c.k, c.v, c.sl, c.kd, c.vd, False), BF16)
    small = fam.flash_attn_paged_func(*compact_pools(c), k_descale=c.kd.to(DEV), v_descale=c.vd.to(DEV))
    assert path == _debug.last_path() and torch.equal(out, small)


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("packed_q", [False, True], ids=["q_compact", "q_packed_rows_past_4GiB"])
def test_paged_varlen(arena, fam, packed_q, causal, pattern):
    from flash_attention_cute_amd import _debug

    c = ragged_case(packed_q)
    r = c.ragged
    with arena.case(pattern):
        q, kc, vc, table, sl = c.load(arena)
        cu_q = arena.load(arena.view(c.plan.placements["cu_q"]), r.cu_q)
        out = fam.flash_attn_paged_varlen_func(q, kc, vc, cu_q, r.max_q, table, sl, causal=causal)
        labels = _debug.last_path(), _debug.last_prefill_paged()
        arena.settle()
    assert labels == ("w4", True)
    check_padded(out, r.oracle(causal), F16)
    small = fam.flash_attn_paged_varlen_func(*dv(r.q, r.kc, r.vc, r.cu_q), r.max_q, *dv(r.table, r.sl), causal=causal)
    assert torch.equal(out, small)


@functools.lru_cache(maxsize=None)
def shared_case(high):
    from test_shared_prefix import make_shared

    b, hq, page, prefix = 6, 8, 64, 128
    q, k, v, kc, vc, table, sl, grp = make_shared(b, hq, HKV, page, prefix, (0, 1, 31, 33, 70, 64), D, F16, 7500)
    n_pre = prefix // page
    lens = sl.tolist()
    # (one group of six sequences: two prefix pages, six suffix pages; the high list starts past 2^32 bytes, then
    # past 2^31, so the two prefix pages -- or the first suffix pages -- lie on both sides of both thresholds)
    lows, highs = [0, 32767, 1, 2, 3, 32766], [65536, 32768, P64 - 1, 65535, 65537, 65538, 65539, 65540]
    pre, suf = (highs, lows) if high == "prefix" else (lows, highs)
    pre, suf, first, ids = list(pre), list(suf), {}, []
    for i in range(b):
        lead = i // grp * grp
        if i == lead:
            first[i] = [pre.pop(0) for _ in range(n_pre)]
        ids.append(first[lead] + [suf.pop(0) for _ in range((lens[i] + page - 1) // page - n_pre)])
    c = PagedCase(f"shared_{high}", (q, k, v, kc, vc, table, sl), P64, page, "phsd", ids=ids)
    return c


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("high", ["prefix", "suffix"])
def test_shared_prefix_with_the_prefix_and_the_suffix_on_opposite_sides(arena, fam, high, pattern):
    from test_shared_prefix import check_bound

    c, prefix = shared_case(high), 128
    q, k, v, sl = c.q, c.k, c.v, c.sl
    with arena.case(pattern):
        args = c.load(arena)
        out = fam.flash_attn_paged_shared_prefix_func(*args, prefix)
        arena.settle()
    check_bound(out, oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, D ** -0.5, False), F16, 1.0, high)
    assert torch.equal(out, fam.flash_attn_paged_shared_prefix_func(*compact_pools(c), prefix))


# ---- (a) appends
APPEND_LENS, APPEND_NEWS, APPEND_SQS = (63, 64, 30, 100, 0), (1, 40, 0, 300, 300), (1, 40, 7, 300, 301)
# the uniform and FP8 appends, lens (0, 31, 95, 449) + 40 tokens: the rows written are positions 0-39 of sequence 0 (its
# page 0), 31-70 of sequence 1 (pages 0, 1), 95-134 of sequence 2 (pages 1, 2), 449-488 of sequence 3 (page 7). The
# destinations are then 32768 and 65535 (between 2^31 and 2^32 bytes), 65536 and P - 1 (past 2^32), 32767 and 0 (below)
UNIFORM_APPEND_IDS = [[32768], [65535, 65536], [65537, 32767, P64 - 1], [65538, 65539, 65540, 65541, 65542, 65543, 65544, 0]]


@functools.lru_cache(maxsize=None)
def append_case(kind, rope):
    """A cache with room for the new tokens (rows without a key hold test_kvcache.PATTERN), its pages at high ids."""
    from test_kvcache import make_cache
    from test_paged_varlen import ragged_cache

    page, cap, dtype, ids = 64, 512, F16 if rope else BF16, None
    if kind == "varlen":
        kc, vc, table, sl = ragged_cache(APPEND_LENS, APPEND_NEWS, HKV, page, cap, D, dtype, 7600, "phsd")
        after = [min(n + m, cap) for n, m in zip(APPEND_LENS, APPEND_NEWS)]
    else:
        lens, sn = (0, 31, 95, 449), 40
        kc, vc, table, sl = make_cache(lens, sn, HKV, page, cap, D, dtype, 7601, "phsd")
        after = [min(n + sn, cap) for n in lens]
        ids = UNIFORM_APPEND_IDS
    reach = torch.tensor(after, dtype=I32)  # (the pages placed are those the sequences reach AFTER the append)
    c = PagedCase(f"append_{kind}{'_rope' if rope else ''}", (torch.zeros(1, 1, 1, D, dtype=dtype), None, None, kc, vc,
                                                              table, reach), P64, page, "phsd", ids=ids,
                  thresholds=(32768, 65536), seed=7600)
    c.sl = sl
    return c


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
def test_append_varlen(arena, fam, rope, pattern):
    from flash_attention_cute_amd import flash_attn_kvcache_append_varlen

    c = append_case("varlen", rope)
    dtype, cap, hq = c.kc.dtype, 512, 8
    cu_new, cu_q = cu_of(APPEND_NEWS), cu_of(APPEND_SQS)
    k, v = packed_rows(sum(APPEND_NEWS), HKV, D, dtype, 1), packed_rows(sum(APPEND_NEWS), HKV, D, dtype, 2)
    q = packed_rows(sum(APPEND_SQS), hq, D, dtype, 3) if rope else None
    cos, sin = rope_tables(cap, D, dtype) if rope else (None, None)
    ref = per_sequence_append(*dv(c.kc, c.vc, k, v, cu_new, c.sl, c.table, cos, sin, q), cu_q.to(DEV) if rope else None)
    with arena.case(pattern):
        _, kc, vc, table, sl = c.load(arena, updated=True)
        ins = small_inputs(arena, c, k=k, v=v, cu_new=cu_new, cos=cos, sin=sin, q_new=q, cu_q=cu_q if rope else None)
        got = flash_attn_kvcache_append_varlen(kc, vc, ins[0], ins[1], ins[2], sl, table, *ins[3:])
        pages = arena.settle()
    new, q_rot = got if rope else (got, None)
    check_appended_pages(c, pages, ref[0], ref[1])
    assert torch.equal(new, ref[2]) and new.tolist() == [min(n + m, cap) for n, m in zip(APPEND_LENS, APPEND_NEWS)]
    if rope:
        assert torch.equal(q_rot.view(torch.int16), ref[3].view(torch.int16))


def small_inputs(arena, c, **tensors):
    """The other inputs of a launch (new tokens, RoPE tables, cumulative lengths, descales ...) as compact views in
    the arena's small zone, loaded; None stays None. The placements join the case's plan the first time."""
    out = []
    for nm, t in tensors.items():
        if t is None:
            out.append(None)
            continue
        if nm not in c.plan.placements:
            c.plan.small(nm, t.dtype, t.shape)
        out.append(arena.load(arena.view(c.plan.placements[nm]), t))
    return out


def check_appended_pages(c, pages, kc_ref, vc_ref):
    """Every page copied out of the arena holds the reference's bits, and something was written."""
    changed = 0
    for small, _ in c.pairs:
        for nm, ref, old in (("kc", kc_ref, c.kc), ("vc", vc_ref, c.vc)):
            got = pages[f"{nm}{small}"].view(torch.int16)
            assert torch.equal(got, ref[small].view(torch.int16)), f"{nm} page {small}"
            changed += int((got.cpu() != old[small].view(torch.int16)).any())
    assert changed > 0


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
def test_append_uniform(arena, fam, rope, pattern):
    from flash_attention_cute_amd import apply_rope, flash_attn_kvcache_append

    c = append_case("uniform", rope)
    dtype, cap, sn, lens = c.kc.dtype, 512, 40, (0, 31, 95, 449)
    k, v = new_tokens(4, HKV, sn, D, dtype, 50), new_tokens(4, HKV, sn, D, dtype, 51)
    cos, sin = rope_tables(cap, D, dtype) if rope else (None, None)
    ek, ev = expected_append(*dv(c.kc, c.vc, k, v), lens, c.table, *dv(cos, sin), apply_rope)
    with arena.case(pattern):
        _, kc, vc, table, sl = c.load(arena, updated=True)
        new = flash_attn_kvcache_append(kc, vc, *small_inputs(arena, c, k=k, v=v), sl, table,
                                        *small_inputs(arena, c, cos=cos, sin=sin))
        pages = arena.settle()
    check_appended_pages(c, pages, ek, ev)
    assert new.tolist() == [min(n + sn, cap) for n in lens]


@functools.lru_cache(maxsize=None)
def append_fp8_case():
    from test_fp8_kvcache import make_fp8_cache

    page, cap, sn, lens = 64, 512, 40, (0, 31, 95, 449)
    kc8, vc8, table, sl = make_fp8_cache(lens, sn, HKV, page, cap, D, 7700, "phsd")
    after = torch.tensor([min(n + sn, cap) for n in lens], dtype=I32)
    c = PagedCase("append_fp8", (torch.zeros(1, 1, 1, D, dtype=F16), None, None, kc8, vc8, table, after), P64, page, "phsd",
                  ids=UNIFORM_APPEND_IDS)
    c.sl, c.after = sl, after
    return c


@pytest.mark.gpu
@PAT
def test_append_fp8(arena, fam, pattern):
    from flash_attention_cute_amd import apply_rope, flash_attn_kvcache_append
    from test_fp8_kvcache import expected_fp8_append, norm_bytes

    page, cap, sn, lens = 64, 512, 40, (0, 31, 95, 449)
    c = append_fp8_case()
    kc8, vc8, table, sl, after = c.kc, c.vc, c.table, c.sl, c.after
    kd, vd = pow2_descales(4, HKV), pow2_descales(4, HKV, 3)
    k, v = new_tokens(4, HKV, sn, D, F16, 52), new_tokens(4, HKV, sn, D, F16, 53)
    cos, sin = rope_tables(cap, D, F16)
    ek, ev = expected_fp8_append(*dv(kc8, vc8, k, v), list(lens), table, *dv(cos, sin), apply_rope, kd, vd)
    with arena.case(pattern):
        _, kc, vc, tb, sl_ = c.load(arena, updated=True)
        dk, dv_, dcos, dsin, dkd, dvd = small_inputs(arena, c, k=k, v=v, cos=cos, sin=sin, kd=kd, vd=vd)
        new = flash_attn_kvcache_append(kc, vc, dk, dv_, sl_, tb, dcos, dsin, k_descale=dkd, v_descale=dvd)
        pages = arena.settle()
    assert new.tolist() == after.tolist()
    for small, _ in c.pairs:
        assert torch.equal(norm_bytes(pages[f"kc{small}"].cpu()), norm_bytes(ek[small].cpu())), f"K page {small}"
        assert torch.equal(norm_bytes(pages[f"vc{small}"].cpu()), norm_bytes(ev[small].cpu())), f"V page {small}"


def step_oracle(q_rot, kc, vc, table, new_lens, counts, causal, page=64):
    """oracle_padded per sequence on the post-append cache (test_paged_varlen's step test): the dense keys gathered
    back from the compact reference pool, q as the append rotated it; q_rot packed [total, Hq, D], sequence b owning
    ``counts[b]`` rows."""
    kc_h, vc_h, qr = kc.cpu(), vc.cpu(), q_rot.cpu()
    want, r = torch.zeros_like(qr), cu_of(counts).tolist()
    for b, n in enumerate(new_lens):
        if counts[b] == 0:
            continue
        ids = table[b, :(n + page - 1) // page].long()
        kd = kc_h[ids].transpose(0, 1).flatten(1, 2)[None, :, :n]
        vd = vc_h[ids].transpose(0, 1).flatten(1, 2)[None, :, :n]
        one = oracle_padded(qr[r[b]:r[b + 1]].transpose(0, 1)[None], kd, vd, torch.tensor([0], dtype=I32),
                            torch.tensor([n], dtype=I32), None, None, D ** -0.5, causal)
        want[r[b]:r[b + 1]] = one[0].transpose(0, 1)
    return want


@pytest.mark.gpu
@PAT
def test_with_kvcache_steps_once_eagerly(arena, fam, pattern):
    """flash_attn_with_kvcache and flash_attn_varlen_with_kvcache, one eager step each on the high pages: the float64
    oracle on the post-append keys and the rotated q under TOL, then the bits of the same step on the compact pool."""
    from flash_attention_cute_amd import flash_attn_varlen_with_kvcache, flash_attn_with_kvcache

    c = append_case("uniform", True)
    dtype, cap, sn, hq = c.kc.dtype, 512, 40, 8
    k, v, q = dv(new_tokens(4, HKV, sn, D, dtype, 60), new_tokens(4, HKV, sn, D, dtype, 61), new_tokens(4, hq, sn, D, dtype, 62))
    cos, sin = dv(*rope_tables(cap, D, dtype))
    kc_s, vc_s = dv(c.kc.clone(), c.vc.clone())
    want = flash_attn_with_kvcache(q, kc_s, vc_s, k, v, cos, sin, c.sl.to(DEV), c.table.to(DEV), causal=True)
    kc_r, vc_r = dv(c.kc.clone(), c.vc.clone())  # the append alone, for the rotated q and the new lengths
    new, q_rot = torch.ops.flash_attention.kvcache_append(kc_r, vc_r, k, v, c.sl.to(DEV), c.table.to(DEV), q, cos, sin)
    with arena.case(pattern):
        _, kc, vc, table, sl = c.load(arena, updated=True)
        out = flash_attn_with_kvcache(q, kc, vc, k, v, cos, sin, sl, table, causal=True)
        pages = arena.settle()
    check_appended_pages(c, pages, kc_s, vc_s)
    ref = step_oracle(q_rot.transpose(1, 2).reshape(-1, hq, D), kc_r, vc_r, c.table, new.tolist(), [sn] * 4, True)
    check_padded(out, ref.reshape(4, sn, hq, D).transpose(1, 2), dtype)
    assert torch.equal(out, want)

    c = append_case("varlen", True)  # (a step's new tokens are its queries: cu_seqlens_q is cu_seqlens_new)
    cu = cu_of(APPEND_NEWS).to(DEV)
    k, v = dv(packed_rows(sum(APPEND_NEWS), HKV, D, dtype, 1), packed_rows(sum(APPEND_NEWS), HKV, D, dtype, 2))
    q = packed_rows(sum(APPEND_NEWS), hq, D, dtype, 3).to(DEV)
    kc_s, vc_s = dv(c.kc.clone(), c.vc.clone())
    want = flash_attn_varlen_with_kvcache(q, kc_s, vc_s, cu, max(APPEND_NEWS), k, v, cu, cos, sin, c.sl.to(DEV),
                                          c.table.to(DEV), causal=True)
    kc_r, vc_r = dv(c.kc.clone(), c.vc.clone())
    new, q_rot = fam.flash_attn_kvcache_append_varlen(kc_r, vc_r, k, v, cu, c.sl.to(DEV), c.table.to(DEV), cos, sin, q, cu)
    with arena.case(pattern):
        _, kc, vc, table, sl = c.load(arena, updated=True)
        out = flash_attn_varlen_with_kvcache(q, kc, vc, cu, max(APPEND_NEWS), k, v, cu, cos, sin, sl, table, causal=True)
        pages = arena.settle()
    check_appended_pages(c, pages, kc_s, vc_s)
    check_padded(out, step_oracle(q_rot, kc_r, vc_r, c.table, new.tolist(), APPEND_NEWS, True), dtype)
    assert torch.equal(out, want)


# ---- (b) dense tensors with large batch, head and part strides, through the C ABI (q, k, v AND o in the arena)
def c_abi_forward(views, causal, dtype, scale, row_strides=None):
    """fa_fwd_gfx950 on the given q, k, v, o views (include/fa_gfx950.h; the host steps of _debug.forward).
    ``row_strides``: (q, k, v, o) sequence strides passed INSTEAD of the views' (None: the view's) -- for calls the
    library must refuse before it touches a buffer."""
    from flash_attention_cute_amd import _debug

    q, k, v, o = views
    lib = _debug.lib()
    b, hq, sq, d = q.shape
    hkv, sk = k.size(1), k.size(2)
    st = lambda t, i: t.stride(i) if t.size(i) > 1 else 0  # noqa: E731
    strides = [st(t, i) for i in range(3) for t in (q, k, v, o)]
    for j, r in enumerate(row_strides or ()):
        strides[8 + j] = strides[8 + j] if r is None else r
    p = _debug.FaFwdParams(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), b, hq, hkv, sq, sk, d, hq // hkv,
                           *strides,
                           float(torch.tensor(scale, dtype=torch.float32).double() * _debug.LOG2E))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.fa_fwd_gfx950(ctypes.byref(p), 0 if dtype == F16 else 1, int(causal), stream)
    return rc, (lib.fa_last_error().decode() if rc else ""), _debug.last_path()


def dense_oracle(q, k, v, causal):
    b, sq, sk = q.size(0), q.size(2), k.size(2)
    zero, full = torch.zeros(b, dtype=I32), torch.full((b,), sk, dtype=I32)
    return oracle_padded(q, k, v, zero, full, None, None, D ** -0.5, causal)


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_forward_with_large_batch_and_head_strides(arena, fam, name, pattern):
    plan, (q, k, v), causal = dense_case(name)
    dtype = q.dtype
    with arena.case(pattern):
        views = [arena.load(arena.view(plan.placements[n]), t) for n, t in (("q", q), ("k", k), ("v", v))]
        views.append(arena.expect(arena.view(plan.placements["o"]), "o"))
        rc, err, path = c_abi_forward(views, causal, dtype, D ** -0.5)
        got = arena.settle()
    assert rc == 0, err
    assert path == ("decode" if q.size(2) == 1 else "w4")
    check_padded(got["o"], dense_oracle(q, k, v, causal), dtype)
    # the same launch on contiguous tensors: the plan depends on the shape alone (grid = q-tiles x heads x batch;
    # decode_plan: units and Sk), never on a stride
    cq, ck, cv = dv(q, k, v)
    co = torch.empty_like(cq)
    rc2, err2, path2 = c_abi_forward((cq, ck, cv, co), causal, dtype, D ** -0.5)
    torch.cuda.synchronize()
    assert rc2 == 0 and path2 == path and torch.equal(got["o"], co)


DENSE_OPS = ["padded", "window", "rope", "varlen"]


@functools.lru_cache(maxsize=None)
def dense_op_case(op):
    """The batch_prefill tensors for one dense entry of the C ABI, q, k, v AND o at a batch stride of 2^31 + 128
    elements (varlen: packed, rows PACKED_ROW_STRIDE elements apart), with the entry's small arrays (key ranges,
    RoPE tables, cumulative lengths) in the arena's small zone. Returns (plan, host tensors by name, oracle)."""
    from test_rope import oracle_rope, tables

    _, (q, k, v), _ = dense_case("batch_prefill")
    b, sq, scale = q.size(0), q.size(2), D ** -0.5
    zero, full = torch.zeros(b, dtype=I32), torch.full((b,), sq, dtype=I32)
    plan, host = Plan(f"dense_{op}"), {}
    if op == "varlen":
        host.update(zip("qkv", varlen_case()[1]))
        for i, nm in enumerate("qkvo"):
            t = host["q" if nm == "o" else nm]
            plan.add(nm, t.dtype, t.shape, (PACKED_ROW_STRIDE, D, 1), BASE_MIN + (i + 1) * (4 << 20), ("packed", "head"),
                     written=nm == "o")
        host["cu"] = cu_of([sq] * b)
        ref = lambda: dense_oracle(q, k, v, True).transpose(1, 2).reshape(-1, q.size(1), D)  # noqa: E731
    else:
        host.update(q=q, k=k, v=v)
        for i, nm in enumerate("qkvo"):
            t = host["q" if nm == "o" else nm]
            plan.add(nm, t.dtype, t.shape, (BATCH_STRIDE, t.size(2) * D, D, 1), BASE_MIN + (i + 1) * (32 << 20),
                     ("batch", "head", "row"), written=nm == "o")
        if op == "padded":
            host["ks"], host["ke"] = torch.tensor([7, 0], dtype=I32), torch.tensor([300, 261], dtype=I32)
            ref = lambda: oracle_padded(q, k, v, host["ks"], host["ke"], None, None, scale, True)  # noqa: E731
        elif op == "window":
            ref = lambda: oracle_padded(q, k, v, zero, full, None, None, scale, True, window_left=100)  # noqa: E731
        else:
            host["cos"], host["sin"] = tables(b, sq, D, q.dtype, 7350)
            ref = lambda: dense_oracle(oracle_rope(q, host["cos"], host["sin"]), k, v, True)  # noqa: E731
    for nm in ("ks", "ke", "cu", "cos", "sin"):
        if nm in host:
            plan.small(nm, host[nm].dtype, host[nm].shape, ("batch", "row")[:host[nm].dim() - 1])
    plan.check_disjoint()
    return plan, host, ref


def abi_base(q, k, v, o, packed=None):
    """fa_fwd_params of include/fa_gfx950.h for 4-D views, or (``packed`` = (batch, max_q, max_k)) for packed 3-D
    ones: rows are dimension 0 and the four batch strides stay 0, as the binding passes them."""
    from flash_attention_cute_amd import _debug
    from test_abi import FaFwdParams

    sc = float(torch.tensor(D ** -0.5, dtype=torch.float32).double() * _debug.LOG2E)
    ptrs = [t.data_ptr() for t in (q, k, v, o)]
    if packed:
        nb, mq, mk = packed
        return FaFwdParams(*ptrs, nb, q.size(1), k.size(1), mq, mk, D, q.size(1) // k.size(1), 0, 0, 0, 0,
                           *(t.stride(1) for t in (q, k, v, o)), *(t.stride(0) for t in (q, k, v, o)), sc)
    st = lambda t, i: t.stride(i) if t.size(i) > 1 else 0  # noqa: E731
    return FaFwdParams(*ptrs, q.size(0), q.size(1), k.size(1), q.size(2), k.size(2), D, q.size(1) // k.size(1),
                       *(st(t, i) for i in range(3) for t in (q, k, v, o)), sc)


def arena_workspace(arena, need):
    """``need`` bytes of the arena, 128 MiB below its end, declared as written (scratch: its content is not compared);
    None for no workspace. Exactly the bytes asked for: one byte more written is a stray byte."""
    if not need:
        return None
    at = ARENA_BYTES - 128 * MIB
    return arena.expect(arena.buf[at:at + need], "ws")


def plain_workspace(need):
    return torch.empty(need, dtype=torch.uint8, device=DEV) if need else None


def ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def abi_dense_op(arena, op, q, k, v, o, aux, dtype):
    """One causal launch of the dense entry ``op`` through the C ABI; ``aux``: its small device arrays by name."""
    from flash_attention_cute_amd import _debug
    from test_abi import FaPaddedParams, FaRopeFwdParams, FaVarlenParams

    lib, i64 = _debug.lib(), ctypes.c_int64
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt = 0 if dtype == F16 else 1
    if op == "varlen":
        cu = aux["cu"]
        p = FaVarlenParams(abi_base(q, k, v, o, packed=(cu.numel() - 1, 300, 300)), cu.data_ptr(), cu.data_ptr())
        rc = lib.fa_fwd_gfx950_varlen(ctypes.byref(p), dt, 1, stream)
    elif op == "window":
        p = abi_base(q, k, v, o)
        rc = lib.fa_fwd_gfx950_window(ctypes.byref(p), dt, 1, i64(100), stream)
    elif op == "rope":
        cos, sin = aux["cos"], aux["sin"]
        p = FaRopeFwdParams(abi_base(q, k, v, o), cos.data_ptr(), sin.data_ptr(), cos.stride(0), cos.stride(1))
        rc = lib.fa_fwd_gfx950_rope(ctypes.byref(p), dt, 1, stream)
    else:
        p = FaPaddedParams(abi_base(q, k, v, o), None, None, aux["ks"].data_ptr(), aux["ke"].data_ptr())
        lib.fa_fwd_gfx950_padded_workspace_size.restype = i64
        need = lib.fa_fwd_gfx950_padded_workspace_size(ctypes.byref(p), dt, 1, i64(-1))
        assert 0 <= need <= 64 * MIB, (need, lib.fa_last_error().decode())
        ws = arena_workspace(arena, need)  # (the lowered ranges; exactly the bytes asked for, pattern all around)
        rc = lib.fa_fwd_gfx950_padded(ctypes.byref(p), dt, 1, i64(-1), ptr(ws), i64(need), stream)
    return rc, (lib.fa_last_error().decode() if rc else ""), _debug.last_path()


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("op", DENSE_OPS)
def test_dense_entries_with_q_k_v_and_o_past_4_gib(arena, fam, op, pattern):
    """fa_fwd_gfx950_padded / _window / _rope / _varlen through the C ABI, so that o lies in the arena as well: every
    tensor's batch stride is 2^31 + 128 elements (varlen: packed rows 6.8 MiB apart, row 599 past 2^32 bytes). Each
    against its float64 oracle, then bit for bit against the public op on contiguous tensors (the grid depends on the
    shape alone)."""
    plan, host, ref = dense_op_case(op)
    dtype = host["q"].dtype
    with arena.case(pattern):
        dev = {nm: arena.load(arena.view(plan.placements[nm]), t) for nm, t in host.items()}
        o = arena.expect(arena.view(plan.placements["o"]), "o")
        assert o.stride(0) * (o.size(0) - 1) * 2 > 2 ** 32
        rc, err, path = abi_dense_op(arena, op, dev["q"], dev["k"], dev["v"], o, dev, dtype)
        got = arena.settle()
    assert rc == 0 and path == "w4", (rc, err, path)
    check_padded(got["o"], ref(), dtype)
    cq, ck, cv = dv(host["q"], host["k"], host["v"])
    if op == "padded":
        small = fam.flash_attn_padded_func(cq, ck, cv, *dv(host["ks"], host["ke"]), causal=True)
    elif op == "window":
        small = fam.flash_attn_window_func(cq, ck, cv, 100, causal=True)
    elif op == "rope":
        small = fam.flash_attn_rope_func(cq, ck, cv, *dv(host["cos"], host["sin"]), causal=True)
    else:
        cu = host["cu"].to(DEV)
        small = fam.flash_attn_varlen_func(cq, ck, cv, cu, cu, 300, 300, causal=True)
    assert torch.equal(got["o"], small)


O_BATCH_STRIDE = {2: 2 ** 31 + 64, 3: 2 ** 30 + 64, 4: 3 * 2 ** 28 + 64}  # elements: the last batch row past 2^32 bytes


@functools.lru_cache(maxsize=None)
def o_case(name):
    """read_case(name) with o in the arena as well, between the pool's live pages, at O_BATCH_STRIDE[B]."""
    lens, hq, sq, page, cap, causal, w, dtype, layout, num_pages, thr = READS[name]
    c = PagedCase(f"o_{name}", read_case(name).compact, num_pages, page, layout, thresholds=thr,
                  seed=7000 + sorted(READS).index(name))
    c.plan.add("o", dtype, (len(lens), hq, sq, D), (O_BATCH_STRIDE[len(lens)], sq * D, D, 1), POOL_BASE + MIB,
               ("batch", "head", "row"), written=True)
    c.plan.check_disjoint()
    return c


def abi_paged(kind, q, kc, vc, o, table, sl, causal, dtype, workspace, w=-1, kd=None, vd=None, cu=None, max_q=None):
    """One launch of a paged entry of the C ABI -- "paged" (fa_fwd_gfx950_paged), "window", "fp8", "prefill",
    "varlen" -- as the binding fills its parameters (decode steps unpacked: g q-heads of one row each).
    ``workspace(need)`` gives the workspace tensor (or None). Returns (rc, error text, last_path, last_prefill_paged)."""
    from flash_attention_cute_amd import _debug
    from test_fp8_abi import FaPagedFp8Params
    from test_paged_abi import FaPagedParams
    from test_paged_varlen_abi import FaPagedVarlenParams

    lib, i64 = _debug.lib(), ctypes.c_int64
    page, num_pages = kc.size(2), kc.size(0)
    base = abi_base(q, kc, vc, o, packed=(sl.numel(), max_q, 0)) if kind == "varlen" else abi_base(q, kc, vc, o)
    base.seqlen_kv = table.size(1) * page
    for t, c in (("k", kc), ("v", vc)):
        for i, dim in enumerate(("batch", "head", "seqlen")):
            setattr(base, f"{t}_{dim}_stride", c.stride(i))
    p = FaPagedParams(base, table.data_ptr(), table.stride(0), table.size(1), num_pages, page, sl.data_ptr())
    dt, ca = (0 if dtype == F16 else 1), int(causal)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    stem, extra = {"paged": ("fa_fwd_gfx950_paged", ()), "window": ("fa_fwd_gfx950_paged_window", (i64(w),)),
                   "fp8": ("fa_fwd_gfx950_paged_fp8", ()), "prefill": ("fa_fwd_gfx950_paged_prefill", (i64(w),)),
                   "varlen": ("fa_fwd_gfx950_paged_varlen", (i64(w),))}[kind]
    if kind == "fp8":
        p = FaPagedFp8Params(p, kd.data_ptr(), vd.data_ptr(), kd.stride(0), kd.stride(1))
    elif kind == "varlen":
        p = FaPagedVarlenParams(p, cu.data_ptr(), q.size(0))
    size = getattr(lib, stem + "_workspace_size")
    size.restype = i64
    need = size(ctypes.byref(p), dt, ca, *extra)
    assert 0 <= need <= 64 * MIB, (need, lib.fa_last_error().decode())
    ws = workspace(need)
    rc = getattr(lib, stem)(ctypes.byref(p), dt, ca, *extra, ptr(ws), i64(need), stream)
    torch.cuda.synchronize()
    return rc, (lib.fa_last_error().decode() if rc else ""), _debug.last_path(), _debug.last_prefill_paged()


PAGED_ABI = [("paged", n) for n in ("unsplit", "split", "split_unfused", "sq3_causal", "g8_sq5_causal", "pshd", "page32")] + \
    [("window", "window"), ("window", "window_full")] + [("prefill", n) for n in PREFILL]


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("kind,name", PAGED_ABI, ids=[f"{k}-{n}" for k, n in PAGED_ABI])
def test_paged_entries_with_o_and_workspace_in_the_arena(arena, fam, kind, name, pattern):
    """The paged decode, windowed decode and paged prefill entries through the C ABI: the pool, q, the table, the
    lengths, o (at a batch stride that crosses 2^31 and 2^32 bytes) and the workspace, when the launch wants one (the
    split cases do), are all views of the arena. The float64 oracle, then the bits of the same entry on a compact copy
    (the same parameters but for addresses and strides: the same plan)."""
    from flash_attention_cute_amd import _debug

    lens, hq, sq, page, cap, causal, w, dtype, layout, num_pages, thr = READS[name]
    c = o_case(name)
    _debug.set_dec_fuse(0 if name == "split_unfused" else None)
    with arena.case(pattern):
        q, kc, vc, table, sl = c.load(arena)
        o = arena.expect(arena.view(c.plan.placements["o"]), "o")
        rc, err, path, in_place = abi_paged(kind, q, kc, vc, o, table, sl, causal, dtype, lambda n: arena_workspace(arena, n), w)
        got = arena.settle()
    assert rc == 0, err
    if kind == "prefill":
        assert (path, in_place) == ("w4", True)
    else:
        assert path == ("decode_paged_split" if name.startswith("split") else "decode_paged")
        assert ("ws" in got) == name.startswith("split")
    check_padded(got["o"], read_oracle(name), dtype)
    cq, ckc, cvc, ctab, csl = compact_pools(c)
    co = torch.empty_like(cq)
    rc2, err2, path2, _ = abi_paged(kind, cq, ckc, cvc, co, ctab, csl, causal, dtype, plain_workspace, w)
    assert rc2 == 0 and path2 == path and torch.equal(got["o"], co), err2


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("split", ["unsplit", "split"])
def test_paged_fp8_entry_with_o_and_workspace_in_the_arena(arena, fam, split, pattern):
    from test_fp8_kvcache import fp8_oracle

    c = fp8_case(split)
    with arena.case(pattern):
        q, kc, vc, table, sl = c.load(arena)
        kd = arena.load(arena.view(c.plan.placements["kd"]), c.kd)
        vd = arena.load(arena.view(c.plan.placements["vd"]), c.vd)
        o = arena.expect(arena.view(c.plan.placements["o"]), "o")
        rc, err, path, _ = abi_paged("fp8", q, kc, vc, o, table, sl, False, BF16, lambda n: arena_workspace(arena, n), kd=kd, vd=vd)
        got = arena.settle()
    assert rc == 0 and path == ("decode_paged_fp8_split" if split == "split" else "decode_paged_fp8"), (rc, err, path)
    check_padded(got["o"], fp8_oracle(c.q, c.k, c.v, c.sl, c.kd, c.vd, False), BF16)
    cq, ckc, cvc, ctab, csl = compact_pools(c)
    co = torch.empty_like(cq)
    rc2, err2, path2, _ = abi_paged("fp8", cq, ckc, cvc, co, ctab, csl, False, BF16, plain_workspace, kd=c.kd.to(DEV),
                                    vd=c.vd.to(DEV))
    assert rc2 == 0 and path2 == path and torch.equal(got["o"], co), err2


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_paged_varlen_entry_with_packed_q_and_o_past_4_gib(arena, fam, causal, pattern):
    """fa_fwd_gfx950_paged_varlen through the C ABI: packed q AND packed o with rows PACKED_Q_STRIDE elements apart
    (row 893 past 2^32 bytes), the pool at high pages, cu_seqlens_q, the table and the lengths in the arena."""
    c = ragged_case(True)
    r = c.ragged
    with arena.case(pattern):
        q, kc, vc, table, sl = c.load(arena)
        cu = arena.load(arena.view(c.plan.placements["cu_q"]), r.cu_q)
        o = arena.expect(arena.view(c.plan.placements["o"]), "o")
        rc, err, path, in_place = abi_paged("varlen", q, kc, vc, o, table, sl, causal, F16, lambda n: arena_workspace(arena, n),
                                            cu=cu, max_q=r.max_q)
        got = arena.settle()
    assert rc == 0 and (path, in_place) == ("w4", True), (rc, err, path, in_place)
    check_padded(got["o"], r.oracle(causal), F16)
    small = fam.flash_attn_paged_varlen_func(*dv(r.q, r.kc, r.vc, r.cu_q), r.max_q, *dv(r.table, r.sl), causal=causal)
    assert torch.equal(got["o"], small)


@functools.lru_cache(maxsize=None)
def merge_out_case():
    """merge_case() with the merged out [B, H, S, D] at a batch stride of 2^31 + 128 elements and its lse [B, H, S]
    (fp32) at 2^30 + 8: batch 1 of both lies past 2^32 bytes."""
    plan0, outs, lses = merge_case()
    plan = Plan("merge_out")
    for p in plan0.placements.values():
        plan.add(p.name, p.dtype, p.shape, p.strides, p.base, p.dims)
    n, b, h, s, d = outs.shape
    plan.add("out", F16, (b, h, s, d), (2 ** 31 + 128, s * d, d, 1), BASE_MIN + (128 << 20), ("batch", "head", "row"), written=True)
    plan.add("lse", F32, (b, h, s), (2 ** 30 + 8, s, 1), BASE_MIN + (192 << 20), ("batch", "head"), written=True)
    plan.check_disjoint()
    return plan, outs, lses


@pytest.mark.gpu
@PAT
def test_merge_states_with_large_part_and_output_strides(arena, fam, pattern):
    """fa_merge_states_gfx950 through the C ABI, n = 3: outs / lses with a part stride of 2.25 GiB, and out / lse in
    the arena with a batch stride that crosses 2^32 bytes."""
    from flash_attention_cute_amd import _debug, flash_attn_merge_states
    from test_lse_abi import FaMergeParams

    plan, outs, lses = merge_out_case()
    lib = _debug.lib()
    with arena.case(pattern):
        do = arena.load(arena.view(plan.placements["outs"]), outs)
        dl = arena.load(arena.view(plan.placements["lses"]), lses)
        o = arena.expect(arena.view(plan.placements["out"]), "out")
        l = arena.expect(arena.view(plan.placements["lse"]), "lse")
        p = FaMergeParams(do.data_ptr(), dl.data_ptr(), o.data_ptr(), l.data_ptr(), *outs.shape, *do.stride()[:4],
                          *dl.stride(), *o.stride()[:3], *l.stride())
        rc = lib.fa_merge_states_gfx950(ctypes.byref(p), 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        got = arena.settle()
    assert rc == 0, lib.fa_last_error().decode()
    ro, rl = merge_oracle(outs, lses)
    check_padded(got["out"], ro, F16)
    check_lse(got["lse"], rl, "large-merge")
    so, sl_ = flash_attn_merge_states(*dv(outs, lses), return_lse=True)
    assert torch.equal(got["out"], so) and torch.equal(got["lse"], sl_)  # (one pass over the rows: no plan at all)


# ---- (c) each host 32-bit rule on both sides
@functools.lru_cache(maxsize=None)
def launch_constants():
    """The ``constexpr int`` constants of csrc/fa_launch.h (kBlockM, kBlockN, kQoSpanRows, kDecMaxRows, ...), read
    from the header the library is built from."""
    import re
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "flash_attention_cute_amd" / "csrc" / "fa_launch.h").read_text()
    env = {}
    for name, expr in re.findall(r"constexpr int (k\w+) = ([^;]+);", text):
        try:
            env[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(env)))
        except Exception:  # (an expression of something else than earlier int constants: not needed here)
            pass
    return env


@functools.lru_cache(maxsize=None)
def rule_constants():
    """The two limits of the host rules, read from the sources the library is built from: ``limit`` (0x7fffffff) of
    check_params' sequence-stride rule in csrc/fa_fwd_gfx950.hip, ``qspan`` (0x7ff00000) of decode_rule in
    csrc/fa_launch.h."""
    import re
    from pathlib import Path

    csrc = Path(__file__).resolve().parent.parent / "flash_attention_cute_amd" / "csrc"
    a = re.search(r"strides\[i\] \* 2 \* rows \+ 256 > (0x[0-9a-f]+)LL", (csrc / "fa_fwd_gfx950.hip").read_text())
    b = re.search(r"qspan >= 0 && qspan < (0x[0-9a-f]+)LL", (csrc / "fa_launch.h").read_text())
    return {"limit": int(a.group(1), 16), "qspan": int(b.group(1), 16)}


def test_model_launch_constants_are_read_from_the_header():
    assert rule_constants() == {"limit": 0x7fffffff, "qspan": 0x7ff00000}
    k = launch_constants()
    assert k["kBlockN"] == 64 and k["kQoSpanRows"] == k["kBlockM"] // 2 + 32 and k["kDecMaxRows"] == 2 * k["kDecRows"]


def rule_plan(name, tensors):
    """``tensors``: (name, host tensor [1, H, S, D], row stride in elements or None) -- each at its own base; a row
    stride puts the heads D apart inside the row's pitch, None is compact."""
    plan = Plan(name)
    for i, (nm, t, row) in enumerate(tensors):
        h, s = t.size(1), t.size(2)
        assert row is None or row >= h * D
        strides = (s * row, D, row, 1) if row is not None else (h * s * D, s * D, D, 1)
        plan.add(nm, t.dtype, t.shape, strides, BASE_MIN + (i + 1) * (4 << 20), ("batch", "head", "row"), written=nm == "o")
    plan.check_disjoint()
    return plan


def rule_views(arena, name, tensors):
    """rule_plan's tensors as views of the arena: "o" is the declared output, the others are loaded."""
    plan = rule_plan(name, tensors)
    return [arena.expect(arena.view(plan.placements[nm]), "o") if nm == "o" else arena.load(arena.view(plan.placements[nm]), t)
            for nm, t, _ in tensors]


def small_qkv(hq, hkv, sq, sk, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, hq, sq, D, generator=g).to(dtype), torch.randn(1, hkv, sk, D, generator=g).to(dtype),
            torch.randn(1, hkv, sk, D, generator=g).to(dtype))


def check_params_case(which):
    k_ = launch_constants()
    rows = k_["kBlockN"] if which == "kv" else k_["kQoSpanRows"]
    st = rule_limit(rows)
    sq, sk, causal = (80, 130, True) if which == "kv" else (330, 70, False)
    assert (max(sq, sk) - 1) * st * 2 > 2 ** 32
    return (st, causal) + small_qkv(4, 2, sq, sk, F16, 7800 + rows)


def check_params_tensors(which, st):
    _, _, q, k, v = check_params_case(which)
    q_row, kv_row = (None, st) if which == "kv" else (st, None)
    return [("q", q, q_row), ("k", k, kv_row), ("v", v, kv_row), ("o", q, q_row)]


@pytest.mark.gpu
@PAT
@pytest.mark.parametrize("which", ["kv", "qo"])
def test_rule_check_params_sequence_strides(arena, fam, which, pattern):
    """check_params: stride * 2 * rows + 256 <= 0x7fffffff, rows = kBlockN (64) for k / v and kQoSpanRows for q / o.
    At the largest admitted stride the prefill kernel runs and matches the oracle -- 130 keys, three tiles with rows
    ~33.5 MB apart (4.03 GiB in all); 330 queries, two 256-row blocks with rows ~13.4 MB apart (4.1 GiB) -- and 8
    elements more is FA_ERR_UNSUPPORTED."""
    st, causal, q, k, v = check_params_case(which)
    with arena.case(pattern):
        views = rule_views(arena, f"rule_{which}", check_params_tensors(which, st))
        rc, err, path = c_abi_forward(views, causal, F16, D ** -0.5)
        got = arena.settle()
    assert rc == 0 and path == "w4", (rc, err, path)
    check_padded(got["o"], dense_oracle(q, k, v, causal), F16)
    # one step over the limit, on views of the arena as well (should the rule ever admit it, the launch reads and
    # writes inside the arena and fails on data): refused, and nothing is written
    with arena.case(pattern):
        views = rule_views(arena, f"rule_{which}_over", check_params_tensors(which, st + 8))
        rc, err, _ = c_abi_forward(views, causal, F16, D ** -0.5)
        arena.settle()
    assert rc == 2 and "sequence stride too large" in err, (rc, err)  # FA_ERR_UNSUPPORTED


def qspan_limit(g):
    """The largest q head stride (a multiple of 8) with ((g - 1) * stride + D) * 2 < kDecQSpanLimit, Sq = 1."""
    return (rule_constants()["qspan"] // 2 - 1 - D) // (g - 1) // 8 * 8


def qspan_plan(want, q, k, stride):
    g = q.size(1)
    plan = Plan(f"rule_qspan_{want}")
    plan.add("q", BF16, q.shape, (g * stride, stride, D, 1), BASE_MIN + (4 << 20), ("batch", "head", "row"))
    for i, nm in enumerate(("k", "v", "o")):
        t = q if nm == "o" else k
        plan.add(nm, BF16, t.shape, (t.size(1) * t.size(2) * D, t.size(2) * D, D, 1), BASE_MIN + (i + 2) * (4 << 20) + 4096,
                 ("batch", "head", "row"), written=nm == "o")
    plan.check_disjoint()
    return plan


@pytest.mark.gpu
@PAT
def test_rule_decode_q_span(arena, fam, pattern):
    """decode_rule: the q rows of a (batch, kv-head) group, addressed by 32-bit offsets from the group's first
    q-head, span less than 0x7ff00000 bytes. g = 8, Sq = 1: at the largest q head stride (~1.53e8 elements, the
    eighth head 2^31 - 1 MiB from the first) the dense launch runs the decode kernel; 8 elements more runs the
    prefill kernel, whose head term is 64-bit -- both within TOL of the oracle."""
    g, sk = 8, 300
    limit, span = qspan_limit(g), rule_constants()["qspan"]
    assert ((g - 1) * limit + D) * 2 < span <= ((g - 1) * (limit + 8) + D) * 2
    q, k, v = small_qkv(g, 1, 1, sk, BF16, 7810)
    ref = dense_oracle(q, k, v, False)
    for stride, want in ((limit, "decode"), (limit + 8, "w4")):
        plan = qspan_plan(want, q, k, stride)
        with arena.case(pattern):
            views = [arena.load(arena.view(plan.placements[n]), t) for n, t in (("q", q), ("k", k), ("v", v))]
            views.append(arena.expect(arena.view(plan.placements["o"]), "o"))
            rc, err, path = c_abi_forward(views, False, BF16, D ** -0.5)
            got = arena.settle()
        assert rc == 0 and path == want, (stride, rc, err, path)
        check_padded(got["o"], ref, BF16)


@pytest.mark.gpu
def test_rule_decode_q_span_paged_refuses(arena, fam):
    """The paged dispatcher has no prefill kernel to fall back to for a decode shape: a q whose group spans
    0x7ff00000 bytes or more is refused by name, before any launch (so nothing is loaded: q is only a view)."""
    c = read_case("unsplit")  # Hq 8, Hkv 2: g = 4
    g = 4
    over = qspan_limit(g) + 8
    flat = arena.buf.view(F16)
    # (Sq = 2: a single query row is packed by the binding, heads into rows, and meets check_params' rule first)
    q = torch.as_strided(flat, (1, 8, 2, D), (8 * over, over, D, 1), BASE_MIN // 2)
    _, kc, vc, table, sl = compact_pools(c)
    with pytest.raises(RuntimeError, match="q strides too large"):
        fam.flash_attn_paged_func(q, kc, vc, table[:1], sl[:1])
    torch.cuda.synchronize()


@pytest.mark.gpu
@PAT
def test_rule_zigzag_q_span(arena, fam, pattern):
    """use_zigzag: big * 2 * (Sq + 32) + 256 <= 0x7fffffff for the larger of the q / o sequence strides. Sq = 130,
    causal: zigzag Q blocks under the limit, the plain layout 8 elements over it, both within TOL of the oracle."""
    from flash_attention_cute_amd import _debug

    sq = 130
    limit = (rule_constants()["limit"] - 256) // (2 * (sq + 32)) // 8 * 8
    assert limit + 8 <= rule_limit(launch_constants()["kQoSpanRows"])  # (check_params admits both sides)
    q, k, v = small_qkv(4, 2, sq, sq, F16, 7820)
    ref = dense_oracle(q, k, v, True)
    for stride, want in ((limit, "zigzag"), (limit + 8, "plain")):
        with arena.case(pattern):
            views = rule_views(arena, f"rule_zigzag_{want}", [("q", q, stride), ("k", k, None), ("v", v, None), ("o", q, stride)])
            rc, err, path = c_abi_forward(views, True, F16, D ** -0.5)
            layout = _debug.last_layout()
            got = arena.settle()
        assert rc == 0 and path == "w4" and layout == want, (stride, rc, err, path, layout)
        check_padded(got["o"], ref, F16)


def strided_pool_plan(name, shape, dtype, row):
    num_pages, hkv, page, d = shape
    plan = Plan(name)
    for nm, off in (("kc", 0), ("vc", hkv * d * item_size(dtype))):
        plan.add(nm, dtype, shape, (page * row, d, row, 1), BASE_MIN + 4096 + off, ("page", "head", "row"))
    plan.check_disjoint()
    return plan


def strided_pool(arena, name, kc, vc, row):
    """The pools kc / vc [P, Hkv, page, D] as views of the arena with the row stride ``row`` (elements; the heads D
    apart inside a row's pitch, V behind K there), a page page * row elements after the last: loaded page by page."""
    num_pages = kc.size(0)
    plan = strided_pool_plan(name, kc.shape, kc.dtype, row)
    out = []
    for nm, t in (("kc", kc), ("vc", vc)):
        view = arena.view(plan.placements[nm])
        for pg in range(num_pages):
            arena.load(view[pg], t[pg])
        out.append(view)
    return out


@pytest.mark.gpu
@PAT
def test_rule_paged_prefill_page_span(arena, fam, pattern):
    """The paged prefill kernel addresses a tile's rows from its page's base: page_size * row_stride * 2 <=
    0x7fffffff. Page 128 with the largest admitted row stride (8388600 elements, 16.8 MB): one page spans 2^31 - 2 KiB
    bytes, the two pages of a 200-key sequence 4 GiB; runs in place and matches the oracle and the compact launch. 8
    elements more is refused (FA_ERR_UNSUPPORTED's text)."""
    from flash_attention_cute_amd import _debug

    page, sq, lens = 128, 40, (200,)
    top = rule_constants()["limit"]
    st = top // (2 * page) // 8 * 8
    assert page * st * 2 <= top < page * (st + 8) * 2
    q, k, v, kc, vc, table, sl = make_paged(lens, 8, HKV, sq, page, 256, D, F16, 7830, "pshd", spare_pages=0)
    with arena.case(pattern):
        bk, bv = strided_pool(arena, "rule_paged_prefill", kc, vc, st)
        assert bk.stride(0) * bk.element_size() * (bk.size(0) - 1) + page * D * 2 > 2 ** 31
        out = fam.flash_attn_paged_func(q.to(DEV), bk, bv, table.to(DEV), sl.to(DEV), causal=True)
        labels = _debug.last_path(), _debug.last_prefill_paged()
        arena.settle()
    assert labels == ("w4", True)
    check_padded(out, oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, D ** -0.5, True), F16)
    assert torch.equal(out, fam.flash_attn_paged_func(*dv(q, kc, vc, table, sl), causal=True))
    flat = arena.buf.view(F16)  # over the limit: a view only, refused before any launch
    over = [torch.as_strided(flat, kc.shape, (page * (st + 8), D, st + 8, 1), BASE_MIN // 2 + o) for o in (0, HKV * D)]
    with pytest.raises(RuntimeError, match="span more than 2\\^31 bytes"):
        fam.flash_attn_paged_func(q.to(DEV), over[0], over[1], table.to(DEV), sl.to(DEV), causal=True)
    torch.cuda.synchronize()


@pytest.mark.gpu
@PAT
def test_rule_fp8_decode_row_stride(arena, fam, pattern):
    """The FP8 decode's slab() forms (rows - 1) * stride + D in 32 bits for the 32 rows of a tile. The host bounds it
    through the dense check on the pool's row stride (stride * 2 * 64 + 256 <= 0x7fffffff, twice what one-byte
    elements need): at the largest admitted stride that is a multiple of 16 (an e4m3 pool's alignment), 16.8 MB a
    row, the four 64-row pages of a 200-key sequence span 4 GiB; 16 more is refused."""
    from flash_attention_cute_amd import _debug
    from test_fp8_kvcache import fp8_oracle

    page, lens = 64, (200,)
    st = rule_limit(launch_constants()["kBlockN"]) // 16 * 16
    top = rule_constants()["limit"]
    assert st * 2 * 64 + 256 <= top < (st + 16) * 2 * 64 + 256 and s32(31 * st + D) == 31 * st + D
    kd, vd = pow2_descales(1, HKV), pow2_descales(1, HKV, 2)
    q, k8, v8, kc8, vc8, table, sl = make_fp8_paged(lens, 8, HKV, 1, page, 256, D, BF16, 7840, "pshd", kd=kd, vd=vd)
    used = sorted(table[0].tolist())  # (make_fp8_paged adds spare pages: keep the four used ones, in their shuffled order)
    kc8, vc8, table = kc8[used], vc8[used], torch.tensor([[used.index(i) for i in table[0].tolist()]], dtype=I32)
    with arena.case(pattern):
        bk, bv = strided_pool(arena, "rule_fp8", kc8, vc8, st)
        assert bk.stride(0) * (bk.size(0) - 1) > 2 ** 31
        out = fam.flash_attn_paged_func(q.to(DEV), bk, bv, table.to(DEV), sl.to(DEV), k_descale=kd.to(DEV), v_descale=vd.to(DEV))
        path = _debug.last_path()
        arena.settle()
    assert path == "decode_paged_fp8"
    check_padded(out, fp8_oracle(q, k8, v8, sl, kd, vd, False), BF16)
    assert torch.equal(out, fam.flash_attn_paged_func(*dv(q, kc8, vc8, table, sl), k_descale=kd.to(DEV), v_descale=vd.to(DEV)))
    flat = arena.buf.view(FP8)
    over = [torch.as_strided(flat, kc8.shape, (page * (st + 16), D, st + 16, 1), BASE_MIN + o) for o in (0, HKV * D)]
    with pytest.raises(RuntimeError, match="too large"):
        fam.flash_attn_paged_func(q.to(DEV), over[0], over[1], table.to(DEV), sl.to(DEV), k_descale=kd.to(DEV),
                                  v_descale=vd.to(DEV))
    torch.cuda.synchronize()
