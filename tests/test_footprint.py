"""What each launch writes: guard bands around every buffer, poisoned scratch, three byte patterns.

include/fa_gfx950.h states the contract -- "the workspace is scratch", outputs are exactly the tensor -- and the
rest of the suite never looks at it: the ops allocate every output and workspace themselves, so no test sees the
bytes next to an output, past the end of a workspace, or in the pad columns of a padded pitch, and fresh memory
is usually zero, where a partial that is consumed without having been written adds 0 * 0.

Three layers (tests/footprint.py is the arena they share):

1. CPU self-tests (not ``gpu``): small torch models of the mistakes the arena exists to catch, each caught and
   attributed to the right region.
2. The C-ABI layer (``gpu``): lib/libfa_gfx950.so through ctypes with EVERY device buffer carved from one arena
   and ``workspace_bytes`` exactly ``*_workspace_size()``. Each case runs under the three patterns and asserts:
   FA_OK (no hand-off error); outputs bit-identical across the patterns; no byte outside the declared write
   set changed (guards, pitch gaps, the workspace region past ``need``); every input byte-identical; and the
   project's existing bars against the float64 oracle (test_gpu_parity.TOL / check, test_padded.check_padded,
   the 2^-12 LSE bound of test_paged_lse.py). The parameter structs are the ones the ABI tests pin by layout;
   the binding's host steps (default scale times log2 e, the Sq == 1 q-head pack, stride_or_zero) are restated
   as _debug.forward restates them, and pinned per entry: on contiguous inputs the helper's launch equals the
   Python op's output bit for bit, with the same _debug.last_path().
3. The op layer (``gpu``, no ctypes): the binding's own allocations (packed / padded copies, the head-dim pad
   path, the composite's outs / lses) are out of the arena's reach, so each public op runs once plainly and
   once with torch's ``fill_uninitialized_memory`` (every torch.empty NaN / max-int) and must give the same
   bits. ASSUMPTION: the extension's ``torch::empty`` goes through the same ATen factory as Python's; the first
   test of that section asserts the fill on a device tensor made from Python, and the third revert below showed
   it reaching the binding's workspaces on an MI355X. Layer 2 does not depend on it.

The tests bite -- each confirmed once by a local edit of the library that was not committed:

* ``decode_ws_bytes`` (csrc/fa_launch.h) returning one slot less: test_ws_decode, test_padded_decode_with_ragged_key_ranges
  and the 64-row paged cases fail with "N bytes past the end of `workspace`";
* ``d < D`` dropped in ``decode_store_o`` (csrc/fa_decode.hpp): test_ws_decode[*-72-unsplit-*] fails with "1 bytes
  past the end of batch 0, head 0, row 0 of `o`, in a pitch gap";
* ``decode_store_partial`` skipped by a split that has no tile: every ragged case (padded decode, paged, paged
  LSE, the no-op window, the op layer's padded_decode_ragged / paged / shared_prefix_tail_group) fails with
  "written view 0 differs between patterns 0xff and 0x7b" -- bit-identity, invisible on zeroed memory.
"""
from __future__ import annotations

import contextlib
import ctypes
import zlib

import pytest
import torch

import footprint
from footprint import PATTERNS, Arena

F16, BF16, F32, I32 = torch.float16, torch.bfloat16, torch.float32, torch.int32
gpu = pytest.mark.gpu
ROWCOL = ("batch", "head", "row", "col")


# =============================================================================== 1. CPU self-tests
def _small_arena(pattern=0xFF):
    return Arena("cpu", pattern, capacity=1 << 18)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_arena_layout_and_a_clean_launch(pattern):
    a = _small_arena(pattern)
    o = a.tensor("o", F16, (2, 3, 5, 40), (3 * 5 * 48, 5 * 48, 48, 1), ROWCOL)
    ws = a.carve(1000, "ws")
    lse = a.tensor("lse", F32, (2, 3, 5))
    for r in a.regions:
        assert (a.buf.data_ptr() + r.offset) % footprint.ALIGN == 0 and r.offset >= footprint.GUARD
    for r0, r1 in zip(a.regions, a.regions[1:]):
        assert r1.offset - (r0.offset + r0.nbytes) >= footprint.GUARD
    assert a.buf.numel() - (a.regions[-1].offset + a.regions[-1].nbytes) >= footprint.GUARD
    assert a.region_of(o).name == "o" and a.region_of(lse).name == "lse"
    assert a.region_of(o).nbytes == ((2 * 3 * 5 - 1) * 48 + 40) * 2  # ends with its last element: 0 bytes to the guard
    a.declare_written(o)
    a.declare_written(lse)
    a.declare_written(a.view(ws, torch.uint8, (996,)))
    assert a.untouched() == []
    o.copy_(torch.randn(2, 3, 5, 40).to(F16))  # a launch that keeps to its footprint
    lse.fill_(1.0)
    a.bytes_of(ws)[:996] = 17
    assert a.untouched() == []
    with pytest.raises(MemoryError):
        a.carve(1 << 18, "too big")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_catches_a_row_store_of_the_whole_d_tile(pattern):
    """D = 40 in a kD = 64 tile, the `kExactD || d < D` mask dropped: the last row's columns 40..63 leave the
    tensor, every other row's land in the pitch gap (pitch 48) and in the next row."""
    a = _small_arena(pattern)
    d, kd, pitch = 40, 64, 48
    o = a.declare_written(a.tensor("o", F16, (1, 2, 3, d), (2 * 3 * pitch, 3 * pitch, pitch, 1), ROWCOL))
    raw = torch.as_strided(a.buf.view(F16), (1, 2, 3, kd), o.stride(), o.storage_offset())  # the "kernel's" view
    raw.view(torch.int16).fill_(0x5555)  # (no byte of it equals a pattern byte)
    got = a.untouched(first=4)
    assert got and "in a pitch gap" in got[0] and "`o`" in got[0] and "head 0, row 0" in got[0], got
    assert got[0].startswith("1 bytes past the end of batch 0, head 0, row 0"), got
    everything = a.untouched(first=4096)
    assert any("past the end of `o`, batch 0, head 1, row 2" in s for s in everything), everything[-3:]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_catches_a_tail_row_block_that_stores_32_rows(pattern):
    """33 rows in 32-row blocks: the second block has one valid row and stores all 32."""
    a = _small_arena(pattern)
    o = a.declare_written(a.tensor("o", BF16, (1, 1, 33, 64), None, ROWCOL))
    nxt = a.tensor("lse", F32, (33,))
    raw = torch.as_strided(a.buf.view(BF16), (64, 64), (64, 1), o.storage_offset())
    raw.view(torch.int16).fill_(0x5555)
    got = a.untouched()
    assert got[0].startswith("1 bytes past the end of `o`, batch 0, head 0, row 32"), got
    assert "bytes in all" in got[-1] and str(31 * 64 * 2) in got[-1], got
    assert not any("lse" in s for s in got) and nxt is not None


def test_catches_a_declared_element_left_unwritten():
    """Bit-identity across the patterns is what proves every declared element was written."""
    outs = []
    for pattern in PATTERNS:
        a = _small_arena(pattern)
        o = a.declare_written(a.tensor("o", F16, (1, 2, 4, 8), None, ROWCOL))
        val = torch.arange(64, dtype=torch.float32).reshape(1, 2, 4, 8).to(F16)
        keep = torch.ones(1, 2, 4, 8, dtype=torch.bool)
        keep[0, 1, 2, 5] = False
        o.copy_(torch.where(keep, val, o))
        assert a.untouched() == []  # the footprint is kept...
        outs.append(o.clone())
    assert not all(torch.equal(outs[0].view(torch.int16), x.view(torch.int16)) for x in outs[1:])  # ...the bits differ
    diff = (outs[0].view(torch.int16) != outs[2].view(torch.int16)).nonzero().tolist()
    assert diff == [[0, 1, 2, 5]]


def _merge(ws_o, ws_lse, select):
    """decode_merge's arithmetic on fp32 partials: w = exp2(lse - max), 0 for the -inf sentinel."""
    mx = ws_lse.max(dim=0).values
    w = torch.where(torch.isinf(ws_lse), torch.zeros_like(ws_lse), torch.exp2(ws_lse - mx))
    terms = torch.where(w[..., None] == 0, torch.zeros_like(ws_o), w[..., None] * ws_o) if select else w[..., None] * ws_o
    return terms.sum(dim=0) / w.sum(dim=0)[..., None]


@pytest.mark.parametrize("select", [False, True], ids=["0_times_x", "w_eq_0_select"])
def test_catches_a_combine_that_reads_a_slot_no_split_wrote(select):
    """Split 1 has no tile: its lse is the sentinel (written) but its partial O is not. `0 * x` hides the finite
    0x7B pattern and not NaN; a `w == 0 ? 0 : w * x` select hides both -- then only a read of the slot's LSE would
    show, which the second half models. Either way the three patterns do not all agree."""
    def run(pattern, skip_lse):
        a = _small_arena(pattern)
        ws = a.carve(2 * 4 * 8 * 4 + 2 * 4 * 4, "ws")
        ws_o = a.view(ws, F32, (2, 4, 8))
        ws_lse = torch.as_strided(a.buf.view(F32), (2, 4), (4, 1), ws.offset // 4 + 64)
        a.declare_written(a.view(ws, torch.uint8, (ws.nbytes,)))
        g = torch.Generator().manual_seed(1)
        ws_o[0] = torch.randn(4, 8, generator=g)
        ws_lse[0] = torch.randn(4, generator=g)
        if not skip_lse:
            ws_lse[1] = float("-inf")
        o = _merge(ws_o, ws_lse, select)
        assert a.untouched() == []
        return o

    outs = [run(p, skip_lse=False) for p in PATTERNS]
    same = [torch.equal(outs[0].view(I32), x.view(I32)) for x in outs[1:]]
    if select:
        assert all(same)  # this form is safe against an unwritten partial O ...
        outs = [run(p, skip_lse=True) for p in PATTERNS]  # ... but not against an unwritten LSE
        same = [torch.equal(outs[0].view(I32), x.view(I32)) for x in outs[1:]]
    assert not all(same)
    assert torch.isnan(outs[0]).any()  # 0xFF: 0 * NaN (or a NaN weight)
    assert torch.isfinite(outs[2]).all()  # 0x00: invisible on fresh memory


@pytest.mark.parametrize("pattern", PATTERNS)
def test_catches_a_workspace_use_4_bytes_past_need(pattern):
    a = _small_arena(pattern)
    need = 4 * 4 * 8 * 4
    ws = a.carve(need + 256, "ws")  # the region is larger: the bytes past `need` are checked like a guard
    a.declare_written(a.view(ws, torch.uint8, (need,), dims=("byte",)))
    slots = torch.as_strided(a.buf.view(F32), (need // 4 + 1,), (1,), ws.offset // 4)
    slots.view(I32).fill_(0x55555555)  # one fp32 slot too many
    got = a.untouched()
    assert len(got) == 4 and got[0].startswith("1 bytes past the end of `ws`") and got[3].startswith("4 bytes past"), got
    a2 = _small_arena(pattern)
    ws2 = a2.carve(need, "ws")  # exact: the stray slot is in the guard band
    a2.declare_written(a2.view(ws2, torch.uint8, (need,), dims=("byte",)))
    a2.tensor("o", F16, (4, 8))
    torch.as_strided(a2.buf.view(F32), (need // 4 + 1,), (1,), ws2.offset // 4).view(I32).fill_(0x55555555)
    got = a2.untouched()
    assert len(got) == 4 and all("past the end of `ws`" in s for s in got), got


def test_refill_dirties_one_region_only():
    a = _small_arena(0x00)
    ws = a.carve(512, "ws")
    o = a.tensor("o", F16, (4, 8))
    a.refill(ws, 0xA5)
    assert len(a.untouched(first=4096)) > 1 and all("`ws`" in s for s in a.untouched()[:8])
    a.declare_written(a.view(ws, torch.uint8, (512,)))
    assert a.untouched() == [] and o is not None


# =============================================================================== 2. the C-ABI layer
_ARENAS: dict = {}
_P, _I, _C = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
SMALL, LARGE = 8 << 20, 40 << 20


def arena_for(device, capacity=SMALL) -> Arena:
    """One allocation per capacity for the whole module, reset for every case."""
    key = (str(device), capacity)
    if key not in _ARENAS:
        _ARENAS[key] = Arena(device, PATTERNS[0], capacity)
    return _ARENAS[key].reset(PATTERNS[0])


class _Abi:
    def __init__(self, device):
        import flash_attention_cute_amd as m
        from flash_attention_cute_amd import _debug
        from flash_attention_cute_amd import flash_attention as fam

        assert fam.flash_attention_cuda is not None, f"gfx950 extension failed to load: {fam._load_error!r}"
        self.m, self.dbg, self.device, self.lib = m, _debug, device, _debug.lib()
        lib = self.lib
        sized = [_P, _C, _C, _P, _I, _P]            # params, dtype, causal, workspace, bytes, stream
        windowed = [_P, _C, _C, _I, _P, _I, _P]     # params, dtype, causal, window_left, workspace, bytes, stream
        for name, args in (("fa_fwd_gfx950_ws", sized), ("fa_fwd_gfx950_paged", sized), ("fa_fwd_gfx950_paged_fp8", sized),
                           ("fa_fwd_gfx950_padded", windowed), ("fa_fwd_gfx950_paged_window", windowed),
                           ("fa_fwd_gfx950_paged_window_fp8", windowed), ("fa_fwd_gfx950_paged_lse", windowed),
                           ("fa_fwd_gfx950_paged_lse_fp8", windowed), ("fa_fwd_gfx950_paged_prefill", windowed),
                           ("fa_fwd_gfx950_varlen", [_P, _C, _C, _P]), ("fa_fwd_gfx950_rope", [_P, _C, _C, _P]),
                           ("fa_fwd_gfx950_window", [_P, _C, _C, _I, _P]), ("fa_rope_gfx950", [_P, _C, _P]),
                           ("fa_merge_states_gfx950", [_P, _C, _P]), ("fa_kvcache_append_gfx950", [_P, _C, _P]),
                           ("fa_kvcache_append_fp8_gfx950", [_P, _C, _P])):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = _C
        for name, args in (("fa_fwd_gfx950_workspace_size", [_P, _C, _C]), ("fa_fwd_gfx950_paged_workspace_size", [_P, _C, _C]),
                           ("fa_fwd_gfx950_paged_fp8_workspace_size", [_P, _C, _C]),
                           ("fa_fwd_gfx950_padded_workspace_size", [_P, _C, _C, _I]),
                           ("fa_fwd_gfx950_paged_window_workspace_size", [_P, _C, _C, _I]),
                           ("fa_fwd_gfx950_paged_window_fp8_workspace_size", [_P, _C, _C, _I]),
                           ("fa_fwd_gfx950_paged_lse_workspace_size", [_P, _C, _C, _I]),
                           ("fa_fwd_gfx950_paged_lse_fp8_workspace_size", [_P, _C, _C, _I]),
                           ("fa_fwd_gfx950_paged_prefill_workspace_size", [_P, _C, _C, _I])):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = _I
        lib.fa_last_error.restype = ctypes.c_char_p

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def defaults(self):
        d = self.dbg
        d.set_knobs()
        for f in (d.set_split, d.set_split_pairs, d.set_head_pack, d.set_dec_fuse, d.set_zigzag):
            f(None)


@pytest.fixture
def abi(device):
    try:  # a device that an earlier test left in an error state runs nothing more
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports an error from an earlier launch: {e}", returncode=3)
    a = _Abi(device)
    a.defaults()
    a.m.split_errors(reset=True)
    yield a
    a.defaults()


def code(dtype) -> int:
    return 0 if dtype == F16 else 1


def log2e_scale(scale: float) -> float:
    """The binding's fill_params: the float32 scale times log2 e (float * double, rounded to float by the field)."""
    from flash_attention_cute_amd._debug import LOG2E

    return float(torch.tensor(scale, dtype=torch.float32).double() * LOG2E)


def o_strides(layout, b, h, s, d):
    """contiguous; a row pitch of d + 8 (pad columns after every row); HF's physical [B, S, H, D]."""
    if layout == "pitch":
        p = d + 8
        return (h * s * p, s * p, p, 1)
    if layout == "hf":
        return (s * h * d, d, h * d, 1)
    return (h * s * d, s * d, d, 1)


class Launch:
    """The buffers of one case, all carved from one arena: inputs (re-written under every pattern), outputs (their
    write sets declared) and the workspace (exactly `need` bytes declared; the region is 256 bytes longer)."""

    def __init__(self, abi, capacity=SMALL):
        self.abi, self.arena = abi, arena_for(abi.device, capacity)
        self.inputs, self.written, self.ws_region, self.need = [], [], None, 0

    def inp(self, name, value, strides=None, dims=None):
        t = self.arena.tensor(name, value.dtype, value.shape, strides, dims)
        self.arena.declare_input(t)
        self.inputs.append((t, value))
        return t

    def out(self, name, dtype, shape, strides=None, dims=ROWCOL, written=None):
        """`written`: the sub-views a launch may write when that is not the whole tensor."""
        t = self.arena.tensor(name, dtype, shape, strides, dims)
        for w in ([t] if written is None else written(t)):
            self.written.append(self.arena.declare_written(w))
        return t

    def workspace(self, need):
        """(pointer, bytes) to pass: NULL / 0 when the entry asks for none."""
        assert need >= 0, self.abi.lib.fa_last_error().decode()
        self.need = need
        if need == 0:
            return None, 0
        self.ws_region = self.arena.carve(need + 256, "workspace")
        self.arena.declare_written(self.arena.view(self.ws_region, torch.uint8, (need,), dims=("byte",)))
        return self.arena.buf.data_ptr() + self.ws_region.offset, need

    def run(self, call, expect=None, split=False):
        """`call()` under the three patterns, one synchronisation; asserts 1-4 of the module docstring and
        returns the written views' values (first pattern). `expect()` runs after every launch (paths)."""
        arena, runs = self.arena, []
        for pattern in PATTERNS:
            arena.fill(pattern)
            for t, value in self.inputs:
                t.copy_(value)
            snap = arena.snapshot()
            rc = call()
            assert rc == 0, (rc, self.abi.lib.fa_last_error().decode())
            if expect is not None:
                expect()
            runs.append(([w.clone() for w in self.written], arena.probe(), arena.inputs_changed(snap)))
        torch.cuda.synchronize()
        for pattern, (outs, probed, changed) in zip(PATTERNS, runs):
            stray = arena.report(probed)
            assert not stray, f"pattern {pattern:#04x}, written outside the footprint: " + "; ".join(stray)
            assert int(changed.item()) == 0, f"pattern {pattern:#04x}: an input changed"
        for pattern, (outs, _, _) in zip(PATTERNS[1:], runs[1:]):
            for i, (a, b) in enumerate(zip(runs[0][0], outs)):
                assert torch.equal(bits(a), bits(b)), f"written view {i} differs between patterns 0xff and {pattern:#04x}"
        if split:
            assert self.abi.m.split_errors() == 0
        return [w.cpu() for w in runs[0][0]]


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def dense_params(q, k, v, o, g, scale):
    """fa_fwd_params as the binding's fill_params describes q [B, H, S, D] (already packed for a decode step)."""
    from test_abi import FaFwdParams

    st = lambda t, i: t.stride(i) if t.size(i) > 1 else 0  # noqa: E731  (stride_or_zero)
    return FaFwdParams(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.size(0), q.size(1), k.size(1),
                       q.size(2), k.size(2), q.size(3), g, *(st(t, i) for i in range(3) for t in (q, k, v, o)),
                       log2e_scale(scale))


def seeded(*key):
    return zlib.crc32(repr(key).encode())


def dense_case(abi, b, hq, hkv, sq, sk, d, dtype, causal, layout="contig", capacity=SMALL, use_ws=True):
    """Buffers and parameters of fa_fwd_gfx950_ws as flash_attention_fwd would pass them (Sq == 1: the q-head
    pack, causal dropped). Returns the launch, its call, the CPU inputs and o."""
    from test_gpu_parity import make

    q, k, v = make(b, hq, hkv, sq, sk, d, dtype, seeded(b, hq, hkv, sq, sk, d, str(dtype), causal))
    pack = sq == 1
    qx = q.reshape(b, hkv, hq // hkv, d) if pack else q
    causal_x = causal and not pack
    L = Launch(abi, capacity)
    qd, kd, vd = L.inp("q", qx, dims=ROWCOL), L.inp("k", k, dims=ROWCOL), L.inp("v", v, dims=ROWCOL)
    o = L.out("o", dtype, qx.shape, o_strides(layout, *qx.shape))
    p = dense_params(qd, kd, vd, o, 1 if pack else hq // hkv, d ** -0.5)
    need = abi.lib.fa_fwd_gfx950_workspace_size(ctypes.byref(p), code(dtype), int(causal_x)) if use_ws else 0
    ws, nbytes = L.workspace(need)
    call = lambda: abi.lib.fa_fwd_gfx950_ws(ctypes.byref(p), code(dtype), int(causal_x), ws, nbytes, abi.stream())  # noqa: E731
    return L, call, (q, k, v), o


# ----------------------------------------------------------------------------------------- fa_fwd_gfx950_ws
@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("layout", ["contig", "pitch", "hf"])
@pytest.mark.parametrize("d", [64, 128, 40, 72, 120])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("s", [1, 33, 257, 300])
def test_ws_prefill(abi, s, causal, d, layout, dtype):
    """The prefill kernel (Sq = Sk = 1 with the decode kernel switched off): o contiguous, with a padded row pitch
    and in HF's [B, S, H, D]; the last batch row's o ends where its guard begins."""
    from test_gpu_parity import check

    with abi.dbg.knobs(decode=False):
        L, call, (q, k, v), o = dense_case(abi, 2, 4, 2, s, s, d, dtype, causal, layout)
        r = L.arena.region_of(o)
        assert r.nbytes == footprint.extent(o.shape, o.stride()) * 2  # 0 bytes between o's last element and the guard
        (got,) = L.run(call, expect=lambda: abi.dbg.last_path() == "w4" or pytest.fail(abi.dbg.last_path()), split=True)
    check(got.reshape(q.shape), q, k, v, d ** -0.5, causal and s > 1, dtype)


BLOCK_LAYOUTS = {  # name: (shape, knobs, expected layout, pairs, head-packed, workspace)
    "halves": ((1, 4, 2, 1024, 1024, 128), {}, "split", None, None, True),
    "piece0_empty": ((3, 2, 2, 200, 200, 128), {}, "split", None, None, True),
    "rows_without_keys": ((1, 4, 4, 1500, 700, 64), {}, "split", None, None, True),
    "pairs": ((2, 12, 4, 1500, 700, 64), {}, "split", True, None, True),            # from test_gpu_parity.PAIRS
    "head_packed": ((1, 4, 1, 300, 300, 128), {"head_pack": 2}, "split", None, True, True),  # from HP_SPLIT
    "zigzag": ((1, 4, 2, 1024, 1024, 128), {}, "zigzag", None, None, False),      # workspace NULL
}


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", list(BLOCK_LAYOUTS))
def test_ws_causal_block_layouts(abi, name, dtype):
    """Key-split causal blocks (set_split(2)): the first piece's fp32 partials and the hand-off records live in
    the workspace; exactly workspace_size() bytes are passed."""
    from test_gpu_parity import HP_SPLIT, PAIRS, check

    shape, knobs, layout, pairs, hp, use_ws = BLOCK_LAYOUTS[name]
    assert name != "pairs" or shape in PAIRS
    assert name != "head_packed" or shape in HP_SPLIT
    b, hq, hkv, sq, sk, d = shape
    abi.dbg.set_split(2)
    if "head_pack" in knobs:
        abi.dbg.set_head_pack(knobs["head_pack"])
    L, call, (q, k, v), _ = dense_case(abi, b, hq, hkv, sq, sk, d, dtype, True, capacity=LARGE, use_ws=use_ws)
    assert (L.need > 0) == use_ws

    def expect():
        assert abi.dbg.last_path() == "w4" and abi.dbg.last_layout() == layout
        assert pairs is None or abi.dbg.last_split_pairs() == pairs
        assert hp is None or abi.dbg.last_head_pack() == hp

    (got,) = L.run(call, expect, split=True)
    check(got, q, k, v, d ** -0.5, True, dtype)


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("fuse", [1, 0, None], ids=["fused", "combine", "unsplit"])
@pytest.mark.parametrize("d", [64, 128, 72])
@pytest.mark.parametrize("rows", [1, 5, 33, 64])
def test_ws_decode(abi, rows, d, fuse, dtype):
    """Split-KV decode, B1 Hkv1 Sk 2048 (4 splits), g * Sq = rows (33: a second row block with ONE valid row); the
    merge in the kernel and in the separate combine launch; workspace NULL runs unsplit. o has a padded row
    pitch, so a store of the whole D tile (d = 72) or of a whole row block shows in a gap or past the end."""
    from test_gpu_parity import check

    if fuse is not None:
        abi.dbg.set_dec_fuse(fuse)
    L, call, (q, k, v), _ = dense_case(abi, 1, rows, 1, 1, 2048, d, dtype, False, "pitch", use_ws=fuse is not None)
    assert (L.need > 0) == (fuse is not None)

    def expect():
        assert abi.dbg.last_path() == ("decode" if fuse is None else "decode_split"), abi.dbg.last_path()
        assert fuse is None or abi.dbg.last_dec_fused() == bool(fuse)

    (got,) = L.run(call, expect, split=True)
    check(got.reshape(q.shape), q, k, v, d ** -0.5, False, dtype)


@gpu
def test_ws_key_split_under_graph_capture_with_a_dirtied_workspace(abi):
    """Under capture the key-split counters live in the workspace and a memset node zeroes them: the workspace
    is re-filled with another byte before every replay and the replays still equal the eager launch."""
    abi.dbg.set_split(2)
    L, call, _, o = dense_case(abi, 1, 4, 2, 1024, 1024, 128, BF16, True, capacity=LARGE)
    arena = L.arena
    for t, value in L.inputs:
        t.copy_(value)
    assert call() == 0 and abi.dbg.last_layout() == "split"
    eager = o.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # one stream, one launch: a linear graph
        assert call() == 0 and abi.dbg.last_layout() == "split"
    outs, probes = [], []
    for pattern in (0x7B, 0x00, 0xA5):
        arena.bytes_of(L.ws_region)[:L.need].fill_(pattern)
        o.fill_(0)
        g.replay()
        outs.append(o.clone())
        probes.append(arena.probe())
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(eager)) for x in outs)
    assert all(arena.report(p) == [] for p in probes)
    assert abi.m.split_errors() == 0


@gpu
@pytest.mark.parametrize("case", ["prefill_causal", "decode_pack", "decode_rows", "key_split"])
def test_ws_helper_restates_the_binding(abi, case):
    """On contiguous inputs the arena launch is the Python op's launch: same bits, same kernel."""
    shape, causal = {"prefill_causal": ((2, 4, 2, 300, 300, 72), True), "decode_pack": ((1, 8, 1, 1, 2048, 128), False),
                     "decode_rows": ((2, 4, 2, 5, 2048, 64), True), "key_split": ((1, 4, 2, 1024, 1024, 128), True)}[case]
    b, hq, hkv, sq, sk, d = shape
    if case == "key_split":
        abi.dbg.set_split(2)
    L, call, (q, k, v), _ = dense_case(abi, b, hq, hkv, sq, sk, d, F16, causal, capacity=LARGE)
    (got,) = L.run(call, split=True)
    path = abi.dbg.last_path(), abi.dbg.last_layout()
    ref = abi.m.flash_attn_func(q.to(abi.device), k.to(abi.device), v.to(abi.device), causal=causal)
    assert (abi.dbg.last_path(), abi.dbg.last_layout()) == path
    assert torch.equal(got.reshape(q.shape), ref.cpu())


# ----------------------------------------------------------------------------------------- fa_fwd_gfx950_padded
def padded_params(base, qs, qe, ks, ke):
    from test_abi import FaPaddedParams

    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return FaPaddedParams(base, ptr(qs), ptr(qe), ptr(ks), ptr(ke))


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 72])
def test_padded_decode_with_ragged_key_ranges(abi, d, dtype):
    """Key ranges of 0, 1, 31, 33 and 2048 keys in one batch: the equal-share rule gives most sequences splits
    with no tile, whose partials the merge must not depend on."""
    from test_padded import check_padded, make_batch, oracle_padded

    lens, hq, hkv, sk = [0, 1, 31, 33, 2048], 8, 2, 2048
    b = len(lens)
    q, k, v = make_batch(b, hq, hkv, 1, sk, d, dtype, seeded("padded", d, str(dtype)), "bhsd")
    ks = torch.tensor([5, 2047, 100, 0, 0], dtype=I32)
    ke = ks + torch.tensor(lens, dtype=I32)
    L = Launch(abi, LARGE)
    qd = L.inp("q", q.reshape(b, hkv, hq // hkv, d), dims=ROWCOL)
    kd, vd = L.inp("k", k, dims=ROWCOL), L.inp("v", v, dims=ROWCOL)
    ksd, ked = L.inp("k_start", ks, dims=("batch",)), L.inp("k_end", ke, dims=("batch",))
    o = L.out("o", dtype, qd.shape, o_strides("pitch", *qd.shape))
    pp = padded_params(dense_params(qd, kd, vd, o, 1, d ** -0.5), None, None, ksd, ked)
    pp.base.k_seqlen_stride, pp.base.v_seqlen_stride = kd.stride(2), vd.stride(2)
    need = abi.lib.fa_fwd_gfx950_padded_workspace_size(ctypes.byref(pp), code(dtype), 0, -1)
    assert need > 0
    ws, nbytes = L.workspace(need)
    call = lambda: abi.lib.fa_fwd_gfx950_padded(ctypes.byref(pp), code(dtype), 0, -1, ws, nbytes, abi.stream())  # noqa: E731
    (got,) = L.run(call, lambda: abi.dbg.last_path() == "decode_split" or pytest.fail(abi.dbg.last_path()), split=True)
    check_padded(got.reshape(q.shape), oracle_padded(q, k, v, ks, ke, None, None, d ** -0.5, False), dtype)
    assert (got[0] == 0).all()  # the sequence without keys
    dev = lambda *ts: tuple(t.to(abi.device) for t in ts)  # noqa: E731  (the pin: the Python op on the same tensors)
    ref = abi.m.flash_attn_padded_func(*dev(q, k, v, ks, ke))
    assert abi.dbg.last_path() == "decode_split" and torch.equal(got.reshape(q.shape), ref.cpu())


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("window_left", [-1, 100])
def test_padded_prefill_with_query_and_key_ranges(abi, window_left, dtype):
    """The prefill path: the workspace is required and holds the row arrays; rows outside the query ranges are
    NOT written (they are outside the declared write set, so they must keep the pattern)."""
    from test_padded import check_padded, make_batch, oracle_padded, ranges

    b, hq, hkv, sq, sk, d = 3, 4, 2, 200, 300, 72
    q, k, v = make_batch(b, hq, hkv, sq, sk, d, dtype, seeded("padded_prefill", str(dtype)), "bhsd")
    ks, ke, qs, qe = ranges(b, sq, sk, 11, "mixed")
    L = Launch(abi, LARGE)
    qd, kd, vd = L.inp("q", q, dims=ROWCOL), L.inp("k", k, dims=ROWCOL), L.inp("v", v, dims=ROWCOL)
    rng = [L.inp(n, t, dims=("batch",)) for n, t in (("q_start", qs), ("q_end", qe), ("k_start", ks), ("k_end", ke))]
    real = lambda t: [t[i, :, int(qs[i]):int(qe[i])] for i in range(b)]  # noqa: E731
    o = L.out("o", dtype, q.shape, written=real)
    pp = padded_params(dense_params(qd, kd, vd, o, hq // hkv, d ** -0.5), *rng)
    for t, x in (("q", qd), ("k", kd), ("v", vd), ("o", o)):
        setattr(pp.base, f"{t}_seqlen_stride", x.stride(2))
    need = abi.lib.fa_fwd_gfx950_padded_workspace_size(ctypes.byref(pp), code(dtype), 1, window_left)
    assert need > 0
    ws, nbytes = L.workspace(need)
    call = lambda: abi.lib.fa_fwd_gfx950_padded(ctypes.byref(pp), code(dtype), 1, window_left, ws, nbytes, abi.stream())  # noqa: E731
    parts = L.run(call, lambda: abi.dbg.last_path() == "w4" or pytest.fail(abi.dbg.last_path()))
    got = torch.zeros(q.shape, dtype=dtype)
    for i, part in enumerate(parts):
        got[i, :, int(qs[i]):int(qe[i])] = part
    check_padded(got, oracle_padded(q, k, v, ks, ke, qs, qe, d ** -0.5, True, window_left=window_left), dtype)
    dev = lambda *ts: tuple(t.to(abi.device) for t in ts)  # noqa: E731  (the pin: the Python op on the same tensors)
    ref = abi.m.flash_attn_padded_func(*dev(q, k, v, ks, ke, qs, qe), causal=True, window_left=window_left)
    assert abi.dbg.last_path() == "w4" and torch.equal(got, ref.cpu())


@gpu
def test_padded_out_of_range_positions_are_clamped_with_a_guarded_output(abi):
    """tests/test_padded.py::test_padded_out_of_range_positions_are_clamped guards q / k / v; here o is guarded too:
    positions far outside [0, Sq] / [0, Sk] are clamped on the device and the launch writes only the rows of
    the clamped query ranges."""
    from test_padded import check_padded, make_batch, oracle_padded

    b, hq, hkv, sq, sk, d, dtype = 3, 4, 2, 70, 90, 64, F16
    q, k, v = make_batch(b, hq, hkv, sq, sk, d, dtype, 17, "bhsd")
    i32 = lambda *a: torch.tensor(a, dtype=I32)  # noqa: E731
    qs, qe, ks, ke = i32(-5, 10, 10 ** 6), i32(10 ** 6, 80, 10 ** 6 + 5), i32(-(10 ** 6), 40, 3), i32(50, 10 ** 6, -7)
    clamp = lambda s, e, n: (s.clamp(0, n), torch.maximum(e.clamp(0, n), s.clamp(0, n)))  # noqa: E731
    (cqs, cqe), (cks, cke) = clamp(qs, qe, sq), clamp(ks, ke, sk)
    L = Launch(abi)
    qd, kd, vd = L.inp("q", q, dims=ROWCOL), L.inp("k", k, dims=ROWCOL), L.inp("v", v, dims=ROWCOL)
    rng = [L.inp(n, t, dims=("batch",)) for n, t in (("q_start", qs), ("q_end", qe), ("k_start", ks), ("k_end", ke))]
    o = L.out("o", dtype, q.shape, written=lambda t: [t[i, :, int(cqs[i]):int(cqe[i])] for i in range(b)])
    pp = padded_params(dense_params(qd, kd, vd, o, hq // hkv, d ** -0.5), *rng)
    for t, x in (("q", qd), ("k", kd), ("v", vd), ("o", o)):
        setattr(pp.base, f"{t}_seqlen_stride", x.stride(2))
    ws, nbytes = L.workspace(abi.lib.fa_fwd_gfx950_padded_workspace_size(ctypes.byref(pp), 0, 1, -1))
    parts = L.run(lambda: abi.lib.fa_fwd_gfx950_padded(ctypes.byref(pp), 0, 1, -1, ws, nbytes, abi.stream()))
    got = torch.zeros(q.shape, dtype=dtype)
    for i, part in enumerate(parts):
        got[i, :, int(cqs[i]):int(cqe[i])] = part
    check_padded(got, oracle_padded(q, k, v, cks, cke, cqs, cqe, d ** -0.5, True), dtype)


# ----------------------------------------------------------------------------------------- the paged entries
# The issue's table asks for page sizes 16 and 64; fa_fwd_gfx950_paged_check rejects a page_size that is not a
# multiple of 32 (the kernel's key tile), so the smaller one is 32, the nearest valid size.
CAP = 2048
LENS = (0, 1, 31, 33, CAP)
QSHAPES = {"sq1_g4": (8, 2, 1), "sq3_g4": (8, 2, 3), "sq8_g8": (16, 2, 8)}  # (Hq, Hkv, Sq); the last: 64 rows


def head_dim(entry, qshape):
    """128, and for the 64-row shape a D tile that is not filled: 72, or 80 for an FP8 pool (the FP8 entries reject
    a head dim that is not a multiple of 16, so 80 is the nearest valid one)."""
    return 128 if qshape != "sq8_g8" else 80 if "fp8" in entry else 72


def paged_case(abi, entry, qshape, page, d, dtype, window_left=-1, lse_layout=None):
    """One launch of a paged decode entry as the binding's paged_fwd_impl / flash_attention_paged_lse_fwd passes it:
    shuffled table, -1 in unused entries, poisoned unused pool rows (tests/test_paged.py make_paged). Returns
    (launch, call, cpu, o, lse): cpu = dict of the host tensors for the oracles."""
    from test_fp8_abi import FaPagedFp8Params
    from test_fp8_kvcache import make_fp8_paged, pow2_descales
    from test_lse_abi import FaPagedFp8LseParams, FaPagedLseParams
    from test_paged import make_paged
    from test_paged_abi import FaPagedParams

    fp8, lse, window = "fp8" in entry, "lse" in entry, "window" in entry
    hq, hkv, sq = QSHAPES[qshape]
    g, b = hq // hkv, len(LENS)
    seed = seeded("paged", qshape, page, d, str(dtype), fp8)
    cpu = dict(kd=None, vd=None)
    if fp8:
        cpu["kd"], cpu["vd"] = pow2_descales(b, hkv), pow2_descales(b, hkv, 2)
        q, k, v, kc, vc, table, sl = make_fp8_paged(LENS, hq, hkv, sq, page, CAP, d, dtype, seed, kd=cpu["kd"], vd=cpu["vd"])
    else:
        q, k, v, kc, vc, table, sl = make_paged(LENS, hq, hkv, sq, page, CAP, d, dtype, seed)
    cpu.update(q=q, k=k, v=v, sl=sl, kc=kc, vc=vc, table=table)
    pack = sq == 1 and not window and not lse  # (the windowed and the LSE entries never pack)
    causal = sq > 1                            # (a decode step drops causal, as the pack does)
    qx = q.reshape(b, hkv, g, d) if pack else q
    L = Launch(abi, LARGE)
    qd = L.inp("q", qx, dims=ROWCOL)
    kcd = L.inp("k_cache", kc, dims=("page", "head", "row", "col"))
    vcd = L.inp("v_cache", vc, dims=("page", "head", "row", "col"))
    td, sld = L.inp("block_table", table, dims=("batch", "entry")), L.inp("cache_seqlens", sl, dims=("batch",))
    o = L.out("o", dtype, qx.shape, o_strides("pitch", *qx.shape))
    base = dense_params(qd, kcd, vcd, o, 1 if pack else g, d ** -0.5)
    base.seqlen_kv = table.size(1) * page
    base.k_seqlen_stride, base.v_seqlen_stride = kcd.stride(2), vcd.stride(2)
    p = FaPagedParams(base, td.data_ptr(), td.stride(0), table.size(1), kc.size(0), page, sld.data_ptr())
    if fp8:
        kdd, vdd = L.inp("k_descale", cpu["kd"], dims=("batch", "head")), L.inp("v_descale", cpu["vd"], dims=("batch", "head"))
        p = FaPagedFp8Params(p, kdd.data_ptr(), vdd.data_ptr(), kdd.stride(0), kdd.stride(1))
    lse_t = None
    if lse:
        # contiguous [B, Hq, Sq], or the (cc * hq, 1, hq) strides flash_attn_paged_shared_prefix_func passes: the
        # positions of one batch row are a group's sequences, each sequence's heads contiguous
        strides = (hq * sq, sq, 1) if lse_layout == "contig" else (sq * hq, 1, hq)
        lse_t = L.out("lse", F32, (b, hq, sq), strides, dims=("batch", "head", "row"))
        p = (FaPagedFp8LseParams if fp8 else FaPagedLseParams)(p, lse_t.data_ptr(), *strides, 0)
    lib, ref, dt, c = abi.lib, ctypes.byref(p), code(dtype), int(causal)
    name = "fa_fwd_gfx950_" + entry
    if window or lse:
        need = getattr(lib, name + "_workspace_size")(ref, dt, c, window_left)
        ws, nbytes = L.workspace(need)
        call = lambda: getattr(lib, name)(ref, dt, c, window_left, ws, nbytes, abi.stream())  # noqa: E731
    else:
        need = getattr(lib, name + "_workspace_size")(ref, dt, c)
        ws, nbytes = L.workspace(need)
        call = lambda: getattr(lib, name)(ref, dt, c, ws, nbytes, abi.stream())  # noqa: E731
    L.keep = p  # (the struct must outlive the calls)
    cpu["causal"] = causal
    return L, call, cpu, o, lse_t


def paged_oracle(cpu, dtype, window_left=-1):
    from test_padded import oracle_padded

    q, k, v, sl = cpu["q"], cpu["k"], cpu["v"], cpu["sl"]
    if cpu["kd"] is not None:  # the widened e4m3 bytes with the power-of-two descales folded in (exact)
        k, v = k.to(dtype) * cpu["kd"][:, :, None, None].to(dtype), v.to(dtype) * cpu["vd"][:, :, None, None].to(dtype)
    return oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, q.size(-1) ** -0.5, cpu["causal"],
                         window_left=window_left)


def expect_path(abi, prefix, split=None):
    def f():
        path = abi.dbg.last_path()
        want = prefix + ("_split" if split else "")
        assert path == want if split is not None else path in (prefix, prefix + "_split"), (path, want)
    return f


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("qshape", list(QSHAPES))
@pytest.mark.parametrize("entry", ["paged", "paged_fp8"])
def test_paged_decode(abi, entry, qshape, page, dtype):
    """Lengths 0, 1, 31, 33 and the capacity in one batch (capacity 2048: the plan splits, most sequences have
    splits with no tile), d = 72 for the 64-row shape (a D tile that is not filled)."""
    from test_padded import check_padded

    d = head_dim(entry, qshape)
    L, call, cpu, _, _ = paged_case(abi, entry, qshape, page, d, dtype)
    assert L.need > 0
    (got,) = L.run(call, expect_path(abi, "decode_paged_fp8" if "fp8" in entry else "decode_paged", split=True), split=True)
    check_padded(got.reshape(cpu["q"].shape), paged_oracle(cpu, dtype), dtype)


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("window_left", [0, 31, 100, CAP])
@pytest.mark.parametrize("entry", ["paged_window", "paged_window_fp8"])
def test_paged_window_decode(abi, entry, window_left, dtype):
    """The same pools under a window: the window plan's (smaller) workspace size is passed exactly."""
    from test_padded import check_padded

    qshape = "sq3_g4" if window_left in (31, CAP) else "sq1_g4"
    L, call, cpu, _, _ = paged_case(abi, entry, qshape, 64, 128, dtype, window_left=window_left)
    full = abi.lib.fa_fwd_gfx950_paged_workspace_size(ctypes.byref(L.keep.paged if "fp8" in entry else L.keep), code(dtype),
                                                      int(cpu["causal"]))
    assert 0 <= L.need <= full
    (got,) = L.run(call, expect_path(abi, "decode_paged_fp8" if "fp8" in entry else "decode_paged"), split=True)
    check_padded(got.reshape(cpu["q"].shape), paged_oracle(cpu, dtype, window_left), dtype)


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("lse_layout", ["contig", "shared_prefix"])
@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("qshape", list(QSHAPES))
@pytest.mark.parametrize("entry", ["paged_lse", "paged_lse_fp8"])
def test_paged_lse_decode(abi, entry, qshape, page, lse_layout, dtype):
    """As test_paged_decode, plus the LSE: contiguous, and scattered by the strides of the shared-prefix
    composite; guards around it."""
    from test_padded import check_padded
    from test_paged_lse import check_lse, lse_oracle

    d = head_dim(entry, qshape)
    L, call, cpu, _, _ = paged_case(abi, entry, qshape, page, d, dtype, lse_layout=lse_layout)
    assert L.need > 0
    fp8 = "fp8" in entry
    got, lse = L.run(call, expect_path(abi, "decode_paged_fp8" if fp8 else "decode_paged", split=True), split=True)
    check_padded(got, paged_oracle(cpu, dtype), dtype)
    k = cpu["k"].float() if fp8 else cpu["k"]
    check_lse(lse, lse_oracle(cpu["q"], k, list(LENS), d ** -0.5, cpu["causal"], kd=cpu["kd"]), f"{entry}-{qshape}-{page}")


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("window_left", [-1, 100])
@pytest.mark.parametrize("sq", [65, 300])
def test_paged_prefill(abi, sq, window_left, dtype):
    """The paged prefill kernel: workspace size 0 and NULL, o in HF's [B, S, H, D]."""
    from test_padded import check_padded, oracle_padded
    from test_paged import make_paged
    from test_paged_abi import FaPagedParams

    lens, hq, hkv, page, cap, d = (0, 1, 65, 301, 512), 4, 2, 64, 512, 72
    b = len(lens)
    q, k, v, kc, vc, table, sl = make_paged(lens, hq, hkv, sq, page, cap, d, dtype, seeded("pp", sq, str(dtype)))
    L = Launch(abi, LARGE)
    qd = L.inp("q", q, dims=ROWCOL)
    kcd, vcd = L.inp("k_cache", kc), L.inp("v_cache", vc)
    td, sld = L.inp("block_table", table, dims=("batch", "entry")), L.inp("cache_seqlens", sl, dims=("batch",))
    o = L.out("o", dtype, q.shape, o_strides("hf", *q.shape))
    base = dense_params(qd, kcd, vcd, o, hq // hkv, d ** -0.5)
    base.seqlen_kv = cap
    base.k_seqlen_stride, base.v_seqlen_stride = kcd.stride(2), vcd.stride(2)
    p = FaPagedParams(base, td.data_ptr(), td.stride(0), table.size(1), kc.size(0), page, sld.data_ptr())
    dt = code(dtype)
    assert abi.lib.fa_fwd_gfx950_paged_prefill_workspace_size(ctypes.byref(p), dt, 1, window_left) == 0
    call = lambda: abi.lib.fa_fwd_gfx950_paged_prefill(ctypes.byref(p), dt, 1, window_left, None, 0, abi.stream())  # noqa: E731

    def expect():
        assert abi.dbg.last_path() == "w4" and abi.dbg.last_prefill_paged()

    (got,) = L.run(call, expect)
    check_padded(got, oracle_padded(q, k, v, torch.zeros_like(sl), sl, None, None, d ** -0.5, True, window_left=window_left), dtype)
    dev = lambda *ts: tuple(t.to(abi.device) for t in ts)  # noqa: E731  (the pin: the Python op on the same tensors)
    ref = abi.m.flash_attn_paged_func(*dev(q, kc, vc, table, sl), causal=True, window_left=window_left)
    assert abi.dbg.last_path() == "w4" and abi.dbg.last_prefill_paged() and torch.equal(got, ref.cpu())


@gpu
@pytest.mark.parametrize("entry", ["paged", "paged_fp8", "paged_window", "paged_lse"])
def test_paged_helper_restates_the_binding(abi, entry):
    """The arena launch equals flash_attn_paged_func's on the same (contiguous) tensors, same kernel."""
    w = 100 if "window" in entry else -1
    L, call, cpu, _, _ = paged_case(abi, entry, "sq1_g4", 64, 128, F16, window_left=w, lse_layout="contig")
    got = L.run(call, split=True)
    path = abi.dbg.last_path()
    q, sl = cpu["q"], cpu["sl"]
    dev = lambda t: t.to(abi.device)  # noqa: E731
    kw = dict(k_descale=dev(cpu["kd"]), v_descale=dev(cpu["vd"])) if "fp8" in entry else {}
    if w >= 0:
        kw["window_left"] = w
    if "lse" in entry:
        kw["return_lse"] = True
    ref = abi.m.flash_attn_paged_func(dev(q), dev(cpu["kc"]), dev(cpu["vc"]), dev(cpu["table"]), dev(sl), **kw)
    assert abi.dbg.last_path() == path
    ref = ref if isinstance(ref, tuple) else (ref,)
    assert torch.equal(got[0].reshape(q.shape), ref[0].cpu())
    if "lse" in entry:
        assert torch.equal(bits(got[1]), bits(ref[1].cpu()))


# ----------------------------------------------------------------------------------------- fa_merge_states_gfx950
@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [8, 72, 128])
@pytest.mark.parametrize("n", [1, 2, 16])
def test_merge_states(abi, n, d, dtype):
    """Row (0, 0, 0) has every part -inf (test_paged_lse.make_states); guards around out and lse, out with a
    padded row pitch."""
    from test_lse_abi import FaMergeParams
    from test_padded import check_padded
    from test_paged_lse import check_lse, make_states, merge_oracle

    b, h, s = 3, 5, 2
    outs, lses = make_states(n, b, h, s, d, dtype, seeded("merge", n, d))
    L = Launch(abi)
    od, ld = L.inp("outs", outs, dims=("part", "batch", "head", "row", "col")), L.inp("lses", lses, dims=("part", "batch", "head", "row"))
    out = L.out("out", dtype, (b, h, s, d), o_strides("pitch", b, h, s, d))
    lse = L.out("lse", F32, (b, h, s), dims=("batch", "head", "row"))
    p = FaMergeParams(od.data_ptr(), ld.data_ptr(), out.data_ptr(), lse.data_ptr(), n, b, h, s, d,
                      *od.stride()[:4], *ld.stride(), *out.stride()[:3], *lse.stride())
    go, gl = L.run(lambda: abi.lib.fa_merge_states_gfx950(ctypes.byref(p), code(dtype), abi.stream()))
    ro, rl = merge_oracle(outs, lses)
    check_padded(go, ro, dtype)
    assert (go[0, 0, 0] == 0).all()
    check_lse(gl, rl, f"merge-n{n}-d{d}")
    ref = abi.m.flash_attn_merge_states(outs.to(abi.device), lses.to(abi.device), return_lse=True)  # the binding's launch
    assert torch.equal(go, ref[0].cpu()) and torch.equal(bits(gl), bits(ref[1].cpu()))


# ----------------------------------------------------------------------------------------- entries without a workspace
@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("window_left", [-1, 100])
def test_varlen(abi, window_left, dtype):
    """Packed lengths 0, 1, 63, 65, 257 at d = 72; o [total, Hq, D] with padded head and row pitches."""
    from oracle import fa_oracle_c as OC
    from test_abi import FaFwdParams, FaVarlenParams
    from test_gpu_parity import TOL
    from test_varlen import pack

    hq, hkv, d = 4, 2, 72
    q, k, v, cu_q, cu_k, mq, mk = pack((hq, hkv, d, [(n, n) for n in (0, 1, 63, 65, 257)]), dtype, seeded("varlen", str(dtype)))
    L = Launch(abi)
    dims = ("row", "head", "col")
    qd, kd, vd = L.inp("q", q, dims=dims), L.inp("k", k, dims=dims), L.inp("v", v, dims=dims)
    cq, ck = L.inp("cu_seqlens_q", cu_q, dims=("entry",)), L.inp("cu_seqlens_k", cu_k, dims=("entry",))
    o = L.out("o", dtype, q.shape, (hq * (d + 8) + 8, d + 8, 1), dims)
    base = FaFwdParams(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), cu_q.numel() - 1, hq, hkv, mq, mk, d,
                       hq // hkv, 0, 0, 0, 0, *(t.stride(1) for t in (qd, kd, vd, o)), *(t.stride(0) for t in (qd, kd, vd, o)),
                       log2e_scale(d ** -0.5))
    vp = FaVarlenParams(base, cq.data_ptr(), ck.data_ptr())
    abi.lib.fa_fwd_gfx950_varlen_window.argtypes = [_P, _C, _C, _I, _P]
    if window_left >= 0:
        call = lambda: abi.lib.fa_fwd_gfx950_varlen_window(ctypes.byref(vp), code(dtype), 1, window_left, abi.stream())  # noqa: E731
    else:
        call = lambda: abi.lib.fa_fwd_gfx950_varlen(ctypes.byref(vp), code(dtype), 1, abi.stream())  # noqa: E731
    (got,) = L.run(call, lambda: abi.dbg.last_path() == "w4" or pytest.fail(abi.dbg.last_path()))
    ref = OC.forward_varlen(q, k, v, cu_q, cu_k, d ** -0.5, True, window_left=window_left).float()
    atol, rtol, mean_tol = TOL[dtype]
    err = (got.float() - ref).abs()
    assert torch.isfinite(got.float()).all() and bool((err <= atol + rtol * ref.abs()).all()), err.max().item()
    assert err.mean().item() <= mean_tol
    dev = lambda *ts: tuple(t.to(abi.device) for t in ts)  # noqa: E731  (the pin: the Python op on the same tensors)
    ref = abi.m.flash_attn_varlen_func(*dev(q, k, v, cu_q, cu_k), mq, mk, causal=True, window_left=window_left)
    assert abi.dbg.last_path() == "w4" and torch.equal(got, ref.cpu())


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_rope_forward(abi, d, dtype):
    """fa_fwd_gfx950_rope: q rotated inside the kernel's load (q itself must not change), o in HF's layout."""
    from test_abi import FaRopeFwdParams
    from test_gpu_parity import check, make
    from test_rope import oracle_rope, tables

    b, hq, hkv, s = 2, 4, 2, 300
    q, k, v = make(b, hq, hkv, s, s, d, dtype, seeded("rope", d, str(dtype)))
    cos, sin = tables(b, s, d, dtype, 3)
    L = Launch(abi)
    qd, kd, vd = L.inp("q", q, dims=ROWCOL), L.inp("k", k, dims=ROWCOL), L.inp("v", v, dims=ROWCOL)
    cd, sd = L.inp("cos", cos, dims=("batch", "row", "col")), L.inp("sin", sin, dims=("batch", "row", "col"))
    o = L.out("o", dtype, q.shape, o_strides("hf", *q.shape))
    rp = FaRopeFwdParams(dense_params(qd, kd, vd, o, hq // hkv, d ** -0.5), cd.data_ptr(), sd.data_ptr(), cd.stride(0), cd.stride(1))
    (got,) = L.run(lambda: abi.lib.fa_fwd_gfx950_rope(ctypes.byref(rp), code(dtype), 1, abi.stream()),
                   lambda: abi.dbg.last_path() == "w4" or pytest.fail(abi.dbg.last_path()))
    check(got, oracle_rope(q, cos, sin), k, v, d ** -0.5, True, dtype)
    dev = lambda *ts: tuple(t.to(abi.device) for t in ts)  # noqa: E731  (the pin: the Python op on the same tensors)
    ref = abi.m.flash_attn_rope_func(*dev(q, k, v, cos, sin), causal=True)
    assert abi.dbg.last_path() == "w4" and torch.equal(got, ref.cpu())


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_window_forward(abi, dtype):
    """fa_fwd_gfx950_window (it cuts the keys left of every window itself): o with a padded row pitch."""
    from oracle import fa_oracle_c as OC
    from test_gpu_parity import TOL, make

    b, hq, hkv, sq, sk, d, w = 2, 4, 2, 200, 300, 72, 100
    q, k, v = make(b, hq, hkv, sq, sk, d, dtype, seeded("window", str(dtype)))
    L = Launch(abi)
    qd, kd, vd = L.inp("q", q, dims=ROWCOL), L.inp("k", k, dims=ROWCOL), L.inp("v", v, dims=ROWCOL)
    o = L.out("o", dtype, q.shape, o_strides("pitch", *q.shape))
    p = dense_params(qd, kd, vd, o, hq // hkv, d ** -0.5)
    (got,) = L.run(lambda: abi.lib.fa_fwd_gfx950_window(ctypes.byref(p), code(dtype), 1, w, abi.stream()),
                   lambda: abi.dbg.last_path() == "w4" or pytest.fail(abi.dbg.last_path()))
    ref = OC.forward(q, k, v, d ** -0.5, True, window_left=w).float()
    tol = TOL[dtype][0]
    err = (got.float() - ref).abs()
    assert bool((err <= tol + tol * ref.abs()).all()), f"max err {err.max().item():.3e}"
    dev = lambda *ts: tuple(t.to(abi.device) for t in ts)  # noqa: E731  (the pin: the Python op on the same tensors)
    ref = abi.m.flash_attn_window_func(*dev(q, k, v), w, causal=True)
    assert abi.dbg.last_path() == "w4" and torch.equal(got, ref.cpu())


class FaRopeParams(ctypes.Structure):
    """include/fa_gfx950.h ``fa_rope_params``."""

    _fields_ = ([(n, _P) for n in ("x", "out", "cos", "sin")] +
                [(n, _I) for n in ("batch_size", "num_heads", "seqlen", "headdim", "x_batch_stride", "x_head_stride",
                                   "x_seqlen_stride", "out_batch_stride", "out_head_stride", "out_seqlen_stride",
                                   "cs_batch_stride", "cs_seqlen_stride")])


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [128, 72])
def test_rope_apply(abi, d, dtype):
    """fa_rope_gfx950 out of place: x in HF's layout, out with a padded row pitch; bit-exact (tests/test_rope.py)."""
    from test_rope import oracle_rope, tables

    b, h, s = 2, 3, 33
    x = torch.randn(b, h, s, d, generator=torch.Generator().manual_seed(d)).to(dtype)
    cos, sin = tables(b, s, d, dtype, 5)
    L = Launch(abi)
    xd = L.inp("x", x, o_strides("hf", b, h, s, d), ROWCOL)
    cd, sd = L.inp("cos", cos, dims=("batch", "row", "col")), L.inp("sin", sin, dims=("batch", "row", "col"))
    out = L.out("out", dtype, x.shape, o_strides("pitch", b, h, s, d))
    p = FaRopeParams(xd.data_ptr(), out.data_ptr(), cd.data_ptr(), sd.data_ptr(), b, h, s, d, *xd.stride()[:3],
                     *out.stride()[:3], cd.stride(0), cd.stride(1))
    (got,) = L.run(lambda: abi.lib.fa_rope_gfx950(ctypes.byref(p), code(dtype), abi.stream()))
    assert torch.equal(got, oracle_rope(x, cos, sin))
    assert torch.equal(got, abi.m.apply_rope(*(t.to(abi.device) for t in (x, cos, sin))).cpu())


@gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_kvcache_append(abi, fp8, dtype):
    """fa_kvcache_append_gfx950 / _fp8: q_out (padded row pitch) and seqlens_out guarded; the pools, which the launch
    writes in place, are compared whole with the hand-written loop of tests/test_kvcache.py / test_fp8_kvcache.py."""
    from flash_attention_cute_amd._debug import FaKvcacheParams
    from test_fp8_abi import kvcache_fp8_type
    from test_fp8_kvcache import expected_fp8_append, make_fp8_cache, pow2_descales
    from test_kvcache import LENS as KV_LENS
    from test_kvcache import expected_append, make_cache, new_tokens, rope_tables

    hq, hkv, page, cap, d, sn = 8, 2, 32, 128, 72 if not fp8 else 128, 3
    b, dev = len(KV_LENS), abi.device
    if fp8:
        kc, vc, table, sl = make_fp8_cache(KV_LENS, sn, hkv, page, cap, d, 81)
    else:
        kc, vc, table, sl = make_cache(KV_LENS, sn, hkv, page, cap, d, dtype, 81)
    k, v = new_tokens(b, hkv, sn, d, dtype, 82), new_tokens(b, hkv, sn, d, dtype, 83)
    q = new_tokens(b, hq, sn, d, dtype, 84)
    cos, sin = rope_tables(cap, d, dtype)
    L = Launch(abi)
    kn, vn, qd = L.inp("k_new", k, dims=ROWCOL), L.inp("v_new", v, dims=ROWCOL), L.inp("q", q, dims=ROWCOL)
    cd, sd = L.inp("cos", cos, dims=("row", "col")), L.inp("sin", sin, dims=("row", "col"))
    td, sld = L.inp("block_table", table, dims=("batch", "entry")), L.inp("cache_seqlens", sl, dims=("batch",))
    pools = []
    for name, pool in (("k_cache", kc), ("v_cache", vc)):  # in and out: re-written under every pattern, declared written
        t = L.arena.tensor(name, pool.dtype, pool.shape, dims=("page", "head", "row", "col"))
        L.inputs.append((L.arena.declare_written(t), pool))
        L.written.append(t)
        pools.append(t)
    q_out = L.out("q_out", dtype, q.shape, o_strides("pitch", *q.shape))
    sl_out = L.out("seqlens_out", I32, (b,), dims=("batch",))
    p = FaKvcacheParams()
    p.k_new, p.v_new, p.q, p.q_out = kn.data_ptr(), vn.data_ptr(), qd.data_ptr(), q_out.data_ptr()
    for pre, t in (("kn", kn), ("vn", vn), ("q", qd), ("qo", q_out)):
        for i, s in enumerate(("batch", "head", "seqlen")):
            setattr(p, f"{pre}_{s}_stride", t.stride(i))
    p.cos, p.sin, p.cs_row_stride, p.max_pos = cd.data_ptr(), sd.data_ptr(), cd.stride(0), cap
    p.k_cache, p.v_cache = pools[0].data_ptr(), pools[1].data_ptr()
    for pre, t in (("k", pools[0]), ("v", pools[1])):
        for i, s in enumerate(("page", "head", "row")):
            setattr(p, f"{pre}_{s}_stride", t.stride(i))
    p.block_table, p.block_table_stride, p.max_pages, p.num_pages, p.page_size = td.data_ptr(), td.stride(0), table.size(1), kc.size(0), page
    p.seqlens_k, p.seqlens_out = sld.data_ptr(), sl_out.data_ptr()
    p.batch_size, p.num_heads_q, p.num_heads_kv, p.seqlen_new, p.seqlen_q, p.headdim = b, hq, hkv, sn, sn, d
    if fp8:
        kd, vd = pow2_descales(b, hkv), pow2_descales(b, hkv, 1)
        kdd, vdd = L.inp("k_descale", kd, dims=("batch", "head")), L.inp("v_descale", vd, dims=("batch", "head"))
        p = kvcache_fp8_type()(p, kdd.data_ptr(), vdd.data_ptr(), kdd.stride(0), kdd.stride(1))
        call = lambda: abi.lib.fa_kvcache_append_fp8_gfx950(ctypes.byref(p), code(dtype), abi.stream())  # noqa: E731
    else:
        call = lambda: abi.lib.fa_kvcache_append_gfx950(ctypes.byref(p), code(dtype), abi.stream())  # noqa: E731
    gk, gv, gq, gl = L.run(call)
    to = lambda *ts: tuple(t.to(dev) for t in ts)  # noqa: E731
    if fp8:
        ek, ev = expected_fp8_append(*to(kc, vc, k, v), KV_LENS, table, *to(cos, sin), abi.m.apply_rope, *to(kd, vd))
    else:
        ek, ev = expected_append(*to(kc, vc, k, v), KV_LENS, table, *to(cos, sin), abi.m.apply_rope)
    assert torch.equal(bits(gk), bits(ek.cpu())) and torch.equal(bits(gv), bits(ev.cpu()))
    assert gl.tolist() == [n + sn for n in KV_LENS]
    qpos = torch.tensor([[max(n + i, 0) for i in range(sn)] for n in KV_LENS], device=dev)
    cdv, sdv = to(cos, sin)
    assert torch.equal(gq, abi.m.apply_rope(q.to(dev), cdv[qpos], sdv[qpos]).cpu())


# =============================================================================== 3. the op layer
@contextlib.contextmanager
def poisoned_empty():
    """Every torch.empty / empty_like is filled: NaN for floats, the maximum value for integers. Both settings
    are restored on exit."""
    det, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    fill = torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.utils.deterministic.fill_uninitialized_memory = fill
        torch.use_deterministic_algorithms(det, warn_only=warn)


def test_poisoned_empty_fills_and_restores_on_the_cpu():
    before = (torch.are_deterministic_algorithms_enabled(), torch.utils.deterministic.fill_uninitialized_memory)
    with poisoned_empty():
        assert torch.isnan(torch.empty(257, dtype=F16)).all() and torch.isnan(torch.empty_like(torch.zeros(9))).all()
        assert (torch.empty(65, dtype=I32) == torch.iinfo(I32).max).all()
    assert (torch.are_deterministic_algorithms_enabled(), torch.utils.deterministic.fill_uninitialized_memory) == before


@gpu
def test_poisoned_empty_fills_device_tensors(device):
    """The assumption of this section, as far as Python can see it: the fill reaches device allocations."""
    with poisoned_empty():
        assert torch.isnan(torch.empty(4099, dtype=BF16, device=device)).all()
        assert torch.isnan(torch.empty_like(torch.zeros(3, 5, device=device))).all()
        assert (torch.empty(65, dtype=torch.uint8, device=device) == 255).all()
        assert (torch.empty(65, dtype=I32, device=device) == torch.iinfo(I32).max).all()


def _op_cases(dev):
    """name -> thunk running one public op on fixed device inputs; returns a tensor or a tuple of tensors."""
    import flash_attention_cute_amd as m
    from test_fp8_kvcache import make_fp8_paged, pow2_descales
    from test_gpu_parity import make
    from test_kvcache import LENS as KV_LENS
    from test_kvcache import make_cache, new_tokens, rope_tables
    from test_padded import make_batch, ranges
    from test_paged import make_paged
    from test_paged_lse import make_states
    from test_rope import tables
    from test_varlen import pack

    to = lambda *ts: tuple(t.to(dev) if isinstance(t, torch.Tensor) else t for t in ts)  # noqa: E731
    cases = {}
    q, k, v = to(*make(2, 4, 2, 300, 300, 72, F16, 1))
    cases["func_causal"] = lambda: m.flash_attn_func(q, k, v, causal=True)
    qd, kd, vd = to(*make(2, 8, 2, 1, 2048, 128, BF16, 2))
    cases["func_decode_split"] = lambda: m.flash_attn_func(qd, kd, vd)
    qp, kp, vp = to(*make(1, 2, 2, 130, 130, 36, F16, 3))
    cases["func_d36_pad_path"] = lambda: m.flash_attn_func(qp, kp, vp, causal=True)
    qn = torch.randn(2, 300, 4, 80, generator=torch.Generator().manual_seed(4)).to(F16).to(dev)[..., 3:75].transpose(1, 2)
    assert not qn.is_contiguous() and qn.data_ptr() % 16 != 0
    cases["func_non_contiguous_q"] = lambda: m.flash_attn_func(qn, k, v, causal=True)
    vq, vk, vv, cu_q, cu_k, mq, mk = to(*pack((4, 2, 72, [(n, n) for n in (0, 1, 63, 65, 257)]), F16, 5))
    cases["varlen"] = lambda: m.flash_attn_varlen_func(vq, vk, vv, cu_q, cu_k, mq, mk, causal=True)
    pq, pk, pv = to(*make_batch(3, 4, 2, 200, 300, 64, BF16, 6, "bshd"))
    rg = to(*ranges(3, 200, 300, 11, "mixed"))
    cases["padded_prefill"] = lambda: m.flash_attn_padded_func(pq, pk, pv, *rg, causal=True)
    dq, dk, dv_ = to(*make_batch(5, 8, 2, 1, 2048, 128, F16, 7, "bhsd"))
    ks = torch.zeros(5, dtype=I32, device=dev)
    ke = torch.tensor([0, 1, 31, 33, 2048], dtype=I32, device=dev)
    cases["padded_decode_ragged"] = lambda: m.flash_attn_padded_func(dq, dk, dv_, ks, ke)
    rq, rk, rv = to(*make(2, 4, 2, 300, 300, 128, F16, 8))
    cos, sin = to(*tables(2, 300, 128, F16, 9))
    cases["rope"] = lambda: m.flash_attn_rope_func(rq, rk, rv, cos, sin, causal=True)
    cases["window"] = lambda: m.flash_attn_window_func(q, k, v, 100, causal=True)
    lens = (0, 1, 31, 33, 2048)
    gq, _, _, kc, vc, table, sl = to(*make_paged(lens, 8, 2, 1, 64, 2048, 128, F16, 10))
    cases["paged"] = lambda: m.flash_attn_paged_func(gq, kc, vc, table, sl)
    cases["paged_window"] = lambda: m.flash_attn_paged_func(gq, kc, vc, table, sl, window_left=100)
    cases["paged_lse"] = lambda: m.flash_attn_paged_func(gq, kc, vc, table, sl, return_lse=True)
    kdsc, vdsc = to(pow2_descales(5, 2), pow2_descales(5, 2, 2))
    fq, _, _, kc8, vc8, t8, sl8 = to(*make_fp8_paged(lens, 8, 2, 3, 64, 2048, 128, BF16, 11, kd=kdsc.cpu(), vd=vdsc.cpu()))
    cases["paged_fp8"] = lambda: m.flash_attn_paged_func(fq, kc8, vc8, t8, sl8, causal=True, k_descale=kdsc, v_descale=vdsc)
    cases["paged_fp8_window_lse"] = lambda: (m.flash_attn_paged_func(fq, kc8, vc8, t8, sl8, causal=True, k_descale=kdsc, v_descale=vdsc, window_left=31),
                                             *m.flash_attn_paged_func(fq, kc8, vc8, t8, sl8, causal=True, k_descale=kdsc, v_descale=vdsc, return_lse=True))
    hq_, _, _, hkc, hvc, ht, hsl = to(*make_paged((0, 65, 301, 512), 4, 2, 300, 64, 512, 72, F16, 12))
    cases["paged_prefill_size"] = lambda: m.flash_attn_paged_func(hq_, hkc, hvc, ht, hsl, causal=True)
    ckc, cvc, ctab, csl = make_cache(KV_LENS, 3, 2, 32, 128, 128, F16, 13)
    nk, nv, nq = to(new_tokens(3, 2, 3, 128, F16, 14), new_tokens(3, 2, 3, 128, F16, 15), new_tokens(3, 8, 3, 128, F16, 16, hf=True))
    rc, rs = to(*rope_tables(128, 128, F16))

    def with_kvcache():
        a, b_ = ckc.to(dev), cvc.to(dev)  # (fresh pools: the op appends in place)
        out = m.flash_attn_with_kvcache(nq, a, b_, nk, nv, rotary_cos=rc, rotary_sin=rs, cache_seqlens=csl.to(dev),
                                        block_table=ctab.to(dev), causal=True)
        return out, a, b_

    cases["with_kvcache"] = with_kvcache
    outs, lses = to(*make_states(3, 3, 5, 2, 72, BF16, 17))
    cases["merge_states"] = lambda: m.flash_attn_merge_states(outs, lses, return_lse=True)
    # B 5 in groups of 2 (g = 4, group rows forced to 8): two full groups and a tail group of one sequence; each
    # group's rows carry its first row's prefix page
    sq_, _, _, skc, svc, stab, ssl = make_paged((64, 100, 300, 65, 2048), 8, 2, 1, 64, 2048, 128, F16, 18)
    for lo in (0, 2):
        stab[lo + 1, 0] = stab[lo, 0]
    sq_, skc, svc, stab, ssl = to(sq_, skc, svc, stab, ssl)
    cases["shared_prefix_tail_group"] = lambda: m.flash_attn_paged_shared_prefix_func(sq_, skc, svc, stab, ssl, 64, return_lse=True,
                                                                                      _group_rows=8)
    return cases


OP_CASES = ["func_causal", "func_decode_split", "func_d36_pad_path", "func_non_contiguous_q", "varlen", "padded_prefill",
            "padded_decode_ragged", "rope", "window", "paged", "paged_window", "paged_lse", "paged_fp8", "paged_fp8_window_lse",
            "paged_prefill_size", "with_kvcache", "merge_states", "shared_prefix_tail_group"]


_OPS: dict = {}


def _same_bits(a, b):
    a, b = (x if isinstance(x, tuple) else (x,) for x in (a, b))
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(bits(x), bits(y)), f"result {i} depends on uninitialised memory"


@gpu
@pytest.mark.parametrize("name", OP_CASES)
def test_op_result_does_not_depend_on_uninitialised_memory(abi, name):
    if str(abi.device) not in _OPS:  # (the inputs are made once and never written, with_kvcache's pools are cloned)
        _OPS[str(abi.device)] = _op_cases(abi.device)
    run = _OPS[str(abi.device)][name]
    plain = run()
    with poisoned_empty():
        poisoned = run()
    torch.cuda.synchronize()
    _same_bits(plain, poisoned)
    assert abi.m.split_errors() == 0
