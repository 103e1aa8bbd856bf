"""The large-address arena: every buffer of a launch at addresses where a 32-bit term is wrong (tests/test_large_address.py).

tests/footprint.py's ``Arena`` keeps three shadow buffers (five times its bytes) and an int32 index, so it stops at
2 GiB. This one is a single uint8 allocation of ``ARENA_BYTES`` (9 GiB) filled with one byte pattern, and a plain
Python-integer model of where every tensor of a case lies in it.

Layout rule (``Placement`` asserts it): a tensor's base lies at least ``BASE_MIN`` (4 GiB) into the arena and its
last live byte at most ``SPAN_MAX`` (4.5 GiB + 1 MiB) past its base. Any ONE term of an address kept in 32 bits -- its
byte offset or its element offset (2-byte and 1-byte elements), signed or unsigned -- then moves the address by a
multiple of 2^32 bytes (or 2^33 for a 2-byte element offset, which a 4.5 GiB span never reaches) downwards by at
most 4 GiB: inside the arena, never outside it. 4-byte elements (LSE, descales) would move by 2^34 bytes on an
element-offset mistake, but 2^31 of them are 8 GiB, beyond any span used here, so that mistake changes nothing and
only their byte-offset mistakes are modelled as reachable.

Two halves:

* ``Placement`` / ``Plan`` / ``MISTAKES`` -- integers only (numpy int64 / Python int), no device: the address of
  every live row, the address each single-term mistake would give instead, and what lies there.
* ``BigArena`` -- the device allocation: ``view`` a placement, ``load`` an input, ``expect`` an output, and
  ``settle``: inputs unchanged, outputs copied out, the pattern put back over exactly those elements, and the WHOLE
  arena compared with the pattern in chunks of 256 MiB. A store that went 2 or 4 GiB astray is a stray byte.

Not a conftest and not a test module.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

GIB = 1 << 30
MIB = 1 << 20
ARENA_BYTES = 9 * GIB
BASE_MIN = 4 * GIB
SPAN_MAX = 4 * GIB + GIB // 2 + MIB
SMALL_ZONE = 8 * GIB + 16 * MIB  # compact tensors (q, tables, lengths, outputs) are bumped from here on
CHUNK = 256 * MIB
PATTERNS = (0xFF, 0x7B)  # NaN in every float type / a large finite number (tests/footprint.py)

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def item_size(dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


def s32(x):
    """x kept in a signed 32-bit register (numpy int64 array or int)."""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def u32(x):
    return x & 0xFFFFFFFF


# name -> f(index, stride_elements, itemsize) = the term's BYTE contribution under that mistake
MISTAKES = {
    "byte_i32": lambda i, st, it: s32(i * st * it),        # the term's byte offset kept in int32
    "byte_u32": lambda i, st, it: u32(i * st * it),        # ... in uint32
    "elem_i32": lambda i, st, it: s32(i * st) * it,        # the term's element offset kept in int32
    "elem_u32": lambda i, st, it: u32(i * st) * it,        # ... in uint32
    "stride2_i32": lambda i, st, it: i * s32(st * it),     # a stride taken as int after scaling to bytes
}


class Placement:
    """One tensor of a case: ``shape`` / element ``strides`` at byte ``base`` of the arena, the last dimension
    contiguous (a row). ``dims`` names the other dimensions ("page", "head", "row", "batch", "part", "packed", ...);
    ``live`` is an int64 array [n, len(shape) - 1] of the rows the case places in the arena (default: all of them);
    ``data`` a bool mask over them: the rows the launch reads or writes (default: all) -- the others are poison rows
    that travel with a page (the NaN tail of a sequence's last page)."""

    def __init__(self, name, dtype, shape, strides, base, dims, live=None, written=False, data=None):
        self.name, self.dtype, self.item = name, dtype, item_size(dtype)
        self.shape, self.strides = tuple(int(n) for n in shape), tuple(int(s) for s in strides)
        self.base, self.dims, self.written = int(base), tuple(dims), written
        assert len(self.dims) == len(self.shape) - 1 and self.strides[-1] == 1 and self.base % self.item == 0
        if live is None:
            grids = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in self.shape[:-1]], indexing="ij")
            live = np.stack([g.reshape(-1) for g in grids], axis=1) if grids else np.zeros((1, 0), np.int64)
        nd = len(self.shape) - 1
        self.live = np.asarray(live, dtype=np.int64).reshape(-1, nd) if nd else np.zeros((1, 0), np.int64)
        self.row_bytes = self.shape[-1] * self.item
        self.data = np.ones(len(self.live), bool) if data is None else np.asarray(data, bool).reshape(-1)
        assert len(self.data) == len(self.live)
        if len(self.live):
            assert (self.live >= 0).all() and (self.live < np.array(self.shape[:-1], np.int64)).all(), name
            last = int(self.right().max()) + self.row_bytes
            assert self.base >= BASE_MIN, f"{name}: base {self.base:#x} lies below 4 GiB"
            assert last - self.base <= SPAN_MAX, f"{name}: live data reaches {last - self.base:#x} past its base"
            assert last <= ARENA_BYTES, f"{name}: live data ends at {last:#x}, past the arena"

    def terms(self):
        """int64 [n, dims]: every live row's byte contribution per dimension, computed in 64 bits."""
        return self.live * (np.array(self.strides[:-1], np.int64) * self.item)

    def right(self):
        """The byte address (arena offset) of every live row."""
        return self.base + self.terms().sum(axis=1)

    def wrong(self, dim: str, mistake: str):
        """The address of every live row when dimension ``dim``'s term alone is computed with ``mistake``."""
        d = self.dims.index(dim)
        bad = MISTAKES[mistake](self.live[:, d], self.strides[d], self.item)
        return self.right() - self.terms()[:, d] + bad


class Plan:
    """The placements of one case, and what a byte of the arena holds under it."""

    def __init__(self, name):
        self.name, self.placements, self._cursor = name, {}, SMALL_ZONE

    def add(self, *a, **kw) -> Placement:
        p = Placement(*a, **kw)
        assert p.name not in self.placements
        self.placements[p.name] = p
        return p

    def small(self, name, dtype, shape, dims=None, written=False) -> Placement:
        """A compact tensor in the small zone above 8 GiB, 4 KiB of pattern between neighbours."""
        shape = tuple(int(n) for n in shape)
        strides, acc = [], 1
        for n in reversed(shape):
            strides.append(acc)
            acc *= n
        dims = dims or tuple(f"dim{i}" for i in range(len(shape) - 1))
        base = (self._cursor + 4095) // 4096 * 4096
        self._cursor = base + max(acc, 1) * item_size(dtype) + 4096
        assert self._cursor <= ARENA_BYTES
        return self.add(name, dtype, shape, tuple(reversed(strides)), base, dims, written=written)

    def rows(self):
        """(starts sorted, row_bytes, owner index, row index) over every live row of every placement."""
        st, rb, who, idx = [], [], [], []
        for k, p in enumerate(self.placements.values()):
            r = p.right()
            st.append(r)
            rb.append(np.full(len(r), p.row_bytes, np.int64))
            who.append(np.full(len(r), k, np.int64))
            idx.append(np.arange(len(r), dtype=np.int64))
        st, rb, who, idx = (np.concatenate(x) for x in (st, rb, who, idx))
        o = np.argsort(st, kind="stable")
        return st[o], rb[o], who[o], idx[o]

    def check_disjoint(self):
        st, rb, _, _ = self.rows()
        assert (st[1:] >= st[:-1] + rb[:-1]).all(), f"{self.name}: two live rows overlap"

    def holder(self, addr):
        """For byte addresses ``addr``: (owner index, row index) of the live row that holds each, -1 where the
        arena holds the pattern there."""
        st, rb, who, idx = self.rows()
        k = np.searchsorted(st, addr, side="right") - 1
        inside = (k >= 0) & (addr < st[np.maximum(k, 0)] + rb[np.maximum(k, 0)])
        return np.where(inside, who[np.maximum(k, 0)], -1), np.where(inside, idx[np.maximum(k, 0)], -1)

    def mistakes(self):
        """Every (tensor, dim, mistake) -> dict(changed rows, lowest / highest wrong address, one example, where it
        lands). Asserts nothing; the self-tests do."""
        out = {}
        names = list(self.placements)
        for k, p in enumerate(self.placements.values()):
            if not len(p.live):
                continue
            right = p.right()
            poison = [q.data for q in self.placements.values()]
            for dim in p.dims:
                for m in MISTAKES:
                    w = p.wrong(dim, m)
                    ch = (w != right) & p.data  # (a poison row is never addressed by the launch)
                    rec = {"changed": int(ch.sum()), "lo": int(w.min()), "hi": int(w.max()) + p.row_bytes}
                    if ch.any():
                        i = int(np.argmax(ch))
                        who, idx = self.holder(w[ch])
                        rec["example"] = (tuple(int(x) for x in p.live[i]), int(right[i]), int(w[i]))
                        rec["lands_on_itself"] = int(((who == k) & (idx == np.nonzero(ch)[0])).sum())
                        rec["lands"] = sorted({"pattern" if o < 0 else names[o] if poison[o][j] else names[o] + ":poison"
                                               for o, j in zip(who.tolist(), idx.tolist())})
                    out[(p.name, dim, m)] = rec
        return out


def high_page_table(counts, num_pages, thresholds, seed):
    """Page ids for sequences of ``counts[b]`` pages in a pool of ``num_pages``: the ids on both sides of each
    threshold (t - 1, t), 0, 1 and num_pages - 1 first -- the longest sequence takes the threshold pairs in
    ascending order, so it crosses each between consecutive pages -- then a seeded shuffle of the ids above the
    highest threshold. Returns a list of lists; every id is used once."""
    pairs = [i for t in sorted(thresholds) for i in (t - 1, t)]
    groups = [pairs, [0, num_pages - 1], [1]]
    g = torch.Generator().manual_seed(seed)
    highs = [max(thresholds) + 1 + int(i) for i in torch.randperm(num_pages - 2 - max(thresholds), generator=g)]
    order = sorted(range(len(counts)), key=lambda b: -counts[b])
    take, spare = {}, []
    for r, b in enumerate(order):
        grp = groups[r] if r < len(groups) else []
        take[b] = grp[:counts[b]]
        spare += grp[counts[b]:]
    for grp in groups[len(order):]:
        spare += grp
    fill = spare + highs
    out = []
    for b in range(len(counts)):
        need = counts[b] - len(take[b])
        assert need <= len(fill), "the pool has too few pages above the highest threshold for this case"
        out.append(take[b] + fill[:need])
        fill = fill[need:]
    flat = [i for row in out for i in row]
    assert len(set(flat)) == len(flat) and all(0 <= i < num_pages for i in flat)
    return out


# ------------------------------------------------------------------------------------------------ the device half
def _pattern_int(pattern: int, size: int) -> int:
    return int.from_bytes(bytes([pattern]) * size, "little", signed=size > 1)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(_BITS[t.element_size()])


def _pieces(view: torch.Tensor, src):
    """``view`` cut along its leading dimensions until each piece spans less than 2^31 bytes."""
    span = sum((n - 1) * s for n, s in zip(view.shape, view.stride())) if view.numel() else 0
    if span * view.element_size() < (1 << 31) or view.dim() <= 1:
        yield view, src
        return
    for i in range(view.size(0)):
        yield from _pieces(view[i], None if src is None else src[i])


class BigArena:
    def __init__(self, device, nbytes: int = ARENA_BYTES):
        self.device = torch.device(device)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.words = self.buf.view(torch.int64)
        self.pattern = None
        self._inputs, self._outputs = [], []

    def fill(self, pattern: int) -> None:
        self.words.fill_(_pattern_int(pattern, 8))
        self.pattern = pattern
        self._inputs, self._outputs = [], []

    def view(self, p: Placement) -> torch.Tensor:
        flat = self.buf if p.dtype == torch.uint8 else self.buf.view(p.dtype)
        return torch.as_strided(flat, p.shape, p.strides, p.base // p.item)

    def load(self, view: torch.Tensor, value: torch.Tensor, updated: str | None = None) -> torch.Tensor:
        """Copy an input in (bit for bit) and remember it: ``settle`` checks it unchanged -- or, for a buffer the
        launch updates in place (a cache page of an append), returns it under the name ``updated``."""
        value = value.to(self.device)
        assert value.shape == view.shape and value.dtype == view.dtype, (value.shape, view.shape, value.dtype)
        for v, s in _pieces(view, value):
            _bits(v).copy_(_bits(s))
            if updated is None:
                self._inputs.append((v, _bits(s).clone()))
        if updated is not None:
            self._outputs.append((updated, view))
        return view

    def expect(self, view: torch.Tensor, name: str) -> torch.Tensor:
        """Declare ``view``'s logical elements as written by the launch."""
        self._outputs.append((name, view))
        return view

    def settle(self) -> dict:
        """After the launch: the inputs hold what was loaded, the declared outputs are copied out (returned by
        name), the pattern goes back over exactly those elements, and the whole arena must equal the pattern
        again."""
        torch.cuda.synchronize(self.device)
        outs = {}
        for name, v in self._outputs:
            outs[name] = torch.empty(v.shape, dtype=v.dtype, device=self.device)
            for piece, dst in _pieces(v, outs[name]):
                _bits(dst).copy_(_bits(piece))
        changed = []
        for v, s in self._inputs:
            if not torch.equal(_bits(v), s):
                changed.append(v.data_ptr() - self.buf.data_ptr())
        self.erase()
        stray = self.stray()
        assert not changed, f"inputs changed by the launch, at arena bytes {[hex(c) for c in changed[:8]]}"
        assert not stray, f"bytes outside the declared write set no longer hold the pattern: {stray}"
        return outs

    def erase(self) -> None:
        for v in [x for x, _ in self._inputs] + [x for _, x in self._outputs]:
            for piece, _ in _pieces(v, None):
                _bits(piece).fill_(_pattern_int(self.pattern, piece.element_size()))
        self._inputs, self._outputs = [], []

    def stray(self, first: int = 4):
        """Byte offsets (hex, 8-byte granules) that do not hold the pattern; [] when the arena is clean."""
        pat, step = _pattern_int(self.pattern, 8), CHUNK // 8
        counts = [(self.words[i:i + step] != pat).sum() for i in range(0, self.words.numel(), step)]
        counts = torch.stack(counts).tolist()
        out = []
        for c, n in enumerate(counts):
            if n and len(out) < first:
                w = self.words[c * step:(c + 1) * step]
                at = torch.nonzero(w != pat)[:first - len(out), 0].tolist()
                out += [hex((c * step + a) * 8) for a in at]
        if out:
            out.append(f"{sum(counts)} 8-byte granules in all")
        return out

    @contextlib.contextmanager
    def case(self, pattern: int):
        """A case under ``pattern``: the arena holds it everywhere on entry, and again after a failure (so one
        failing case does not fail the next through leftovers)."""
        if self.pattern != pattern:
            self.fill(pattern)
        try:
            yield self
        except BaseException:
            self.fill(pattern)
            raise
        assert not self._inputs and not self._outputs, "a case must end with settle()"
