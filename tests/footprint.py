"""The footprint arena: what a launch writes, and what its result may depend on (tests/test_footprint.py).

Every device buffer of a launch -- inputs, tables, lengths, outputs, the workspace -- is carved from ONE
uint8 allocation filled with a repeating byte pattern. Each region is 256-byte aligned and has at least
``GUARD`` pattern bytes on both sides, so a store past an output, into the pad columns of a padded pitch or
past the bytes a ``*_workspace_size()`` function asked for lands in memory the test owns and shows up as a
byte that no longer holds the pattern: a data mismatch, never a fault.

    arena = Arena(device, 0xFF)
    o = arena.tensor("o", torch.float16, (b, h, s, d), strides, dims=("batch", "head", "row", "col"))
    arena.declare_written(o)        # its logical elements only: pitch gaps stay outside the write set
    ... launch ...
    assert arena.untouched() == []  # else e.g. ["12 bytes past the end of `o`, head 3, row 32 (0x..)"]

The three patterns (``PATTERNS``) make scratch that is consumed before it is written visible whichever way the
consumer hides it: 0xFF is NaN in fp32 / fp16 / bf16 (and -1 as int32), 0x7B a large FINITE number (a
``w == 0 ? 0 : w * x`` select hides NaN but not this; ``0 * x`` hides this but not NaN), 0x00 what fresh
memory usually holds. A result that is bit-identical under all three cannot depend on memory the launch does
not own, and every declared element was written (an unwritten one would hold three different patterns).

Not a conftest and not a test module: a helper both the CPU self-tests and the GPU tests import.
"""
from __future__ import annotations

import math

import torch

GUARD = 4096
ALIGN = 256
PATTERNS = (0xFF, 0x7B, 0x00)
_MASK_DTYPE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def extent(shape, strides) -> int:
    """Elements from the first to one past the last element a (shape, strides) view addresses."""
    if any(s == 0 for s in shape):
        return 0
    return sum((n - 1) * st for n, st in zip(shape, strides)) + 1


def contiguous_strides(shape):
    out, acc = [], 1
    for n in reversed(shape):
        out.append(acc)
        acc *= n
    return tuple(reversed(out))


class Region:
    """``nbytes`` bytes at byte ``offset`` of the arena; ``layout`` (itemsize, shape, strides, dims) of the last
    view made of it, for naming a stray byte."""

    def __init__(self, name, offset, nbytes):
        self.name, self.offset, self.nbytes, self.layout = name, offset, nbytes, None

    def __repr__(self):
        return f"Region({self.name!r}, {self.offset:#x}, {self.nbytes})"


class Arena:
    def __init__(self, device, pattern=0xFF, capacity=8 << 20):
        assert capacity % ALIGN == 0
        self.device = torch.device(device)
        self.pattern = pattern
        self.buf = torch.full((capacity,), pattern, dtype=torch.uint8, device=self.device)
        self.owned = torch.zeros(capacity, dtype=torch.uint8, device=self.device)  # != 0: in a declared write set
        self.inputs = torch.zeros(capacity, dtype=torch.uint8, device=self.device)  # != 0: an input's element
        self.regions: list[Region] = []
        base = self.buf.data_ptr()
        self._skew = (-base) % ALIGN  # (torch's allocators align far beyond 256; kept exact all the same)
        self._cursor = GUARD
        self._index = torch.arange(capacity, dtype=torch.int32, device=self.device)

    # ------------------------------------------------------------------ layout
    def carve(self, nbytes: int, name: str = "region") -> Region:
        """A 256-byte aligned region of exactly ``nbytes`` bytes with >= GUARD pattern bytes on both sides."""
        off = self._skew + math.ceil((self._cursor - self._skew) / ALIGN) * ALIGN
        end = off + nbytes
        if end + GUARD > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is too small for `{name}` ({nbytes} bytes)")
        self._cursor = end + GUARD
        r = Region(name, off, nbytes)
        self.regions.append(r)
        return r

    def view(self, region: Region, dtype, shape, strides=None, dims=None) -> torch.Tensor:
        """``region`` as a tensor of ``dtype`` / ``shape`` / element ``strides`` (as_strided): a padded row pitch,
        a padded head pitch or the [B, S, H, D] layout are all just strides. ``dims`` names the dimensions in
        reports."""
        shape = tuple(int(n) for n in shape)
        strides = contiguous_strides(shape) if strides is None else tuple(int(s) for s in strides)
        item = torch.empty((), dtype=dtype).element_size()
        assert region.offset % item == 0 and extent(shape, strides) * item <= region.nbytes, (region, shape, strides)
        assert all(s >= 0 for s in strides)
        region.layout = (item, shape, strides, dims or tuple(f"dim{i}" for i in range(len(shape))))
        flat = self.buf[region.offset:region.offset + region.nbytes - region.nbytes % item].view(dtype)
        return torch.as_strided(flat, shape, strides)

    def tensor(self, name, dtype, shape, strides=None, dims=None, tail_bytes=0) -> torch.Tensor:
        """carve + view: the region ends exactly where the view's last element ends (plus ``tail_bytes``), so
        the very next byte is guard."""
        shape = tuple(int(n) for n in shape)
        strides = contiguous_strides(shape) if strides is None else tuple(int(s) for s in strides)
        item = torch.empty((), dtype=dtype).element_size()
        region = self.carve(extent(shape, strides) * item + tail_bytes, name)
        return self.view(region, dtype, shape, strides, dims)

    def region_of(self, t: torch.Tensor) -> Region:
        off = t.data_ptr() - self.buf.data_ptr()
        for r in self.regions:
            if r.offset <= off < r.offset + max(r.nbytes, 1):
                return r
        raise KeyError("tensor is not a view of this arena")

    # ------------------------------------------------------------------ patterns and write sets
    def fill(self, pattern: int) -> None:
        """A new pattern everywhere; the layout and the declared write sets stay."""
        self.pattern = pattern
        self.buf.fill_(pattern)

    def refill(self, region: Region, pattern: int) -> None:
        """Dirty one region (scratch between two launches) with any byte value."""
        self.buf[region.offset:region.offset + region.nbytes].fill_(pattern)

    def bytes_of(self, region: Region) -> torch.Tensor:
        return self.buf[region.offset:region.offset + region.nbytes]

    def _same_layout(self, of: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        assert t.untyped_storage().data_ptr() == self.buf.untyped_storage().data_ptr(), "not a view of this arena"
        return torch.as_strided(of.view(_MASK_DTYPE[t.element_size()]), t.shape, t.stride(), t.storage_offset())

    def declare_written(self, t: torch.Tensor) -> torch.Tensor:
        """``t``'s logical elements, exactly, join the set of bytes a launch may write. The gaps of a strided
        view (between rows, heads, batch rows) do not."""
        if t.numel():
            self._same_layout(self.owned, t).fill_(-1 if t.element_size() > 1 else 255)
        return t

    def declare_input(self, t: torch.Tensor, value: torch.Tensor | None = None) -> torch.Tensor:
        """``t``'s logical elements hold an input (``value`` is copied in): they are exempt from the pattern
        check and compared with a snapshot instead (:meth:`inputs_changed`). Their pitch gaps are not exempt."""
        if t.numel():
            self._same_layout(self.inputs, t).fill_(-1 if t.element_size() > 1 else 255)
            if value is not None:
                t.copy_(value)
        return t

    def reset(self, pattern: int | None = None) -> "Arena":
        """Forget the layout and every declaration; the allocation is kept (a test reuses one arena)."""
        self.regions.clear()
        self._cursor = GUARD
        self.owned.zero_()
        self.inputs.zero_()
        self.fill(self.pattern if pattern is None else pattern)
        return self

    def snapshot(self) -> torch.Tensor:
        return self.buf.clone()

    def inputs_changed(self, snapshot: torch.Tensor) -> torch.Tensor:
        """Bytes of the declared inputs that differ from ``snapshot`` (a device scalar, no synchronisation)."""
        return ((self.buf != snapshot) & (self.inputs != 0)).sum()

    # ------------------------------------------------------------------ the check
    def probe(self, first: int = 8):
        """Device side of :meth:`untouched`: (count, first offsets) as device tensors, no synchronisation."""
        bad = (self.buf != self.pattern) & (self.owned == 0) & (self.inputs == 0)
        count = bad.sum()
        big = self.buf.numel()
        offs = torch.where(bad, self._index, torch.full_like(self._index, big))
        return count, torch.topk(offs, min(first, big), largest=False, sorted=True).values

    def report(self, probed) -> list[str]:
        count, offs = probed
        n = int(count.item())  # (one small transfer; the comparison ran on the device)
        if n == 0:
            return []
        out = [self.describe(o) for o in offs.tolist()[:n]]
        if n > len(out):
            out.append(f"... {n} bytes in all")
        return out

    def untouched(self, first: int = 8) -> list[str]:
        """Bytes outside every declared write set that no longer hold the pattern, by name; [] when the launch
        kept to its footprint."""
        return self.report(self.probe(first))

    def describe(self, off: int) -> str:
        """`off` (a byte offset of the arena) in terms of the nearest region and its layout."""
        where = f"(arena byte {off:#x})"
        best, best_d = None, None
        for r in self.regions:
            d = 0 if r.offset <= off < r.offset + r.nbytes else min(abs(off - r.offset), abs(off - (r.offset + r.nbytes - 1)))
            if best is None or d < best_d:
                best, best_d = r, d
        if best is None:
            return f"a byte of the empty arena {where}"
        r = best
        rel = off - r.offset
        if rel < 0:
            return f"{-rel} bytes before the start of `{r.name}` {where}"
        if r.layout is None:
            if rel >= r.nbytes:
                return f"{rel - r.nbytes + 1} bytes past the end of `{r.name}` {where}"
            return f"byte {rel} of `{r.name}` {where}"
        item, shape, strides, dims = r.layout
        used = extent(shape, strides) * item
        # the element at or before the byte, largest stride first (for the views used here the strides nest)
        last = len(shape) - 1
        order = sorted(range(last), key=lambda i: -strides[i])
        el, idx = min(rel, max(used - 1, 0)) // item, {}
        for i in order:
            idx[i] = min(el // strides[i], shape[i] - 1) if strides[i] else 0
            el -= idx[i] * strides[i]
        at = ", ".join(f"{dims[i]} {idx[i]}" for i in range(last)) or f"{dims[last]} {shape[last] - 1}"
        if rel >= used:
            return f"{rel - used + 1} bytes past the end of `{r.name}`, {at} {where}"
        col = el // max(strides[last], 1)  # position along the innermost dimension, counted from the row start
        if col >= shape[last]:
            past = (el - (shape[last] - 1) * strides[last] - 1) * item + rel % item + 1
            return f"{past} bytes past the end of {at} of `{r.name}`, in a pitch gap {where}"
        return f"`{r.name}`, {at}, {dims[last]} {col}: outside the declared write set {where}"
