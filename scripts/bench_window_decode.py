"""Same-process A/B of the sliding-window paged decode, and of the unwindowed paged decodes against another
build of the library.

    timeout -k 10 900 python scripts/bench_window_decode.py [--rounds R] [--inner N] [--parent-lib LIB.so]
                                                            [--regression-only] [--out FILE.json]

Window arms (``flash_attn_paged_func``; bf16 q, Hq 32 / Hkv 8 / D 128, page size 64, shuffled pages, window_left
4095), on a 16-bit pool and on an FP8 (e4m3) pool, for B 16 with lengths spread over 8192..32768 and for B 1 with
131072 keys:

  (a)  the windowed decode on the full cache
  (b)  the unwindowed decode on the full cache
  (c)  the unwindowed decode on a cache that holds only each sequence's last window_left + 1 keys: the floor of (a)
  (c') (c) again: the run's own A/A spread

Every round times a, b, c, c' in that order; a sample is ``--inner`` back-to-back calls between two device
events, ending in a synchronise; the figure per arm is the median over the rounds. Recorded per shape: a/b, a/c
and the spread |c - c'| / mean. (a) is checked against (c) before timing: the same visible keys, so the outputs
agree within the 16-bit tolerance (not bit for bit: the window may start mid-tile in (a)).

Regression arms (``--parent-lib``: the library of another build, e.g. the parent commit's): the UNWINDOWED 16-bit
and FP8 paged decodes (fa_fwd_gfx950_paged, fa_fwd_gfx950_paged_fp8) of this build's library and of that one,
called through the C ABI on the same buffers, on bench_paged_decode.py's shapes (B 32 capacity 4096 lengths
1024..4000; B 1 131072 keys) at page size 64, and the WINDOWED ones (fa_fwd_gfx950_paged_window,
fa_fwd_gfx950_paged_window_fp8, window_left 4095) on the window shapes above. Every round times new, parent, new
again; recorded: the ratio new / parent (new = the mean of its two medians), the spread |new - new'| / mean and
whether new / parent <= 1 + 2 x that spread. The outputs of the two libraries are checked bit-equal before timing.
``--regression-only`` skips the window arms.

Prints one JSON object (and writes it to ``--out``, by default profiles/window_decode_ab.json).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
HQ, HKV, D, PAGE, W = 32, 8, 128, 64, 4095
WINDOW_SHAPES = {
    "b16_8k_32k": dict(B=16, cap=32768, lens=[8192 + (24576 * i) // 15 for i in range(16)]),
    "b1_128k": dict(B=1, cap=131072, lens=[131072]),
}
REGRESSION_SHAPES = {  # scripts/bench_paged_decode.py SHAPES
    "decode_padded": dict(B=32, cap=4096, lens=[1024 + 96 * i for i in range(32)]),
    "decode_long": dict(B=1, cap=131072, lens=[131072]),
}


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def timed(variants, rounds, inner):
    for _, fn in variants:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            times[n].append(sample(fn, inner))
    return {n: statistics.median(t) for n, t in times.items()}


def random_pool(b, cap, fp8, gen, dev):
    """A pool [B * cap / PAGE, Hkv, PAGE, D] of random keys under a random page permutation, and its table."""
    n = b * cap // PAGE
    pool = lambda: torch.randn(n, HKV, PAGE, D, generator=gen, device=dev, dtype=BF16)  # noqa: E731
    kc, vc = pool(), pool()
    if fp8:
        kc, vc = kc.to(FP8), vc.to(FP8)
    table = torch.randperm(n, generator=gen, device=dev).reshape(b, cap // PAGE).to(torch.int32)
    return kc, vc, table


def tail_cache(kc, vc, table, lens, keep):
    """The last `keep` keys of every sequence (`keep` and the lengths multiples of PAGE here) as a cache of
    its own: the pages' table entries, in order -- no copy, the pool is shared."""
    rows = [table[i, (n - keep) // PAGE:n // PAGE] for i, n in enumerate(lens)]
    return torch.stack(rows).contiguous()


def run_window_shape(name, s, fp8, rounds, inner, dev):
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    gen = torch.Generator(device=dev).manual_seed(1)
    lens = [n // PAGE * PAGE for n in s["lens"]]  # (page multiples, so that (c) shares the pool's pages)
    q = torch.randn(s["B"], HQ, 1, D, generator=gen, device=dev, dtype=BF16)
    kc, vc, table = random_pool(s["B"], s["cap"], fp8, gen, dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    keep = W + 1
    tail_table = tail_cache(kc, vc, table, lens, keep)
    tail_sl = torch.full_like(sl, keep)
    ds = {}
    if fp8:
        ds = dict(k_descale=torch.full((s["B"], HKV), 0.5, device=dev), v_descale=torch.full((s["B"], HKV), 2.0, device=dev))
    a = lambda: flash_attn_paged_func(q, kc, vc, table, sl, window_left=W, **ds)  # noqa: E731
    b = lambda: flash_attn_paged_func(q, kc, vc, table, sl, **ds)  # noqa: E731
    c = lambda: flash_attn_paged_func(q, kc, vc, tail_table, tail_sl, **ds)  # noqa: E731
    out_a = a()
    path_a = _debug.last_path()
    out_c = c()
    path_c = _debug.last_path()
    b()
    path_b = _debug.last_path()
    torch.cuda.synchronize()
    err = (out_a.float() - out_c.float()).abs().max().item()
    if not err <= 1.6e-2:
        raise AssertionError(f"{name}: the windowed decode differs from the decode of the window's keys by {err}")
    med = timed([("a", a), ("b", b), ("c", c), ("c2", c)], rounds, inner)
    c_ms = 0.5 * (med["c"] + med["c2"])
    return {"shape": name, "cache": "fp8" if fp8 else "bf16", "B": s["B"], "Hq": HQ, "Hkv": HKV, "D": D, "page_size": PAGE,
            "window_left": W, "lens_min": min(lens), "lens_max": max(lens), "paths": {"a": path_a, "b": path_b, "c": path_c},
            "max_abs_a_minus_c": err, "a_windowed_ms": round(med["a"], 5), "b_unwindowed_ms": round(med["b"], 5),
            "c_window_only_ms": round(med["c"], 5), "c2_window_only_ms": round(med["c2"], 5),
            "ratio_a_over_b": round(med["a"] / med["b"], 4), "ratio_a_over_c": round(med["a"] / c_ms, 4),
            "aa_spread_pct": round(100.0 * abs(med["c"] - med["c2"]) / c_ms, 3)}


# ---- the C ABI, for the regression arms (two libraries in one process) -------------------------------------------
class FwdParams(ctypes.Structure):  # include/fa_gfx950.h fa_fwd_params
    _fields_ = ([(n, ctypes.c_void_p) for n in ("q", "k", "v", "o")]
                + [(n, ctypes.c_int64) for n in ("B", "Hq", "Hkv", "Sq", "Sk", "D", "g")]
                + [(f"{t}_{dim}", ctypes.c_int64) for dim in ("batch", "head", "seq") for t in "qkvo"]
                + [("scale", ctypes.c_float)])


class PagedParams(ctypes.Structure):  # include/fa_gfx950_paged.h fa_paged_params
    _fields_ = [("base", FwdParams), ("block_table", ctypes.c_void_p), ("block_table_stride", ctypes.c_int64),
                ("max_pages", ctypes.c_int64), ("num_pages", ctypes.c_int64), ("page_size", ctypes.c_int64),
                ("seqlens_k", ctypes.c_void_p)]


class PagedFp8Params(ctypes.Structure):  # include/fa_gfx950_fp8.h fa_paged_fp8_params
    _fields_ = [("paged", PagedParams), ("k_descale", ctypes.c_void_p), ("v_descale", ctypes.c_void_p),
                ("descale_batch_stride", ctypes.c_int64), ("descale_head_stride", ctypes.c_int64)]


def abi_call(lib, fp8, q, o, kc, vc, table, sl, kd, vd, window_left=None):
    """A closure that launches the paged decode of `lib` (window_left None: the unwindowed entry) on the current
    stream: the Sq == 1 decode step as the binding passes it (the q-heads of a kv group packed into the rows of
    an MHA problem)."""
    g = HQ // HKV
    base = FwdParams(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), q.size(0), HKV, HKV, g,
                     table.size(1) * PAGE, D, 1,
                     HQ * D, kc.stride(0), vc.stride(0), HQ * D, g * D, kc.stride(1), vc.stride(1), g * D,
                     D, kc.stride(2), vc.stride(2), D, D ** -0.5 * 1.4426950408889634)
    paged = PagedParams(base, table.data_ptr(), table.stride(0), table.size(1), kc.size(0), PAGE, sl.data_ptr())
    p = PagedFp8Params(paged, kd.data_ptr(), vd.data_ptr(), HKV, 1) if fp8 else paged
    win = () if window_left is None else (ctypes.c_int64(window_left),)
    stem = "fa_fwd_gfx950_paged" + ("_window" if win else "") + ("_fp8" if fp8 else "")
    size = getattr(lib, stem + "_workspace_size")
    size.restype = ctypes.c_int64
    n = size(ctypes.byref(p), 1, 0, *win)
    if n < 0:
        raise AssertionError(f"{stem}_workspace_size failed")
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=q.device)
    fn = getattr(lib, stem)
    fn.argtypes = ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * len(win)
                   + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        rc = fn(ctypes.byref(p), 1, 0, *win, ws.data_ptr() if n > 0 else None, n, stream)
        if rc != 0:
            raise AssertionError(f"{stem} failed ({rc})")

    call.keep = (p, ws)
    return call


def run_regression_shape(name, s, fp8, new_lib, parent_lib, rounds, inner, dev, window_left=None):
    gen = torch.Generator(device=dev).manual_seed(2)
    q = torch.randn(s["B"], HQ, 1, D, generator=gen, device=dev, dtype=BF16)
    kc, vc, table = random_pool(s["B"], s["cap"], fp8, gen, dev)
    sl = torch.tensor(s["lens"], dtype=torch.int32, device=dev)
    kd, vd = torch.full((s["B"], HKV), 0.5, device=dev), torch.full((s["B"], HKV), 2.0, device=dev)
    o_new, o_parent = torch.empty_like(q), torch.empty_like(q)
    new = abi_call(new_lib, fp8, q, o_new, kc, vc, table, sl, kd, vd, window_left)
    parent = abi_call(parent_lib, fp8, q, o_parent, kc, vc, table, sl, kd, vd, window_left)
    new()
    parent()
    torch.cuda.synchronize()
    if not torch.equal(o_new, o_parent):
        raise AssertionError(f"{name}: the decode of the two libraries differs")
    med = timed([("new", new), ("parent", parent), ("new2", new)], rounds, inner)
    new_ms = 0.5 * (med["new"] + med["new2"])
    spread = 100.0 * abs(med["new"] - med["new2"]) / new_ms
    ratio = new_ms / med["parent"]
    return {"shape": name, "cache": "fp8" if fp8 else "bf16", "B": s["B"], "capacity": s["cap"], "page_size": PAGE,
            "window_left": window_left, "bit_equal": True, "new_ms": round(med["new"], 5), "parent_ms": round(med["parent"], 5),
            "new2_ms": round(med["new2"], 5), "ratio_new_over_parent": round(ratio, 4),
            "aa_spread_pct": round(spread, 3), "within_twice_the_spread": abs(ratio - 1.0) * 100.0 <= 2.0 * spread,
            "not_slower_than_twice_the_spread": (ratio - 1.0) * 100.0 <= 2.0 * spread}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libfa_gfx950.so of the build to compare the unwindowed decodes with")
    ap.add_argument("--regression-only", action="store_true", help="skip the window arms (a / b / c)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "window_decode_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_decode needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    result = {"script": "scripts/bench_window_decode.py", "device": torch.cuda.get_device_name(dev),
              "rounds": args.rounds, "inner": args.inner,
              "method": "median over rounds of (inner calls between two device events) / inner; window arms per round: "
                        "a (windowed, full cache), b (unwindowed, full cache), c (unwindowed, the window's keys only), c "
                        "again; regression arms per round: new, parent, new again",
              "window": [] if args.regression_only else
                        [run_window_shape(n, s, fp8, args.rounds, args.inner, dev)
                         for fp8 in (False, True) for n, s in WINDOW_SHAPES.items()]}
    if args.parent_lib:
        from flash_attention_cute_amd import _build

        new_lib, parent_lib = ctypes.CDLL(str(_build.ABI_LIB)), ctypes.CDLL(str(Path(args.parent_lib).resolve()))
        result["regression"] = [run_regression_shape(n, s, fp8, new_lib, parent_lib, args.rounds, args.inner, dev)
                                for fp8 in (False, True) for n, s in REGRESSION_SHAPES.items()]
        result["regression"] += [run_regression_shape(n, s, fp8, new_lib, parent_lib, args.rounds, args.inner, dev, W)
                                 for fp8 in (False, True) for n, s in WINDOW_SHAPES.items()]
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
