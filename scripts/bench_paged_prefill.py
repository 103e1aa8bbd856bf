"""Same-process A/B of the in-place paged prefill against the copying path and the dense floor.

    timeout -k 10 900 python scripts/bench_paged_prefill.py [--rounds R] [--inner N] [--out FILE.json]

Chunked prefill at the Llama-3-8B head shape (bf16, Hq 32, Hkv 8, D 128, causal): a chunk of 512 positions
for each of 8 sequences over caches of 4k, 16k and 32k keys, and one sequence's 2048 positions over 32k and
128k keys. Every cache is full (length = capacity, the copying path's best case: its gather moves the
capacity, whatever the lengths). For page sizes 64 / 128 / 256, once through a random permutation of the
pages and once with the pages in sequence order, every round times

  (a) the in-place call, ``flash_attn_paged_func`` (the paged fa_fwd_w4);
  (b) the path it replaces: ``_gather_pages`` of K and of V, then ``flash_attn_padded_func`` on the copies;
  (c) ``flash_attn_padded_func`` on an already-gathered dense cache -- the floor: no lookup, no copy;

with (c) timed at the start AND at the end of the round, so the run carries its own A/A spread (the two
medians of c) next to every ratio. At these shapes the padded op runs head-packed causal blocks, which the
paged kernel does not have; ``c_plain`` is (c) held to plain 256-row blocks (the head_pack knob off), the
same layout as (a), so a / c_plain is the cost of the lookup alone. One process, one ``timeout``. A sample is ``--inner`` back-to-back calls
between two device events; the figure per variant is the median over the rounds. Outputs are checked
bit-equal before timing. Prints one JSON object (and writes it to ``--out``).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from scripts.bench_paged_decode import paged_layout, sample  # noqa: E402

PAGE_SIZES = (64, 128, 256)
HEADS = dict(Hq=32, Hkv=8, D=128)
SHAPES = {
    "chunk512_b8_4k": dict(B=8, Sq=512, cap=4096, **HEADS),
    "chunk512_b8_16k": dict(B=8, Sq=512, cap=16384, **HEADS),
    "chunk512_b8_32k": dict(B=8, Sq=512, cap=32768, **HEADS),
    "chunk2048_b1_32k": dict(B=1, Sq=2048, cap=32768, **HEADS),
    "chunk2048_b1_128k": dict(B=1, Sq=2048, cap=131072, **HEADS),
}


def run_shape(name, s, rounds, inner, dev):
    from flash_attention_cute_amd import _debug, flash_attn_padded_func, flash_attn_paged_func
    from flash_attention_cute_amd.flash_attention import _gather_pages

    gen = torch.Generator().manual_seed(1)
    bf = torch.bfloat16
    q = torch.randn(s["B"], s["Hq"], s["Sq"], s["D"], device=dev, dtype=bf)
    k = torch.randn(s["B"], s["Hkv"], s["cap"], s["D"], device=dev, dtype=bf)
    v = torch.randn(s["B"], s["Hkv"], s["cap"], s["D"], device=dev, dtype=bf)
    lens = torch.full((s["B"],), s["cap"], dtype=torch.int32, device=dev)
    zero = torch.zeros_like(lens)
    floor = lambda: flash_attn_padded_func(q, k, v, zero, lens, causal=True)  # noqa: E731
    ref = floor()
    floor_layout = _debug.last_layout()
    torch.cuda.synchronize()

    def floor_plain():  # (c) held to the plain 256-row blocks the paged kernel runs (no head-packed blocks)
        _debug.set_head_pack(0)
        try:
            return floor()
        finally:
            _debug.set_head_pack(None)

    if not torch.equal(floor_plain(), ref) or _debug.last_layout() != "plain":
        raise AssertionError(f"{name}: the plain-block floor differs")
    rows = []
    for page in PAGE_SIZES:
        for tag, g in (("shuffled", gen), ("inorder", None)):
            kc, vc, table = paged_layout(k, v, page, g)
            inplace = lambda: flash_attn_paged_func(q, kc, vc, table, lens, causal=True)  # noqa: E731
            copying = lambda: flash_attn_padded_func(q, _gather_pages(kc, table), _gather_pages(vc, table), zero,  # noqa: E731
                                                     lens, causal=True)
            out = inplace()
            if not (_debug.last_path() == "w4" and _debug.last_prefill_paged()):
                raise AssertionError(f"{name}: page size {page} did not run the paged prefill kernel")
            old = copying()
            torch.cuda.synchronize()
            if not (torch.equal(out, ref) and torch.equal(old, ref)):
                raise AssertionError(f"{name}: page size {page} ({tag}) differs from the padded op on the dense cache")
            variants = [("c_a", floor), ("a", inplace), ("b", copying), ("c_plain", floor_plain), ("c_b", floor)]
            for _, fn in variants:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {n: [] for n, _ in variants}
            for _ in range(rounds):
                for n, fn in variants:
                    times[n].append(sample(fn, inner))
            med = {n: statistics.median(t) for n, t in times.items()}
            c = 0.5 * (med["c_a"] + med["c_b"])
            rows.append({"page_size": page, "pages": tag, "bit_equal": True,
                         "a_inplace_ms": round(med["a"], 4), "b_copying_ms": round(med["b"], 4),
                         "c_a_ms": round(med["c_a"], 4), "c_b_ms": round(med["c_b"], 4), "c_floor_ms": round(c, 4),
                         "aa_spread_pct": round(100.0 * abs(med["c_a"] - med["c_b"]) / c, 3),
                         "ratio_a_over_b": round(med["a"] / med["b"], 4),
                         "ratio_a_over_c": round(med["a"] / c, 4),
                         # the lookup alone: against the floor on the same block layout
                         "c_plain_ms": round(med["c_plain"], 4),
                         "ratio_a_over_c_plain": round(med["a"] / med["c_plain"], 4)})
            del kc, vc, table, out, old
            torch.cuda.empty_cache()
    return {"shape": name, **s, "dtype": "bf16", "causal": True, "lengths": "capacity", "floor_layout": floor_layout,
            "gather_bytes": 4 * s["B"] * s["Hkv"] * s["cap"] * s["D"] * 2, "cases": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_prefill needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    result = {"script": "scripts/bench_paged_prefill.py", "device": torch.cuda.get_device_name(dev),
              "rounds": args.rounds, "inner": args.inner,
              "method": "median over rounds of (inner calls between two device events) / inner; per round and (page "
                        "size, page order): c (padded op on the dense cache), a (in place), b (gather K, gather V, "
                        "padded op), c again; A/A spread = the two medians of c",
              "shapes": [run_shape(n, SHAPES[n], args.rounds, args.inner, dev) for n in args.shapes.split(",")]}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
