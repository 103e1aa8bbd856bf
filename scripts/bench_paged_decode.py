"""Same-process A/B of the paged decode against the dense padded decode on the same keys.

    timeout -k 10 600 python scripts/bench_paged_decode.py [--rounds R] [--inner N] [--out FILE.json]

For bench.py's ``decode_padded`` shape (bf16 B32 Hq32 Hkv8 D128, capacity 4096, lengths 1024..4000) and
its ``decode_long`` shape (B1, 131072 keys), and page sizes 32 / 64 / 128 / 256, the K / V of every
sequence are laid out densely ([B, Hkv, capacity, D], keys from position 0 -- the dense side is
``flash_attn_padded_func(q, K, V, 0, lens)``, the code as it was before the paged kernel) and in a page
pool (``flash_attn_paged_func``): once through a random permutation of the pages, and once with the
pages in sequence order, which separates the cost of the lookup from that of the scattered pages.

One process, one ``timeout``: every round times the dense call, each page size and order, and the dense
call AGAIN, so the run carries its own A/A spread (the two dense medians) next to every paged / dense
ratio. A sample is ``--inner`` back-to-back calls between two device events; the figure per variant is
the median over the rounds. Outputs are checked bit-equal before timing. Prints one JSON object (and
writes it to ``--out``).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PAGE_SIZES = (32, 64, 128, 256)
SHAPES = {  # bench.py CONFIGS decode_padded / decode_long
    "decode_padded": dict(B=32, Hq=32, Hkv=8, D=128, cap=4096, lens=[1024 + 96 * i for i in range(32)]),
    "decode_long": dict(B=1, Hq=32, Hkv=8, D=128, cap=131072, lens=[131072]),
}


def paged_layout(k, v, page, gen):
    """The dense [B, Hkv, cap, D] keys as a pool [B * cap / page, Hkv, page, D] under a random page
    permutation (gen None: pages in sequence order), and the table that undoes it."""
    b, hkv, cap, d = k.shape
    mp = cap // page
    perm = (torch.randperm(b * mp, generator=gen) if gen is not None else torch.arange(b * mp)).to(k.device)
    table = perm.reshape(b, mp).to(torch.int32)

    def scatter(x):
        pages = x.reshape(b, hkv, mp, page, d).transpose(1, 2).reshape(b * mp, hkv, page, d)
        pool = torch.empty_like(pages)
        pool[perm] = pages
        return pool

    return scatter(k), scatter(v), table


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def run_shape(name, s, rounds, inner, dev):
    from flash_attention_cute_amd import _debug, flash_attn_padded_func, flash_attn_paged_func

    gen = torch.Generator().manual_seed(1)
    q = torch.randn(s["B"], s["Hq"], 1, s["D"], generator=gen).to(torch.bfloat16).to(dev)
    k = torch.randn(s["B"], s["Hkv"], s["cap"], s["D"], generator=gen).to(torch.bfloat16).to(dev)
    v = torch.randn(s["B"], s["Hkv"], s["cap"], s["D"], generator=gen).to(torch.bfloat16).to(dev)
    lens = torch.tensor(s["lens"], dtype=torch.int32, device=dev)
    zero = torch.zeros_like(lens)
    dense = lambda: flash_attn_padded_func(q, k, v, zero, lens)  # noqa: E731
    ref = dense()
    dense_path = _debug.last_path()
    variants = [("dense_a", dense)]
    paths = {}
    for page in PAGE_SIZES:
        for tag, g in (("page", gen), ("inorder", None)):  # a random page permutation; pages in order
            kc, vc, table = paged_layout(k, v, page, g)
            fn = (lambda kc=kc, vc=vc, table=table: flash_attn_paged_func(q, kc, vc, table, lens))
            out = fn()
            paths[page] = _debug.last_path()
            torch.cuda.synchronize()
            if not torch.equal(out, ref):
                raise AssertionError(f"{name}: page size {page} ({tag}) differs from the dense padded decode")
            variants.append((f"{tag}{page}", fn))
    variants.append(("dense_b", dense))
    for _, fn in variants:  # warm-up: every variant, every shape of the timed window
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            times[n].append(sample(fn, inner))
    med = {n: statistics.median(t) for n, t in times.items()}
    dense_ms = 0.5 * (med["dense_a"] + med["dense_b"])
    kv_bytes = 2 * 2 * s["Hkv"] * s["D"] * sum(s["lens"])
    return {
        "shape": name, "B": s["B"], "Hq": s["Hq"], "Hkv": s["Hkv"], "D": s["D"], "capacity": s["cap"],
        "dtype": "bf16", "kv_bytes": kv_bytes, "dense_path": dense_path,
        "dense_a_ms": round(med["dense_a"], 5), "dense_b_ms": round(med["dense_b"], 5), "dense_ms": round(dense_ms, 5),
        "dense_kv_gbs": round(kv_bytes / dense_ms / 1e6, 1),
        # the run's own A/A spread: the two dense medians, same code, same data, same process
        "aa_spread_pct": round(100.0 * abs(med["dense_a"] - med["dense_b"]) / dense_ms, 3),
        "pages": [{"page_size": p, "path": paths[p], "paged_ms": round(med[f"page{p}"], 5),
                   "ratio_paged_over_dense": round(med[f"page{p}"] / dense_ms, 4),
                   "paged_kv_gbs": round(kv_bytes / med[f"page{p}"] / 1e6, 1),
                   "inorder_ms": round(med[f"inorder{p}"], 5),
                   "ratio_inorder_over_dense": round(med[f"inorder{p}"] / dense_ms, 4), "bit_equal": True}
                  for p in PAGE_SIZES],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_decode needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    result = {"script": "scripts/bench_paged_decode.py", "device": torch.cuda.get_device_name(dev),
              "rounds": args.rounds, "inner": args.inner,
              "method": "median over rounds of (inner calls between two device events) / inner; per round: dense, "
                        "page 32 / 64 / 128 / 256 (each: random page permutation, then pages in order), dense again",
              "shapes": [run_shape(n, s, args.rounds, args.inner, dev) for n, s in SHAPES.items()]}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
