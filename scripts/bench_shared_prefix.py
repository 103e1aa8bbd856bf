"""Same-process A/B of the shared-prefix decode step against the plain paged decode on the same tables.

    timeout -k 10 900 python scripts/bench_shared_prefix.py [--rounds R] [--inner N] [--out FILE.json]

Shapes: bf16 q, Hq 32 / Hkv 8 / D 128, page size 64, shuffled pages, on a 16-bit pool and on an FP8 (e4m3) pool;
B 8 and 32 sequences that share a prefix of 2048 / 8192 / 32768 keys (the SAME physical pages in every table row)
and hold 128..1024 keys of their own. Arms:

  (a32) ``flash_attn_paged_shared_prefix_func`` with prefix-phase groups of 32 (q-head, sequence) rows (c = 32 / g)
  (a64) the same with groups of 64 rows (c = 64 / g): two row blocks per (group, kv-head)
  (b)   ``flash_attn_paged_func`` on the same tables
  (b')  (b) again: the run's own A/A spread
  (c)   the LSE variant of the decode alone (``return_lse=True``) on (b)'s call: c / b is the cost of the LSE store

Every round times a32, a64, b, b', c in that order; a sample is ``--inner`` back-to-back calls between two device
events, ending in a synchronise; the figure per arm is the median over the rounds. Recorded per shape: a32 / b,
a64 / b, c / b, the spread |b - b'| / mean, and beside each a / b the byte ratio ((B / c) P + sum suffix) /
sum (P + suffix) -- what a / b would be if time were bytes. (a) is checked against (b) before timing (twice the
bf16 parity bound), and (c)'s output against (b)'s bit for bit.

Measured (profiles/shared_prefix_ab.json; DESIGN.md section 5 has the table): an eager shared-prefix step costs
0.037-0.040 ms whatever it reads (three launches), so (a) LOSES to (b) for short prefixes and wins for long ones. The
crossover: B 32 wins from prefix 8192 on (a / b 0.64 bf16, 0.58 FP8; 0.32 / 0.26 at 32768) and loses at 2048 (1.21 /
1.37); B 8 wins at 32768 (0.45 / 0.67), ties at 8192 on bf16 (1.04), loses there on FP8 (1.53) and at 2048 (2.0 /
2.3). Groups of 32 rows are the rule: groups of 64 were 4-10 % slower at B 32 on bf16 and tied elsewhere.

Prints one JSON object (and writes it to ``--out``, by default profiles/shared_prefix_ab.json; the file's
"lse_error" and "gates" entries, recorded from the test suite and the regression scripts, are kept).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
HQ, HKV, D, PAGE = 32, 8, 128, 64
BATCHES, PREFIXES = (8, 32), (2048, 8192, 32768)


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


def shared_cache(b, prefix, suffixes, fp8, gen, dev):
    """A pool of random keys under a random page permutation: prefix / PAGE pages that every table row starts
    with, then each sequence's own pages."""
    n_pre, n_suf = prefix // PAGE, (max(suffixes) + PAGE - 1) // PAGE
    n = n_pre + b * n_suf
    pool = lambda: torch.randn(n, HKV, PAGE, D, generator=gen, device=dev, dtype=BF16)  # noqa: E731
    kc, vc = pool(), pool()
    if fp8:
        kc, vc = kc.to(FP8), vc.to(FP8)
    ids = torch.randperm(n, generator=gen, device=dev).to(torch.int32)
    table = torch.cat([ids[:n_pre].expand(b, n_pre), ids[n_pre:].reshape(b, n_suf)], dim=1).contiguous()
    sl = torch.tensor([prefix + s for s in suffixes], dtype=torch.int32, device=dev)
    return kc, vc, table, sl


def byte_ratio(b, c, prefix, suffixes):
    groups = (b + c - 1) // c
    return (groups * prefix + sum(suffixes)) / sum(prefix + s for s in suffixes)


def run_shape(b, prefix, fp8, rounds, inner, dev):
    from flash_attention_cute_amd import flash_attn_paged_func, flash_attn_paged_shared_prefix_func

    gen = torch.Generator(device=dev).manual_seed(1)
    suffixes = [128 + (896 * i) // max(b - 1, 1) for i in range(b)]
    q = torch.randn(b, HQ, 1, D, generator=gen, device=dev, dtype=BF16)
    kc, vc, table, sl = shared_cache(b, prefix, suffixes, fp8, gen, dev)
    ds = {}
    if fp8:
        ds = dict(k_descale=torch.full((b, HKV), 0.5, device=dev), v_descale=torch.full((b, HKV), 2.0, device=dev))
    g = HQ // HKV
    a32 = lambda: flash_attn_paged_shared_prefix_func(q, kc, vc, table, sl, prefix, _group_rows=32, **ds)  # noqa: E731
    a64 = lambda: flash_attn_paged_shared_prefix_func(q, kc, vc, table, sl, prefix, _group_rows=64, **ds)  # noqa: E731
    pb = lambda: flash_attn_paged_func(q, kc, vc, table, sl, **ds)  # noqa: E731
    pc = lambda: flash_attn_paged_func(q, kc, vc, table, sl, return_lse=True, **ds)  # noqa: E731
    ref = pb().float()
    bound = 2.0 * (1.6e-2 + 1.6e-2 * ref.abs())
    errs = {}
    for name, fn in (("a32", a32), ("a64", a64)):
        err = (fn().float() - ref).abs()
        errs[name] = err.max().item()
        if not bool((err <= bound).all()):
            raise AssertionError(f"B{b} P{prefix}: {name} differs from the paged decode by {errs[name]}")
    if not torch.equal(pc()[0].float(), ref):
        raise AssertionError(f"B{b} P{prefix}: the LSE variant's output differs from the paged decode's")
    med = timed([("a32", a32), ("a64", a64), ("b", pb), ("b2", pb), ("c", pc)], rounds, inner)
    b_ms = 0.5 * (med["b"] + med["b2"])
    return {"cache": "fp8" if fp8 else "bf16", "B": b, "prefix": prefix, "suffix_min": min(suffixes),
            "suffix_max": max(suffixes), "Hq": HQ, "Hkv": HKV, "D": D, "page_size": PAGE,
            "max_abs_a32_minus_b": errs["a32"], "max_abs_a64_minus_b": errs["a64"],
            "a32_ms": round(med["a32"], 5), "a64_ms": round(med["a64"], 5), "b_ms": round(med["b"], 5),
            "b2_ms": round(med["b2"], 5), "c_lse_ms": round(med["c"], 5),
            "ratio_a32_over_b": round(med["a32"] / b_ms, 4), "byte_ratio_32": round(byte_ratio(b, 32 // g, prefix, suffixes), 4),
            "ratio_a64_over_b": round(med["a64"] / b_ms, 4), "byte_ratio_64": round(byte_ratio(b, 64 // g, prefix, suffixes), 4),
            "ratio_c_over_b": round(med["c"] / b_ms, 4),
            "aa_spread_pct": round(100.0 * abs(med["b"] - med["b2"]) / b_ms, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shared_prefix_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shared_prefix needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    result = {"script": "scripts/bench_shared_prefix.py", "device": torch.cuda.get_device_name(dev),
              "rounds": args.rounds, "inner": args.inner,
              "method": "median over rounds of (inner calls between two device events) / inner; per round: a32, a64 "
                        "(shared-prefix step, groups of 32 / 64 rows), b (flash_attn_paged_func), b again, c (b with "
                        "return_lse=True)",
              "shared_prefix": [run_shape(b, p, fp8, args.rounds, args.inner, dev)
                                for fp8 in (False, True) for b in BATCHES for p in PREFIXES]}
    if args.out and Path(args.out).exists():  # keep what the other tools recorded in the same file
        try:
            old = json.loads(Path(args.out).read_text())
            result.update({k: v for k, v in old.items() if k in ("lse_error", "gates")})
        except ValueError:
            pass
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
