"""Same-process A/B of (1) the ragged paged prefill that also writes the LSE against the launches without it, and
(2) the ragged shared-prefix step against the one-launch ragged call on the same tables.

    timeout -k 10 900 python scripts/bench_paged_varlen_shared_prefix.py [--rounds R] [--inner N] [--only lse|prefix]

1. "lse" -> profiles/paged_varlen_lse_ab.json. The shapes and buffers of scripts/bench_paged_varlen_sink.py (8
   sequences, chunks of 128..2048 positions over 4k..32k keys, causal, bf16, page 64; gpt-oss heads without a window
   and with ``window_left`` 127, Llama-3-8B heads). Per round, through the public wrapper on the same buffers:
     (l)  return_lse=True, no sinks   (u)  the unsinked op   (u') (u) again: the A/A spread
     (ls) return_lse=True with sinks  (s)  the sinked op     (s') (s) again
   Recorded: l / u and ls / s, the baseline arm's spread, and whether the ratio lies within twice that spread. Before
   timing, ``out`` of the LSE launches is checked bit-equal to the launches without it.

2. "prefix" -> profiles/paged_varlen_shared_prefix_ab.json. Hq 32 / Hkv 8 / D 128, bf16, page 64; B sequences of S
   new positions each behind a shared prefix of P keys, suffix lengths spread over 128..1024 (at least S):
     (p)  flash_attn_paged_varlen_shared_prefix_func, one group   (o)  flash_attn_paged_varlen_func   (o') (o) again
   for B 32 x S 8 and B 8 x S 64 over P 2048 / 8192 / 32768, and B 8 x S 1024 over P 8192 (blocks already full: no
   gain expected). The two results are checked against each other within the 16-bit tolerance before timing.

A sample is ``--inner`` back-to-back calls between two device events; the figure per arm is the median over the
rounds. The comparison of this tree's other ragged launches with the parent commit's library is
scripts/bench_paged_varlen_sink.py's ``--parent-lib`` section, unchanged.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_paged_varlen_sink import BF16, CASES, CHUNKS, PAGE, buffers, timed  # noqa: E402


def ratio(med, arm, base, base2):
    b = 0.5 * (med[base] + med[base2])
    spread = abs(med[base] - med[base2]) / b
    r = med[arm] / b
    return {f"{arm}_ms": med[arm], f"{base}_ms": b, "ratio": r, "aa_spread": spread,
            "within_twice_the_spread": abs(r - 1) <= 2 * spread, "difference_us_per_call": 1e3 * (med[arm] - b)}


def lse_case(name, h, w, rounds, inner, dev):
    from flash_attention_cute_amd import flash_attn_paged_varlen_func as fn

    q, kc, vc, cu, table, sl, sinks = buffers(h, dev)
    kw = dict(causal=True, window_left=w)
    arms = {"l": lambda: fn(q, kc, vc, cu, max(CHUNKS), table, sl, return_lse=True, **kw),
            "u": lambda: fn(q, kc, vc, cu, max(CHUNKS), table, sl, **kw),
            "ls": lambda: fn(q, kc, vc, cu, max(CHUNKS), table, sl, sinks=sinks, return_lse=True, **kw),
            "s": lambda: fn(q, kc, vc, cu, max(CHUNKS), table, sl, sinks=sinks, **kw)}
    (ol, ll), ou, (ols, lls), os_ = arms["l"](), arms["u"](), arms["ls"](), arms["s"]()
    torch.cuda.synchronize()
    if not (torch.equal(ol, ou) and torch.equal(ols, os_)):
        raise AssertionError(f"{name}: out of the LSE launch differs from the launch without it")
    if not (torch.isfinite(ll).all() and torch.isfinite(lls).all() and (lls >= ll).all()):
        raise AssertionError(f"{name}: the LSE is not finite, or the sink lowered it")
    med = timed([("l", arms["l"]), ("u", arms["u"]), ("u2", arms["u"]), ("ls", arms["ls"]), ("s", arms["s"]),
                 ("s2", arms["s"])], rounds, inner)
    return {"case": name, **h, "window_left": w, "unsinked": ratio(med, "l", "u", "u2"),
            "sinked": ratio(med, "ls", "s", "s2")}


def prefix_case(b, s, p, rounds, inner, dev):
    from flash_attention_cute_amd import flash_attn_paged_varlen_func as one
    from flash_attention_cute_amd import flash_attn_paged_varlen_shared_prefix_func as shared

    hq, hkv, d = 32, 8, 128
    gen = torch.Generator(device=dev).manual_seed(2)
    suffix = [max(s, 128 + (896 * i // max(b - 1, 1)) // PAGE * PAGE) for i in range(b)]
    n_pre, n_suf = p // PAGE, [(x + PAGE - 1) // PAGE for x in suffix]
    n = n_pre + sum(n_suf)
    q = torch.randn(b * s, hq, d, generator=gen, device=dev, dtype=BF16)
    kc = torch.randn(n, hkv, PAGE, d, generator=gen, device=dev, dtype=BF16)
    vc = torch.randn(n, hkv, PAGE, d, generator=gen, device=dev, dtype=BF16)
    ids = torch.randperm(n, generator=gen, device=dev).to(torch.int32)
    table = torch.zeros((b, n_pre + max(n_suf)), dtype=torch.int32, device=dev)
    table[:, :n_pre] = ids[:n_pre]
    at = n_pre
    for i, k in enumerate(n_suf):
        table[i, n_pre:n_pre + k] = ids[at:at + k]
        at += k
    cu = torch.arange(b + 1, dtype=torch.int32, device=dev) * s
    sl = torch.tensor([p + x for x in suffix], dtype=torch.int32, device=dev)
    f_p = lambda: shared(q, kc, vc, cu, s, table, sl, p, None, causal=True)  # noqa: E731
    f_o = lambda: one(q, kc, vc, cu, s, table, sl, causal=True)  # noqa: E731
    a, o = f_p(), f_o()
    torch.cuda.synchronize()
    worst = (a.float() - o.float()).abs().max().item()
    if not worst <= 1.6e-2:
        raise AssertionError(f"B{b} S{s} P{p}: the shared-prefix step differs from the one-launch call by {worst}")
    med = timed([("p", f_p), ("o", f_o), ("o2", f_o)], rounds, inner)
    return {"B": b, "S": s, "P": p, "suffix_min": min(suffix), "suffix_max": max(suffix), "max_abs_diff": worst,
            **ratio(med, "p", "o", "o2")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--only", choices=("lse", "prefix"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    meta = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner}
    if args.only != "prefix":
        res = {**meta, "cases": [lse_case(n, h, w, args.rounds, args.inner, dev) for n, h, w in CASES]}
        (ROOT / "profiles" / "paged_varlen_lse_ab.json").write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
    if args.only != "lse":
        shapes = [(b, s, p) for b, s in ((32, 8), (8, 64)) for p in (2048, 8192, 32768)] + [(8, 1024, 8192)]
        res = {**meta, "Hq": 32, "Hkv": 8, "D": 128, "dtype": "bf16", "page_size": PAGE,
               "cases": [prefix_case(b, s, p, args.rounds, args.inner, dev) for b, s, p in shapes]}
        (ROOT / "profiles" / "paged_varlen_shared_prefix_ab.json").write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))


if __name__ == "__main__":
    main()
