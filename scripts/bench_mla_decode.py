"""A/B of the MLA decode (flash_attn_mla_decode_func) against what a user has without it: torch gathers the pages
and computes softmax(scale q kv^T) kv[..., :512] in bf16, with none of this project's code in that arm.

One process, the arms interleaved round by round, device events around each arm's calls, the baseline measured
twice (A and A') so its own A/A spread is known: a ratio inside twice that spread is a tie. Writes
profiles/mla_decode_ab.json.

  python scripts/bench_mla_decode.py [--rounds 7] [--calls 20] [--out profiles/mla_decode_ab.json]

Shapes (bf16, page 64): Hq 128 and 16 (DeepSeek-V3 at TP1 and TP8), Sq 1 and 2, B 32 with lengths 1024..4000 and
B 1 with 131072 keys. Reported per shape: median times, the ratio, the A/A spread, the latent bytes per second
counted once per (batch, key split) -- the bytes the algorithm needs, whatever the row groups re-read through L2 --
and for Hq 128 its time over Hq 16's on the same keys.
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

SCALE = 192 ** -0.5
PAGE = 64


def make(batch, lens, hq, sq, seed):
    g = torch.Generator().manual_seed(seed)
    max_pages = (max(lens) + PAGE - 1) // PAGE
    num_pages = batch * max_pages
    pool = (torch.randn(num_pages, PAGE, 576, generator=g) * 0.5).to(torch.bfloat16).cuda()
    table = torch.randperm(num_pages, generator=g).to(torch.int32).view(batch, max_pages).cuda()
    q = torch.randn(batch, hq, sq, 576, generator=g).to(torch.bfloat16).cuda()
    return q, pool, table, torch.tensor(lens, dtype=torch.int32).cuda()


def torch_arm(q, pool, table, lens_host):
    """gather + matmul + softmax + matmul per sequence, bf16 (lengths on the host, as a serving engine has them)"""
    outs = []
    sq = q.size(2)
    for b, n in enumerate(lens_host):
        kv = pool[table[b, :(n + PAGE - 1) // PAGE].long()].flatten(0, 1)[:n]
        s = torch.matmul(q[b], kv.t()) * SCALE
        if sq > 1:
            s = s.masked_fill(torch.arange(n, device=q.device)[None, :] >
                              torch.arange(sq, device=q.device)[:, None] + n - sq, float("-inf"))
        outs.append(torch.matmul(torch.softmax(s, dim=-1, dtype=torch.float32).to(q.dtype), kv[:, :512]))
    return torch.stack(outs)


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls * 1e3  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mla_decode_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_decode needs the GPU: nothing is measured without one")
    from flash_attention_cute_amd import flash_attn_mla_decode_func

    g = torch.Generator().manual_seed(7)
    ragged = torch.randint(1024, 4001, (32,), generator=g).tolist()
    results = []
    for name, batch, lens in (("B32_len1024-4000", 32, ragged), ("B1_len131072", 1, [131072])):
        for sq in (1, 2):
            per_hq = {}
            for hq in (16, 128):
                q, pool, table, sl = make(batch, lens, hq, sq, 11)
                new = lambda: flash_attn_mla_decode_func(q, pool, table, sl, SCALE, causal=True)  # noqa: E731
                base = lambda: torch_arm(q, pool, table, lens)  # noqa: E731
                err = (new().float() - base().float()).abs().max().item()
                for fn in (new, base):  # warm-up: code objects, library algorithm choices
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                t = {"new": [], "base": [], "base2": []}
                for _ in range(args.rounds):
                    t["base"].append(timed(base, args.calls))
                    t["new"].append(timed(new, args.calls))
                    t["base2"].append(timed(base, args.calls))
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = abs(med["base"] - med["base2"]) / min(med["base"], med["base2"])
                ratio = 0.5 * (med["base"] + med["base2"]) / med["new"]
                latent_bytes = sum(lens) * 576 * 2
                flops = 2 * sum(lens) * hq * sq * (576 + 512)
                rec = {"shape": name, "batch": batch, "keys": sum(lens), "hq": hq, "sq": sq, "dtype": "bf16",
                       "page_size": PAGE, "mla_us": med["new"], "torch_us": med["base"], "torch_again_us": med["base2"],
                       "aa_spread": spread, "speedup": ratio, "tie": abs(ratio - 1) <= 2 * spread,
                       "latent_TBps": latent_bytes / med["new"] * 1e-6, "TFLOPs": flops / med["new"] * 1e-6,
                       "max_abs_diff_vs_torch": err, "mla_us_rounds": t["new"]}
                per_hq[hq] = rec
                results.append(rec)
                print(json.dumps(rec), flush=True)
            per_hq[128]["time_over_hq16"] = per_hq[128]["mla_us"] / per_hq[16]["mla_us"]
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.calls,
           "method": "one process, arms interleaved (torch, mla, torch), device events, medians of rounds",
           "results": results}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
