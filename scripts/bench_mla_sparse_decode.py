"""A/B of the sparse MLA decode (flash_attn_mla_decode_func(indices=)) against the dense calls a user has without it.

One process, the arms interleaved round by round, device events around each arm's calls, the sparse arm measured
twice (A and A') so its own A/A spread is known: a ratio inside twice that spread is a tie. Writes
profiles/mla_sparse_decode_ab.json.

  python scripts/bench_mla_sparse_decode.py [--rounds 7] [--calls 20] [--out profiles/mla_sparse_decode_ab.json]

Shapes (bf16, page 64, Sq 1, topk 2048): Hq 16 and 128, B 32 with lengths 4096..32768 and B 1 with 131072 keys;
a list is 2048 random distinct positions of its sequence. Arms:

  sparse      the sparse call (the plan's splits: at least 2 tiles a split); sparse_ns8 / sparse_ns32 the same
              with num_splits forced to 8 (fa_mla_decode's 8 tiles a split at topk 2048) and to 32 (2 tiles);
  dense       flash_attn_mla_decode_func on the same cache: what a user runs today, a DIFFERENT function (all keys),
              timed only;
  floor       the dense call on a cache of exactly 2048 contiguous keys per sequence: the same rows of work without
              a gather, so sparse / floor is the price of the gather;
  skip        the sparse call with every length 500 (lists of 500 positions and 1548 entries of -1 padding), and
              floor500, the dense call over 500 contiguous keys: what the tile skip leaves of a padded list.

Correctness at the timed sizes: the sparse output against a torch gather + softmax in fp32 (max_abs_diff)."""
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
PAGE, TOPK = 64, 2048


def make(batch, lens, hq, seed):
    g = torch.Generator().manual_seed(seed)
    max_pages = (max(lens) + PAGE - 1) // PAGE
    num_pages = batch * max_pages
    gd = torch.Generator(device="cuda").manual_seed(seed)  # (the pool is up to 1.2 GB: drawn on the device)
    pool = (torch.randn(num_pages, PAGE, 576, generator=gd, device="cuda") * 0.5).to(torch.bfloat16)
    table = torch.randperm(num_pages, generator=g).to(torch.int32).view(batch, max_pages).cuda()
    q = torch.randn(batch, hq, 1, 576, generator=g).to(torch.bfloat16).cuda()
    idx = torch.full((batch, 1, TOPK), -1, dtype=torch.int32)
    for b, n in enumerate(lens):
        idx[b, 0, :min(n, TOPK)] = torch.randperm(n, generator=g)[:TOPK].to(torch.int32)
    return q, pool, table, torch.tensor(lens, dtype=torch.int32).cuda(), idx.cuda()


def torch_sparse(q, pool, table, idx):
    outs = []
    for b in range(q.size(0)):
        ids = idx[b, 0][idx[b, 0] >= 0].long()
        kv = pool[table[b, ids // PAGE].long(), ids % PAGE].float()
        p = torch.softmax(torch.matmul(q[b, :, 0].float(), kv.t()) * SCALE, dim=-1)
        outs.append(torch.matmul(p, kv[:, :512])[:, None])
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mla_sparse_decode_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_sparse_decode needs the GPU: nothing is measured without one")
    from flash_attention_cute_amd import flash_attn_mla_decode_func as mla

    g = torch.Generator().manual_seed(7)
    ragged = torch.randint(4096, 32769, (32,), generator=g).tolist()
    results = []
    for name, batch, lens in (("B32_len4096-32768", 32, ragged), ("B1_len131072", 1, [131072])):
        for hq in (16, 128):
            q, pool, table, sl, idx = make(batch, lens, hq, 11)
            sl_k = torch.full_like(sl, TOPK)
            _, _, _, sl_500, idx_500 = make(batch, [500] * batch, hq, 12)  # (the big pool and its table serve)
            arms = {
                "sparse": lambda: mla(q, pool, table, sl, SCALE, indices=idx),
                "sparse_ns8": lambda: mla(q, pool, table, sl, SCALE, indices=idx, num_splits=8),
                "sparse_ns32": lambda: mla(q, pool, table, sl, SCALE, indices=idx, num_splits=32),
                "dense": lambda: mla(q, pool, table, sl, SCALE),
                "floor": lambda: mla(q, pool, table, sl_k, SCALE),
                "skip": lambda: mla(q, pool, table, sl_500, SCALE, indices=idx_500),
                "floor500": lambda: mla(q, pool, table, sl_500, SCALE),
                "sparse_again": lambda: mla(q, pool, table, sl, SCALE, indices=idx),
            }
            err = (arms["sparse"]().float() - torch_sparse(q, pool, table, idx)).abs().max().item()
            for fn in arms.values():  # warm-up: code objects, the allocator's workspace blocks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in arms}
            for _ in range(args.rounds):
                for k, fn in arms.items():
                    t[k].append(timed(fn, args.calls))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = abs(med["sparse"] - med["sparse_again"]) / min(med["sparse"], med["sparse_again"])
            sparse = 0.5 * (med["sparse"] + med["sparse_again"])
            ratios = {"dense_over_sparse": med["dense"] / sparse, "sparse_over_floor": sparse / med["floor"],
                      "ns8_over_sparse": med["sparse_ns8"] / sparse, "ns32_over_sparse": med["sparse_ns32"] / sparse,
                      "skip_over_sparse": med["skip"] / sparse,
                      "skip_over_floor500": med["skip"] / med["floor500"]}
            rec = {"shape": name, "batch": batch, "keys": sum(lens), "hq": hq, "topk": TOPK, "dtype": "bf16",
                   "page_size": PAGE, **{f"{k}_us": v for k, v in med.items()}, "aa_spread": spread, **ratios,
                   "ties": [k for k, v in ratios.items() if abs(v - 1) <= 2 * spread],
                   "gathered_TBps": batch * TOPK * 1152 / sparse * 1e-6, "max_abs_diff_vs_torch": err,
                   "sparse_us_rounds": t["sparse"]}
            results.append(rec)
            print(json.dumps(rec), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.calls,
           "method": "one process, arms interleaved round by round, device events, medians of rounds; the sparse "
                     "arm twice for the A/A spread",
           "results": results}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
