"""A/B of the mixed-row sparse MLA decode and append (a torch.uint8 cache of 656-byte rows: DeepSeek-V3.2's FP8 latent
cache) against the calls on the other caches: the 16-bit sparse decode on the same positions and lists, and the e4m3
append.

One process, the arms interleaved round by round, device events around each arm's calls, the reference arm measured
twice (A and A') so its own A/A spread is known: a ratio inside twice that spread is a tie. There is no time
threshold; the script reports. Writes profiles/mla_mixed_decode_ab.json.

  python scripts/bench_mla_mixed_decode.py [--rounds 7] [--calls 20] [--out profiles/mla_mixed_decode_ab.json]

Decode shapes (bf16 q, page 64, Sq 1, topk 2048): Hq 16 and 128, B 32 with lengths 4096..32768 and B 1 with 131072
keys; a list is 2048 random distinct positions of its sequence. The mixed pool holds the bf16 pool's rows, packed by
the write formula, under the same table. Append shapes: B 32 with 1 new token (a decode step) and B 8 with 512 (a
prefill chunk), into pools of the same pages.

Correctness at the timed sizes: the mixed output against a torch gather + softmax in fp32 over the dequantised
rows (max_abs_diff)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from scripts.bench_mla_sparse_decode import PAGE, SCALE, TOPK, make, timed  # noqa: E402


def torch_sparse_mixed(q, pool8, table, idx):
    from flash_attention_cute_amd.flash_attention import unpack_mla_mixed_rows

    outs = []
    for b in range(q.size(0)):
        ids = idx[b, 0][idx[b, 0] >= 0].long()
        kv = unpack_mla_mixed_rows(pool8[table[b, ids // PAGE].long(), ids % PAGE])
        p = torch.softmax(torch.matmul(q[b, :, 0].float(), kv.t()) * SCALE, dim=-1)
        outs.append(torch.matmul(p, kv[:, :512])[:, None])
    return torch.stack(outs)


def rounds_of(arms, rounds, calls):
    for fn in arms.values():  # warm-up: code objects, the allocator's workspace blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, calls))
    return {k: statistics.median(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mla_mixed_decode_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_mixed_decode needs the GPU: nothing is measured without one")
    from flash_attention_cute_amd import flash_attn_mla_append as append, flash_attn_mla_decode_func as mla
    from flash_attention_cute_amd.flash_attention import pack_mla_mixed_rows

    g = torch.Generator().manual_seed(7)
    ragged = torch.randint(4096, 32769, (32,), generator=g).tolist()
    results = []
    for name, batch, lens in (("B32_len4096-32768", 32, ragged), ("B1_len131072", 1, [131072])):
        for hq in (16, 128):
            q, pool, table, sl, idx = make(batch, lens, hq, 11)
            pool8 = torch.cat([pack_mla_mixed_rows(c[..., :512], c[..., 512:]) for c in pool.split(256)])
            arms = {"sparse16": lambda: mla(q, pool, table, sl, SCALE, indices=idx),
                    "mixed": lambda: mla(q, pool8, table, sl, SCALE, indices=idx),
                    "sparse16_again": lambda: mla(q, pool, table, sl, SCALE, indices=idx)}
            err = (arms["mixed"]().float() - torch_sparse_mixed(q, pool8, table, idx)).abs().max().item()
            med = rounds_of(arms, args.rounds, args.calls)
            spread = abs(med["sparse16"] - med["sparse16_again"]) / min(med["sparse16"], med["sparse16_again"])
            ratio = med["mixed"] / (0.5 * (med["sparse16"] + med["sparse16_again"]))
            rec = {"what": "decode", "shape": name, "batch": batch, "keys": sum(lens), "hq": hq, "topk": TOPK,
                   "page_size": PAGE, **{f"{k}_us": v for k, v in med.items()}, "aa_spread": spread,
                   "mixed_over_sparse16": ratio, "tie": abs(ratio - 1) <= 2 * spread,
                   "gathered_TBps": batch * TOPK * 656 / med["mixed"] * 1e-6, "max_abs_diff_vs_torch": err}
            results.append(rec)
            print(json.dumps(rec), flush=True)
            del pool, pool8
    for batch, sn in ((32, 1), (8, 512)):
        max_pages = 16
        gd = torch.Generator(device="cuda").manual_seed(3)
        c_kv = torch.randn(batch, sn, 512, generator=gd, device="cuda").to(torch.bfloat16)
        k_pe = torch.randn(batch, sn, 64, generator=gd, device="cuda").to(torch.bfloat16)
        table = torch.randperm(batch * max_pages).to(torch.int32).view(batch, max_pages).cuda()
        sl = torch.full((batch,), 100, dtype=torch.int32, device="cuda")
        p8 = torch.zeros(batch * max_pages, PAGE, 576, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn)
        pm = torch.zeros(batch * max_pages, PAGE, 656, dtype=torch.uint8, device="cuda")
        ds = torch.full((batch,), 0.05, device="cuda")
        arms = {"e4m3": lambda: append(p8, c_kv, k_pe, sl, table, ds), "mixed": lambda: append(pm, c_kv, k_pe, sl, table),
                "e4m3_again": lambda: append(p8, c_kv, k_pe, sl, table, ds)}
        med = rounds_of(arms, args.rounds, args.calls)
        spread = abs(med["e4m3"] - med["e4m3_again"]) / min(med["e4m3"], med["e4m3_again"])
        ratio = med["mixed"] / (0.5 * (med["e4m3"] + med["e4m3_again"]))
        rec = {"what": "append", "batch": batch, "seqlen_new": sn, **{f"{k}_us": v for k, v in med.items()},
               "aa_spread": spread, "mixed_over_e4m3": ratio, "tie": abs(ratio - 1) <= 2 * spread}
        results.append(rec)
        print(json.dumps(rec), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.calls,
           "method": "one process, arms interleaved round by round, device events, medians of rounds; the reference "
                     "arm (16-bit sparse decode, e4m3 append) twice for the A/A spread",
           "results": results}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
