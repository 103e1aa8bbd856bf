"""A/B of the FP8 (e4m3) latent cache of the MLA decode against the 16-bit MLA decode on the same keys, and of the
append + decode step (flash_attn_mla_with_kvcache) against index_put_ of a torch-quantised row plus the decode.

One process, the arms interleaved round by round, device events around each arm's calls, the 16-bit arm measured
twice (A and A') so its own A/A spread is known: a ratio inside twice that spread is a tie. Writes
profiles/mla_fp8_decode_ab.json.

  python scripts/bench_mla_fp8_decode.py [--rounds 7] [--calls 20] [--out profiles/mla_fp8_decode_ab.json]

Shapes (bf16 q, page 64) as scripts/bench_mla_decode.py: Hq 16 and 128, Sq 1 and 2, B 32 with lengths 1024..4000
and B 1 with 131072 keys. The FP8 pool holds the 16-bit pool's rows quantised with one descale per sequence, so the
two arms attend over the same keys up to the quantisation.
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
    from flash_attention_cute_amd.flash_attention import quantize_e4m3

    g = torch.Generator().manual_seed(seed)
    max_pages = (max(lens) + 2 * sq + PAGE - 1) // PAGE  # (room for the step's append)
    num_pages = batch * max_pages
    pool = (torch.randn(num_pages, PAGE, 576, generator=g) * 0.5).to(torch.bfloat16).cuda()
    table = torch.randperm(num_pages, generator=g).to(torch.int32).view(batch, max_pages).cuda()
    ds = torch.full((batch,), 0.011, dtype=torch.float32).cuda()
    pool8 = quantize_e4m3(pool, 0.011)
    q = torch.randn(batch, hq, sq, 576, generator=g).to(torch.bfloat16).cuda()
    c_kv = (torch.randn(batch, sq, 512, generator=g) * 0.5).to(torch.bfloat16).cuda()
    k_pe = (torch.randn(batch, sq, 64, generator=g) * 0.5).to(torch.bfloat16).cuda()
    return q, pool, pool8, table, torch.tensor(lens, dtype=torch.int32).cuda(), ds, c_kv, k_pe


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls * 1e3  # microseconds per call


def ab(base, new, rounds, calls):
    for fn in (new, base):  # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {"new": [], "base": [], "base2": []}
    for _ in range(rounds):
        t["base"].append(timed(base, calls))
        t["new"].append(timed(new, calls))
        t["base2"].append(timed(base, calls))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = abs(med["base"] - med["base2"]) / min(med["base"], med["base2"])
    ratio = med["new"] / (0.5 * (med["base"] + med["base2"]))  # time of the new arm over the base arm's
    return med, spread, ratio, t["new"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mla_fp8_decode_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_fp8_decode needs the GPU: nothing is measured without one")
    from flash_attention_cute_amd import flash_attn_mla_decode_func, flash_attn_mla_with_kvcache
    from flash_attention_cute_amd.flash_attention import quantize_e4m3

    g = torch.Generator().manual_seed(7)
    ragged = torch.randint(1024, 4001, (32,), generator=g).tolist()
    results = []
    for name, batch, lens in (("B32_len1024-4000", 32, ragged), ("B1_len131072", 1, [131072])):
        for sq in (1, 2):
            for hq in (16, 128):
                q, pool, pool8, table, sl, ds, c_kv, k_pe = make(batch, lens, hq, sq, 11)
                f16 = lambda: flash_attn_mla_decode_func(q, pool, table, sl, SCALE)  # noqa: E731
                f8 = lambda: flash_attn_mla_decode_func(q, pool8, table, sl, SCALE, kv_descale=ds)  # noqa: E731
                err = (f8().float() - f16().float()).abs().max().item()
                med, spread, ratio, rounds = ab(f16, f8, args.rounds, args.calls)
                rec = {"what": "decode", "shape": name, "batch": batch, "keys": sum(lens), "hq": hq, "sq": sq,
                       "q_dtype": "bf16", "page_size": PAGE, "fp8_us": med["new"], "bf16_us": med["base"],
                       "bf16_again_us": med["base2"], "aa_spread": spread, "fp8_time_over_bf16": ratio,
                       "tie": abs(ratio - 1) <= 2 * spread, "fp8_latent_TBps": sum(lens) * 576 / med["new"] * 1e-6,
                       "max_abs_diff_vs_bf16": err, "fp8_us_rounds": rounds}
                results.append(rec)
                print(json.dumps(rec), flush=True)

                # the serving step: append Sq rows, decode over the advanced lengths. Base arm: the rows quantised
                # by torch and scattered with index_put_ (page and row indices precomputed, as an engine has its
                # slot mapping), then the same FP8 decode.
                pos = sl.long()[:, None] + torch.arange(sq, device="cuda")[None]
                pages, rows = table.long().gather(1, pos // PAGE), pos % PAGE
                new_sl, bytes8 = sl + sq, pool8.view(torch.uint8)

                def torch_step():
                    row8 = quantize_e4m3(torch.cat([c_kv, k_pe], -1), ds[:, None, None])
                    bytes8.index_put_((pages, rows), row8.view(torch.uint8))
                    return flash_attn_mla_decode_func(q, pool8, table, new_sl, SCALE, kv_descale=ds)

                fused = lambda: flash_attn_mla_with_kvcache(q, pool8, c_kv, k_pe, sl, table, SCALE,  # noqa: E731
                                                            kv_descale=ds)
                err = (fused().float() - torch_step().float()).abs().max().item()
                med, spread, ratio, rounds = ab(torch_step, fused, args.rounds, args.calls)
                rec = {"what": "append+decode", "shape": name, "batch": batch, "keys": sum(lens), "hq": hq, "sq": sq,
                       "step_us": med["new"], "index_put_us": med["base"], "index_put_again_us": med["base2"],
                       "aa_spread": spread, "step_time_over_index_put": ratio, "tie": abs(ratio - 1) <= 2 * spread,
                       "max_abs_diff": err, "step_us_rounds": rounds}
                results.append(rec)
                print(json.dumps(rec), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.calls,
           "method": "one process, arms interleaved (base, new, base), device events, medians of rounds; ratios are "
                     "the new arm's time over the base arm's (below 1: the new arm is faster)",
           "results": results}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
