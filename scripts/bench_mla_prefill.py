"""A/B of the MLA prefill attention (flash_attn_mla_prefill_func, 192 key / 128 value columns) against what a user has
without it, and against this project's own D 128 kernel as a yardstick for the MFMA rate.

One process, the arms interleaved round by round, device events around each arm's calls (as many as fill about a
third of a second), the new arm measured twice (A and A') so its own A/A spread is known: a ratio inside twice that
spread is a tie. Writes profiles/mla_prefill_ab.json.

  python scripts/bench_mla_prefill.py [--rounds 5] [--out profiles/mla_prefill_ab.json]

Arms:
  mla    flash_attn_mla_prefill_func;
  sdpa   torch.nn.functional.scaled_dot_product_attention per sequence at D 192 with v zero-padded to 192 (the pad is
         made once, outside the timing: only the quarter more P.V work is charged);
  d128   flash_attn_varlen_func of this project on the same lengths at D 128: 0.8 of the FLOPs;
  cat    (one shape) torch.cat of k_nope and the expanded k_pe, then the call, against k_pe= read in place.
TFLOP/s are counted from the shapes: 2 (Dqk + Dv) per visible (query, key) pair and head.
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
BF16 = torch.bfloat16


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls * 1e3  # microseconds per call


def calls_for(fn, budget_us=3.3e5):
    for _ in range(2):  # warm-up: code objects, library algorithm choices
        fn()
    torch.cuda.synchronize()
    return max(1, min(200, int(budget_us / timed(fn, 1))))


def pairs(sq, sk, causal):
    """visible (query, key) pairs of one sequence, bottom-right causal"""
    return sum(max(0, min(sk, m + sk - sq + 1)) for m in range(sq)) if causal else sq * sk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mla_prefill_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_prefill needs the GPU: nothing is measured without one")
    from flash_attention_cute_amd import flash_attn_mla_prefill_func, flash_attn_varlen_func

    sdpa = torch.nn.functional.scaled_dot_product_attention
    shapes = [(f"causal_B{b}_S{s}_H{h}", b, s, s, h, True) for h in (16, 128) for b in (1, 4) for s in (4096, 8192)]
    shapes += [(f"context_Sq2048_Sk32768_H{h}", 1, 2048, 32768, h, False) for h in (16, 128)]
    results = []
    for name, b, sq, sk, h, causal in shapes:
        g = torch.Generator().manual_seed(5)
        q = (torch.randn(b * sq, h, 192, generator=g) * 0.5).to(BF16).cuda()
        k = (torch.randn(b * sk, h, 192, generator=g) * 0.5).to(BF16).cuda()
        v = (torch.randn(b * sk, h, 128, generator=g) * 0.5).to(BF16).cuda()
        cq = torch.arange(b + 1, dtype=torch.int32, device="cuda") * sq
        ck = torch.arange(b + 1, dtype=torch.int32, device="cuda") * sk
        v192 = torch.nn.functional.pad(v, (0, 64))
        q128, k128 = q[..., :128].contiguous(), k[..., :128].contiguous()

        def mla():
            return flash_attn_mla_prefill_func(q, k, v, cq, ck, sq, sk, SCALE, causal=causal)

        def base():
            return [sdpa(q[i * sq:(i + 1) * sq].transpose(0, 1), k[i * sk:(i + 1) * sk].transpose(0, 1),
                         v192[i * sk:(i + 1) * sk].transpose(0, 1), is_causal=causal, scale=SCALE)
                    for i in range(b)]

        def d128():
            return flash_attn_varlen_func(q128, k128, v, cq, ck, sq, sk, SCALE, causal=causal)

        err = (mla()[:sq].float() - base()[0].transpose(0, 1)[..., :128].float()).abs().max().item()
        arms = {"mla": mla, "sdpa": base, "d128": d128}
        calls = {n: calls_for(fn) for n, fn in arms.items()}
        t = {"mla": [], "sdpa": [], "d128": [], "mla2": []}
        for _ in range(args.rounds):
            t["mla"].append(timed(mla, calls["mla"]))
            t["sdpa"].append(timed(base, calls["sdpa"]))
            t["d128"].append(timed(d128, calls["d128"]))
            t["mla2"].append(timed(mla, calls["mla"]))
        med = {n: statistics.median(x) for n, x in t.items()}
        spread = abs(med["mla"] - med["mla2"]) / min(med["mla"], med["mla2"])
        new = 0.5 * (med["mla"] + med["mla2"])
        n_pairs = b * h * pairs(sq, sk, causal)
        rec = {"shape": name, "batch": b, "sq": sq, "sk": sk, "heads": h, "causal": causal, "dtype": "bf16",
               "mla_us": med["mla"], "mla_again_us": med["mla2"], "aa_spread": spread, "sdpa_pad192_us": med["sdpa"],
               "d128_us": med["d128"], "calls": calls, "speedup_vs_sdpa": med["sdpa"] / new,
               "tie_vs_sdpa": abs(med["sdpa"] / new - 1) <= 2 * spread, "time_over_d128": new / med["d128"],
               "mla_TFLOPs": n_pairs * 2 * (192 + 128) / new * 1e-6,
               "d128_TFLOPs": n_pairs * 2 * (128 + 128) / med["d128"] * 1e-6,
               "sdpa_TFLOPs_useful": n_pairs * 2 * (192 + 128) / med["sdpa"] * 1e-6, "max_abs_diff_vs_sdpa": err}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        if name == "causal_B1_S4096_H128":  # the split key: k_pe= in place against the copy that only feeds a kernel
            k_nope, k_pe = k128, k[:, :1, 128:].contiguous()

            def split():
                return flash_attn_mla_prefill_func(q, k_nope, v, cq, ck, sq, sk, SCALE, causal=causal, k_pe=k_pe)

            def cat():
                return flash_attn_mla_prefill_func(q, torch.cat([k_nope, k_pe.expand(-1, h, -1)], -1), v, cq, ck, sq, sk,
                                                   SCALE, causal=causal)

            n = {"split": calls_for(split), "cat": calls_for(cat)}
            ts = {"split": [], "cat": [], "split2": []}
            for _ in range(args.rounds):
                ts["split"].append(timed(split, n["split"]))
                ts["cat"].append(timed(cat, n["cat"]))
                ts["split2"].append(timed(split, n["split"]))
            m = {x: statistics.median(y) for x, y in ts.items()}
            sp = abs(m["split"] - m["split2"]) / min(m["split"], m["split2"])
            ratio = m["cat"] / (0.5 * (m["split"] + m["split2"]))
            rec = {"shape": name + "_k_pe", "k_pe_us": m["split"], "k_pe_again_us": m["split2"], "aa_spread": sp,
                   "cat_then_call_us": m["cat"], "speedup_vs_cat": ratio, "tie": abs(ratio - 1) <= 2 * sp,
                   "bit_equal": bool(torch.equal(split(), cat()))}
            results.append(rec)
            print(json.dumps(rec), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "method": "one process, arms interleaved (mla, sdpa, d128, mla), device events around calls that fill about a "
                     "third of a second, medians of rounds; a ratio within twice aa_spread is a tie",
           "results": results}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
