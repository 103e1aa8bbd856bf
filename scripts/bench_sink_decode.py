"""Same-process A/B of the paged decode with attention sinks against the paged decode without them.

    timeout -k 10 900 python scripts/bench_sink_decode.py [--rounds R] [--inner N] [--out FILE.json]

Arms (``flash_attn_paged_func``; bf16 q, page size 64, shuffled pages), on a 16-bit pool and on an FP8 (e4m3) pool,
without a window and with ``window_left`` 127, for the gpt-oss head shape (Hq 64 / Hkv 8 / D 64) at B 32 with
lengths 1024..4000 and at B 1 with 131072 keys, and for the Llama head shape (Hq 32 / Hkv 8 / D 128) at B 32:

  (s)  the decode with sinks (2 randn(Hq))
  (u)  the decode without sinks, same buffers
  (u') (u) again: the run's own A/A spread

Every round times s, u, u' in that order; a sample is ``--inner`` back-to-back calls between two device events,
ending in a synchronise; the figure per arm is the median over the rounds. Recorded per case: s / u (u = the mean
of its two medians), the spread |u - u'| / mean and whether |s / u - 1| <= 2 x that spread. Before timing, the
sinked launch with sinks of -inf is checked bit-equal to (u), and (s) against the LSE identity
``u * sigmoid(lse - sinks)`` where the LSE exists (no window).

The sink adds one scalar-sized load and two exp2 per row outside the key loop, so the expectation under test is a
ratio inside twice the A/A spread. Both arms go through the public wrapper: (u) takes the q-head pack of a decode
step where there is no window, (s) never does (the same kernel rows), and (s) converts and checks one more argument
on the host.

Prints one JSON object and writes it to ``--out`` (default profiles/sink_decode_ab.json; entries of that file that
this script does not produce, such as the "code_shape" entry of scripts/compare_decode_objs.py, are kept).
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
PAGE, W = 64, 127
GPT_OSS, LLAMA = dict(Hq=64, Hkv=8, D=64), dict(Hq=32, Hkv=8, D=128)
CASES = [
    ("gpt_oss_b32_1k_4k", GPT_OSS, dict(B=32, cap=4096, lens=[1024 + 96 * i for i in range(32)])),
    ("gpt_oss_b1_128k", GPT_OSS, dict(B=1, cap=131072, lens=[131072])),
    ("llama_b32_1k_4k", LLAMA, dict(B=32, cap=4096, lens=[1024 + 96 * i for i in range(32)])),
]


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


def run_case(name, h, s, fp8, window_left, rounds, inner, dev):
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    gen = torch.Generator(device=dev).manual_seed(1)
    hq, hkv, d, b = h["Hq"], h["Hkv"], h["D"], s["B"]
    n = b * s["cap"] // PAGE
    q = torch.randn(b, hq, 1, d, generator=gen, device=dev, dtype=BF16)
    kc = torch.randn(n, hkv, PAGE, d, generator=gen, device=dev, dtype=BF16)
    vc = torch.randn(n, hkv, PAGE, d, generator=gen, device=dev, dtype=BF16)
    ds = {}
    if fp8:
        kc, vc = kc.to(FP8), vc.to(FP8)
        ds = dict(k_descale=torch.full((b, hkv), 0.5, device=dev), v_descale=torch.full((b, hkv), 2.0, device=dev))
    table = torch.randperm(n, generator=gen, device=dev).reshape(b, s["cap"] // PAGE).to(torch.int32)
    sl = torch.tensor(s["lens"], dtype=torch.int32, device=dev)
    sinks = 2 * torch.randn(hq, generator=gen, device=dev)
    kw = dict(window_left=window_left, **ds)
    sinked = lambda: flash_attn_paged_func(q, kc, vc, table, sl, sinks=sinks, **kw)  # noqa: E731
    plain = lambda: flash_attn_paged_func(q, kc, vc, table, sl, **kw)  # noqa: E731
    out_s = sinked()
    path_s = _debug.last_path()
    out_u = plain()
    path_u = _debug.last_path()
    none = flash_attn_paged_func(q, kc, vc, table, sl, sinks=torch.full_like(sinks, float("-inf")), **kw)
    torch.cuda.synchronize()
    if not torch.equal(none, out_u):
        raise AssertionError(f"{name}: sinks of -inf do not give the bits of the call without sinks")
    err = None
    if window_left < 0:
        _, lse = flash_attn_paged_func(q, kc, vc, table, sl, return_lse=True, **ds)
        ident = out_u.float() * torch.sigmoid(lse - sinks[None, :, None])[..., None]
        err = (out_s.float() - ident).abs().max().item()
        if not err <= 1.6e-2 * (1 + ident.abs().max().item()):
            raise AssertionError(f"{name}: the sinked decode differs from u * sigmoid(lse - sinks) by {err}")
    med = timed([("s", sinked), ("u", plain), ("u2", plain)], rounds, inner)
    u_ms = 0.5 * (med["u"] + med["u2"])
    spread = 100.0 * abs(med["u"] - med["u2"]) / u_ms
    ratio = med["s"] / u_ms
    return {"case": name, "cache": "fp8" if fp8 else "bf16", "window_left": window_left, "B": b, "Hq": hq, "Hkv": hkv,
            "D": d, "page_size": PAGE, "lens_min": min(s["lens"]), "lens_max": max(s["lens"]),
            "paths": {"s": path_s, "u": path_u}, "max_abs_s_minus_lse_identity": err,
            "s_sinked_ms": round(med["s"], 5), "u_unsinked_ms": round(med["u"], 5), "u2_unsinked_ms": round(med["u2"], 5),
            "ratio_s_over_u": round(ratio, 4), "aa_spread_pct": round(spread, 3),
            "within_twice_the_spread": abs(ratio - 1.0) * 100.0 <= 2.0 * spread}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sink_decode_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sink_decode needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    result = {"script": "scripts/bench_sink_decode.py", "device": torch.cuda.get_device_name(dev),
              "rounds": args.rounds, "inner": args.inner,
              "method": "median over rounds of (inner calls between two device events) / inner; per round: s (with "
                        "sinks), u (without), u again; ratio = s / mean(u, u')",
              "sink": [run_case(n, h, s, fp8, w, args.rounds, args.inner, dev)
                       for n, h, s in CASES for fp8 in (False, True) for w in (-1, W)]}
    print(json.dumps(result, indent=1), flush=True)
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        doc = json.loads(out.read_text()) if out.exists() else {}
        doc.update(result)
        body = json.dumps(doc, indent=1)
        if "code_shape" in doc:  # (one kernel per line, as compare_decode_objs.py writes them)
            import re

            body = re.sub(r"\{\s*\"kernel\": [^\[\]]*?\"waitcnt\": \d+\s*\}\s*\}", lambda m: re.sub(r"\s+", " ", m.group(0)), body)
        out.write_text(body + "\n")


if __name__ == "__main__":
    main()
