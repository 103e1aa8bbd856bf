"""Same-process A/B of the fused KV-cache append: one serving step, and the append alone.

    timeout -k 10 600 python scripts/bench_kvcache_append.py [--rounds R] [--inner N] [--out FILE.json]

(a) One decode step at bench.py's ``decode_long`` sizes (bf16 B1 Hq32 Hkv8 D128, 131072 keys of capacity,
    page 128, shuffled pages, the sequence one token short of full): ``flash_attn_with_kvcache`` -- one
    append launch for K, V and q, then the paged decode -- against the same step composed from what the
    project offered before: a torch gather of the cos / sin rows, ``apply_rope`` on k and on q, the
    (page, row) arithmetic and two ``index_put_`` in torch, ``flash_attn_paged_func`` and the
    ``cache_seqlens`` add. The lengths are not advanced between calls, so every call does the same work
    and writes the same row. Every round times composed, fused, composed AGAIN: the run carries the
    composed step's own A/A spread next to the fused / composed ratio.
(b) The append alone at a prefill size (bf16 B4 Hkv8 Sn4096 D128, page 128, shuffled pages, with and
    without the rotation), as bytes moved (read + written: 2 x (|k| + |v|)) per second, against
    ``torch.Tensor.copy_`` of the same byte count on the same device, copy / append / copy per round.

A sample is ``--inner`` back-to-back calls between two device events; the figure per variant is the
median over the rounds. Every variant is timed twice. The eager figures are END-TO-END CALL TIMES: a call
is a few small launches behind a custom-op dispatch, so where the host cannot issue them faster than
the device runs them they measure the host. The ``graph`` figures replay the same ``--inner`` calls
captured once in a HIP graph, so the host is out of the window and the device time remains; the same
alternation and A/A spread apply. Results are checked bit-equal before timing. Prints one JSON object
(and writes it to ``--out``).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BF16 = torch.bfloat16
DECODE = dict(B=1, Hq=32, Hkv=8, D=128, cap=131072, page=128)  # bench.py CONFIGS decode_long
PREFILL = dict(B=4, Hkv=8, Sn=4096, D=128, page=128)


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def graphed(fn, inner):
    """`inner` calls of fn captured in one graph; returns its replay."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g.replay


def measure(variants, rounds, inner):
    """(eager, graph) medians in ms per call of every variant, alternating per round."""
    for _, fn in variants:  # warm-up: every variant of the timed window
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            times[n].append(sample(fn, inner))
    replays = [(n, graphed(fn, inner)) for n, fn in variants]
    for _, replay in replays:
        replay()
    torch.cuda.synchronize()
    gtimes = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, replay in replays:
            gtimes[n].append(sample(replay, 1) / inner)
    return ({n: statistics.median(t) for n, t in times.items()}, {n: statistics.median(t) for n, t in gtimes.items()})


def rope_tables(max_pos, d, dev):
    ang = torch.rand(max_pos, d // 2, generator=torch.Generator().manual_seed(7)) * 6.283
    ang = torch.cat((ang, ang), dim=-1)
    return ang.cos().to(BF16).to(dev), ang.sin().to(BF16).to(dev)


def shuffled_pool(b, hkv, max_pages, page, d, dev, gen, fill=True):
    num_pages = b * max_pages
    table = torch.randperm(num_pages, generator=gen).reshape(b, max_pages).to(torch.int32).to(dev)
    make = (lambda: torch.randn(num_pages, hkv, page, d, generator=gen).to(BF16).to(dev)) if fill else \
        (lambda: torch.zeros(num_pages, hkv, page, d, dtype=BF16, device=dev))
    return make(), make(), table


def decode_step(rounds, inner, dev):
    from flash_attention_cute_amd import _debug, apply_rope, flash_attn_paged_func, flash_attn_with_kvcache

    s = DECODE
    b, hq, hkv, d, cap, page = s["B"], s["Hq"], s["Hkv"], s["D"], s["cap"], s["page"]
    gen = torch.Generator().manual_seed(1)
    kc, vc, table = shuffled_pool(b, hkv, cap // page, page, d, dev, gen)
    q = torch.randn(b, hq, 1, d, generator=gen).to(BF16).to(dev)
    k = torch.randn(b, hkv, 1, d, generator=gen).to(BF16).to(dev)
    v = torch.randn(b, hkv, 1, d, generator=gen).to(BF16).to(dev)
    cos, sin = rope_tables(cap, d, dev)
    lens = torch.full((b,), cap - 1, dtype=torch.int32, device=dev)

    def fused(kc=kc, vc=vc):
        return flash_attn_with_kvcache(q, kc, vc, k, v, cos, sin, cache_seqlens=lens, block_table=table,
                                       return_seqlens=True)

    def composed(kc=kc, vc=vc):
        pos = lens.long()[:, None]                                  # [B, 1]: the new token's position
        c, sn = cos[pos], sin[pos]                                  # [B, 1, D]
        kr, qr = apply_rope(k, c, sn), apply_rope(q, c, sn)
        pg = table.gather(1, pos // page).long()[:, 0]              # key n: row n % page of page table[b][n / page]
        row = (pos % page)[:, 0]
        kc[pg, :, row] = kr[:, :, 0]                                # (index_put_)
        vc[pg, :, row] = v[:, :, 0]
        new = lens + 1
        return flash_attn_paged_func(qr, kc, vc, table, new), new

    kc2, vc2 = kc.clone(), vc.clone()
    (o1, n1), (o2, n2) = fused(), composed(kc2, vc2)
    path = _debug.last_path()
    torch.cuda.synchronize()
    if not (torch.equal(o1, o2) and torch.equal(n1, n2) and torch.equal(kc, kc2) and torch.equal(vc, vc2)):
        raise AssertionError("the fused step differs from the composed step")
    eager, graph = measure([("composed_a", composed), ("fused", fused), ("composed_b", composed)], rounds, inner)

    def figures(med):
        comp = 0.5 * (med["composed_a"] + med["composed_b"])
        return {"composed_a_ms": round(med["composed_a"], 5), "composed_b_ms": round(med["composed_b"], 5),
                "composed_ms": round(comp, 5), "fused_ms": round(med["fused"], 5),
                "ratio_fused_over_composed": round(med["fused"] / comp, 4),
                # the run's own A/A spread: the two composed medians, same code, same data, same process
                "aa_spread_pct": round(100.0 * abs(med["composed_a"] - med["composed_b"]) / comp, 3)}

    return {"shape": "decode_long", **s, "dtype": "bf16", "len_before": cap - 1, "pages": "shuffled",
            "attention_path": path, **figures(eager), "graph": figures(graph), "bit_equal": True}


def prefill_append(rounds, inner, dev):
    from flash_attention_cute_amd import apply_rope, flash_attn_kvcache_append

    s = PREFILL
    b, hkv, sn, d, page = s["B"], s["Hkv"], s["Sn"], s["D"], s["page"]
    gen = torch.Generator().manual_seed(2)
    kc, vc, table = shuffled_pool(b, hkv, sn // page, page, d, dev, gen, fill=False)
    k = torch.randn(b, hkv, sn, d, generator=gen).to(BF16).to(dev)
    v = torch.randn(b, hkv, sn, d, generator=gen).to(BF16).to(dev)
    cos, sin = rope_tables(sn, d, dev)
    lens = torch.zeros(b, dtype=torch.int32, device=dev)
    moved = 2 * 2 * k.numel() * 2  # k and v, read and written, 2 bytes per element
    src, dst = torch.cat((k.reshape(-1), v.reshape(-1))), torch.empty(2 * k.numel(), dtype=BF16, device=dev)
    assert 2 * src.numel() * 2 == moved

    # the pool through the table is the dense [B, Hkv, Sn, D] again: check both variants before timing
    def gathered(c):
        return c[table.long().reshape(-1)].reshape(b, sn // page, hkv, page, d).transpose(1, 2).reshape(b, hkv, sn, d)

    new = flash_attn_kvcache_append(kc, vc, k, v, lens, table)
    ok = torch.equal(gathered(kc), k) and torch.equal(gathered(vc), v) and new.tolist() == [sn] * b
    flash_attn_kvcache_append(kc, vc, k, v, lens, table, cos, sin)
    ok = ok and torch.equal(gathered(kc), apply_rope(k, cos, sin)) and torch.equal(gathered(vc), v)
    torch.cuda.synchronize()
    if not ok:
        raise AssertionError("the appended pool differs from apply_rope(k) / v")
    eager, graph = measure([("copy_a", lambda: dst.copy_(src)),
                            ("append", lambda: flash_attn_kvcache_append(kc, vc, k, v, lens, table)),
                            ("append_rope", lambda: flash_attn_kvcache_append(kc, vc, k, v, lens, table, cos, sin)),
                            ("copy_b", lambda: dst.copy_(src))], rounds, inner)
    gbs = lambda ms: round(moved / ms / 1e6, 1)  # noqa: E731

    def figures(med):
        copy = 0.5 * (med["copy_a"] + med["copy_b"])
        return {"copy_a_ms": round(med["copy_a"], 5), "copy_b_ms": round(med["copy_b"], 5), "copy_ms": round(copy, 5),
                "copy_gbs": gbs(copy), "aa_spread_pct": round(100.0 * abs(med["copy_a"] - med["copy_b"]) / copy, 3),
                "append_ms": round(med["append"], 5), "append_gbs": gbs(med["append"]),
                "ratio_append_over_copy_rate": round(copy / med["append"], 4),
                "append_rope_ms": round(med["append_rope"], 5), "append_rope_gbs": gbs(med["append_rope"]),
                "ratio_append_rope_over_copy_rate": round(copy / med["append_rope"], 4)}

    return {"shape": "prefill_append", **s, "dtype": "bf16", "pages": "shuffled", "bytes_moved": moved,
            **figures(eager), "graph": figures(graph), "bit_equal": True}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kvcache_append needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    result = {"script": "scripts/bench_kvcache_append.py", "device": torch.cuda.get_device_name(dev),
              "rounds": args.rounds, "inner": args.inner,
              "method": "median over rounds of (inner calls between two device events) / inner; per round: "
                        "composed, fused, composed again (decode step); copy_, append, append + RoPE, copy_ again "
                        "(prefill append). Top-level figures: eager calls, end to end (host dispatch included); "
                        "'graph': the same inner calls captured in one HIP graph and replayed (device time)",
              "decode_step": decode_step(args.rounds, args.inner, dev),
              "prefill_append": prefill_append(args.rounds, args.inner, dev)}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
