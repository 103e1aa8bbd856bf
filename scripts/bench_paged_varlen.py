"""Same-process A/B of the ragged step on the paged KV cache against what a caller does without it.

    timeout -k 10 900 python scripts/bench_paged_varlen.py [--rounds R] [--inner N] [--out FILE.json]

Llama-3-8B head shape (bf16, Hq 32, Hkv 8, D 128, causal), page sizes 64 and 256, the pages under a random
permutation. Every round times, interleaved,

  step (8 sequences, chunks of 128 .. 2048 positions over 4k .. 32k keys):
    (f_a / f_b) the floor: ``flash_attn_varlen_func`` on already-gathered packed keys, timed at the start AND at the
        end of the round, so the run carries its own A/A spread next to every ratio;
    (ragged)    ``flash_attn_paged_varlen_func``: one launch over the block table;
    (per_seq)   one ``flash_attn_paged_func`` call per sequence (B = 1 each);
    (gather)    the pages gathered into packed dense keys (one ``index_select`` per pool), then
                ``flash_attn_varlen_func``;
  mixed (one 2048-position chunk plus 31 one-token sequences -- the cost of empty q-tiles and of the unbalanced
  order):
    (ragged)    one ``flash_attn_paged_varlen_func`` launch over all 32 sequences;
    (split)     the chunk alone through ``flash_attn_paged_varlen_func`` plus one ``flash_attn_paged_func`` decode
                of the 31;
    (chunk_a / chunk_b) the chunk alone, at the start and the end of the round: the A/A spread;
  append (the step's chunks as new tokens, K rotated):
    (ragged)    ``flash_attn_kvcache_append_varlen``: one launch;
    (per_seq)   one ``flash_attn_kvcache_append`` per sequence;
    (copy_a / copy_b) ``copy_`` of the same K and V bytes (the HBM floor of any append), start and end of the round.

One process, one ``timeout``. A sample is ``--inner`` back-to-back calls between two device events; the figure per
variant is the median over the rounds. Outputs are checked bit-equal before timing. Prints one JSON object and
writes it to ``--out`` (default profiles/paged_varlen_ab.json).
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

from scripts.bench_paged_decode import paged_layout, sample  # noqa: E402

PAGE_SIZES = (64, 256)
HQ, HKV, D = 32, 8, 128
BF = torch.bfloat16
STEP_CHUNKS = (128, 2048, 512, 256, 1024, 384, 768, 1536)
STEP_LENS = (4096, 32768, 8192, 16384, 12288, 6144, 24576, 20480)  # keys AFTER the chunk (multiples of 256)
MIXED_CHUNK, MIXED_CHUNK_LEN, MIXED_DECODES = 2048, 16384, 31


def cu_of(counts, dev):
    out = [0]
    for n in counts:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32, device=dev)


def timed(variants, rounds, inner):
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            times[n].append(sample(fn, inner))
    return {n: statistics.median(t) for n, t in times.items()}


def spread(a, b):
    return round(100.0 * abs(a - b) / (0.5 * (a + b)), 3)


def page_ids(table, lens, page):
    """The page ids of every sequence's keys, in sequence order (lengths are multiples of the page size)."""
    return torch.cat([table[b, :n // page] for b, n in enumerate(lens)]).to(torch.int64)


def gather_packed(cache, ids):
    """[num_pages, Hkv, page, D] pool -> packed [total_k, Hkv, D]: one copy."""
    return cache.transpose(1, 2).index_select(0, ids).flatten(0, 1)


def dense_keys(lens, cap, dev, seed):
    gen = torch.Generator().manual_seed(seed)  # (the page permutation and the queries; the keys: the device's generator)
    torch.manual_seed(seed)
    k = torch.randn(len(lens), HKV, cap, D, device=dev, dtype=BF)
    v = torch.randn(len(lens), HKV, cap, D, device=dev, dtype=BF)
    return k, v, gen


def run_step(page, rounds, inner, dev):
    from flash_attention_cute_amd import (_debug, flash_attn_paged_func, flash_attn_paged_varlen_func,
                                          flash_attn_varlen_func)

    cap = max(STEP_LENS)
    k, v, gen = dense_keys(STEP_LENS, cap, dev, 1)
    q = torch.randn(sum(STEP_CHUNKS), HQ, D, generator=gen).to(BF).to(dev)
    kc, vc, table = paged_layout(k, v, page, gen)
    lens = torch.tensor(STEP_LENS, dtype=torch.int32, device=dev)
    cu_q, cu_k = cu_of(STEP_CHUNKS, dev), cu_of(STEP_LENS, dev)
    ids = page_ids(table, STEP_LENS, page)
    kp, vp = gather_packed(kc, ids), gather_packed(vc, ids)
    del k, v
    max_q, max_k = max(STEP_CHUNKS), max(STEP_LENS)
    r = cu_q.tolist()
    q4 = [q[r[b]:r[b + 1]].transpose(0, 1)[None] for b in range(len(STEP_CHUNKS))]  # views: [1, Hq, Sq_b, D]

    floor = lambda: flash_attn_varlen_func(q, kp, vp, cu_q, cu_k, max_q, max_k, causal=True)  # noqa: E731
    ragged = lambda: flash_attn_paged_varlen_func(q, kc, vc, cu_q, max_q, table, lens, causal=True)  # noqa: E731

    def per_seq():
        return [flash_attn_paged_func(q4[b], kc, vc, table[b:b + 1], lens[b:b + 1], causal=True)
                for b in range(len(STEP_CHUNKS))]

    def gather():
        return flash_attn_varlen_func(q, gather_packed(kc, ids), gather_packed(vc, ids), cu_q, cu_k, max_q, max_k,
                                      causal=True)

    ref = floor()
    out = ragged()
    if not (_debug.last_path() == "w4" and _debug.last_prefill_paged()):
        raise AssertionError("the ragged call did not run the paged prefill kernel")
    ones = per_seq()
    torch.cuda.synchronize()
    if not (torch.equal(out, ref) and torch.equal(gather(), ref)):
        raise AssertionError(f"step, page size {page}: the ragged launch differs from the dense varlen op")
    for b, one in enumerate(ones):
        if not torch.equal(one[0].transpose(0, 1), ref[r[b]:r[b + 1]]):
            raise AssertionError(f"step, page size {page}: sequence {b} alone differs")
    med = timed([("f_a", floor), ("ragged", ragged), ("per_seq", per_seq), ("gather", gather), ("f_b", floor)], rounds, inner)
    f = 0.5 * (med["f_a"] + med["f_b"])
    return {"case": "step", "page_size": page, "pages": "shuffled", "bit_equal": True, "chunks": STEP_CHUNKS,
            "lens": STEP_LENS, "ragged_ms": round(med["ragged"], 4), "per_seq_ms": round(med["per_seq"], 4),
            "gather_ms": round(med["gather"], 4), "floor_a_ms": round(med["f_a"], 4), "floor_b_ms": round(med["f_b"], 4),
            "aa_spread_pct": spread(med["f_a"], med["f_b"]), "ratio_ragged_over_per_seq": round(med["ragged"] / med["per_seq"], 4),
            "ratio_ragged_over_gather": round(med["ragged"] / med["gather"], 4),
            "ratio_ragged_over_floor": round(med["ragged"] / f, 4)}


def run_mixed(page, rounds, inner, dev):
    from flash_attention_cute_amd import _debug, flash_attn_paged_func, flash_attn_paged_varlen_func

    dec_lens = tuple(4096 + 256 * i for i in range(MIXED_DECODES))
    all_lens = (MIXED_CHUNK_LEN,) + dec_lens
    chunks = (MIXED_CHUNK,) + (1,) * MIXED_DECODES
    k, v, gen = dense_keys(all_lens, max(all_lens), dev, 2)
    q = torch.randn(sum(chunks), HQ, D, generator=gen).to(BF).to(dev)
    kc, vc, table = paged_layout(k, v, page, gen)
    del k, v
    lens = torch.tensor(all_lens, dtype=torch.int32, device=dev)
    cu_all, cu_one = cu_of(chunks, dev), cu_of(chunks[:1], dev)
    q_chunk, q_dec = q[:MIXED_CHUNK], q[MIXED_CHUNK:, :, None]  # [31, Hq, 1, D]
    ragged = lambda: flash_attn_paged_varlen_func(q, kc, vc, cu_all, MIXED_CHUNK, table, lens, causal=True)  # noqa: E731
    chunk = lambda: flash_attn_paged_varlen_func(q_chunk, kc, vc, cu_one, MIXED_CHUNK, table[:1], lens[:1], causal=True)  # noqa: E731
    decode = lambda: flash_attn_paged_func(q_dec, kc, vc, table[1:], lens[1:], causal=True)  # noqa: E731

    def split():
        return chunk(), decode()

    out = ragged()
    if not (_debug.last_path() == "w4" and _debug.last_prefill_paged()):
        raise AssertionError("the ragged call did not run the paged prefill kernel")
    a, b = split()
    torch.cuda.synchronize()
    if not torch.equal(out[:MIXED_CHUNK], a):
        raise AssertionError(f"mixed, page size {page}: the chunk alone differs")
    err = (out[MIXED_CHUNK:].float() - b[:, :, 0].float()).abs().max().item()  # (another kernel: close, not equal)
    if not err < 2e-2:
        raise AssertionError(f"mixed, page size {page}: the decode rows differ by {err}")
    med = timed([("chunk_a", chunk), ("ragged", ragged), ("split", split), ("decode", decode), ("chunk_b", chunk)], rounds, inner)
    return {"case": "mixed", "page_size": page, "pages": "shuffled", "chunk": MIXED_CHUNK, "chunk_len": MIXED_CHUNK_LEN,
            "decodes": MIXED_DECODES, "ragged_ms": round(med["ragged"], 4), "split_ms": round(med["split"], 4),
            "chunk_a_ms": round(med["chunk_a"], 4), "chunk_b_ms": round(med["chunk_b"], 4), "decode_ms": round(med["decode"], 4),
            "aa_spread_pct": spread(med["chunk_a"], med["chunk_b"]),
            "ratio_ragged_over_split": round(med["ragged"] / med["split"], 4)}


def run_append(page, rounds, inner, dev):
    from flash_attention_cute_amd import flash_attn_kvcache_append, flash_attn_kvcache_append_varlen

    news = STEP_CHUNKS
    before = tuple(n - m for n, m in zip(STEP_LENS, news))
    cap = max(STEP_LENS)
    b, mp = len(news), cap // page
    gen = torch.Generator().manual_seed(3)
    table = torch.randperm(b * mp, generator=gen).reshape(b, mp).to(torch.int32).to(dev)
    kc = torch.zeros(b * mp, HKV, page, D, dtype=BF, device=dev)
    vc = torch.zeros_like(kc)
    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
    k = torch.randn(sum(news), HKV, D, generator=gen).to(BF).to(dev)
    v = torch.randn(sum(news), HKV, D, generator=gen).to(BF).to(dev)
    ang = torch.rand(cap, D // 2, generator=gen) * 6.283
    ang = torch.cat((ang, ang), dim=-1)
    cos, sin = ang.cos().to(BF).to(dev), ang.sin().to(BF).to(dev)
    lens = torch.tensor(before, dtype=torch.int32, device=dev)
    cu = cu_of(news, dev)
    r = cu.tolist()
    k4 = [k[r[i]:r[i + 1]].transpose(0, 1)[None] for i in range(b)]
    v4 = [v[r[i]:r[i + 1]].transpose(0, 1)[None] for i in range(b)]
    dst_k, dst_v = torch.empty_like(k), torch.empty_like(v)
    ragged = lambda: flash_attn_kvcache_append_varlen(kc, vc, k, v, cu, lens, table, cos, sin)  # noqa: E731

    def per_seq():
        for i in range(b):
            flash_attn_kvcache_append(kc2, vc2, k4[i], v4[i], lens[i:i + 1], table[i:i + 1], cos, sin)

    def copy():
        dst_k.copy_(k)
        dst_v.copy_(v)

    ragged()
    per_seq()
    torch.cuda.synchronize()
    if not (torch.equal(kc.view(torch.int16), kc2.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc2.view(torch.int16))):
        raise AssertionError(f"append, page size {page}: the ragged append differs from the per-sequence appends")
    med = timed([("copy_a", copy), ("ragged", ragged), ("per_seq", per_seq), ("copy_b", copy)], rounds, inner)
    c = 0.5 * (med["copy_a"] + med["copy_b"])
    return {"case": "append", "page_size": page, "pages": "shuffled", "bit_equal": True, "new_tokens": news,
            "bytes_moved": 2 * 2 * k.numel() * 2, "ragged_ms": round(med["ragged"], 4), "per_seq_ms": round(med["per_seq"], 4),
            "copy_a_ms": round(med["copy_a"], 4), "copy_b_ms": round(med["copy_b"], 4),
            "aa_spread_pct": spread(med["copy_a"], med["copy_b"]),
            "ratio_ragged_over_per_seq": round(med["ragged"] / med["per_seq"], 4),
            "ratio_ragged_over_copy": round(med["ragged"] / c, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "paged_varlen_ab.json"))
    ap.add_argument("--cases", default="step,mixed,append")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_varlen needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    runs = {"step": run_step, "mixed": run_mixed, "append": run_append}
    rows = []
    for case in args.cases.split(","):
        for page in PAGE_SIZES:
            rows.append(runs[case](page, args.rounds, args.inner, dev))
            torch.cuda.empty_cache()
    result = {"script": "scripts/bench_paged_varlen.py", "rounds": args.rounds,
              "inner": args.inner, "dtype": "bf16", "Hq": HQ, "Hkv": HKV, "D": D, "causal": True,
              "method": "median over rounds of (inner calls between two device events) / inner; every round runs all "
                        "variants of a case interleaved, the reference variant at its start and its end (A/A spread = "
                        "the two medians)",
              "cases": rows}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
