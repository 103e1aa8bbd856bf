"""Same-process A/B of the ragged paged prefill with attention sinks against the one without them, and of this
tree's unsinked ragged launch against another build's (the parent commit's library).

    timeout -k 10 900 python scripts/bench_paged_varlen_sink.py [--rounds R] [--inner N] [--parent-lib LIB.so]
                                                                 [--out FILE.json]

Shapes: the step of profiles/paged_varlen_ab.json -- 8 sequences with chunks of 128..2048 positions over 4k..32k keys,
causal, bf16, page size 64, shuffled pages -- for the gpt-oss head shape (Hq 64 / Hkv 8 / D 64) without a window and
with ``window_left`` 127, and for the Llama-3-8B head shape (Hq 32 / Hkv 8 / D 128).

1. "sink" (``flash_attn_paged_varlen_func``, the public wrapper on both arms):
     (s)  with sinks (2 randn(Hq))     (u)  without, same buffers     (u') (u) again: the run's own A/A spread
   Every round times s, u, u' in that order. Recorded per case: s / u (u = the mean of its two medians), the spread
   |u - u'| / mean, whether |s / u - 1| <= 2 x that spread, and the absolute difference per call. Before timing, the
   sinked launch with sinks of -inf is checked bit-equal to (u), and a sample of (s)'s rows against a float64 softmax
   with the extra column. The sink adds one scalar load per block and a handful of epilogue instructions per row,
   so the expectation under test is a ratio inside twice the A/A spread.

2. "parent" (the C entry ``fa_fwd_gfx950_paged_varlen`` through ctypes on both arms, so the host path is the same):
     (a)  this tree's library     (p)  ``--parent-lib``, a libfa_gfx950.so built from the parent commit, loaded from
   its own path     (a') (a) again. The two outputs are checked bit-equal. The kernels' code objects are meant to be
   identical, so p / a is expected inside the A/A spread. Without ``--parent-lib`` the section says "not measured".

A sample is ``--inner`` back-to-back calls between two device events, ending in a synchronise; the figure per arm is
the median over the rounds. Prints one JSON object and writes it to ``--out`` (default
profiles/paged_varlen_sink_ab.json).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BF16 = torch.bfloat16
PAGE, W = 64, 127
CHUNKS = [128, 2048, 512, 256, 1024, 384, 768, 1536]
LENS = [4096, 32768, 8192, 16384, 12288, 6144, 24576, 20480]
GPT_OSS, LLAMA = dict(Hq=64, Hkv=8, D=64), dict(Hq=32, Hkv=8, D=128)
CASES = [("gpt_oss", GPT_OSS, -1), ("gpt_oss_w127", GPT_OSS, W), ("llama3_8b", LLAMA, -1)]


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
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            times[n].append(sample(fn, inner))
    return {n: statistics.median(t) for n, t in times.items()}


def buffers(h, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    hq, hkv, d, b = h["Hq"], h["Hkv"], h["D"], len(LENS)
    max_pages = max(LENS) // PAGE
    n = sum(LENS) // PAGE
    q = torch.randn(sum(CHUNKS), hq, d, generator=gen, device=dev, dtype=BF16)
    kc = torch.randn(n, hkv, PAGE, d, generator=gen, device=dev, dtype=BF16)
    vc = torch.randn(n, hkv, PAGE, d, generator=gen, device=dev, dtype=BF16)
    ids = torch.randperm(n, generator=gen, device=dev).to(torch.int32)
    table = torch.full((b, max_pages), -1, dtype=torch.int32, device=dev)
    at = 0
    for i, length in enumerate(LENS):
        table[i, :length // PAGE] = ids[at:at + length // PAGE]
        at += length // PAGE
    cu = torch.tensor([sum(CHUNKS[:i]) for i in range(b + 1)], dtype=torch.int32, device=dev)
    sl = torch.tensor(LENS, dtype=torch.int32, device=dev)
    sinks = 2 * torch.randn(hq, generator=gen, device=dev)
    return q, kc, vc, cu, table, sl, sinks


def spot_check(name, out, q, kc, vc, cu, table, sl, sinks, w):
    """Rows 0, the middle and the last of sequence 0's chunk, q-heads 0 and the last: the float64 softmax with the
    extra column over the gathered keys."""
    hq, hkv = q.size(1), kc.size(1)
    s0, n = CHUNKS[0], LENS[0]
    keys = kc[table[0, :n // PAGE].long()].transpose(0, 1).flatten(1, 2).double()  # [Hkv, n, D]
    vals = vc[table[0, :n // PAGE].long()].transpose(0, 1).flatten(1, 2).double()
    worst = 0.0
    for m in (0, s0 // 2, s0 - 1):
        for hd in (0, hq - 1):
            hi = m + n - s0 + 1
            lo = max(0, m + n - s0 - w) if w >= 0 else 0
            sc = (keys[hd // (hq // hkv), lo:hi] @ q[m, hd].double()) * q.size(-1) ** -0.5
            p = torch.softmax(torch.cat([sc, sinks[hd].double()[None]]), 0)[:-1]
            worst = max(worst, (out[m, hd].double() - p @ vals[hd // (hq // hkv), lo:hi]).abs().max().item())
    if not worst <= 1.6e-2:
        raise AssertionError(f"{name}: the sinked launch differs from the float64 softmax by {worst}")
    return worst


def sink_case(name, h, w, rounds, inner, dev):
    from flash_attention_cute_amd import _debug, flash_attn_paged_varlen_func

    q, kc, vc, cu, table, sl, sinks = buffers(h, dev)
    kw = dict(causal=True, window_left=w)
    sinked = lambda: flash_attn_paged_varlen_func(q, kc, vc, cu, max(CHUNKS), table, sl, sinks=sinks, **kw)  # noqa: E731
    plain = lambda: flash_attn_paged_varlen_func(q, kc, vc, cu, max(CHUNKS), table, sl, **kw)  # noqa: E731
    out_s = sinked()
    path_s = _debug.last_path(), _debug.last_prefill_paged()
    out_u = plain()
    none = flash_attn_paged_varlen_func(q, kc, vc, cu, max(CHUNKS), table, sl, sinks=torch.full_like(sinks, float("-inf")), **kw)
    torch.cuda.synchronize()
    if path_s != ("w4", True):
        raise AssertionError(f"{name}: the sinked launch ran {path_s}")
    if not torch.equal(none, out_u):
        raise AssertionError(f"{name}: sinks of -inf do not give the bits of the call without sinks")
    err = spot_check(name, out_s, q, kc, vc, cu, table, sl, sinks, w)
    med = timed([("s", sinked), ("u", plain), ("u2", plain)], rounds, inner)
    u_ms = 0.5 * (med["u"] + med["u2"])
    spread = 100.0 * abs(med["u"] - med["u2"]) / u_ms
    ratio = med["s"] / u_ms
    return {"case": name, "window_left": w, "B": len(LENS), "Hq": h["Hq"], "Hkv": h["Hkv"], "D": h["D"], "page_size": PAGE,
            "chunks": CHUNKS, "lens": LENS, "spot_check_max_abs_err": err,
            "s_sinked_ms": round(med["s"], 5), "u_unsinked_ms": round(med["u"], 5), "u2_unsinked_ms": round(med["u2"], 5),
            "ratio_s_over_u": round(ratio, 4), "aa_spread_pct": round(spread, 3),
            "s_minus_u_us_per_call": round(1e3 * (med["s"] - u_ms), 2),
            "within_twice_the_spread": abs(ratio - 1.0) * 100.0 <= 2.0 * spread}


# ---- the C entry through ctypes (include/fa_gfx950_paged_varlen.h), for a library loaded from any path
def c_structs():
    from flash_attention_cute_amd._debug import FaFwdParams

    class Paged(ctypes.Structure):
        _fields_ = [("base", FaFwdParams), ("block_table", ctypes.c_void_p), ("block_table_stride", ctypes.c_int64),
                    ("max_pages", ctypes.c_int64), ("num_pages", ctypes.c_int64), ("page_size", ctypes.c_int64),
                    ("seqlens_k", ctypes.c_void_p)]

    class Varlen(ctypes.Structure):
        _fields_ = [("paged", Paged), ("cu_seqlens_q", ctypes.c_void_p), ("total_q", ctypes.c_int64)]

    return FaFwdParams, Paged, Varlen


def c_params(q, kc, vc, o, cu, table, sl):
    from flash_attention_cute_amd._debug import LOG2E

    FaFwdParams, Paged, Varlen = c_structs()
    hq, hkv, d = q.size(1), kc.size(1), q.size(2)
    base = FaFwdParams()
    base.q_ptr, base.k_ptr, base.v_ptr, base.o_ptr = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr()
    base.batch_size, base.num_heads_q, base.num_heads_kv = len(LENS), hq, hkv
    base.seqlen_q, base.seqlen_kv, base.headdim, base.head_q_per_group = max(CHUNKS), table.size(1) * PAGE, d, hq // hkv
    base.q_head_stride, base.o_head_stride, base.q_seqlen_stride, base.o_seqlen_stride = q.stride(1), o.stride(1), q.stride(0), o.stride(0)
    base.k_batch_stride, base.v_batch_stride = kc.stride(0), vc.stride(0)
    base.k_head_stride, base.v_head_stride = kc.stride(1), vc.stride(1)
    base.k_seqlen_stride, base.v_seqlen_stride = kc.stride(2), vc.stride(2)
    base.softmax_scale = float(torch.tensor(d ** -0.5, dtype=torch.float32).double() * LOG2E)
    paged = Paged(base, table.data_ptr(), table.stride(0), table.size(1), kc.size(0), PAGE, sl.data_ptr())
    return Varlen(paged, cu.data_ptr(), q.size(0))


def entry_of(lib):
    fn = lib.fa_fwd_gfx950_paged_varlen
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                   ctypes.c_void_p]
    fn.restype = ctypes.c_int
    lib.fa_last_error.restype = ctypes.c_char_p
    return fn


def parent_case(name, h, w, parent, rounds, inner, dev):
    from flash_attention_cute_amd import _debug

    q, kc, vc, cu, table, sl, _ = buffers(h, dev)
    outs = {k: torch.empty_like(q) for k in ("a", "p")}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    arms = {}
    for key, lib in (("a", _debug.lib()), ("p", parent)):
        vp, fn = c_params(q, kc, vc, outs[key], cu, table, sl), entry_of(lib)

        def call(vp=vp, fn=fn, lib=lib):
            rc = fn(ctypes.byref(vp), 1, 1, w, None, 0, stream)
            if rc != 0:
                raise RuntimeError(lib.fa_last_error().decode())

        arms[key] = call
    arms["a"]()
    arms["p"]()
    torch.cuda.synchronize()
    if not torch.equal(outs["a"], outs["p"]):
        raise AssertionError(f"{name}: this tree's unsinked launch and the parent's differ")
    med = timed([("a", arms["a"]), ("p", arms["p"]), ("a2", arms["a"])], rounds, inner)
    a_ms = 0.5 * (med["a"] + med["a2"])
    spread = 100.0 * abs(med["a"] - med["a2"]) / a_ms
    ratio = med["p"] / a_ms
    return {"case": name, "window_left": w, "Hq": h["Hq"], "Hkv": h["Hkv"], "D": h["D"], "bit_equal": True,
            "a_this_tree_ms": round(med["a"], 5), "p_parent_ms": round(med["p"], 5), "a2_this_tree_ms": round(med["a2"], 5),
            "ratio_parent_over_this": round(ratio, 4), "aa_spread_pct": round(spread, 3),
            "within_twice_the_spread": abs(ratio - 1.0) * 100.0 <= 2.0 * spread}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="a libfa_gfx950.so built from the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "paged_varlen_sink_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_varlen_sink needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    result = {"script": "scripts/bench_paged_varlen_sink.py", "device": torch.cuda.get_device_name(dev),
              "rounds": args.rounds, "inner": args.inner, "dtype": "bf16", "causal": True,
              "method": "median over rounds of (inner calls between two device events) / inner; per round the three "
                        "arms of a case interleaved, the reference arm at its start and its end (A/A spread = its two "
                        "medians); ratio = the middle arm / mean of the reference arm's medians",
              "sink": [sink_case(n, h, w, args.rounds, args.inner, dev) for n, h, w in CASES]}
    if args.parent_lib:
        import flash_attention_cute_amd  # noqa: F401  (this tree's library first)

        parent = ctypes.CDLL(str(Path(args.parent_lib).resolve()))
        result["parent"] = [parent_case(n, h, w, parent, args.rounds, args.inner, dev) for n, h, w in CASES]
    else:
        result["parent"] = "not measured (no --parent-lib)"
    print(json.dumps(result, indent=1), flush=True)
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
