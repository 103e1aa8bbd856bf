"""Same-process A/B of the FP8 (e4m3) paged decode against the bf16 paged decode on the same keys.

    timeout -k 10 900 python scripts/bench_fp8_decode.py [--rounds R] [--inner N] [--out FILE.json]
                                                         [--ring-lib LIB.so[,LIB.so...]]

For bench.py's ``decode_padded`` shape (bf16 B32 Hq32 Hkv8 D128, capacity 4096, lengths 1024..4000) and its
``decode_long`` shape (B1, 131072 keys), at page sizes 32 and 256 with the pages shuffled, the keys are
quantized once (descale 1.0, passed as fp32 tensors so the kernel loads them) and laid out twice: as an
e4m3 pool, and -- the dequantized bytes, exact in bf16 -- as a bf16 pool, so both kernels compute the same
function and their outputs are checked against each other within the parity tolerance (bf16: 1.6e-2 +
1.6e-2 |ref|) before anything is timed.

One process, one ``timeout``: every round times the bf16 paged decode (the code as it was before the FP8
kernel), the FP8 paged decode, and the bf16 decode AGAIN, so the run carries its own A/A spread (the two
bf16 medians) next to every fp8 / bf16 ratio. The same rounds time a FULL STEP -- ``flash_attn_with_kvcache``
with one new token per sequence, append and decode together -- on the FP8 and on the bf16 cache. A sample
is ``--inner`` back-to-back calls between two device events; the figure per variant is the median over the
rounds. Achieved bytes/s count the K / V bytes a step must read: 1 byte per element for FP8, 2 for bf16.

``--ring-lib``: further builds of the C-ABI library (``_build.build_abi(tag=..., defines=("FA_FP8_RING=2",))``:
the two-slot LDS ring) whose fa_fwd_gfx950_paged_fp8 is timed through ctypes in the same rounds, next to the
product library called the same way: the ring-depth A/B.

``--target-ab``: instead, the split-plan A/B of the FP8 decode on ``decode_long`` (page size 256): the
``dec_target`` knob (workgroups the split plan aims at) at 96 / 128 / 159 / 192 / 256 and 159 again (the A/A
spread; 159 gives the 16-bit default's plan, 20 splits), interleaved per round.

Prints one JSON object (and writes it to ``--out``).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PAGE_SIZES = (32, 256)
SHAPES = {  # bench.py CONFIGS decode_padded / decode_long
    "decode_padded": dict(B=32, Hq=32, Hkv=8, D=128, cap=4096, lens=[1024 + 96 * i for i in range(32)]),
    "decode_long": dict(B=1, Hq=32, Hkv=8, D=128, cap=131072, lens=[131072]),
}
FP8 = torch.float8_e4m3fn
ATOL, RTOL = 1.6e-2, 1.6e-2  # tests/test_gpu_parity.py TOL[bf16]


def paged_layout(x, page, perm):
    """Dense [B, Hkv, cap, D] as a pool [B * cap / page, Hkv, page, D] under the page permutation."""
    b, hkv, cap, d = x.shape
    mp = cap // page
    pages = x.reshape(b, hkv, mp, page, d).transpose(1, 2).reshape(b * mp, hkv, page, d)
    pool = torch.empty_like(pages)
    pool.view(torch.uint8 if x.dtype == FP8 else x.dtype)[perm] = pages.view(torch.uint8 if x.dtype == FP8 else x.dtype)
    return pool


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def close(a, b):
    return bool(((a.float() - b.float()).abs() <= ATOL + RTOL * b.float().abs()).all())


def ctypes_launcher(lib_path, q, kc8, vc8, table, lens, ones, out):
    """fa_fwd_gfx950_paged_fp8 of the library at lib_path on these tensors, as the torch binding calls it
    (Sq == 1: q-heads packed into the rows of a kv-head), its workspace allocated once."""
    from flash_attention_cute_amd._debug import FaFwdParams

    class Paged(ctypes.Structure):
        _fields_ = [("base", FaFwdParams), ("block_table", ctypes.c_void_p), ("block_table_stride", ctypes.c_int64),
                    ("max_pages", ctypes.c_int64), ("num_pages", ctypes.c_int64), ("page_size", ctypes.c_int64),
                    ("seqlens_k", ctypes.c_void_p)]

    class PagedFp8(ctypes.Structure):
        _fields_ = [("paged", Paged), ("k_descale", ctypes.c_void_p), ("v_descale", ctypes.c_void_p),
                    ("descale_batch_stride", ctypes.c_int64), ("descale_head_stride", ctypes.c_int64)]

    lib = ctypes.CDLL(str(lib_path))
    lib.fa_fwd_gfx950_paged_fp8_workspace_size.restype = ctypes.c_int64
    lib.fa_fwd_gfx950_paged_fp8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_int64, ctypes.c_void_p]
    lib.fa_last_error.restype = ctypes.c_char_p
    b, hq, _, d = q.shape
    hkv, g = kc8.size(1), q.size(1) // kc8.size(1)
    p = PagedFp8()
    f = p.paged.base
    f.q_ptr, f.k_ptr, f.v_ptr, f.o_ptr = q.data_ptr(), kc8.data_ptr(), vc8.data_ptr(), out.data_ptr()
    f.batch_size, f.num_heads_q, f.num_heads_kv, f.seqlen_q, f.headdim, f.head_q_per_group = b, hkv, hkv, g, d, 1
    f.seqlen_kv = table.size(1) * kc8.size(2)
    f.q_batch_stride = f.o_batch_stride = hq * d
    f.q_head_stride = f.o_head_stride = g * d
    f.q_seqlen_stride = f.o_seqlen_stride = d
    f.k_batch_stride, f.k_head_stride, f.k_seqlen_stride = kc8.stride(0), kc8.stride(1), kc8.stride(2)
    f.v_batch_stride, f.v_head_stride, f.v_seqlen_stride = vc8.stride(0), vc8.stride(1), vc8.stride(2)
    f.softmax_scale = d ** -0.5 * 1.4426950408889634
    p.paged.block_table, p.paged.block_table_stride = table.data_ptr(), table.stride(0)
    p.paged.max_pages, p.paged.num_pages, p.paged.page_size = table.size(1), kc8.size(0), kc8.size(2)
    p.paged.seqlens_k = lens.data_ptr()
    p.k_descale = p.v_descale = ones.data_ptr()
    p.descale_batch_stride, p.descale_head_stride = ones.stride(0), ones.stride(1)
    n = lib.fa_fwd_gfx950_paged_fp8_workspace_size(ctypes.byref(p), 1, 0)
    if n < 0:
        raise RuntimeError(f"{lib_path}: {lib.fa_last_error().decode()}")
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=q.device)
    stream = torch.cuda.current_stream().cuda_stream

    def fn():
        rc = lib.fa_fwd_gfx950_paged_fp8(ctypes.byref(p), 1, 0, ws.data_ptr() if n else None, n, stream)
        if rc != 0:
            raise RuntimeError(f"{lib_path}: {lib.fa_last_error().decode()}")

    fn.keep = (p, ws, lib)
    return fn


def run_shape(name, s, rounds, inner, dev, ring_libs):
    from flash_attention_cute_amd import _build, _debug, flash_attn_paged_func, flash_attn_with_kvcache

    gen = torch.Generator().manual_seed(1)
    b, hq, hkv, d, cap = s["B"], s["Hq"], s["Hkv"], s["D"], s["cap"]
    q = torch.randn(b, hq, 1, d, generator=gen).to(torch.bfloat16).to(dev)
    k8 = torch.randn(b, hkv, cap, d, generator=gen).to(dev).clamp(-448, 448).to(FP8)
    v8 = torch.randn(b, hkv, cap, d, generator=gen).to(dev).clamp(-448, 448).to(FP8)
    k16, v16 = k8.to(torch.bfloat16), v8.to(torch.bfloat16)  # the dequantized keys: exact
    lens = torch.tensor(s["lens"], dtype=torch.int32, device=dev)
    step_lens = lens.clamp(max=cap - 1)  # the full step appends one token: leave room for it
    ones = torch.ones(b, hkv, dtype=torch.float32, device=dev)
    k_new = torch.randn(b, hkv, 1, d, generator=gen).to(torch.bfloat16).to(dev)
    v_new = torch.randn(b, hkv, 1, d, generator=gen).to(torch.bfloat16).to(dev)
    pages = []
    for page in PAGE_SIZES:
        perm = torch.randperm(b * cap // page, generator=gen).to(dev)
        table = perm.reshape(b, cap // page).to(torch.int32)
        kc16, vc16, kc8, vc8 = (paged_layout(x, page, perm) for x in (k16, v16, k8, v8))
        bf16 = lambda kc16=kc16, vc16=vc16, table=table: flash_attn_paged_func(q, kc16, vc16, table, lens)  # noqa: E731
        fp8 = (lambda kc8=kc8, vc8=vc8, table=table:
               flash_attn_paged_func(q, kc8, vc8, table, lens, k_descale=ones, v_descale=ones))
        step16 = (lambda kc16=kc16, vc16=vc16, table=table:
                  flash_attn_with_kvcache(q, kc16, vc16, k_new, v_new, cache_seqlens=step_lens, block_table=table))
        step8 = (lambda kc8=kc8, vc8=vc8, table=table:
                 flash_attn_with_kvcache(q, kc8, vc8, k_new, v_new, cache_seqlens=step_lens, block_table=table,
                                         k_descale=ones, v_descale=ones))
        ref = bf16()
        bf16_path = _debug.last_path()
        out = fp8()
        fp8_path = _debug.last_path()
        torch.cuda.synchronize()
        if not close(out, ref):
            raise AssertionError(f"{name}: page size {page}: fp8 decode differs from the bf16 decode on the same keys")
        if not close(step8(), step16()):
            raise AssertionError(f"{name}: page size {page}: fp8 full step differs from the bf16 full step")
        variants = [("bf16_a", bf16), ("fp8", fp8)]
        for i, path in enumerate([_build.ABI_LIB, *ring_libs]):
            o = torch.empty_like(q)
            fn = ctypes_launcher(path, q, kc8, vc8, table, lens, ones, o)
            fn()
            torch.cuda.synchronize()
            if not close(o, ref):
                raise AssertionError(f"{name}: page size {page}: {path} differs from the bf16 decode")
            if ring_libs:
                variants.append((f"lib{i}", fn))
        variants += [("step_bf16", step16), ("step_fp8", step8), ("bf16_b", bf16)]
        for _, fn in variants:  # warm-up: every variant of the timed window
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n, _ in variants}
        for _ in range(rounds):
            for n, fn in variants:
                times[n].append(sample(fn, inner))
        med = {n: statistics.median(t) for n, t in times.items()}
        bf16_ms = 0.5 * (med["bf16_a"] + med["bf16_b"])
        elems = 2 * hkv * d * sum(s["lens"])  # K and V elements a step reads
        entry = {
            "page_size": page, "bf16_path": bf16_path, "fp8_path": fp8_path, "within_parity_tolerance": True,
            "bf16_a_ms": round(med["bf16_a"], 5), "bf16_b_ms": round(med["bf16_b"], 5), "bf16_ms": round(bf16_ms, 5),
            # the run's own A/A spread: the two bf16 medians, same code, same data, same process
            "aa_spread_pct": round(100.0 * abs(med["bf16_a"] - med["bf16_b"]) / bf16_ms, 3),
            "fp8_ms": round(med["fp8"], 5), "ratio_fp8_over_bf16": round(med["fp8"] / bf16_ms, 4),
            "bf16_kv_gbs": round(2 * elems / bf16_ms / 1e6, 1), "fp8_kv_gbs": round(elems / med["fp8"] / 1e6, 1),
            "step_bf16_ms": round(med["step_bf16"], 5), "step_fp8_ms": round(med["step_fp8"], 5),
            "ratio_step_fp8_over_bf16": round(med["step_fp8"] / med["step_bf16"], 4),
        }
        if ring_libs:
            entry["ring_ab"] = [{"lib": str(pth), "ms": round(med[f"lib{i}"], 5),
                                 "ratio_over_product_lib": round(med[f"lib{i}"] / med["lib0"], 4)}
                                for i, pth in enumerate([_build.ABI_LIB, *ring_libs])]
        pages.append(entry)
    return {"shape": name, "B": b, "Hq": hq, "Hkv": hkv, "D": d, "capacity": cap, "q_dtype": "bf16",
            "kv_elements": 2 * hkv * d * sum(s["lens"]), "pages": pages}


def run_target_ab(rounds, inner, dev):
    from flash_attention_cute_amd import _debug, flash_attn_paged_func

    s, page = SHAPES["decode_long"], 256
    gen = torch.Generator().manual_seed(1)
    b, hq, hkv, d, cap = s["B"], s["Hq"], s["Hkv"], s["D"], s["cap"]
    q = torch.randn(b, hq, 1, d, generator=gen).to(torch.bfloat16).to(dev)
    k8 = torch.randn(b, hkv, cap, d, generator=gen).to(dev).to(FP8)
    v8 = torch.randn(b, hkv, cap, d, generator=gen).to(dev).to(FP8)
    perm = torch.randperm(b * cap // page, generator=gen).to(dev)
    table = perm.reshape(b, cap // page).to(torch.int32)
    kc8, vc8 = paged_layout(k8, page, perm), paged_layout(v8, page, perm)
    lens = torch.tensor(s["lens"], dtype=torch.int32, device=dev)
    ones = torch.ones(b, hkv, dtype=torch.float32, device=dev)
    # 159 gives the plan of 160 (20 splits of the 8 units); the knob at exactly 160 is its default, under
    # which the FP8 dispatcher aims at its own 256
    targets = [96, 128, 159, 192, 256, 159]

    def run(t):
        _debug.set_knobs(dec_target=t)  # (the FP8 plan's own target applies only while the knob is at its default)
        return flash_attn_paged_func(q, kc8, vc8, table, lens, k_descale=ones, v_descale=ones)

    try:
        ref = run(159)
        for t in targets:
            if not close(run(t), ref):
                raise AssertionError(f"dec_target {t} differs")
            for _ in range(10):
                run(t)
        torch.cuda.synchronize()
        times = [[] for _ in targets]
        for _ in range(rounds):
            for i, t in enumerate(targets):
                times[i].append(sample(lambda t=t: run(t), inner))
    finally:
        _debug.set_knobs()
    return {"shape": "decode_long", "page_size": page,
            "targets": [{"dec_target": t, "fp8_ms": round(statistics.median(times[i]), 5)} for i, t in enumerate(targets)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ring-lib", default="", help="comma-separated further libfa_gfx950.so builds (ring-depth A/B)")
    ap.add_argument("--target-ab", action="store_true", help="the split-plan target A/B on decode_long instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8_decode needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    ring_libs = [Path(p).resolve() for p in args.ring_lib.split(",") if p]
    if args.target_ab:
        result = {"script": "scripts/bench_fp8_decode.py --target-ab", "device": torch.cuda.get_device_name(dev),
                  "rounds": args.rounds, "inner": args.inner,
                  "method": "median over rounds of (inner calls between two device events) / inner; per round: the "
                            "fp8 paged decode at every dec_target in turn (159, the plan of the 16-bit default 160, twice: the A/A spread)",
                  "target_ab": run_target_ab(args.rounds, args.inner, dev)}
        text = json.dumps(result, indent=1)
        print(text, flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return
    result = {"script": "scripts/bench_fp8_decode.py", "device": torch.cuda.get_device_name(dev),
              "rounds": args.rounds, "inner": args.inner,
              "method": "median over rounds of (inner calls between two device events) / inner; per round and page "
                        "size: bf16 paged decode, fp8 paged decode [, the C-ABI of each --ring-lib], bf16 full step, "
                        "fp8 full step (flash_attn_with_kvcache: append + decode), bf16 paged decode again",
              "shapes": [run_shape(n, s, args.rounds, args.inner, dev, ring_libs) for n, s in SHAPES.items()]}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
