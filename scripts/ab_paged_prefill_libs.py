"""Interleaved A/B of the UNIFORM paged prefill (C-ABI ``fa_fwd_gfx950_paged_prefill``) between two builds of the
library -- a parent commit's and this tree's -- in one process, on the same buffers, on bench_paged_prefill's shapes.

    timeout -k 10 300 python scripts/ab_paged_prefill_libs.py PARENT_LIB.so [THIS_LIB.so] [--rounds R] [--out FILE.json]

bf16, Hq 32, Hkv 8, D 128, causal, full caches, the pages under a random permutation, page sizes 64 and 256. The
parent's library is loaded twice (the second time from a copy, so that it is another handle): its two medians are the
A/A spread that the ratio ``this / parent`` is read against. The order of the three rotates every round, so no
library always runs after the same one. A sample is ``--inner`` back-to-back calls between two device events; the
figure per library is the median over the rounds. The outputs must be bit-equal. THIS_LIB defaults to the product
library of this tree; build both the same way for a like-for-like comparison (``_build.build_abi(tag=..., only=...)``
in a checkout of each commit). Prints one JSON object (and writes it to ``--out``, default
profiles/paged_varlen_parent_ab.json).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from scripts.bench_paged_decode import paged_layout, sample  # noqa: E402
from test_abi import FaFwdParams  # noqa: E402
from test_paged_abi import FaPagedParams  # noqa: E402

HEADS = dict(Hq=32, Hkv=8, D=128)
SHAPES = {"chunk512_b8_16k": dict(B=8, Sq=512, cap=16384, **HEADS), "chunk2048_b1_32k": dict(B=1, Sq=2048, cap=32768, **HEADS),
          "chunk512_b8_4k": dict(B=8, Sq=512, cap=4096, **HEADS)}
PAGE_SIZES = (64, 256)
I64, P, C = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int


def load(path):
    lib = ctypes.CDLL(str(path))
    lib.fa_fwd_gfx950_paged_prefill.argtypes = [P, C, C, I64, P, I64, P]
    lib.fa_last_error.restype = ctypes.c_char_p
    return lib


def run_case(libs, name, s, page, rounds, inner, dev):
    gen = torch.Generator().manual_seed(1)
    torch.manual_seed(1)
    bf = torch.bfloat16
    q = torch.randn(s["B"], s["Hq"], s["Sq"], s["D"], device=dev, dtype=bf)
    k = torch.randn(s["B"], s["Hkv"], s["cap"], s["D"], device=dev, dtype=bf)
    v = torch.randn(s["B"], s["Hkv"], s["cap"], s["D"], device=dev, dtype=bf)
    kc, vc, table = paged_layout(k, v, page, gen)
    del k, v
    lens = torch.full((s["B"],), s["cap"], dtype=torch.int32, device=dev)
    outs = {n: torch.empty_like(q) for n in libs}
    stream = P(torch.cuda.current_stream().cuda_stream)
    st = lambda t, i: t.stride(i) if t.size(i) > 1 else 0  # noqa: E731  (the binding's stride_or_zero)

    def params(o):
        base = FaFwdParams(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), s["B"], s["Hq"], s["Hkv"], s["Sq"],
                           s["cap"], s["D"], s["Hq"] // s["Hkv"], *(st(t, i) for i in range(3) for t in (q, kc, vc, o)),
                           s["D"] ** -0.5 * 1.4426950408889634)
        return FaPagedParams(base, table.data_ptr(), table.stride(0), table.size(1), kc.size(0), page, lens.data_ptr())

    ps = {n: params(outs[n]) for n in libs}

    def call(n):
        def f():
            rc = libs[n].fa_fwd_gfx950_paged_prefill(ctypes.byref(ps[n]), 1, 1, -1, None, 0, stream)
            assert rc == 0, libs[n].fa_last_error()
        return f

    fns = {n: call(n) for n in libs}
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    equal = all(torch.equal(outs[n], outs["parent_a"]) for n in libs)
    names, times = list(libs), {n: [] for n in libs}
    for r in range(rounds):
        for n in names[r % 3:] + names[:r % 3]:
            times[n].append(sample(fns[n], inner))
    med = {n: statistics.median(t) for n, t in times.items()}
    a = 0.5 * (med["parent_a"] + med["parent_b"])
    return dict(shape=name, page_size=page, bit_equal=equal, parent_a_ms=round(med["parent_a"], 4),
                parent_b_ms=round(med["parent_b"], 4), this_ms=round(med["this"], 4),
                aa_spread_pct=round(100 * abs(med["parent_a"] - med["parent_b"]) / a, 3),
                this_over_parent=round(med["this"] / a, 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_lib")
    ap.add_argument("this_lib", nargs="?", default=str(ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"))
    ap.add_argument("--rounds", type=int, default=45)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "paged_varlen_parent_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_paged_prefill_libs needs an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        copy = Path(tmp) / f"parent_copy_{os.getpid()}.so"
        shutil.copyfile(args.parent_lib, copy)
        libs = {"parent_a": load(args.parent_lib), "this": load(args.this_lib), "parent_b": load(copy)}
        rows = []
        for name, s in SHAPES.items():
            for page in PAGE_SIZES:
                rows.append(run_case(libs, name, s, page, args.rounds, args.inner, dev))
                torch.cuda.empty_cache()
    result = {"script": "scripts/ab_paged_prefill_libs.py", "entry": "fa_fwd_gfx950_paged_prefill", "rounds": args.rounds,
              "inner": args.inner, "dtype": "bf16", "causal": True, "pages": "shuffled", **HEADS,
              "method": "both libraries in one process through the C ABI on the same buffers; parent, this tree, parent "
                        "again (a copy), the order rotated every round; medians; A/A spread = the parent's two medians",
              "cases": rows}
    text = json.dumps(result, indent=1)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
