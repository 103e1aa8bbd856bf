#!/usr/bin/env python3
"""Compare the split-KV decode kernels of two build/obj trees (the -save-temps assembly that _build.build_abi
keeps beside every instantiation's object): a code-shape gate for refactors of the decode kernels, no GPU needed.

    python scripts/compare_decode_objs.py PARENT/build/obj build/obj [--out profiles/decode_unify_ab.json]

For each of the 5 kernels x 16 instantiations x 2 (with / without the fused merge) the gate is:
  * .vgpr_count not higher than the parent's;
  * .group_segment_fixed_size equal;
  * .private_segment_fixed_size, .sgpr_spill_count and .vgpr_spill_count all 0;
  * equal counts of v_mfma*, LDS-DMA loads (buffer_load ... lds), ds_read*, v_exp* and FP8 converts
    (v_cvt_scalef32_pk_*_fp8).
Scalar and address bookkeeping may drift: instruction totals, SGPRs and s_waitcnt counts are recorded, not gated.
With --out the result becomes the "code_shape" entry of that JSON file (its other entries are kept).
Exit status 1 when a kernel misses the gate or the two trees do not hold the same kernels.
"""
from __future__ import annotations

import argparse
import json
import re
import sys
from pathlib import Path

KERNEL = re.compile(r"^(_ZN2fa\d+(fa_decode(?:_paged|_fp8kv)?(?:_window)?)I\w+):[^\n]*\n(.*?)^\.Lfunc_end", re.S | re.M)
META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "sgpr_spill_count", "vgpr_spill_count")
COUNTED = {  # gated: the work a kernel does
    "mfma": re.compile(r"^\s+v_mfma"),
    "lds_dma": re.compile(r"^\s+buffer_load_dword\w*\s.*\blds\b"),
    "ds_read": re.compile(r"^\s+ds_read"),
    "exp": re.compile(r"^\s+v_exp"),
    "fp8_cvt": re.compile(r"^\s+v_cvt_scalef32_pk_\w+_fp8"),
}
RECORDED = {  # not gated: bookkeeping
    "instructions": re.compile(r"^\s+[a-z][a-z0-9_]+(\s|$)"),
    "waitcnt": re.compile(r"^\s+s_waitcnt"),
}
ZERO = ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")


def kernels_of(obj: Path) -> dict:
    """{"<instantiation dir>/<kernel>/<fused|plain>": {metadata and instruction counts}} of one build/obj tree."""
    out = {}
    for s in sorted(obj.glob("*/fa_*inst-hip-amdgcn-amd-amdhsa-gfx950.s")):
        text = s.read_text()
        meta = {}
        for block in text.split("  - .agpr_count:")[1:]:
            block = ".agpr_count:" + block
            name = re.search(r"\.name:\s+(\S+)", block)
            if name:
                meta[name.group(1)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in META}
        for sym, kernel, body in KERNEL.findall(text):
            fused = "fused" if re.search(r"Lb1EEEv13fa_fwd_params", sym) else "plain"  # (kFuse: the last flag)
            lines = [ln for ln in body.splitlines() if not ln.lstrip().startswith((";", "."))]
            rec = dict(meta[sym])
            for k, rx in {**COUNTED, **RECORDED}.items():
                rec[k] = sum(1 for ln in lines if rx.search(ln))
            out[f"{s.parent.name}/{kernel}/{fused}"] = rec
    return out


def compare(parent: dict, new: dict) -> tuple[list, list]:
    rows, problems = [], []
    if sorted(parent) != sorted(new):
        problems.append(f"kernel sets differ: {sorted(set(parent) ^ set(new))[:6]}")
    for key in sorted(set(parent) & set(new)):
        a, b = parent[key], new[key]
        bad = []
        if b["vgpr_count"] > a["vgpr_count"]:
            bad.append(f"vgpr_count {a['vgpr_count']} -> {b['vgpr_count']}")
        if b["group_segment_fixed_size"] != a["group_segment_fixed_size"]:
            bad.append(f"group_segment_fixed_size {a['group_segment_fixed_size']} -> {b['group_segment_fixed_size']}")
        bad += [f"{k} = {b[k]}" for k in ZERO if b[k] != 0]
        bad += [f"{k} {a[k]} -> {b[k]}" for k in COUNTED if a[k] != b[k]]
        rows.append({"kernel": key, "ok": not bad, "parent": a, "new": b})
        problems += [f"{key}: {q}" for q in bad]
    return rows, problems


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_obj", type=Path)
    ap.add_argument("new_obj", type=Path)
    ap.add_argument("--out", type=Path)
    args = ap.parse_args()
    parent, new = kernels_of(args.parent_obj), kernels_of(args.new_obj)
    rows, problems = compare(parent, new)
    drift = [r["new"]["instructions"] - r["parent"]["instructions"] for r in rows]
    vdrift = [r["new"]["vgpr_count"] - r["parent"]["vgpr_count"] for r in rows]
    summary = {"kernels": len(rows), "passed": sum(r["ok"] for r in rows), "problems": problems,
               "instruction_drift_min_max": [min(drift, default=0), max(drift, default=0)],
               "vgpr_drift_min_max": [min(vdrift, default=0), max(vdrift, default=0)]}
    print(json.dumps(summary, indent=1))
    if args.out:
        doc = json.loads(args.out.read_text()) if args.out.exists() else {}
        doc["code_shape"] = {"gate": __doc__.split("gate is:")[1].split("With --out")[0].strip().splitlines(),
                             "summary": summary, "kernels": rows}
        body = json.dumps(doc, indent=1)
        # (one kernel per line: 160 rows of nested counts stay readable and small)
        body = re.sub(r"\{\s*\"kernel\": [^\[\]]*?\"waitcnt\": \d+\s*\}\s*\}", lambda m: re.sub(r"\s+", " ", m.group(0)), body)
        args.out.write_text(body + "\n")
    return 1 if problems or not rows else 0


if __name__ == "__main__":
    sys.exit(main())
