"""The FP8 KV-cache addition to the C-ABI boundary (include/fa_gfx950_fp8.h): the header declares its
functions beside the three unchanged headers, both libraries export them, the structs have the header's
layout and the descriptions are validated with the documented codes -- host-only calls, no GPU needed."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK
from test_kvcache_abi import kv_params, params_type
from test_paged_abi import FaPagedParams, paged_params

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "fa_gfx950_fp8.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
FP8 = {"fa_fwd_gfx950_paged_fp8", "fa_fwd_gfx950_paged_fp8_workspace_size", "fa_fwd_gfx950_paged_fp8_check",
       "fa_kvcache_append_fp8_gfx950", "fa_kvcache_append_fp8_gfx950_check", "fa_fp8_version"}
_TAIL = [("k_descale", ctypes.c_void_p), ("v_descale", ctypes.c_void_p), ("descale_batch_stride", ctypes.c_int64),
         ("descale_head_stride", ctypes.c_int64)]


class FaPagedFp8Params(ctypes.Structure):
    _fields_ = [("paged", FaPagedParams)] + _TAIL


def kvcache_fp8_type():
    class FaKvcacheFp8Params(ctypes.Structure):
        _fields_ = [("base", params_type())] + _TAIL

    return FaKvcacheFp8Params


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    for name in ("fa_fwd_gfx950_paged_fp8_workspace_size", "fa_fwd_gfx950_paged_workspace_size"):
        getattr(lib, name).restype = ctypes.c_int64
    lib.fa_fwd_gfx950_paged_fp8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_int64, ctypes.c_void_p]
    lib.fa_kvcache_append_fp8_gfx950.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return lib


def fp8_params(descales=True, **kw):
    """test_paged_abi.paged_params' decode step on a byte pool (the element strides are the same numbers)."""
    tail = {k: kw.pop(k) for k in list(kw) if k in ("k_descale", "v_descale", "descale_batch_stride",
                                                    "descale_head_stride")}
    p = FaPagedFp8Params(paged_params(**kw), 0x70000 if descales else None, 0x71000 if descales else None, 8, 1)
    for key, val in tail.items():
        setattr(p, key, val)
    return p


def kv_fp8_params(**kw):
    tail = {k: kw.pop(k) for k in list(kw) if k in ("k_descale", "v_descale", "descale_batch_stride",
                                                    "descale_head_stride")}
    p = kvcache_fp8_type()(kv_params(**kw), 0xa0000, 0xa1000, 8, 1)
    for key, val in tail.items():
        setattr(p, key, val)
    return p


def check(lib, p, dtype=1, causal=0):
    rc = lib.fa_fwd_gfx950_paged_fp8_check(ctypes.byref(p), dtype, causal)
    return rc, lib.fa_last_error().decode()


def kv_check(lib, p, dtype=1):
    rc = lib.fa_kvcache_append_fp8_gfx950_check(ctypes.byref(p), dtype)
    return rc, lib.fa_last_error().decode()


def test_fp8_header_declares_its_functions_and_leaves_the_old_headers_alone():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == FP8
    assert '#include "fa_gfx950.h"' in text and re.search(r"#define FA_GFX950_FP8_VERSION 1\b", text)
    for old in ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h"):
        assert "fp8" not in (ROOT / "include" / old).read_text().lower(), old
    import test_abi
    import test_kvcache_abi
    import test_paged_abi

    test_abi.test_header_declares_the_boundary()
    test_paged_abi.test_paged_header_declares_its_four_functions_and_leaves_the_old_header_alone()
    test_kvcache_abi.test_kvcache_header_declares_its_functions_and_leaves_the_old_headers_alone()


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_fp8_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert FP8 <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_fp8_version_and_the_other_versions(lib):
    assert lib.fa_fp8_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.fp8_version() == 1


def test_fp8_struct_layouts():
    for outer, inner in ((FaPagedFp8Params, FaPagedParams), (kvcache_fp8_type(), params_type())):
        base = ctypes.sizeof(inner)
        assert ctypes.sizeof(outer) == base + 4 * 8
        assert [getattr(outer, n).offset for n, _ in _TAIL] == [base + 8 * i for i in range(4)]
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, first in (("fa_paged_fp8_params", "fa_paged_params paged;"), ("fa_kvcache_fp8_params", "fa_kvcache_params base;")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        body = " ".join(body.split())
        assert body == (f"{first} const float *k_descale; const float *v_descale; "
                        "int64_t descale_batch_stride, descale_head_stride;"), body


def test_fp8_paged_check_accepts_valid(lib):
    assert check(lib, fp8_params()) == (FA_OK, "")
    assert check(lib, fp8_params(descales=False, descale_batch_stride=0, descale_head_stride=0), dtype=0)[0] == FA_OK
    assert check(lib, fp8_params(page_size=32, max_pages=128), dtype=0)[0] == FA_OK
    assert check(lib, fp8_params(sq=16, pack=False), causal=1)[0] == FA_OK  # 64 rows: the last decode shape
    assert check(lib, fp8_params(d=96))[0] == FA_OK and check(lib, fp8_params(d=16))[0] == FA_OK
    # flash-attn's [num_pages, page_size, Hkv, D] pool: a transposed view, row stride Hkv * D
    assert check(lib, fp8_params(k_head_stride=128, v_head_stride=128, k_seqlen_stride=8 * 128,
                                 v_seqlen_stride=8 * 128))[0] == FA_OK
    # stride-0 descales: the per-tensor case
    assert check(lib, fp8_params(descale_batch_stride=0, descale_head_stride=0))[0] == FA_OK


@pytest.mark.parametrize("kw,code,msg", [
    ({"d": 72}, FA_ERR_INVALID_ARGUMENT, "multiple of 16"),
    ({"d": 8}, FA_ERR_INVALID_ARGUMENT, "multiple of 16"),
    ({"headdim": 144}, FA_ERR_UNSUPPORTED, "<= 128"),
    ({"k_ptr": 0x20008}, FA_ERR_INVALID_ARGUMENT, "16-byte aligned"),
    ({"v_ptr": 0x30004}, FA_ERR_INVALID_ARGUMENT, "16-byte aligned"),
    ({"k_seqlen_stride": 136}, FA_ERR_INVALID_ARGUMENT, "multiples of 16"),
    ({"v_head_stride": 128 * 128 + 8}, FA_ERR_INVALID_ARGUMENT, "multiples of 16"),
    ({"v_batch_stride": 8 * 128 * 128 + 8}, FA_ERR_INVALID_ARGUMENT, "multiples of 16"),
    ({"page_size": 48}, FA_ERR_INVALID_ARGUMENT, "multiple of 32"),
    ({"page_size": 16}, FA_ERR_INVALID_ARGUMENT, "multiple of 32"),
    ({"block_table": None}, FA_ERR_INVALID_ARGUMENT, "non-NULL"),
    ({"seqlens_k": 0x60002}, FA_ERR_INVALID_ARGUMENT, "4-byte aligned"),
    ({"num_pages": 0}, FA_ERR_INVALID_ARGUMENT, "at least 1"),
    ({"seqlen_kv": 4096 + 32}, FA_ERR_INVALID_ARGUMENT, "max_pages * page_size"),
    ({"descale_batch_stride": -1}, FA_ERR_INVALID_ARGUMENT, "descale strides"),
    ({"k_descale": 0x70002}, FA_ERR_INVALID_ARGUMENT, "4-byte aligned"),
    ({"softmax_scale": 0.0}, FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    ({"softmax_scale": -0.1275}, FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    ({"softmax_scale": float("inf")}, FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    ({"softmax_scale": float("nan")}, FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
])
def test_fp8_paged_check_and_launch_reject_without_touching_the_device(lib, kw, code, msg):
    p = fp8_params(**kw)
    rc, err = check(lib, p)
    assert rc == code and msg in err, err
    # the launch entry validates first: NULL stream, bogus pointers, nothing is launched
    assert lib.fa_fwd_gfx950_paged_fp8(ctypes.byref(p), 1, 0, None, 0, None) == code
    assert lib.fa_fwd_gfx950_paged_fp8_workspace_size(ctypes.byref(p), 1, 0) == -1


def test_fp8_paged_serves_decode_shapes_only(lib):
    p = fp8_params(sq=17, pack=False)  # 4 heads x 17 positions = 68 rows
    rc, err = check(lib, p, causal=1)
    assert rc == FA_ERR_UNSUPPORTED and "decode rule" in err and "head_q_per_group * seqlen_q" in err
    assert lib.fa_fwd_gfx950_paged_fp8(ctypes.byref(p), 1, 1, None, 0, None) == FA_ERR_UNSUPPORTED
    assert check(lib, fp8_params(hq=40, sq=13, pack=False))[0] == FA_ERR_UNSUPPORTED  # 65 rows
    assert check(lib, fp8_params(hq=32, sq=16, pack=False))[0] == FA_OK  # 64 rows
    assert lib.fa_fwd_gfx950_paged_fp8_check(None, 1, 0) == FA_ERR_INVALID_ARGUMENT


def fp8_plan_workspace(b, hkv, rows, keys, d, target=256):
    """The rule the FP8 dispatcher states: decode_plan's arithmetic (32-key tiles, 4 waves with at least 4
    tiles each, at most 64 splits) aiming at 256 workgroups, one per CU, instead of the 16-bit decode's 160;
    the workspace is units * n_split * 32 fp32 rows of the head-dim tile plus one fp32 each."""
    units = b * hkv * ((rows + 31) // 32)
    n_tiles = (keys + 31) // 32
    ns = max(1, min((target + units - 1) // units, n_tiles // 16, 64))
    tps = (n_tiles + ns - 1) // ns
    n_split = (n_tiles + tps - 1) // tps
    return 0 if n_split <= 1 else units * n_split * 32 * ((64 if d <= 64 else 128) * 4 + 4)


def test_fp8_workspace_follows_the_stated_plan(lib):
    """Where the workgroup target does not bind -- no split, or the length limits the splits -- the plan and
    the workspace are the 16-bit paged decode's; where it binds, the FP8 plan aims at 256 workgroups."""
    same = 0
    for b, max_pages, page_size in ((1, 256, 128), (1, 2, 128), (32, 32, 128), (2, 64, 32), (4, 16, 256), (1, 1024, 128)):
        for d in (64, 96, 128):
            p = fp8_params(b=b, max_pages=max_pages, page_size=page_size, d=d)
            n = lib.fa_fwd_gfx950_paged_fp8_workspace_size(ctypes.byref(p), 1, 0)
            assert n == fp8_plan_workspace(b, 8, 4, max_pages * page_size, d), (b, max_pages, page_size, d)
            n16 = lib.fa_fwd_gfx950_paged_workspace_size(ctypes.byref(p.paged), 1, 0)
            assert n16 == fp8_plan_workspace(b, 8, 4, max_pages * page_size, d, target=160)
            same += n == n16
    assert 0 < same < 18
    p = fp8_params(b=1, max_pages=256, page_size=128)
    n = lib.fa_fwd_gfx950_paged_fp8_workspace_size(ctypes.byref(p), 1, 0)
    assert n > 0
    # a too-small or misaligned workspace is an error; NULL means unsplit and passes validation
    rc = lib.fa_fwd_gfx950_paged_fp8(ctypes.byref(p), 1, 0, ctypes.c_void_p(0x100000), ctypes.c_int64(n - 16), None)
    assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()
    rc = lib.fa_fwd_gfx950_paged_fp8(ctypes.byref(p), 1, 0, ctypes.c_void_p(0x100008), ctypes.c_int64(n), None)
    assert rc == FA_ERR_INVALID_ARGUMENT and b"aligned" in lib.fa_last_error()


def test_fp8_append_check_accepts_valid(lib):
    assert kv_check(lib, kv_fp8_params()) == (FA_OK, "")
    assert kv_check(lib, kv_fp8_params(d=96, sn=3), dtype=0)[0] == FA_OK
    assert kv_check(lib, kv_fp8_params(pshd=True))[0] == FA_OK
    assert kv_check(lib, kv_fp8_params(dense=True, page_size=1000, d=64))[0] == FA_OK  # a dense cache: any length
    assert kv_check(lib, kv_fp8_params(rope=False, sq=0))[0] == FA_OK
    assert kv_check(lib, kv_fp8_params(k_descale=None, v_descale=None))[0] == FA_OK


@pytest.mark.parametrize("kw,code,msg", [
    ({"d": 72}, FA_ERR_INVALID_ARGUMENT, "multiple of 16"),
    ({"d": 144}, FA_ERR_UNSUPPORTED, "<= 128"),
    ({"k_cache": 0x100008}, FA_ERR_INVALID_ARGUMENT, "16-byte aligned"),
    ({"v_row_stride": 136}, FA_ERR_INVALID_ARGUMENT, "multiples of 16"),
    ({"k_page_stride": 8 * 128 * 128 + 8}, FA_ERR_INVALID_ARGUMENT, "multiples of 16"),
    ({"page_size": 48}, FA_ERR_INVALID_ARGUMENT, "multiple of 32"),
    ({"seqlens_out": 0x80004}, FA_ERR_INVALID_ARGUMENT, "overlap"),
    ({"seqlens_out": 0x80000}, FA_ERR_INVALID_ARGUMENT, "overlap"),
    ({"kn_seqlen_stride": 132}, FA_ERR_INVALID_ARGUMENT, "k_new / v_new"),
    ({"q": 0x30008}, FA_ERR_INVALID_ARGUMENT, "q / q_out"),
    ({"cs_row_stride": 132}, FA_ERR_INVALID_ARGUMENT, "cos / sin"),
    ({"descale_head_stride": -1}, FA_ERR_INVALID_ARGUMENT, "descale strides"),
    ({"v_descale": 0xa1002}, FA_ERR_INVALID_ARGUMENT, "4-byte aligned"),
])
def test_fp8_append_check_and_launch_reject_without_touching_the_device(lib, kw, code, msg):
    p = kv_fp8_params(**kw)
    rc, err = kv_check(lib, p)
    assert rc == code and msg in err, err
    assert lib.fa_kvcache_append_fp8_gfx950(ctypes.byref(p), 1, None) == code
    assert lib.fa_kvcache_append_fp8_gfx950_check(None, 1) == FA_ERR_INVALID_ARGUMENT


def test_debug_names_of_the_fp8_paths():
    from flash_attention_cute_amd import _debug

    assert _debug.PATHS[11] == "decode_paged_fp8" and _debug.PATHS[12] == "decode_paged_fp8_split"
    text = (ROOT / "flash_attention_cute_amd" / "csrc" / "fa_paged_launch.h").read_text()
    assert "kPathDecodePagedFp8 = 11" in text and "kPathDecodePagedFp8Split = 12" in text


def test_fp8_asm_gate_passes_on_the_built_instantiations():
    """One FP8 translation unit per dense one, in directories that neither the dense nor the paged count
    matches, and the build's assembly gate -- no VGPR spills -- holds on them; the page id, the lengths and
    the descales are scalar loads (a vector load ahead of the key loop's last LDS-DMA would count against
    the vmcnt that the loop's waits are written for) and V is read by the 8-bit transposed LDS read."""
    from flash_attention_cute_amd import _asm_check as A
    from flash_attention_cute_amd import _build

    obj = _build.ROOT / "build" / "obj"
    files = sorted(obj.glob("fp8_*/fa_paged_fp8_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not files:
        pytest.skip("no -save-temps assembly (library built elsewhere)")
    assert len(files) == len(_build.INSTANCES)
    assert len(list(obj.glob("*/fa_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))) == len(_build.INSTANCES)
    assert len(list(obj.glob("paged_*/fa_paged_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))) == len(_build.INSTANCES)
    for f in files:
        text = f.read_text()
        assert A.check_file(f) == [], f
        assert "fa_fwd_w4" not in text and "fa_decode_paged" not in text
        kernels = re.findall(r"^(_ZN2fa15fa_decode_fp8kv\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M)
        assert len(kernels) == 2, f  # with and without the fused merge
        for name, body in kernels:
            lines = body.splitlines()
            dma = [i for i, ln in enumerate(lines) if "buffer_load_dwordx4" in ln and " lds" in ln]
            assert dma, name
            loads = [ln for ln in lines[:dma[-1]] if re.search(r"\b(global|flat|buffer)_load_", ln) and " lds" not in ln]
            assert loads == [], (name, loads[:3])
            assert any(re.search(r"\bs_load_dword\b", ln) for ln in lines), name
            assert any("ds_read_b64_tr_b8" in ln for ln in lines), name
            assert any(re.search(r"v_cvt_scalef32_pk_(f16|bf16)_fp8", ln) for ln in lines), name


def test_fp8_host_validation_under_asan_ubsan(tmp_path):
    """The FP8 entries' and the quantizing append's host code (csrc/fa_paged_gfx950.hip,
    csrc/fa_kvcache_fp8.hip, with the 16-bit dispatchers they validate through) built with AddressSanitizer
    + UBSan on the host side only and linked with host-only stub instantiations, run as a stand-alone
    program (tests/asan/fp8_validation_driver.cpp)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    csrc = ROOT / "flash_attention_cute_amd" / "csrc"
    asan = ROOT / "tests" / "asan"
    inc = [f"-I{ROOT / 'include'}", f"-I{csrc}"]
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined"]
    base = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fPIC", *san, *inc, "-c"]
    objs = []
    for src in (csrc / "fa_fwd_gfx950.hip", csrc / "fa_paged_gfx950.hip", csrc / "fa_kvcache.hip",
                csrc / "fa_kvcache_fp8.hip", asan / "stub_instances.hip", asan / "paged_stub_instances.hip",
                asan / "fp8_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "fp8_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "fp8 validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
