"""The paged-decode addition to the C-ABI boundary (include/fa_gfx950_paged.h): the header declares its
four functions beside the unchanged fa_gfx950.h, both libraries export them, and the page pool / block
table description is validated with the documented codes -- host-only calls, no GPU needed."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_abi import (FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK, FaFwdParams, FaPaddedParams,
                      decode_params)

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "fa_gfx950_paged.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
PAGED = {"fa_fwd_gfx950_paged", "fa_fwd_gfx950_paged_workspace_size", "fa_fwd_gfx950_paged_check", "fa_paged_version"}


class FaPagedParams(ctypes.Structure):
    _fields_ = [("base", FaFwdParams), ("block_table", ctypes.c_void_p), ("block_table_stride", ctypes.c_int64),
                ("max_pages", ctypes.c_int64), ("num_pages", ctypes.c_int64), ("page_size", ctypes.c_int64),
                ("seqlens_k", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    lib.fa_fwd_gfx950_paged_workspace_size.restype = ctypes.c_int64
    lib.fa_fwd_gfx950_paged.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_void_p]
    return lib


def paged_params(b=32, hq=32, hkv=8, max_pages=32, page_size=128, num_pages=2048, d=128, sq=1, pack=True, **kw):
    """A decode step on a [num_pages, Hkv, page_size, D] pool, as the torch binding passes it."""
    base = decode_params(b=b, hq=hq, hkv=hkv, sk=max_pages * page_size, d=d, sq=sq, pack=pack)
    for t in "kv":
        setattr(base, f"{t}_batch_stride", hkv * page_size * d)  # the page stride
        setattr(base, f"{t}_head_stride", page_size * d)
    p = FaPagedParams(base, 0x50000, max_pages, max_pages, num_pages, page_size, 0x60000)
    for key, val in kw.items():
        if hasattr(p.base, key):
            setattr(p.base, key, val)
        else:
            setattr(p, key, val)
    return p


def check(lib, p, dtype=1, causal=0):
    rc = lib.fa_fwd_gfx950_paged_check(ctypes.byref(p), dtype, causal)
    return rc, lib.fa_last_error().decode()


def test_paged_header_declares_its_four_functions_and_leaves_the_old_header_alone():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == PAGED
    assert '#include "fa_gfx950.h"' in text and re.search(r"#define FA_GFX950_PAGED_VERSION 1\b", text)
    import test_abi

    test_abi.test_header_declares_the_boundary()  # include/fa_gfx950.h: the same set as before
    assert "paged" not in (ROOT / "include" / "fa_gfx950.h").read_text()


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_paged_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert PAGED <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_paged_version_and_abi_version(lib):
    assert lib.fa_paged_version() == 1
    assert lib.fa_abi_version() == 8  # the dense boundary did not move


def test_paged_struct_layout():
    assert ctypes.sizeof(FaPagedParams) == ctypes.sizeof(FaFwdParams) + 6 * 8
    base = ctypes.sizeof(FaFwdParams)
    offsets = [getattr(FaPagedParams, n).offset for n in ("block_table", "block_table_stride", "max_pages",
                                                          "num_pages", "page_size", "seqlens_k")]
    assert offsets == [base + 8 * i for i in range(6)]


def test_paged_check_accepts_valid(lib):
    assert check(lib, paged_params()) == (FA_OK, "")
    assert check(lib, paged_params(page_size=32, max_pages=128), dtype=0)[0] == FA_OK
    # unpacked GQA with a few positions, causal: 4 heads x 16 positions = 64 rows, the last decode shape
    assert check(lib, paged_params(sq=16, pack=False), causal=1)[0] == FA_OK
    # flash-attn's [num_pages, page_size, Hkv, D] pool: a transposed view, row stride Hkv * D
    assert check(lib, paged_params(k_head_stride=128, v_head_stride=128, k_seqlen_stride=8 * 128,
                                   v_seqlen_stride=8 * 128))[0] == FA_OK


@pytest.mark.parametrize("kw,code,msg", [
    ({"page_size": 48}, FA_ERR_INVALID_ARGUMENT, "multiple of 32"),
    ({"page_size": 0}, FA_ERR_INVALID_ARGUMENT, "multiple of 32"),
    ({"block_table": None}, FA_ERR_INVALID_ARGUMENT, "non-NULL"),
    ({"block_table": 0x50002}, FA_ERR_INVALID_ARGUMENT, "4-byte aligned"),
    ({"seqlens_k": None}, FA_ERR_INVALID_ARGUMENT, "non-NULL"),
    ({"seqlens_k": 0x60002}, FA_ERR_INVALID_ARGUMENT, "4-byte aligned"),
    ({"num_pages": 0}, FA_ERR_INVALID_ARGUMENT, "at least 1"),
    ({"max_pages": 0}, FA_ERR_INVALID_ARGUMENT, "at least 1"),
    ({"seqlen_kv": 4096 + 32}, FA_ERR_INVALID_ARGUMENT, "max_pages * page_size"),
    ({"block_table_stride": 16}, FA_ERR_INVALID_ARGUMENT, "block_table_stride"),
    ({"k_seqlen_stride": 132}, FA_ERR_INVALID_ARGUMENT, "multiples of 8"),
    ({"v_batch_stride": 8 * 128 * 128 + 4}, FA_ERR_INVALID_ARGUMENT, "multiples of 8"),
    ({"headdim": 136}, FA_ERR_UNSUPPORTED, "<= 128"),
    ({"softmax_scale": 0.0}, FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    ({"softmax_scale": -0.1275}, FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    ({"softmax_scale": float("inf")}, FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
    ({"softmax_scale": float("nan")}, FA_ERR_INVALID_ARGUMENT, "softmax_scale"),
])
def test_paged_check_and_launch_reject_without_touching_the_device(lib, kw, code, msg):
    p = paged_params(**kw)
    rc, err = check(lib, p)
    assert rc == code and msg in err, err
    # the launch entry validates first: NULL stream, bogus pointers, nothing is launched
    assert lib.fa_fwd_gfx950_paged(ctypes.byref(p), 1, 0, None, 0, None) == code
    assert lib.fa_fwd_gfx950_paged_workspace_size(ctypes.byref(p), 1, 0) == -1


def test_paged_serves_decode_shapes_only(lib):
    p = paged_params(sq=17, pack=False)  # 4 heads x 17 positions = 68 rows
    rc, err = check(lib, p, causal=1)
    assert rc == FA_ERR_UNSUPPORTED and "decode rule" in err and "head_q_per_group * seqlen_q" in err
    assert lib.fa_fwd_gfx950_paged(ctypes.byref(p), 1, 1, None, 0, None) == FA_ERR_UNSUPPORTED
    # one row past the rule (fa_launch.h decode_rule, shared with the dense dispatcher): 5 heads x 13 = 65
    rc, err = check(lib, paged_params(hq=40, sq=13, pack=False))
    assert rc == FA_ERR_UNSUPPORTED and "decode shapes only" in err and "got 65" in err
    assert check(lib, paged_params(hq=32, sq=16, pack=False))[0] == FA_OK  # 64 rows
    assert lib.fa_fwd_gfx950_paged_check(None, 1, 0) == FA_ERR_INVALID_ARGUMENT
    from flash_attention_cute_amd import _debug

    with _debug.knobs(decode=False):  # the decode knob off: no kernel for it, and no silent other path
        rc, err = check(lib, paged_params())
        assert rc == FA_ERR_UNSUPPORTED and "decode" in err
    assert check(lib, paged_params())[0] == FA_OK


def test_paged_workspace_is_the_padded_decode_workspace(lib):
    lib.fa_fwd_gfx950_padded_workspace_size.restype = ctypes.c_int64
    lib.fa_fwd_gfx950_padded_workspace_size.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64]

    def both(b, max_pages, page_size):
        paged = paged_params(b=b, max_pages=max_pages, page_size=page_size)
        dense = FaPaddedParams(decode_params(b=b, sk=max_pages * page_size), None, None, 0x50000, 0x50100)
        return (lib.fa_fwd_gfx950_paged_workspace_size(ctypes.byref(paged), 1, 0),
                lib.fa_fwd_gfx950_padded_workspace_size(ctypes.byref(dense), 1, 0, -1))

    n, dense = both(1, 256, 128)  # B1 Hkv8, 32768 keys: split
    assert n == dense and n > 0
    assert both(1, 2, 128) == (0, 0)  # 256 keys: every wave keeps its 4 tiles, no split
    assert both(32, 32, 128) == (0, 0)  # 256 row blocks fill the chip
    # a too-small or misaligned workspace is an error; NULL means unsplit and passes validation
    p = paged_params(b=1, max_pages=256, page_size=128, headdim=136)
    assert lib.fa_fwd_gfx950_paged(ctypes.byref(p), 1, 0, None, 0, None) == FA_ERR_UNSUPPORTED
    p = paged_params(b=1, max_pages=256, page_size=128)
    rc = lib.fa_fwd_gfx950_paged(ctypes.byref(p), 1, 0, ctypes.c_void_p(0x100000), ctypes.c_int64(n - 16), None)
    assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()
    rc = lib.fa_fwd_gfx950_paged(ctypes.byref(p), 1, 0, ctypes.c_void_p(0x100008), ctypes.c_int64(n), None)
    assert rc == FA_ERR_INVALID_ARGUMENT and b"aligned" in lib.fa_last_error()


def test_debug_names_of_the_paged_paths():
    from flash_attention_cute_amd import _debug

    assert _debug.PATHS[9] == "decode_paged" and _debug.PATHS[10] == "decode_paged_split"
    text = (ROOT / "flash_attention_cute_amd" / "csrc" / "fa_launch.h").read_text()
    assert "kPathDecodePaged = 9" in text and "kPathDecodePagedSplit = 10" in text


def test_paged_asm_gate_passes_on_the_built_instantiations():
    """One paged translation unit per dense one, in directories of their own (the 16 fa_inst files that
    test_abi counts stay 16), and the build's assembly gate -- no VGPR spills -- holds on them."""
    from flash_attention_cute_amd import _asm_check as A
    from flash_attention_cute_amd import _build

    obj = _build.ROOT / "build" / "obj"
    files = sorted(obj.glob("paged_*/fa_paged_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not files:
        pytest.skip("no -save-temps assembly (library built elsewhere)")
    assert len(files) == len(_build.INSTANCES)
    assert len(list(obj.glob("*/fa_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))) == len(_build.INSTANCES)
    for f in files:
        text = f.read_text()
        assert A.check_file(f) == [], f
        assert "fa_fwd_w4" not in text
        kernels = re.findall(r"^(_ZN2fa15fa_decode_paged\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M)
        assert len(kernels) == 2, f  # with and without the fused merge
        for name, body in kernels:
            # the page id is a scalar load: a vector load in the key loop would count against the vmcnt
            # that the loop's waits are written for. Up to the last LDS-DMA issue, every vector load from
            # memory is an LDS-DMA (the merges' loads come after the loop).
            lines = body.splitlines()
            dma = [i for i, ln in enumerate(lines) if "buffer_load_dwordx4" in ln and " lds" in ln]
            assert dma, name
            loads = [ln for ln in lines[:dma[-1]] if re.search(r"\b(global|flat|buffer)_load_", ln) and " lds" not in ln]
            assert loads == [], (name, loads[:3])
            assert any(re.search(r"\bs_load_dword\b", ln) for ln in lines), name


def test_paged_host_validation_under_asan_ubsan(tmp_path):
    """The paged dispatcher's host code (csrc/fa_paged_gfx950.hip, with csrc/fa_fwd_gfx950.hip for the
    error channel and knobs) built with AddressSanitizer + UBSan on the host side only and linked with
    host-only stub instantiations, run as a stand-alone program (tests/asan/paged_validation_driver.cpp)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    csrc = ROOT / "flash_attention_cute_amd" / "csrc"
    inc = [f"-I{ROOT / 'include'}", f"-I{csrc}"]
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined"]
    base = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fPIC", *san, *inc, "-c"]
    objs = []
    for src in (csrc / "fa_fwd_gfx950.hip", csrc / "fa_paged_gfx950.hip", ROOT / "tests" / "asan" / "stub_instances.hip",
                ROOT / "tests" / "asan" / "paged_stub_instances.hip",
                ROOT / "tests" / "asan" / "paged_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "paged_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "paged validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
