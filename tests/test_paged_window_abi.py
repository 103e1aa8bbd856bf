"""The sliding-window addition to the C-ABI boundary (include/fa_gfx950_paged_window.h): the header declares
its seven functions beside the four unchanged headers, both libraries export them, validation is the
unwindowed entries' for every window, and the workspace follows the window's split plan -- host-only calls,
no GPU needed."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK
from test_fp8_abi import fp8_params, fp8_plan_workspace
from test_paged_abi import paged_params

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "fa_gfx950_paged_window.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
WINDOW = {"fa_fwd_gfx950_paged_window", "fa_fwd_gfx950_paged_window_workspace_size", "fa_fwd_gfx950_paged_window_check",
          "fa_fwd_gfx950_paged_window_fp8", "fa_fwd_gfx950_paged_window_fp8_workspace_size",
          "fa_fwd_gfx950_paged_window_fp8_check", "fa_paged_window_version"}
OLD_HEADERS = ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h", "fa_gfx950_fp8.h")
WINDOWS = (-1, 0, 31, 2 ** 40)
I64 = ctypes.c_int64


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    for name in ("fa_fwd_gfx950_paged_workspace_size", "fa_fwd_gfx950_paged_fp8_workspace_size"):
        getattr(lib, name).restype = I64
    for name in ("fa_fwd_gfx950_paged_window", "fa_fwd_gfx950_paged_window_fp8"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64, ctypes.c_void_p, I64,
                                       ctypes.c_void_p]
        getattr(lib, name + "_workspace_size").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64]
        getattr(lib, name + "_workspace_size").restype = I64
        getattr(lib, name + "_check").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64]
    return lib


# (entry stem, unwindowed stem, parameter factory)
KINDS = {"16bit": ("fa_fwd_gfx950_paged_window", "fa_fwd_gfx950_paged", paged_params),
         "fp8": ("fa_fwd_gfx950_paged_window_fp8", "fa_fwd_gfx950_paged_fp8", fp8_params)}


def test_window_header_declares_its_functions_and_leaves_the_old_headers_alone():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == WINDOW
    assert re.search(r"#define FA_GFX950_PAGED_WINDOW_VERSION 1\b", text)
    assert '#include "fa_gfx950_paged.h"' in text and '#include "fa_gfx950_fp8.h"' in text
    for old in OLD_HEADERS:  # none of them knows about this one
        assert "paged_window" not in (ROOT / "include" / old).read_text().lower(), old
    import test_abi
    import test_fp8_abi
    import test_kvcache_abi
    import test_paged_abi

    test_abi.test_header_declares_the_boundary()
    test_paged_abi.test_paged_header_declares_its_four_functions_and_leaves_the_old_header_alone()
    test_kvcache_abi.test_kvcache_header_declares_its_functions_and_leaves_the_old_headers_alone()
    test_fp8_abi.test_fp8_header_declares_its_functions_and_leaves_the_old_headers_alone()


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_window_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert WINDOW <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_window_version_and_the_other_versions(lib):
    assert lib.fa_paged_window_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    assert lib.fa_fp8_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.paged_window_version() == 1


ACCEPTED = [{}, {"page_size": 32, "max_pages": 128}, {"sq": 16, "pack": False},
            {"k_head_stride": 128, "v_head_stride": 128, "k_seqlen_stride": 8 * 128, "v_seqlen_stride": 8 * 128}]
BAD_SCALES = [{"softmax_scale": s} for s in (0.0, -0.1275, float("inf"), float("nan"))]  # finite and > 0 only
REJECTED = [{"page_size": 48}, {"page_size": 0}, {"block_table": None}, {"seqlens_k": 0x60002}, {"num_pages": 0},
            {"max_pages": 0}, {"seqlen_kv": 4096 + 32}, {"block_table_stride": 16}, {"k_seqlen_stride": 132},
            {"headdim": 136}, {"sq": 17, "pack": False}, {"hq": 40, "sq": 13, "pack": False}] + BAD_SCALES



@pytest.mark.parametrize("kind", list(KINDS))
def test_window_checks_are_the_unwindowed_checks_for_every_window(lib, kind):
    stem, plain, make = KINDS[kind]
    check, plain_check = getattr(lib, stem + "_check"), getattr(lib, plain + "_check")
    for kw in ACCEPTED + REJECTED:
        for dtype, causal in ((1, 0), (0, 1)):
            p = make(**kw)
            want = plain_check(ctypes.byref(p), dtype, causal)
            want_err = lib.fa_last_error()
            assert (want == FA_OK) == (kw in ACCEPTED), kw
            for w in WINDOWS:
                assert check(ctypes.byref(p), dtype, causal, w) == want, (kw, w)
                assert lib.fa_last_error() == want_err
                if want != FA_OK:  # the launch and sizing entries validate first: nothing is launched
                    assert getattr(lib, stem)(ctypes.byref(p), dtype, causal, w, None, 0, None) == want
                    assert getattr(lib, stem + "_workspace_size")(ctypes.byref(p), dtype, causal, w) == -1
    assert check(None, 1, 0, 5) == FA_ERR_INVALID_ARGUMENT
    assert {plain_check(ctypes.byref(make(**kw)), 1, 0) for kw in REJECTED} == {FA_ERR_INVALID_ARGUMENT,
                                                                               FA_ERR_UNSUPPORTED}


@pytest.mark.parametrize("kind", list(KINDS))
def test_window_entries_name_the_scale_they_reject(lib, kind):
    stem, _, make = KINDS[kind]
    for kw in BAD_SCALES:
        p = make(**kw)
        for w in WINDOWS:
            assert getattr(lib, stem + "_check")(ctypes.byref(make()), 1, 0, w) == FA_OK  # (clears the message)
            assert getattr(lib, stem + "_check")(ctypes.byref(p), 1, 0, w) == FA_ERR_INVALID_ARGUMENT
            assert b"softmax_scale" in lib.fa_last_error()
            assert getattr(lib, stem)(ctypes.byref(p), 1, 0, w, None, 0, None) == FA_ERR_INVALID_ARGUMENT


def window_plan_keys(cap, sq, w):
    """Keys the header states the plan is made for: the most tiles a window can intersect, at most the capacity."""
    return cap if w < 0 else min(cap, 32 * ((min(w, 2 ** 30) + sq + 31) // 32 + 1))


def plan_workspace(b, hkv, rows, keys, d, target):
    return fp8_plan_workspace(b, hkv, rows, keys, d, target=target)  # (decode_plan's arithmetic, any target)


@pytest.mark.parametrize("kind", list(KINDS))
def test_window_workspace_follows_the_window_plan(lib, kind):
    stem, plain, make = KINDS[kind]
    size, plain_size = getattr(lib, stem + "_workspace_size"), getattr(lib, plain + "_workspace_size")
    target = 160 if kind == "16bit" else 256
    smaller = 0
    for b, max_pages, page_size in ((1, 256, 128), (1, 1024, 128), (2, 64, 32), (4, 16, 256), (32, 32, 128), (1, 2, 128)):
        cap = max_pages * page_size
        for d in (64, 128):
            p = make(b=b, max_pages=max_pages, page_size=page_size, d=d)
            full = plain_size(ctypes.byref(p), 1, 0)
            assert full == plan_workspace(b, 8, 4, cap, d, target)
            for w in (-1, cap, cap + 7, 2 ** 40):  # no window, or one that covers the capacity: today's plan
                assert size(ctypes.byref(p), 1, 0, w) == full, (b, cap, d, w)
            for w in (0, 31, 255, 511, 2047, 4095, cap - 200):
                n = size(ctypes.byref(p), 1, 0, w)
                # (the packed decode step of paged_params: seqlen_q = 4 rows of one kv-head)
                assert n == plan_workspace(b, 8, 4, window_plan_keys(cap, 4, w), d, target), (b, cap, d, w)
                assert 0 <= n <= full
                smaller += n < full
    assert smaller > 0
    # capacity 131072, window_left 255: 10 tiles, every wave keeps its 4: no split, no workspace
    p = make(b=1, max_pages=1024, page_size=128)
    assert plain_size(ctypes.byref(p), 1, 0) > 0 and size(ctypes.byref(p), 1, 0, 255) == 0
    # a too-small or misaligned workspace is an error, as for the unwindowed entries
    n = size(ctypes.byref(p), 1, 0, 4095)
    assert 0 < n < plain_size(ctypes.byref(p), 1, 0)
    launch = getattr(lib, stem)
    rc = launch(ctypes.byref(p), 1, 0, 4095, ctypes.c_void_p(0x100000), n - 16, None)
    assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()
    rc = launch(ctypes.byref(p), 1, 0, 4095, ctypes.c_void_p(0x100008), n, None)
    assert rc == FA_ERR_INVALID_ARGUMENT and b"aligned" in lib.fa_last_error()


def test_window_asm_gate_passes_on_the_built_instantiations():
    """The windowed kernels are translation units of their own, in directories that none of the counts of the
    dense, paged and FP8 tests match; the build's assembly gate -- no VGPR spills -- holds on them, and the window
    arithmetic added no vector load to the key loop (up to the last LDS-DMA issue every vector load from memory is
    an LDS-DMA; the page id, the length and window_left are scalar loads)."""
    from flash_attention_cute_amd import _asm_check as A
    from flash_attention_cute_amd import _build

    obj = _build.ROOT / "build" / "obj"
    kinds = (("win_*/fa_paged_window_inst", r"_ZN2fa22fa_decode_paged_window\w+"),
             ("win8_*/fa_paged_fp8_window_inst", r"_ZN2fa22fa_decode_fp8kv_window\w+"))
    if not list(obj.glob(kinds[0][0] + "-hip-amdgcn-amd-amdhsa-gfx950.s")):
        pytest.skip("no -save-temps assembly (library built elsewhere)")
    for pattern, kernel in kinds:
        files = sorted(obj.glob(pattern + "-hip-amdgcn-amd-amdhsa-gfx950.s"))
        assert len(files) == len(_build.INSTANCES)
        for f in files:
            text = f.read_text()
            assert A.check_file(f) == [], f
            assert "fa_fwd_w4" not in text
            kernels = re.findall(r"^(%s):[^\n]*\n(.*?)^\.Lfunc_end" % kernel, text, flags=re.S | re.M)
            assert len(kernels) == 2, f  # with and without the fused merge
            for name, body in kernels:
                lines = body.splitlines()
                dma = [i for i, ln in enumerate(lines) if "buffer_load_dwordx4" in ln and " lds" in ln]
                assert dma, name
                loads = [ln for ln in lines[:dma[-1]]
                         if re.search(r"\b(global|flat|buffer)_load_", ln) and " lds" not in ln]
                assert loads == [], (name, loads[:3])
                assert any(re.search(r"\bs_load_dword\b", ln) for ln in lines), name
    # the unwindowed translation units are still the 16 + 16 + 16 the other tests count
    assert len(list(obj.glob("*/fa_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))) == len(_build.INSTANCES)
    assert len(list(obj.glob("*/fa_paged_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))) == len(_build.INSTANCES)
    assert len(list(obj.glob("*/fa_paged_fp8_inst-hip-amdgcn-amd-amdhsa-gfx950.s"))) == len(_build.INSTANCES)


def test_window_host_validation_under_asan_ubsan(tmp_path):
    """The window entries' host code (csrc/fa_paged_gfx950.hip, with the dense dispatcher it validates through)
    built with AddressSanitizer + UBSan on the host side only and linked with the host-only stub
    instantiations, those of the windowed launches among them, run as a stand-alone program
    (tests/asan/paged_window_validation_driver.cpp)."""
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
    for src in (csrc / "fa_fwd_gfx950.hip", csrc / "fa_paged_gfx950.hip", asan / "stub_instances.hip",
                asan / "paged_stub_instances.hip", asan / "paged_window_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "paged_window_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "paged window validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
