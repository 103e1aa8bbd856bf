"""The paged-prefill addition to the C-ABI boundary (include/fa_gfx950_paged_prefill.h): the header declares
its four functions beside the five unchanged headers, both libraries export them, validation is the paged
decode check's (minus its decode-shape rule, plus whole 64-key tiles per page), and the workspace rule is the
other entries' -- host-only calls, no GPU needed."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK
from test_paged_abi import paged_params

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "fa_gfx950_paged_prefill.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
PREFILL = {"fa_fwd_gfx950_paged_prefill", "fa_fwd_gfx950_paged_prefill_workspace_size",
           "fa_fwd_gfx950_paged_prefill_check", "fa_paged_prefill_version"}
OLD_HEADERS = ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h", "fa_gfx950_fp8.h", "fa_gfx950_paged_window.h")
WINDOWS = (-1, 0, 63, 2 ** 40)
I64 = ctypes.c_int64


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    stem = "fa_fwd_gfx950_paged_prefill"
    getattr(lib, stem).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64, ctypes.c_void_p, I64,
                                   ctypes.c_void_p]
    getattr(lib, stem + "_workspace_size").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64]
    getattr(lib, stem + "_workspace_size").restype = I64
    getattr(lib, stem + "_check").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    return lib


def chunk_params(sq=512, **kw):
    """paged_params for a chunk of sq positions: 4 q-heads per kv-head, unpacked -- no decode shape."""
    return paged_params(sq=sq, pack=False, **kw)


def test_prefill_header_declares_its_functions_and_leaves_the_old_headers_alone():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == PREFILL
    assert re.search(r"#define FA_GFX950_PAGED_PREFILL_VERSION 1\b", text)
    assert '#include "fa_gfx950_paged.h"' in text and "fa_paged_params" in text
    assert "struct" not in text  # fa_paged_params is reused unchanged
    for old in OLD_HEADERS:  # none of them knows about this one
        assert "paged_prefill" not in (ROOT / "include" / old).read_text().lower(), old
    import test_abi
    import test_fp8_abi
    import test_kvcache_abi
    import test_paged_abi
    import test_paged_window_abi

    test_abi.test_header_declares_the_boundary()
    test_paged_abi.test_paged_header_declares_its_four_functions_and_leaves_the_old_header_alone()
    test_kvcache_abi.test_kvcache_header_declares_its_functions_and_leaves_the_old_headers_alone()
    test_fp8_abi.test_fp8_header_declares_its_functions_and_leaves_the_old_headers_alone()
    test_paged_window_abi.test_window_header_declares_its_functions_and_leaves_the_old_headers_alone()


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_prefill_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert PREFILL | {"fa_debug_last_prefill_paged"} <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_prefill_version_and_the_other_versions(lib):
    assert lib.fa_paged_prefill_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    assert lib.fa_fp8_version() == 1 and lib.fa_paged_window_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.paged_prefill_version() == 1


# decode-shaped parameter sets (page sizes that are multiples of 64): the verdict of the paged decode check
ACCEPTED = [{}, {"page_size": 64, "max_pages": 64}, {"sq": 16, "pack": False},
            {"k_head_stride": 128, "v_head_stride": 128, "k_seqlen_stride": 8 * 128, "v_seqlen_stride": 8 * 128}]
BAD_SCALES = [{"softmax_scale": s} for s in (0.0, -0.1275, float("inf"), float("nan"))]  # finite and > 0 only
REJECTED = [{"page_size": 48}, {"page_size": 0}, {"block_table": None}, {"seqlens_k": 0x60002}, {"num_pages": 0},
            {"max_pages": 0}, {"seqlen_kv": 4096 + 64}, {"block_table_stride": 16}, {"k_seqlen_stride": 132},
            {"headdim": 136}] + BAD_SCALES


def test_prefill_check_is_the_paged_check_for_decode_shapes(lib):
    for kw in ACCEPTED + REJECTED:
        for dtype, causal in ((1, 0), (0, 1)):
            p = paged_params(**kw)
            want = lib.fa_fwd_gfx950_paged_check(ctypes.byref(p), dtype, causal)
            want_err = lib.fa_last_error()
            assert (want == FA_OK) == (kw in ACCEPTED), kw
            assert lib.fa_fwd_gfx950_paged_prefill_check(ctypes.byref(p), dtype, causal) == want, kw
            assert lib.fa_last_error() == want_err
            if want != FA_OK:  # the launch and sizing entries validate first: nothing is launched
                for w in WINDOWS:
                    assert lib.fa_fwd_gfx950_paged_prefill(ctypes.byref(p), dtype, causal, w, None, 0, None) == want
                    assert lib.fa_fwd_gfx950_paged_prefill_workspace_size(ctypes.byref(p), dtype, causal, w) == -1
    assert lib.fa_fwd_gfx950_paged_prefill_check(None, 1, 0) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_fwd_gfx950_paged_prefill_workspace_size(None, 1, 0, 5) == -1


def test_prefill_check_takes_any_query_block_and_checks_the_pool_the_same_way(lib):
    """No decode-shape rule here: a 512-position chunk is refused by the paged decode check and accepted by this
    one; what is wrong with the pool or the table is still reported with the paged decode check's code."""
    for sq in (17, 512, 2048):
        p = chunk_params(sq=sq)
        assert lib.fa_fwd_gfx950_paged_check(ctypes.byref(p), 1, 1) == FA_ERR_UNSUPPORTED
        assert lib.fa_fwd_gfx950_paged_prefill_check(ctypes.byref(p), 1, 1) == FA_OK
        assert lib.fa_last_error() == b""
    for kw in REJECTED:
        want = lib.fa_fwd_gfx950_paged_check(ctypes.byref(paged_params(**kw)), 1, 1)
        assert lib.fa_fwd_gfx950_paged_prefill_check(ctypes.byref(chunk_params(**kw)), 1, 1) == want, kw
    assert lib.fa_fwd_gfx950_paged_prefill_check(ctypes.byref(chunk_params(q_seqlen_stride=132)), 1, 1) != FA_OK


def test_prefill_entries_name_the_scale_they_reject(lib):
    for kw in BAD_SCALES:
        p = chunk_params(**kw)
        assert lib.fa_fwd_gfx950_paged_prefill_check(ctypes.byref(chunk_params()), 1, 1) == FA_OK  # (clears the message)
        assert lib.fa_fwd_gfx950_paged_prefill_check(ctypes.byref(p), 1, 1) == FA_ERR_INVALID_ARGUMENT
        assert b"softmax_scale" in lib.fa_last_error()
        for w in WINDOWS:
            assert lib.fa_fwd_gfx950_paged_prefill(ctypes.byref(p), 1, 1, w, None, 0, None) == FA_ERR_INVALID_ARGUMENT
            assert lib.fa_fwd_gfx950_paged_prefill_workspace_size(ctypes.byref(p), 1, 1, w) == -1


@pytest.mark.parametrize("page_size", [32, 96])
def test_prefill_needs_whole_tiles_per_page(lib, page_size):
    p = chunk_params(page_size=page_size, max_pages=32)
    step = paged_params(page_size=page_size, max_pages=32)
    assert lib.fa_fwd_gfx950_paged_check(ctypes.byref(step), 1, 0) == FA_OK  # a valid pool for the decode entries
    for q in (p, step):
        assert lib.fa_fwd_gfx950_paged_prefill_check(ctypes.byref(q), 1, 0) == FA_ERR_UNSUPPORTED
        assert b"multiple of 64" in lib.fa_last_error()
        assert lib.fa_fwd_gfx950_paged_prefill(ctypes.byref(q), 1, 0, -1, None, 0, None) == FA_ERR_UNSUPPORTED
        assert lib.fa_fwd_gfx950_paged_prefill_workspace_size(ctypes.byref(q), 1, 0, -1) == -1


def test_prefill_workspace_size_and_a_smaller_workspace(lib):
    bad = chunk_params(num_pages=0)
    for w in WINDOWS:
        assert lib.fa_fwd_gfx950_paged_prefill_workspace_size(ctypes.byref(bad), 1, 1, w) == -1
        for kw in ({}, {"page_size": 64, "max_pages": 512}, {"page_size": 256, "max_pages": 8, "b": 1}):
            p = chunk_params(**kw)
            n = lib.fa_fwd_gfx950_paged_prefill_workspace_size(ctypes.byref(p), 1, 1, w)
            assert n >= 0
            # one byte less than it asks for is rejected before anything is launched
            rc = lib.fa_fwd_gfx950_paged_prefill(ctypes.byref(p), 1, 1, w, ctypes.c_void_p(0x100000), n - 1, None)
            assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()


def test_prefill_host_validation_under_asan_ubsan(tmp_path):
    """The paged-prefill dispatcher's host code (csrc/fa_paged_prefill_gfx950.hip, with the two dispatchers it
    validates through) built with AddressSanitizer + UBSan on the host side only and linked with host-only stub
    instantiations, run as a stand-alone program (tests/asan/paged_prefill_validation_driver.cpp)."""
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
    for src in (csrc / "fa_fwd_gfx950.hip", csrc / "fa_paged_gfx950.hip", csrc / "fa_paged_prefill_gfx950.hip",
                asan / "stub_instances.hip", asan / "paged_stub_instances.hip",
                asan / "paged_prefill_stub_instances.hip", asan / "paged_prefill_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "paged_prefill_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "paged prefill validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
