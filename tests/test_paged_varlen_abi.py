"""The ragged paged-prefill addition to the C-ABI boundary (include/fa_gfx950_paged_varlen.h): the header
declares its four functions and no older header knows of them, both libraries export them, validation is the
paged prefill check's on the packed layout plus the rules of the cumulative array, and the workspace rule is the
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
from test_paged_abi import FaPagedParams, paged_params

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "fa_gfx950_paged_varlen.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
VARLEN = {"fa_fwd_gfx950_paged_varlen", "fa_fwd_gfx950_paged_varlen_workspace_size",
          "fa_fwd_gfx950_paged_varlen_check", "fa_paged_varlen_version"}
OLD_HEADERS = ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h", "fa_gfx950_fp8.h", "fa_gfx950_paged_window.h",
               "fa_gfx950_paged_prefill.h", "fa_gfx950_lse.h")
WINDOWS = (-1, 0, 63, 2 ** 40)
I64 = ctypes.c_int64


class FaPagedVarlenParams(ctypes.Structure):
    _fields_ = [("paged", FaPagedParams), ("cu_seqlens_q", ctypes.c_void_p), ("total_q", ctypes.c_int64)]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    stem = "fa_fwd_gfx950_paged_varlen"
    getattr(lib, stem).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64, ctypes.c_void_p, I64,
                                   ctypes.c_void_p]
    getattr(lib, stem + "_workspace_size").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64]
    getattr(lib, stem + "_workspace_size").restype = I64
    getattr(lib, stem + "_check").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.fa_fwd_gfx950_paged_prefill_check.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    return lib


def packed(p: FaPagedParams) -> FaPagedParams:
    """The description as the packed [total_q, Hq, D] layout: rows, then heads; the batch strides are ignored."""
    b = p.base
    b.q_head_stride = b.o_head_stride = b.headdim
    b.q_seqlen_stride = b.o_seqlen_stride = b.num_heads_q * b.headdim
    b.q_batch_stride = b.o_batch_stride = 12345  # (ignored by the entry: not even a multiple of 8)
    return p


def varlen_params(max_q=512, total_q=3000, cu=0x70000, **kw):
    """A ragged step: at most max_q rows per sequence, total_q in all, over paged_params' pool."""
    return FaPagedVarlenParams(packed(paged_params(sq=max_q, pack=False, **kw)), cu, total_q)


def uniform(v: FaPagedVarlenParams) -> FaPagedParams:
    """The same description as the uniform entry sees it: the batch strides zeroed."""
    p = FaPagedParams.from_buffer_copy(v.paged)
    p.base.q_batch_stride = p.base.o_batch_stride = 0
    return p


def test_varlen_header_declares_its_functions_and_no_other_header_mentions_them():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == VARLEN
    assert re.search(r"#define FA_GFX950_PAGED_VARLEN_VERSION 1\b", text)
    assert '#include "fa_gfx950_paged.h"' in text
    assert re.search(r"typedef struct fa_paged_varlen_params \{\s*fa_paged_params paged;[^}]*const int32_t \*cu_seqlens_q;"
                     r"[^}]*int64_t total_q;[^}]*\} fa_paged_varlen_params;", text)
    for old in OLD_HEADERS:
        assert "paged_varlen" not in (ROOT / "include" / old).read_text().lower(), old
    import test_paged_prefill_abi

    test_paged_prefill_abi.test_prefill_header_declares_its_functions_and_leaves_the_old_headers_alone()


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_varlen_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert VARLEN | {"fa_debug_last_prefill_paged"} <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_varlen_version_and_the_other_versions(lib):
    assert lib.fa_paged_varlen_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    assert lib.fa_fp8_version() == 1 and lib.fa_paged_window_version() == 1 and lib.fa_paged_prefill_version() == 1
    assert lib.fa_lse_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.paged_varlen_version() == 1


BAD_SCALES = [{"softmax_scale": s} for s in (0.0, -0.1275, float("inf"), float("nan"))]
REJECTED = [{"page_size": 48}, {"page_size": 96, "max_pages": 32}, {"page_size": 32}, {"page_size": 0},
            {"block_table": None}, {"seqlens_k": 0x60002}, {"num_pages": 0}, {"max_pages": 0},
            {"seqlen_kv": 4096 + 64}, {"block_table_stride": 16}, {"k_seqlen_stride": 132}, {"headdim": 136},
            {"q_seqlen_stride": 132}] + BAD_SCALES


def test_varlen_check_is_the_prefill_check_on_the_packed_layout(lib):
    for kw in [{}] + REJECTED:
        for dtype, causal in ((1, 0), (0, 1)):
            v = varlen_params()
            for key, val in kw.items():
                setattr(v.paged.base if hasattr(v.paged.base, key) else v.paged, key, val)
            want = lib.fa_fwd_gfx950_paged_prefill_check(ctypes.byref(uniform(v)), dtype, causal)
            want_err = lib.fa_last_error()
            assert (want == FA_OK) == (kw == {}), kw
            assert lib.fa_fwd_gfx950_paged_varlen_check(ctypes.byref(v), dtype, causal) == want, kw
            assert lib.fa_last_error() == want_err
            if want != FA_OK:  # the launch and sizing entries validate first: nothing is launched
                for w in WINDOWS:
                    assert lib.fa_fwd_gfx950_paged_varlen(ctypes.byref(v), dtype, causal, w, None, 0, None) == want
                    assert lib.fa_fwd_gfx950_paged_varlen_workspace_size(ctypes.byref(v), dtype, causal, w) == -1
    assert lib.fa_fwd_gfx950_paged_varlen_check(None, 1, 0) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_fwd_gfx950_paged_varlen_workspace_size(None, 1, 0, 5) == -1


# the table of the rules that are new here, and the ones the issue names: (how to break it, code, a word of the message)
TABLE = [
    (dict(cu=None), FA_ERR_INVALID_ARGUMENT, b"cu_seqlens_q"),
    (dict(cu=0x70002), FA_ERR_INVALID_ARGUMENT, b"aligned"),
    (dict(total_q=-1), FA_ERR_INVALID_ARGUMENT, b"total_q"),
    (dict(total_q=2 ** 31), FA_ERR_UNSUPPORTED, b"32 bits"),
    (dict(b=2 ** 31 - 1), FA_ERR_UNSUPPORTED, b"32 bits"),
    (dict(max_q=2 ** 30 + 1), FA_ERR_UNSUPPORTED, b"2^30"),
    (dict(page_size=96, max_pages=32), FA_ERR_UNSUPPORTED, b"multiple of 64"),
]


@pytest.mark.parametrize("kw,want,word", TABLE, ids=[",".join(f"{k}={v}" for k, v in t[0].items()) for t in TABLE])
def test_varlen_check_table(lib, kw, want, word):
    v = varlen_params(**kw)
    assert lib.fa_fwd_gfx950_paged_varlen_check(ctypes.byref(varlen_params()), 1, 1) == FA_OK  # (clears the message)
    assert lib.fa_last_error() == b""
    assert lib.fa_fwd_gfx950_paged_varlen_check(ctypes.byref(v), 1, 1) == want
    assert word in lib.fa_last_error(), lib.fa_last_error()
    for w in WINDOWS:
        assert lib.fa_fwd_gfx950_paged_varlen(ctypes.byref(v), 1, 1, w, None, 0, None) == want
        assert lib.fa_fwd_gfx950_paged_varlen_workspace_size(ctypes.byref(v), 1, 1, w) == -1


def test_varlen_refuses_an_fp8_dtype(lib):
    v = varlen_params()
    for dtype in (2, 3, -1):  # (0 / 1 are fp16 / bf16: there is no code for an FP8 pool here)
        assert lib.fa_fwd_gfx950_paged_varlen_check(ctypes.byref(v), dtype, 1) == FA_ERR_UNSUPPORTED
        assert lib.fa_fwd_gfx950_paged_varlen(ctypes.byref(v), dtype, 1, -1, None, 0, None) == FA_ERR_UNSUPPORTED
        assert lib.fa_fwd_gfx950_paged_varlen_workspace_size(ctypes.byref(v), dtype, 1, -1) == -1


def test_varlen_workspace_is_empty_and_a_negative_size_is_refused(lib):
    for w in WINDOWS:
        for kw in ({}, {"page_size": 64, "max_pages": 512}, {"page_size": 256, "max_pages": 8, "b": 1}, {"max_q": 1},
                   {"total_q": 0}):
            v = varlen_params(**kw)
            assert lib.fa_fwd_gfx950_paged_varlen_workspace_size(ctypes.byref(v), 1, 1, w) == 0
            # one byte less than it asks for is rejected before anything is launched
            rc = lib.fa_fwd_gfx950_paged_varlen(ctypes.byref(v), 1, 1, w, ctypes.c_void_p(0x100000), -1, None)
            assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()
    # no row at all: valid, and nothing is launched (no device is touched)
    assert lib.fa_fwd_gfx950_paged_varlen(ctypes.byref(varlen_params(total_q=0)), 1, 1, -1, None, 0, None) == FA_OK


def test_ragged_variant_is_compiled_in_translation_units_of_its_own():
    """The uniform paged prefill's launcher and header do not know the ragged variant: it has its own macro,
    instantiation file, launch function and argument struct, and its own row in the build's instantiation list."""
    from flash_attention_cute_amd import _build

    csrc = _build.CSRC
    assert ("pvar_", "fa_paged_varlen_inst") in _build.INST_TUS and ("pfill_", "fa_paged_prefill_inst") in _build.INST_TUS
    for name in ("fa_paged_prefill.hpp", "fa_paged_prefill_launch.h", "fa_paged_prefill_inst.hip", "fa_paged_prefill_gfx950.hip"):
        text = (csrc / name).read_text()
        assert "VARLEN" not in text and "cu_seqlens" not in text and "varlen" not in text.lower(), name
    ragged = (csrc / "fa_paged_varlen.hpp").read_text()
    assert "#define FA_W4_PAGED 1" in ragged and "#define FA_W4_PAGED_VARLEN 1" in ragged
    assert "struct PagedVarlenArgs" in (csrc / "fa_paged_varlen_launch.h").read_text()
    assert "launch_prefill_paged_varlen<" in (csrc / "fa_paged_varlen_gfx950.hip").read_text()


def test_varlen_host_validation_under_asan_ubsan(tmp_path):
    """The ragged dispatcher's host code (csrc/fa_paged_varlen_gfx950.hip, with the three dispatchers it
    validates through) built with AddressSanitizer + UBSan on the host side only and linked with host-only stub
    instantiations, run as a stand-alone program (tests/asan/paged_varlen_validation_driver.cpp)."""
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
                csrc / "fa_paged_varlen_gfx950.hip", asan / "stub_instances.hip", asan / "paged_stub_instances.hip",
                asan / "paged_prefill_stub_instances.hip", asan / "paged_varlen_stub_instances.hip",
                asan / "paged_varlen_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "paged_varlen_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "paged varlen validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
