"""The LSE addition to the ragged paged prefill at the C-ABI boundary (include/fa_gfx950_paged_varlen_lse.h): the
header declares its four functions beside the unchanged headers, both libraries export them, the struct has the
header's layout, validation is the ragged entry's (its codes and messages) plus the rules of the LSE array and of an
OPTIONAL sinks array, and the workspace is empty -- host-only calls, no GPU needed."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK
from test_paged_varlen_abi import REJECTED, TABLE, WINDOWS, FaPagedVarlenParams, varlen_params

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "fa_gfx950_paged_varlen_lse.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
VLSE = {"fa_fwd_gfx950_paged_varlen_lse", "fa_fwd_gfx950_paged_varlen_lse_workspace_size",
        "fa_fwd_gfx950_paged_varlen_lse_check", "fa_paged_varlen_lse_version"}
OLD_HEADERS = ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h", "fa_gfx950_fp8.h", "fa_gfx950_paged_window.h",
               "fa_gfx950_paged_prefill.h", "fa_gfx950_lse.h", "fa_gfx950_paged_varlen.h", "fa_gfx950_kvcache_varlen.h",
               "fa_gfx950_sink.h", "fa_gfx950_paged_varlen_sink.h")
I64 = ctypes.c_int64


class FaPagedVarlenLseParams(ctypes.Structure):
    _fields_ = [("varlen", FaPagedVarlenParams), ("sinks", ctypes.c_void_p), ("lse_ptr", ctypes.c_void_p),
                ("lse_head_stride", I64), ("lse_row_stride", I64)]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    for stem in ("fa_fwd_gfx950_paged_varlen", "fa_fwd_gfx950_paged_varlen_lse"):
        getattr(lib, stem).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64, ctypes.c_void_p, I64,
                                       ctypes.c_void_p]
        getattr(lib, stem + "_workspace_size").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64]
        getattr(lib, stem + "_workspace_size").restype = I64
        getattr(lib, stem + "_check").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    return lib


def lse_params(sinks=0x90000, lse=0xa0000, head_stride=4096, row_stride=1, **kw):
    """test_paged_varlen_abi.varlen_params' ragged step with a sinks array and an LSE destination."""
    return FaPagedVarlenLseParams(varlen_params(**kw), sinks, lse, head_stride, row_stride)


def test_header_declares_its_functions_and_no_other_header_mentions_them():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == VLSE
    assert re.search(r"#define FA_GFX950_PAGED_VARLEN_LSE_VERSION 1\b", text)
    assert '#include "fa_gfx950_paged_varlen.h"' in text
    body = " ".join(re.search(r"typedef struct fa_paged_varlen_lse_params \{(.*?)\} fa_paged_varlen_lse_params;", text,
                              flags=re.S).group(1).split())
    assert body == ("fa_paged_varlen_params varlen; const float *sinks; float *lse_ptr; "
                    "int64_t lse_head_stride, lse_row_stride;"), body
    for old in OLD_HEADERS:
        assert "paged_varlen_lse" not in (ROOT / "include" / old).read_text().lower(), old
    doc = " ".join(HEADER.read_text().split())
    for words in ("natural-log units", "lse = ln( sum_n exp(s_n) + exp(sinks[h]) )", "gets -inf", "lse = sinks[h]",
                  "exactly ONE of the states", "nothing else of the array is touched"):
        assert words in doc, words


def test_struct_layout():
    base = ctypes.sizeof(FaPagedVarlenParams)
    assert ctypes.sizeof(FaPagedVarlenLseParams) == base + 32
    assert [getattr(FaPagedVarlenLseParams, f).offset - base
            for f in ("sinks", "lse_ptr", "lse_head_stride", "lse_row_stride")] == [0, 8, 16, 24]


def test_the_other_ragged_dispatchers_reference_no_new_symbol():
    csrc = ROOT / "flash_attention_cute_amd" / "csrc"
    for name in ("fa_paged_varlen_gfx950.hip", "fa_paged_varlen.hpp", "fa_paged_varlen_launch.h",
                 "fa_paged_varlen_inst.hip", "fa_paged_prefill_gfx950.hip", "fa_paged_varlen_sink_gfx950.hip",
                 "fa_paged_varlen_sink.hpp", "fa_paged_varlen_sink_launch.h", "fa_paged_varlen_sink_inst.hip"):
        text = (csrc / name).read_text()
        assert "varlen_lse" not in text.lower() and "FA_W4_LSE" not in text and "VarlenLse" not in text, name


def test_lse_variant_is_one_family_in_translation_units_of_its_own():
    from flash_attention_cute_amd import _build

    csrc = _build.CSRC
    assert ("pvarl_", "fa_paged_varlen_lse_inst") in _build.INST_TUS
    assert ("pvars_", "fa_paged_varlen_sink_inst") in _build.INST_TUS and ("pvar_", "fa_paged_varlen_inst") in _build.INST_TUS
    assert "fa_paged_varlen_lse_inst" in _build.SHARED_WITH_DEBUG
    assert sum("varlen_lse" in name for _, name in _build.INST_TUS) == 1  # (not one sinked and one unsinked)
    text = (csrc / "fa_paged_varlen_lse.hpp").read_text()
    for macro in ("FA_W4_PAGED", "FA_W4_PAGED_VARLEN", "FA_W4_SINK", "FA_W4_LSE"):
        assert f"#define {macro} 1" in text
    kernels = (csrc / "fa_fwd_kernels.hpp").read_text()
    assert re.search(r"#ifndef FA_W4_LSE\n#define FA_W4_LSE 0\n#endif\n#if FA_W4_LSE && !FA_W4_SINK\n#error", kernels)
    # the counted wait of the next block's prologue includes the LSE stores, and a key-split piece cannot be compiled
    assert "vmcnt_enc(kOStores + kLseStores)" in kernels and "constexpr int kLseStores = 2;" in kernels
    assert re.search(r"#if FA_W4_LSE\n\s*static_assert\(!spl,", kernels)
    assert "struct PagedVarlenLseArgs" in (csrc / "fa_paged_varlen_lse_launch.h").read_text()
    disp = (csrc / "fa_paged_varlen_lse_gfx950.hip").read_text()
    assert "launch_prefill_paged_varlen_lse<" in disp and "fa_fwd_gfx950_paged_varlen_check(&v->varlen" in disp
    assert "hipMalloc" not in disp and "__global__" not in disp  # (host-only)


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert VLSE <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_version_and_the_other_versions(lib):
    assert lib.fa_paged_varlen_lse_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    assert lib.fa_fp8_version() == 1 and lib.fa_paged_window_version() == 1 and lib.fa_paged_prefill_version() == 1
    assert lib.fa_lse_version() == 1 and lib.fa_paged_varlen_version() == 1 and lib.fa_kvcache_varlen_version() == 1
    assert lib.fa_sink_version() == 1 and lib.fa_paged_varlen_sink_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.paged_varlen_lse_version() == 1


def broken(kw):
    """lse_params with test_paged_varlen_abi's way of breaking a field of the paged description."""
    s = lse_params()
    for key, val in kw.items():
        setattr(s.varlen.paged.base if hasattr(s.varlen.paged.base, key) else s.varlen.paged, key, val)
    return s


def test_check_is_the_ragged_check_below_the_new_rules(lib):
    """Every description the ragged entry rejects is rejected here with its code and its message, by all three
    entries; the valid one passes, with and without sinks."""
    cases = [broken(kw) for kw in [{}] + REJECTED] + [lse_params(**kw) for kw, _, _ in TABLE]
    rejected = 0
    for s in cases:
        for dtype, causal in ((1, 0), (0, 1)):
            want = lib.fa_fwd_gfx950_paged_varlen_check(ctypes.byref(s.varlen), dtype, causal)
            want_err = lib.fa_last_error()
            assert lib.fa_fwd_gfx950_paged_varlen_lse_check(ctypes.byref(s), dtype, causal) == want
            assert lib.fa_last_error() == want_err
            if want != FA_OK:
                rejected += 1
                for w in WINDOWS:
                    assert lib.fa_fwd_gfx950_paged_varlen_lse(ctypes.byref(s), dtype, causal, w, None, 0, None) == want
                    assert lib.fa_fwd_gfx950_paged_varlen_lse_workspace_size(ctypes.byref(s), dtype, causal, w) == -1
    assert rejected == 2 * (len(REJECTED) + len(TABLE))
    for dtype in (2, 3, -1):  # (there is no code for an FP8 pool here)
        assert lib.fa_fwd_gfx950_paged_varlen_lse_check(ctypes.byref(lse_params()), dtype, 1) == FA_ERR_UNSUPPORTED
    assert lib.fa_fwd_gfx950_paged_varlen_lse_check(None, 1, 0) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_fwd_gfx950_paged_varlen_lse_workspace_size(None, 1, 0, 5) == -1


def test_sinks_null_is_accepted(lib):
    for kw in ({"sinks": None}, {"sinks": None, "row_stride": 0, "head_stride": 0}, {"row_stride": 2},
               {"row_stride": 1 << 20}):
        s = lse_params(**kw)
        assert lib.fa_fwd_gfx950_paged_varlen_lse_check(ctypes.byref(s), 1, 1) == FA_OK, lib.fa_last_error()
        assert lib.fa_last_error() == b""
        assert lib.fa_fwd_gfx950_paged_varlen_lse_workspace_size(ctypes.byref(s), 1, 1, 127) == 0


@pytest.mark.parametrize("kw,word", [
    ({"sinks": 0x90002}, b"sinks must be NULL or a 4-byte aligned"), ({"sinks": 0x90001}, b"sinks must be NULL or a 4-byte aligned"),
    ({"lse": None}, b"lse_ptr is NULL"), ({"lse": 0xa0002}, b"lse_ptr must be a 4-byte aligned"),
    ({"lse": 0xa0001}, b"lse_ptr must be a 4-byte aligned"),
    ({"head_stride": -1}, b"lse strides must be non-negative (got head -1, row 1)"),
    ({"row_stride": -8}, b"lse strides must be non-negative (got head 4096, row -8)"),
    ({"row_stride": (1 << 20) + 1}, b"lse_row_stride 1048577 is larger than the 1048576 elements served")],
    ids=["sinks+2", "sinks+1", "lse-null", "lse+2", "lse+1", "head-stride", "row-stride", "row-stride-large"])
def test_the_new_errors_are_an_invalid_argument(lib, kw, word):
    assert lib.fa_fwd_gfx950_paged_varlen_lse_check(ctypes.byref(lse_params()), 1, 1) == FA_OK  # (clears the message)
    assert lib.fa_last_error() == b""
    s = lse_params(**kw)
    assert lib.fa_fwd_gfx950_paged_varlen_check(ctypes.byref(s.varlen), 1, 1) == FA_OK
    assert lib.fa_fwd_gfx950_paged_varlen_lse_check(ctypes.byref(s), 1, 1) == FA_ERR_INVALID_ARGUMENT
    assert word in lib.fa_last_error(), lib.fa_last_error()
    for w in WINDOWS:
        assert lib.fa_fwd_gfx950_paged_varlen_lse(ctypes.byref(s), 1, 1, w, None, 0, None) == FA_ERR_INVALID_ARGUMENT
        assert word in lib.fa_last_error()
        assert lib.fa_fwd_gfx950_paged_varlen_lse_workspace_size(ctypes.byref(s), 1, 1, w) == -1


def test_workspace_is_empty_and_a_negative_size_is_refused(lib):
    for w in WINDOWS:
        for kw in ({}, {"page_size": 64, "max_pages": 512}, {"page_size": 256, "max_pages": 8, "b": 1}, {"max_q": 1},
                   {"total_q": 0}, {"hq": 64, "d": 64}):
            for sinks in (0x90000, None):
                s = lse_params(sinks=sinks, **kw)
                assert lib.fa_fwd_gfx950_paged_varlen_lse_workspace_size(ctypes.byref(s), 1, 1, w) == 0
                rc = lib.fa_fwd_gfx950_paged_varlen_lse(ctypes.byref(s), 1, 1, w, ctypes.c_void_p(0x100000), -1, None)
                assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()
    # no row at all: valid, and nothing is launched (no device is touched)
    for sinks in (0x90000, None):
        assert lib.fa_fwd_gfx950_paged_varlen_lse(ctypes.byref(lse_params(sinks=sinks, total_q=0)), 1, 1, -1, None, 0,
                                                  None) == FA_OK


def test_host_validation_under_asan_ubsan(tmp_path):
    """The dispatcher's host code (csrc/fa_paged_varlen_lse_gfx950.hip, with the four dispatchers it validates
    through) built with AddressSanitizer + UBSan on the host side only and linked with host-only stub
    instantiations, run as a stand-alone program (tests/asan/paged_varlen_lse_validation_driver.cpp)."""
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
                csrc / "fa_paged_varlen_gfx950.hip", csrc / "fa_paged_varlen_lse_gfx950.hip",
                asan / "stub_instances.hip", asan / "paged_stub_instances.hip", asan / "paged_prefill_stub_instances.hip",
                asan / "paged_varlen_stub_instances.hip", asan / "paged_varlen_lse_stub_instances.hip",
                asan / "paged_varlen_lse_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "paged_varlen_lse_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "paged varlen lse validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
