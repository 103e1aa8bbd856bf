"""The sinked ragged paged-prefill addition to the C-ABI boundary (include/fa_gfx950_paged_varlen_sink.h): the header
declares its four functions beside the unchanged headers, both libraries export them, the struct has the header's
layout, validation is the ragged entry's (its codes and messages) plus the sinks rule, and the workspace is empty --
host-only calls, no GPU needed."""
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
HEADER = ROOT / "include" / "fa_gfx950_paged_varlen_sink.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
VSINK = {"fa_fwd_gfx950_paged_varlen_sink", "fa_fwd_gfx950_paged_varlen_sink_workspace_size",
         "fa_fwd_gfx950_paged_varlen_sink_check", "fa_paged_varlen_sink_version"}
OLD_HEADERS = ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h", "fa_gfx950_fp8.h", "fa_gfx950_paged_window.h",
               "fa_gfx950_paged_prefill.h", "fa_gfx950_lse.h", "fa_gfx950_paged_varlen.h", "fa_gfx950_kvcache_varlen.h",
               "fa_gfx950_sink.h")
I64 = ctypes.c_int64


class FaPagedVarlenSinkParams(ctypes.Structure):
    _fields_ = [("varlen", FaPagedVarlenParams), ("sinks", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    for stem in ("fa_fwd_gfx950_paged_varlen", "fa_fwd_gfx950_paged_varlen_sink"):
        getattr(lib, stem).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64, ctypes.c_void_p, I64,
                                       ctypes.c_void_p]
        getattr(lib, stem + "_workspace_size").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, I64]
        getattr(lib, stem + "_workspace_size").restype = I64
        getattr(lib, stem + "_check").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    return lib


def sink_params(sinks=0x90000, **kw):
    """test_paged_varlen_abi.varlen_params' ragged step with a sinks array."""
    return FaPagedVarlenSinkParams(varlen_params(**kw), sinks)


def test_header_declares_its_functions_and_no_other_header_mentions_them():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == VSINK
    assert re.search(r"#define FA_GFX950_PAGED_VARLEN_SINK_VERSION 1\b", text)
    assert '#include "fa_gfx950_paged_varlen.h"' in text
    body = " ".join(re.search(r"typedef struct fa_paged_varlen_sink_params \{(.*?)\} fa_paged_varlen_sink_params;", text,
                              flags=re.S).group(1).split())
    assert body == "fa_paged_varlen_params varlen; const float *sinks;", body
    for old in OLD_HEADERS:
        assert "paged_varlen_sink" not in (ROOT / "include" / old).read_text().lower(), old
    # the semantics, in fa_gfx950_sink.h's words
    doc = " ".join(HEADER.read_text().split())
    for words in ("FINAL-LOGIT units", "NOT * multiplied by softmax_scale", "A row without a visible key stays 0",
                  "applied once per row", "-inf"):
        assert words in doc, words


def test_struct_layout():
    base = ctypes.sizeof(FaPagedVarlenParams)
    assert ctypes.sizeof(FaPagedVarlenSinkParams) == base + 8 and FaPagedVarlenSinkParams.sinks.offset == base


def test_the_unsinked_ragged_dispatcher_references_no_new_symbol():
    csrc = ROOT / "flash_attention_cute_amd" / "csrc"
    for name in ("fa_paged_varlen_gfx950.hip", "fa_paged_varlen.hpp", "fa_paged_varlen_launch.h",
                 "fa_paged_varlen_inst.hip", "fa_paged_prefill_gfx950.hip"):
        assert "sink" not in (csrc / name).read_text().lower(), name


def test_sink_variant_is_compiled_in_translation_units_of_its_own():
    from flash_attention_cute_amd import _build

    csrc = _build.CSRC
    assert ("pvars_", "fa_paged_varlen_sink_inst") in _build.INST_TUS and ("pvar_", "fa_paged_varlen_inst") in _build.INST_TUS
    sinked = (csrc / "fa_paged_varlen_sink.hpp").read_text()
    for macro in ("FA_W4_PAGED", "FA_W4_PAGED_VARLEN", "FA_W4_SINK"):
        assert f"#define {macro} 1" in sinked
    kernels = (csrc / "fa_fwd_kernels.hpp").read_text()
    assert re.search(r"#ifndef FA_W4_SINK\n#define FA_W4_SINK 0\n#endif\n#if FA_W4_SINK && !FA_W4_PAGED_VARLEN\n#error", kernels)
    assert "struct PagedVarlenSinkArgs" in (csrc / "fa_paged_varlen_sink_launch.h").read_text()
    assert "launch_prefill_paged_varlen_sink<" in (csrc / "fa_paged_varlen_sink_gfx950.hip").read_text()


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert VSINK <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_version_and_the_other_versions(lib):
    assert lib.fa_paged_varlen_sink_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    assert lib.fa_fp8_version() == 1 and lib.fa_paged_window_version() == 1 and lib.fa_paged_prefill_version() == 1
    assert lib.fa_lse_version() == 1 and lib.fa_paged_varlen_version() == 1 and lib.fa_kvcache_varlen_version() == 1
    assert lib.fa_sink_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.paged_varlen_sink_version() == 1


def broken(kw):
    """sink_params with test_paged_varlen_abi's way of breaking a field of the paged description."""
    s = sink_params()
    for key, val in kw.items():
        setattr(s.varlen.paged.base if hasattr(s.varlen.paged.base, key) else s.varlen.paged, key, val)
    return s


def test_check_is_the_ragged_check_below_the_sinks(lib):
    """Every description the ragged entry rejects is rejected here with its code and its message, by all three
    entries; the valid one passes."""
    cases = [broken(kw) for kw in [{}] + REJECTED] + [sink_params(**kw) for kw, _, _ in TABLE]
    rejected = 0
    for s in cases:
        for dtype, causal in ((1, 0), (0, 1)):
            want = lib.fa_fwd_gfx950_paged_varlen_check(ctypes.byref(s.varlen), dtype, causal)
            want_err = lib.fa_last_error()
            assert lib.fa_fwd_gfx950_paged_varlen_sink_check(ctypes.byref(s), dtype, causal) == want
            assert lib.fa_last_error() == want_err
            if want != FA_OK:
                rejected += 1
                for w in WINDOWS:
                    assert lib.fa_fwd_gfx950_paged_varlen_sink(ctypes.byref(s), dtype, causal, w, None, 0, None) == want
                    assert lib.fa_fwd_gfx950_paged_varlen_sink_workspace_size(ctypes.byref(s), dtype, causal, w) == -1
    assert rejected == 2 * (len(REJECTED) + len(TABLE))
    for dtype in (2, 3, -1):  # (there is no code for an FP8 pool here)
        assert lib.fa_fwd_gfx950_paged_varlen_sink_check(ctypes.byref(sink_params()), dtype, 1) == FA_ERR_UNSUPPORTED
    assert lib.fa_fwd_gfx950_paged_varlen_sink_check(None, 1, 0) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_fwd_gfx950_paged_varlen_sink_workspace_size(None, 1, 0, 5) == -1


@pytest.mark.parametrize("sinks,word", [(None, b"sinks is NULL"), (0x90002, b"4-byte aligned"), (0x90001, b"4-byte aligned")])
def test_bad_sinks_are_an_invalid_argument(lib, sinks, word):
    assert lib.fa_fwd_gfx950_paged_varlen_sink_check(ctypes.byref(sink_params()), 1, 1) == FA_OK  # (clears the message)
    assert lib.fa_last_error() == b""
    s = sink_params(sinks=sinks)
    assert lib.fa_fwd_gfx950_paged_varlen_check(ctypes.byref(s.varlen), 1, 1) == FA_OK
    assert lib.fa_fwd_gfx950_paged_varlen_sink_check(ctypes.byref(s), 1, 1) == FA_ERR_INVALID_ARGUMENT
    assert word in lib.fa_last_error(), lib.fa_last_error()
    for w in WINDOWS:
        assert lib.fa_fwd_gfx950_paged_varlen_sink(ctypes.byref(s), 1, 1, w, None, 0, None) == FA_ERR_INVALID_ARGUMENT
        assert word in lib.fa_last_error()
        assert lib.fa_fwd_gfx950_paged_varlen_sink_workspace_size(ctypes.byref(s), 1, 1, w) == -1


def test_workspace_is_empty_and_a_negative_size_is_refused(lib):
    for w in WINDOWS:
        for kw in ({}, {"page_size": 64, "max_pages": 512}, {"page_size": 256, "max_pages": 8, "b": 1}, {"max_q": 1},
                   {"total_q": 0}, {"hq": 64, "d": 64}):
            s = sink_params(**kw)
            assert lib.fa_fwd_gfx950_paged_varlen_sink_workspace_size(ctypes.byref(s), 1, 1, w) == 0
            rc = lib.fa_fwd_gfx950_paged_varlen_sink(ctypes.byref(s), 1, 1, w, ctypes.c_void_p(0x100000), -1, None)
            assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()
    # no row at all: valid, and nothing is launched (no device is touched)
    assert lib.fa_fwd_gfx950_paged_varlen_sink(ctypes.byref(sink_params(total_q=0)), 1, 1, -1, None, 0, None) == FA_OK


def test_host_validation_under_asan_ubsan(tmp_path):
    """The dispatcher's host code (csrc/fa_paged_varlen_sink_gfx950.hip, with the four dispatchers it validates
    through) built with AddressSanitizer + UBSan on the host side only and linked with host-only stub
    instantiations, run as a stand-alone program (tests/asan/paged_varlen_sink_validation_driver.cpp)."""
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
                csrc / "fa_paged_varlen_gfx950.hip", csrc / "fa_paged_varlen_sink_gfx950.hip",
                asan / "stub_instances.hip", asan / "paged_stub_instances.hip", asan / "paged_prefill_stub_instances.hip",
                asan / "paged_varlen_stub_instances.hip", asan / "paged_varlen_sink_stub_instances.hip",
                asan / "paged_varlen_sink_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "paged_varlen_sink_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "paged varlen sink validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
