"""The attention-sink addition to the C-ABI boundary (include/fa_gfx950_sink.h): the header declares its functions
beside the unchanged headers, both libraries export them, the structs have the header's layout, the descriptions
are validated with the documented codes and the workspace is the one of the entry without sinks -- host-only
calls, no GPU needed. The built assembly of the 4 x 16 new translation units keeps the key loop's load order."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK
from test_fp8_abi import FaPagedFp8Params, fp8_params
from test_paged_abi import FaPagedParams, paged_params

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "fa_gfx950_sink.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
SINK = {"fa_fwd_gfx950_paged_sink", "fa_fwd_gfx950_paged_sink_workspace_size", "fa_fwd_gfx950_paged_sink_check",
        "fa_fwd_gfx950_paged_sink_fp8", "fa_fwd_gfx950_paged_sink_fp8_workspace_size",
        "fa_fwd_gfx950_paged_sink_fp8_check", "fa_sink_version"}
OLD_HEADERS = ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h", "fa_gfx950_fp8.h", "fa_gfx950_paged_window.h",
               "fa_gfx950_paged_prefill.h", "fa_gfx950_lse.h", "fa_gfx950_paged_varlen.h", "fa_gfx950_kvcache_varlen.h")
_I64 = ctypes.c_int64
WINDOWS = (-1, -(2 ** 40), 0, 1, 127, 4095, 2 ** 40)


class FaPagedSinkParams(ctypes.Structure):
    _fields_ = [("paged", FaPagedParams), ("sinks", ctypes.c_void_p)]


class FaPagedFp8SinkParams(ctypes.Structure):
    _fields_ = [("fp8", FaPagedFp8Params), ("sinks", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    for name in ("fa_fwd_gfx950_paged_sink", "fa_fwd_gfx950_paged_sink_fp8"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64, ctypes.c_void_p, _I64,
                                       ctypes.c_void_p]
        getattr(lib, name + "_check").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64]
        getattr(lib, name + "_workspace_size").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64]
        getattr(lib, name + "_workspace_size").restype = _I64
    for name in ("fa_fwd_gfx950_paged_window_workspace_size", "fa_fwd_gfx950_paged_window_fp8_workspace_size"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64]
        getattr(lib, name).restype = _I64
    for name in ("fa_fwd_gfx950_paged_workspace_size", "fa_fwd_gfx950_paged_fp8_workspace_size"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        getattr(lib, name).restype = _I64
    return lib


def sink_params(fp8=False, b=32, hq=32, sq=1, sinks=0x90000, **kw):
    """A decode step as the torch binding passes it to the sink entries: no q-head pack."""
    if fp8:
        return FaPagedFp8SinkParams(fp8_params(b=b, hq=hq, sq=sq, pack=False, **kw), sinks)
    return FaPagedSinkParams(paged_params(b=b, hq=hq, sq=sq, pack=False, **kw), sinks)


def check(lib, p, dtype=1, causal=0, window_left=-1):
    fn = lib.fa_fwd_gfx950_paged_sink_fp8_check if isinstance(p, FaPagedFp8SinkParams) else lib.fa_fwd_gfx950_paged_sink_check
    rc = fn(ctypes.byref(p), dtype, causal, window_left)
    return rc, lib.fa_last_error().decode()


def test_sink_header_declares_its_functions_and_leaves_the_old_headers_alone():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == SINK
    assert re.search(r"#define FA_GFX950_SINK_VERSION 1\b", text)
    for inc in ("fa_gfx950_paged.h", "fa_gfx950_fp8.h", "fa_gfx950_paged_window.h"):
        assert f'#include "{inc}"' in text
    for old in OLD_HEADERS:
        assert "sink" not in (ROOT / "include" / old).read_text().lower(), old


def test_the_older_dispatchers_reference_no_new_symbol():
    csrc = ROOT / "flash_attention_cute_amd" / "csrc"
    for name in ("fa_fwd_gfx950.hip", "fa_paged_gfx950.hip", "fa_paged_lse_gfx950.hip"):
        assert "sink" not in (csrc / name).read_text().lower(), name


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_sink_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert SINK <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_sink_version_and_the_other_versions(lib):
    assert lib.fa_sink_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    assert lib.fa_fp8_version() == 1 and lib.fa_paged_window_version() == 1 and lib.fa_paged_prefill_version() == 1
    assert lib.fa_lse_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.sink_version() == 1


def test_sink_struct_layouts():
    for outer, inner in ((FaPagedSinkParams, FaPagedParams), (FaPagedFp8SinkParams, FaPagedFp8Params)):
        base = ctypes.sizeof(inner)
        assert ctypes.sizeof(outer) == base + 8 and outer.sinks.offset == base
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, first in (("fa_paged_sink_params", "fa_paged_params paged;"),
                        ("fa_paged_fp8_sink_params", "fa_paged_fp8_params fp8;")):
        body = " ".join(re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1).split())
        assert body == f"{first} const float *sinks;", body


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sink_check_accepts_valid(lib, fp8):
    assert check(lib, sink_params(fp8)) == (FA_OK, "")
    assert check(lib, sink_params(fp8, page_size=32, max_pages=128), dtype=0)[0] == FA_OK
    assert check(lib, sink_params(fp8, sq=2), causal=1)[0] == FA_OK  # g 4 x Sq 2
    assert check(lib, sink_params(fp8, hq=64, d=64))[0] == FA_OK  # the gpt-oss head shape: g 8, D 64
    for w in WINDOWS:  # every window_left is valid
        assert check(lib, sink_params(fp8), window_left=w)[0] == FA_OK, w
        assert check(lib, sink_params(fp8, sq=16), causal=1, window_left=w)[0] == FA_OK, w  # 64 rows


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sink_check_rejects_invalid(lib, fp8):
    def bad(code, word, window_left=-1, **kw):
        for w in (window_left, 127):
            rc, msg = check(lib, sink_params(fp8, **kw), window_left=w)
            assert rc == code and word in msg, (rc, msg)

    bad(FA_ERR_INVALID_ARGUMENT, "sinks is NULL", sinks=None)
    bad(FA_ERR_INVALID_ARGUMENT, "4-byte aligned", sinks=0x90002)
    # the base description is the paged decode check's: its codes and its messages
    bad(FA_ERR_INVALID_ARGUMENT, "page_size", page_size=48, max_pages=32)
    bad(FA_ERR_UNSUPPORTED, "decode", sq=17)  # g 4 x Sq 17: past the decode rule
    bad(FA_ERR_INVALID_ARGUMENT, "block_table", block_table=None)
    bad(FA_ERR_INVALID_ARGUMENT, "seqlens_k", seqlens_k=None)
    assert lib.fa_fwd_gfx950_paged_sink_check(None, 1, 0, -1) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_fwd_gfx950_paged_sink_fp8_check(None, 1, 0, 5) == FA_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sink_workspace_is_the_one_of_the_entry_without_sinks(lib, fp8):
    size = lib.fa_fwd_gfx950_paged_sink_fp8_workspace_size if fp8 else lib.fa_fwd_gfx950_paged_sink_workspace_size
    plain = lib.fa_fwd_gfx950_paged_fp8_workspace_size if fp8 else lib.fa_fwd_gfx950_paged_workspace_size
    win = lib.fa_fwd_gfx950_paged_window_fp8_workspace_size if fp8 else lib.fa_fwd_gfx950_paged_window_workspace_size
    entry = lib.fa_fwd_gfx950_paged_sink_fp8 if fp8 else lib.fa_fwd_gfx950_paged_sink
    split = 0
    for kw in (dict(b=1, max_pages=256), dict(b=2, max_pages=64), dict(b=64, max_pages=8),
               dict(b=1, hq=64, d=64, max_pages=1024)):
        p = sink_params(fp8, **kw)
        inner = p.fp8 if fp8 else p.paged
        n = size(ctypes.byref(p), 1, 0, -1)
        assert n == plain(ctypes.byref(inner), 1, 0) and n >= 0
        sizes = {-1: n}
        for w in (0, 127, 1000, 4095, 2 ** 40):  # a window: the window plan's bytes, never more than the full plan's
            sizes[w] = size(ctypes.byref(p), 1, 0, w)
            assert sizes[w] == win(ctypes.byref(inner), 1, 0, w) and 0 <= sizes[w] <= n
        for w, nw in sizes.items():
            if nw > 0:  # one byte less than it asks for is rejected before anything is launched
                split += 1
                rc = entry(ctypes.byref(p), 1, 0, w, ctypes.c_void_p(0x100000), nw - 1, None)
                assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()
    assert split >= 6
    assert size(ctypes.byref(sink_params(fp8, sinks=None)), 1, 0, -1) == -1
    assert size(None, 1, 0, -1) == -1


def test_sink_asm_gate_passes_on_the_built_instantiations():
    """The sink kernels are translation units of their own, in directories that none of the counts of the other
    tests match; the build's assembly gate -- no VGPR spills -- holds on them, and the sink added no vector load
    to the key loop: up to the last LDS-DMA issue every vector load from memory is an LDS-DMA, so the sink's load
    was not hoisted in front of the ring's counted vmcnt waits."""
    from flash_attention_cute_amd import _asm_check as A
    from flash_attention_cute_amd import _build

    obj = _build.ROOT / "build" / "obj"
    kinds = (("sink_*/fa_paged_sink_inst", r"_ZN2fa\d+fa_decode_paged_sinkI\w+"),
             ("sink8_*/fa_paged_fp8_sink_inst", r"_ZN2fa\d+fa_decode_fp8kv_sinkI\w+"),
             ("sinkw_*/fa_paged_window_sink_inst", r"_ZN2fa\d+fa_decode_paged_window_sinkI\w+"),
             ("sinkw8_*/fa_paged_fp8_window_sink_inst", r"_ZN2fa\d+fa_decode_fp8kv_window_sinkI\w+"))
    if not list(obj.glob(kinds[0][0] + "-hip-amdgcn-amd-amdhsa-gfx950.s")):
        pytest.skip("no -save-temps assembly (library built elsewhere)")
    for pattern, kernel in kinds:
        files = sorted(obj.glob(pattern + "-hip-amdgcn-amd-amdhsa-gfx950.s"))
        assert len(files) == len(_build.INSTANCES)
        for f in files:
            text = f.read_text()
            assert A.check_file(f) == [], f
            assert "fa_fwd_w4" not in text and "fa_decode_combine_sink" in text
            kernels = re.findall(r"^(%s):[^\n]*\n(.*?)^\.Lfunc_end" % kernel, text, flags=re.S | re.M)
            assert len(kernels) == 2, f  # with and without the fused merge
            for name, body in kernels:
                lines = body.splitlines()
                dma = [i for i, ln in enumerate(lines) if "buffer_load_dwordx4" in ln and " lds" in ln]
                assert dma, name
                loads = [ln for ln in lines[:dma[-1]]
                         if re.search(r"\b(global|flat|buffer)_load_", ln) and " lds" not in ln]
                assert loads == [], (name, loads[:3])
                after = [ln for ln in lines[dma[-1]:] if re.search(r"\b(global|flat)_load_dword\b", ln)]
                assert after, name  # the sink's own load, behind the key loop
    # the existing translation-unit directories are still the 16 each that the other tests count
    for prefix, name in _build.INST_TUS:
        assert len(list(obj.glob(f"*/{name}-hip-amdgcn-amd-amdhsa-gfx950.s"))) == len(_build.INSTANCES), name
    for glob in ("paged_*", "fp8_*", "win_*", "win8_*", "lse_*", "lse8_*", "pfill_*", "pvar_*"):
        assert len(list(obj.glob(glob))) == len(_build.INSTANCES), glob


def test_sink_host_validation_under_asan_ubsan(tmp_path):
    """The sink dispatcher's host code (csrc/fa_paged_sink_gfx950.hip, with the two dispatchers it validates
    through) built with AddressSanitizer + UBSan on the host side only and linked with host-only stub
    instantiations, run as a stand-alone program (tests/asan/paged_sink_validation_driver.cpp)."""
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
    for src in (csrc / "fa_fwd_gfx950.hip", csrc / "fa_paged_gfx950.hip", csrc / "fa_paged_sink_gfx950.hip",
                asan / "stub_instances.hip", asan / "paged_stub_instances.hip", asan / "paged_sink_stub_instances.hip",
                asan / "paged_sink_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "paged_sink_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "paged sink validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
