"""The LSE / merge addition to the C-ABI boundary (include/fa_gfx950_lse.h): the header declares its functions
beside the unchanged headers, both libraries export them, the structs have the header's layout and the
descriptions are validated with the documented codes -- host-only calls, no GPU needed."""
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
HEADER = ROOT / "include" / "fa_gfx950_lse.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
LSE = {"fa_fwd_gfx950_paged_lse", "fa_fwd_gfx950_paged_lse_workspace_size", "fa_fwd_gfx950_paged_lse_check",
       "fa_fwd_gfx950_paged_lse_fp8", "fa_fwd_gfx950_paged_lse_fp8_workspace_size", "fa_fwd_gfx950_paged_lse_fp8_check",
       "fa_merge_states_gfx950", "fa_merge_states_gfx950_check", "fa_lse_version"}
_TAIL = [("lse_ptr", ctypes.c_void_p), ("lse_batch_stride", ctypes.c_int64), ("lse_head_stride", ctypes.c_int64),
         ("lse_seqlen_stride", ctypes.c_int64), ("seqlen_offset", ctypes.c_int64)]
_I64 = ctypes.c_int64


class FaPagedLseParams(ctypes.Structure):
    _fields_ = [("paged", FaPagedParams)] + _TAIL


class FaPagedFp8LseParams(ctypes.Structure):
    _fields_ = [("fp8", FaPagedFp8Params)] + _TAIL


class FaMergeParams(ctypes.Structure):
    _fields_ = ([("outs", ctypes.c_void_p), ("lses", ctypes.c_void_p), ("out", ctypes.c_void_p),
                 ("lse", ctypes.c_void_p)] +
                [(n, _I64) for n in ("num_parts", "batch_size", "num_heads", "seqlen", "headdim")] +
                [(f"{t}_{d}_stride", _I64) for t in ("outs", "lses") for d in ("part", "batch", "head", "seqlen")] +
                [(f"{t}_{d}_stride", _I64) for t in ("out", "lse") for d in ("batch", "head", "seqlen")])


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    for name in ("fa_fwd_gfx950_paged_lse_workspace_size", "fa_fwd_gfx950_paged_lse_fp8_workspace_size",
                 "fa_fwd_gfx950_paged_workspace_size", "fa_fwd_gfx950_paged_fp8_workspace_size"):
        getattr(lib, name).restype = ctypes.c_int64
    for name in ("fa_fwd_gfx950_paged_lse", "fa_fwd_gfx950_paged_lse_fp8"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64, ctypes.c_void_p, _I64,
                                       ctypes.c_void_p]
        getattr(lib, name + "_check").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64]
        getattr(lib, name + "_workspace_size").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _I64]
    return lib


def lse_params(fp8=False, b=32, hq=32, sq=1, **kw):
    """A decode step as the torch binding passes it to the LSE entries: no q-head pack."""
    tail = {k: kw.pop(k) for k in list(kw) if k in dict(_TAIL)}
    if fp8:
        p = FaPagedFp8LseParams(fp8_params(b=b, hq=hq, sq=sq, pack=False, **kw), 0x90000, hq * sq, sq, 1, 0)
    else:
        p = FaPagedLseParams(paged_params(b=b, hq=hq, sq=sq, pack=False, **kw), 0x90000, hq * sq, sq, 1, 0)
    for key, val in tail.items():
        setattr(p, key, val)
    return p


def check(lib, p, dtype=1, causal=0, window_left=-1):
    fn = lib.fa_fwd_gfx950_paged_lse_fp8_check if isinstance(p, FaPagedFp8LseParams) else lib.fa_fwd_gfx950_paged_lse_check
    rc = fn(ctypes.byref(p), dtype, causal, window_left)
    return rc, lib.fa_last_error().decode()


def merge_params(n=2, b=4, h=8, s=1, d=128, **kw):
    p = FaMergeParams(0x100000, 0x200000, 0x300000, 0x400000, n, b, h, s, d,
                      b * h * s * d, h * s * d, s * d, d, b * h * s, h * s, s, 1, h * s * d, s * d, d, h * s, s, 1)
    for key, val in kw.items():
        setattr(p, key, val)
    return p


def merge_check(lib, p, dtype=1):
    rc = lib.fa_merge_states_gfx950_check(ctypes.byref(p), dtype)
    return rc, lib.fa_last_error().decode()


def test_lse_header_declares_its_functions_and_leaves_the_old_headers_alone():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == LSE
    assert '#include "fa_gfx950_paged.h"' in text and re.search(r"#define FA_GFX950_LSE_VERSION 1\b", text)
    assert re.search(r"#define FA_MERGE_MAX_PARTS (\d+)\b", text) and int(
        re.search(r"#define FA_MERGE_MAX_PARTS (\d+)\b", text).group(1)) >= 8
    for old in ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h", "fa_gfx950_fp8.h",
                "fa_gfx950_paged_window.h", "fa_gfx950_paged_prefill.h"):
        low = (ROOT / "include" / old).read_text().lower()
        assert "lse" not in low.replace("else", "").replace("false", ""), old


def test_the_existing_dispatchers_reference_no_new_symbol():
    csrc = ROOT / "flash_attention_cute_amd" / "csrc"
    for name in ("fa_fwd_gfx950.hip", "fa_paged_gfx950.hip"):
        text = (csrc / name).read_text()
        assert "_lse" not in text and "merge_states" not in text and "fa_gfx950_lse.h" not in text, name


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_lse_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert LSE <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_lse_version_and_the_other_versions(lib):
    assert lib.fa_lse_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    assert lib.fa_fp8_version() == 1 and lib.fa_paged_window_version() == 1 and lib.fa_paged_prefill_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.lse_version() == 1


def test_lse_struct_layouts():
    for outer, inner in ((FaPagedLseParams, FaPagedParams), (FaPagedFp8LseParams, FaPagedFp8Params)):
        base = ctypes.sizeof(inner)
        assert ctypes.sizeof(outer) == base + 5 * 8
        assert [getattr(outer, n).offset for n, _ in _TAIL] == [base + 8 * i for i in range(5)]
    assert ctypes.sizeof(FaMergeParams) == (4 + 5 + 8 + 6) * 8
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, first in (("fa_paged_lse_params", "fa_paged_params paged;"),
                        ("fa_paged_fp8_lse_params", "fa_paged_fp8_params fp8;")):
        body = " ".join(re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1).split())
        assert body == (f"{first} float *lse_ptr; int64_t lse_batch_stride, lse_head_stride, lse_seqlen_stride; "
                        "int64_t seqlen_offset;"), body
    body = " ".join(re.search(r"typedef struct fa_merge_params \{(.*?)\} fa_merge_params;", text, flags=re.S).group(1).split())
    names = re.findall(r"(\w+)(?=[,;])", body)
    assert names == [n for n, _ in FaMergeParams._fields_], names


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_lse_check_accepts_valid(lib, fp8):
    assert check(lib, lse_params(fp8)) == (FA_OK, "")
    assert check(lib, lse_params(fp8, page_size=32, max_pages=128), dtype=0)[0] == FA_OK
    assert check(lib, lse_params(fp8, sq=2), causal=1)[0] == FA_OK  # g 4 x Sq 2
    assert check(lib, lse_params(fp8, b=2, hq=32, sq=16, lse_batch_stride=16 * 32, lse_head_stride=1,
                                 lse_seqlen_stride=32))[0] == FA_OK  # a shared-prefix group: 64 rows, permuted lse
    assert check(lib, lse_params(fp8, seqlens_k=None, seqlen_offset=2048))[0] == FA_OK
    assert check(lib, lse_params(fp8, seqlen_offset=-2048))[0] == FA_OK
    assert check(lib, lse_params(fp8, seqlen_offset=2 ** 30))[0] == FA_OK
    assert check(lib, lse_params(fp8, lse_batch_stride=0, lse_head_stride=0, lse_seqlen_stride=0))[0] == FA_OK
    assert check(lib, lse_params(fp8), window_left=-(2 ** 40))[0] == FA_OK


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_lse_check_rejects_invalid(lib, fp8):
    def bad(code, word, window_left=-1, **kw):
        rc, msg = check(lib, lse_params(fp8, **kw), window_left=window_left)
        assert rc == code and word in msg, (rc, msg)

    bad(FA_ERR_INVALID_ARGUMENT, "lse_ptr is NULL", lse_ptr=None)
    bad(FA_ERR_INVALID_ARGUMENT, "4-byte aligned", lse_ptr=0x90002)
    for field in ("lse_batch_stride", "lse_head_stride", "lse_seqlen_stride"):
        bad(FA_ERR_INVALID_ARGUMENT, "non-negative", **{field: -1})
    bad(FA_ERR_INVALID_ARGUMENT, "seqlen_offset", seqlen_offset=2 ** 30 + 1)
    bad(FA_ERR_INVALID_ARGUMENT, "seqlen_offset", seqlen_offset=-(2 ** 30) - 1)
    for w in (0, 1, 4095, 2 ** 40):
        bad(FA_ERR_UNSUPPORTED, "window", window_left=w)
    # the base description is the paged decode check's: its codes and its messages
    bad(FA_ERR_INVALID_ARGUMENT, "page_size", page_size=48, max_pages=32)
    bad(FA_ERR_UNSUPPORTED, "decode", sq=17)  # g 4 x Sq 17: past the decode rule
    bad(FA_ERR_INVALID_ARGUMENT, "block_table", block_table=None)
    bad(FA_ERR_INVALID_ARGUMENT, "block_table", block_table=None, seqlens_k=None)
    assert lib.fa_fwd_gfx950_paged_lse_check(None, 1, 0, -1) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_fwd_gfx950_paged_lse_fp8_check(None, 1, 0, -1) == FA_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_lse_workspace_is_the_one_of_the_entry_without_the_lse(lib, fp8):
    size = lib.fa_fwd_gfx950_paged_lse_fp8_workspace_size if fp8 else lib.fa_fwd_gfx950_paged_lse_workspace_size
    old = lib.fa_fwd_gfx950_paged_fp8_workspace_size if fp8 else lib.fa_fwd_gfx950_paged_workspace_size
    entry = lib.fa_fwd_gfx950_paged_lse_fp8 if fp8 else lib.fa_fwd_gfx950_paged_lse
    for kw in (dict(b=1, max_pages=256), dict(b=2, max_pages=64), dict(b=64, max_pages=8)):
        p = lse_params(fp8, **kw)
        inner = p.fp8 if fp8 else p.paged
        n = size(ctypes.byref(p), 1, 0, -1)
        assert n == old(ctypes.byref(inner), 1, 0) and n >= 0
        assert size(ctypes.byref(p), 1, 0, 5) == -1  # a window
        if n > 0:  # one byte less than it asks for is rejected before anything is launched
            rc = entry(ctypes.byref(p), 1, 0, -1, ctypes.c_void_p(0x100000), n - 1, None)
            assert rc == FA_ERR_INVALID_ARGUMENT and b"workspace" in lib.fa_last_error()
    assert size(ctypes.byref(lse_params(fp8, lse_ptr=None)), 1, 0, -1) == -1
    assert size(None, 1, 0, -1) == -1


def test_merge_check(lib):
    assert merge_check(lib, merge_params())[0] == FA_OK  # (a stand-alone entry: success leaves fa_last_error as it was)
    assert merge_check(lib, merge_params(n=1), dtype=0)[0] == FA_OK
    assert merge_check(lib, merge_params(n=16, d=72))[0] == FA_OK
    assert merge_check(lib, merge_params(lse=None))[0] == FA_OK
    assert merge_check(lib, merge_params(b=0))[0] == FA_OK
    # a bshd-transposed input: head stride D, seq stride H * D
    assert merge_check(lib, merge_params(s=3, outs_head_stride=128, outs_seqlen_stride=8 * 128))[0] == FA_OK

    def bad(code, word, dtype=1, **kw):
        rc, msg = merge_check(lib, merge_params(**kw), dtype)
        assert rc == code and word in msg, (rc, msg)

    bad(FA_ERR_INVALID_ARGUMENT, "num_parts", n=0)
    bad(FA_ERR_INVALID_ARGUMENT, "num_parts", n=17)
    bad(FA_ERR_INVALID_ARGUMENT, "multiple of 8", d=68)
    bad(FA_ERR_INVALID_ARGUMENT, "multiple of 8", d=0)
    bad(FA_ERR_INVALID_ARGUMENT, "non-NULL", outs=None)
    bad(FA_ERR_INVALID_ARGUMENT, "non-NULL", lses=None)
    bad(FA_ERR_INVALID_ARGUMENT, "non-NULL", out=None)
    bad(FA_ERR_INVALID_ARGUMENT, "16-byte aligned", outs=0x100008)
    bad(FA_ERR_INVALID_ARGUMENT, "16-byte aligned", out=0x300002)
    bad(FA_ERR_INVALID_ARGUMENT, "4-byte aligned", lses=0x200002)
    bad(FA_ERR_INVALID_ARGUMENT, "4-byte aligned", lse=0x400001)
    bad(FA_ERR_INVALID_ARGUMENT, "multiples of 8", outs_head_stride=132)
    bad(FA_ERR_INVALID_ARGUMENT, "multiples of 8", out_batch_stride=-8)
    bad(FA_ERR_INVALID_ARGUMENT, "non-negative", lses_part_stride=-1)
    bad(FA_ERR_INVALID_ARGUMENT, "non-negative", b=-1)
    bad(FA_ERR_UNSUPPORTED, "fp16 / bf16", dtype=7)
    bad(FA_ERR_UNSUPPORTED, "too many rows", b=2 ** 31)
    assert lib.fa_merge_states_gfx950_check(None, 1) == FA_ERR_INVALID_ARGUMENT
    # the launch validates first (nothing is launched for an invalid description)
    lib.fa_merge_states_gfx950.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert lib.fa_merge_states_gfx950(ctypes.byref(merge_params(n=0)), 1, None) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_merge_states_gfx950(ctypes.byref(merge_params(b=0)), 1, None) == FA_OK  # no rows: no launch


def test_lse_host_validation_under_asan_ubsan(tmp_path):
    """The LSE dispatcher's host code (csrc/fa_paged_lse_gfx950.hip, with the two dispatchers it validates
    through) built with AddressSanitizer + UBSan on the host side only and linked with host-only stub
    instantiations, run as a stand-alone program (tests/asan/paged_lse_validation_driver.cpp)."""
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
    for src in (csrc / "fa_fwd_gfx950.hip", csrc / "fa_paged_gfx950.hip", csrc / "fa_paged_lse_gfx950.hip",
                asan / "stub_instances.hip", asan / "paged_stub_instances.hip", asan / "paged_lse_stub_instances.hip",
                asan / "paged_lse_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "paged_lse_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "paged lse validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
