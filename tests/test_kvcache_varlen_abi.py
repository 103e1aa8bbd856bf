"""The ragged KV-cache append's addition to the C-ABI boundary (include/fa_gfx950_kvcache_varlen.h): the header
declares its three functions and no older header knows of them, both libraries export them, and the check entry
rejects what the launch would -- host-only calls, no GPU needed."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_abi import FA_ERR_INVALID_ARGUMENT, FA_ERR_UNSUPPORTED, FA_OK

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "fa_gfx950_kvcache_varlen.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
ENTRIES = {"fa_kvcache_append_varlen_gfx950", "fa_kvcache_append_varlen_gfx950_check", "fa_kvcache_varlen_version"}
OLD_HEADERS = ("fa_gfx950.h", "fa_gfx950_paged.h", "fa_gfx950_kvcache.h", "fa_gfx950_fp8.h", "fa_gfx950_paged_window.h",
               "fa_gfx950_paged_prefill.h", "fa_gfx950_lse.h")
P, I64 = ctypes.c_void_p, ctypes.c_int64


class FaKvcacheVarlenParams(ctypes.Structure):
    _fields_ = [("k_new", P), ("v_new", P), ("kn_row_stride", I64), ("kn_head_stride", I64), ("vn_row_stride", I64),
                ("vn_head_stride", I64), ("cu_seqlens_new", P), ("total_new", I64), ("q", P), ("q_out", P),
                ("q_row_stride", I64), ("q_head_stride", I64), ("qo_row_stride", I64), ("qo_head_stride", I64),
                ("cu_seqlens_q", P), ("total_q", I64), ("cos", P), ("sin", P), ("cs_row_stride", I64), ("max_pos", I64),
                ("k_cache", P), ("v_cache", P), ("k_page_stride", I64), ("k_head_stride", I64), ("k_row_stride", I64),
                ("v_page_stride", I64), ("v_head_stride", I64), ("v_row_stride", I64), ("block_table", P),
                ("block_table_stride", I64), ("max_pages", I64), ("num_pages", I64), ("page_size", I64),
                ("seqlens_k", P), ("seqlens_out", P), ("batch_size", I64), ("num_heads_q", I64), ("num_heads_kv", I64),
                ("headdim", I64)]


def params(b=7, hkv=2, g=4, total_new=341, total_q=341, max_pages=8, page=64, d=128, **kw):
    p = FaKvcacheVarlenParams()
    if total_new > 0:
        p.k_new, p.v_new = 0x10000, 0x20000
    p.kn_row_stride = p.vn_row_stride = hkv * d
    p.kn_head_stride = p.vn_head_stride = d
    p.cu_seqlens_new, p.total_new = 0x30000, total_new
    if total_q > 0:
        p.q, p.q_out, p.cu_seqlens_q = 0x40000, 0x50000, 0x60000
    p.q_row_stride = p.qo_row_stride = hkv * g * d
    p.q_head_stride = p.qo_head_stride = d
    p.total_q = total_q
    p.cos, p.sin, p.cs_row_stride, p.max_pos = 0x70000, 0x80000, d, max_pages * page
    p.k_cache, p.v_cache = 0x90000, 0xA0000
    p.k_page_stride = p.v_page_stride = hkv * page * d
    p.k_head_stride = p.v_head_stride = page * d
    p.k_row_stride = p.v_row_stride = d
    p.block_table, p.block_table_stride, p.max_pages, p.num_pages, p.page_size = 0xB0000, max_pages, max_pages, 4096, page
    p.seqlens_k, p.seqlens_out = 0xC0000, 0xD0000
    p.batch_size, p.num_heads_q, p.num_heads_kv, p.headdim = b, hkv * g, hkv, d
    for key, val in kw.items():
        assert hasattr(p, key), key
        setattr(p, key, val)
    return p


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    lib.fa_kvcache_append_varlen_gfx950.argtypes = [P, ctypes.c_int, P]
    lib.fa_kvcache_append_varlen_gfx950_check.argtypes = [P, ctypes.c_int]
    return lib


def test_header_declares_its_functions_and_no_old_header_mentions_them():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == ENTRIES
    assert re.search(r"#define FA_GFX950_KVCACHE_VARLEN_VERSION 1\b", text)
    assert '#include "fa_gfx950.h"' in text
    # the ctypes mirror above has the header's fields, in its order
    body = re.search(r"typedef struct fa_kvcache_varlen_params \{(.*?)\} fa_kvcache_varlen_params;", text, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)  # (a field's name is what a `,` or `;` follows)
    assert names == [f[0] for f in FaKvcacheVarlenParams._fields_], names
    for old in OLD_HEADERS:
        assert "kvcache_varlen" not in (ROOT / "include" / old).read_text().lower(), old
    import test_kvcache_abi

    test_kvcache_abi.test_kvcache_header_declares_its_functions_and_leaves_the_old_headers_alone()


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert ENTRIES <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_version_and_the_other_versions(lib):
    assert lib.fa_kvcache_varlen_version() == 1
    assert lib.fa_abi_version() == 8 and lib.fa_paged_version() == 1 and lib.fa_kvcache_version() == 1
    assert lib.fa_fp8_version() == 1 and lib.fa_paged_window_version() == 1 and lib.fa_paged_prefill_version() == 1
    assert lib.fa_lse_version() == 1
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.kvcache_varlen_version() == 1


ACCEPTED = [{}, {"total_new": 0}, {"total_q": 0}, {"total_new": 0, "total_q": 0}, {"page": 96, "max_pages": 4},
            {"d": 2}, {"b": 1, "block_table_stride": 0}, {"seqlens_out": None}]
TABLE = [  # (how to break it, code, a word of the message)
    ({"cu_seqlens_q": None}, FA_ERR_INVALID_ARGUMENT, b"cu_seqlens_q"),
    ({"cu_seqlens_q": 0x60002}, FA_ERR_INVALID_ARGUMENT, b"aligned"),
    ({"cu_seqlens_new": None}, FA_ERR_INVALID_ARGUMENT, b"cu_seqlens_new"),
    ({"cu_seqlens_new": 0x30001}, FA_ERR_INVALID_ARGUMENT, b"aligned"),
    ({"total_q": -1}, FA_ERR_INVALID_ARGUMENT, b"non-negative"),
    ({"total_new": -5}, FA_ERR_INVALID_ARGUMENT, b"non-negative"),
    ({"total_q": 2 ** 31}, FA_ERR_UNSUPPORTED, b"too large"),
    ({"page_size": 48}, FA_ERR_INVALID_ARGUMENT, b"page_size"),
    ({"page_size": 0}, FA_ERR_INVALID_ARGUMENT, b"page_size"),
    ({"block_table": None}, FA_ERR_UNSUPPORTED, b"paged caches only"),
    ({"seqlens_k": None}, FA_ERR_INVALID_ARGUMENT, b"seqlens_k"),
    ({"seqlens_out": 0xC0004}, FA_ERR_INVALID_ARGUMENT, b"overlap"),
    ({"num_pages": 0}, FA_ERR_INVALID_ARGUMENT, b"num_pages"),
    ({"block_table_stride": 4}, FA_ERR_INVALID_ARGUMENT, b"block_table_stride"),
    ({"k_new": None}, FA_ERR_INVALID_ARGUMENT, b"k_new"),
    ({"q_out": None}, FA_ERR_INVALID_ARGUMENT, b"q_out"),
    ({"sin": None}, FA_ERR_INVALID_ARGUMENT, b"together"),
    ({"cos": None, "sin": None}, FA_ERR_INVALID_ARGUMENT, b"rotated only"),
    ({"num_heads_q": 3}, FA_ERR_INVALID_ARGUMENT, b"num_heads_q"),
    ({"headdim": 127}, FA_ERR_INVALID_ARGUMENT, b"even"),
    ({"max_pos": 0}, FA_ERR_INVALID_ARGUMENT, b"max_pos"),
]


def test_check_accepts_ragged_steps(lib):
    for kw in ACCEPTED:
        for dtype in (0, 1):
            assert lib.fa_kvcache_append_varlen_gfx950_check(ctypes.byref(params(**kw)), dtype) == FA_OK, kw
            assert lib.fa_last_error() == b""
    assert lib.fa_kvcache_append_varlen_gfx950(ctypes.byref(params(b=0, total_new=0, total_q=0)), 1, None) == FA_OK


@pytest.mark.parametrize("kw,want,word", TABLE, ids=[",".join(f"{k}={v}" for k, v in t[0].items()) for t in TABLE])
def test_check_table(lib, kw, want, word):
    p = params(**kw)
    assert lib.fa_kvcache_append_varlen_gfx950_check(ctypes.byref(params()), 1) == FA_OK  # (clears the message)
    assert lib.fa_kvcache_append_varlen_gfx950_check(ctypes.byref(p), 1) == want
    assert word in lib.fa_last_error(), lib.fa_last_error()
    assert lib.fa_kvcache_append_varlen_gfx950(ctypes.byref(p), 1, None) == want  # validates first: nothing is launched


def test_check_refuses_fp8_and_null(lib):
    for dtype in (2, 3, -1):  # (0 / 1 are fp16 / bf16: the quantizing append is fa_gfx950_fp8.h's)
        assert lib.fa_kvcache_append_varlen_gfx950_check(ctypes.byref(params()), dtype) == FA_ERR_UNSUPPORTED
        assert b"fp16 / bf16" in lib.fa_last_error()
    assert lib.fa_kvcache_append_varlen_gfx950_check(None, 1) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_kvcache_append_varlen_gfx950(None, 1, None) == FA_ERR_INVALID_ARGUMENT


def test_both_append_kernels_share_one_definition_of_the_movers():
    """move_vec / move_pair (the rotation with fa_rope.hip's fp32 pin) are DEFINED once, in fa_kvcache_move.h, and
    both append sources include that header instead of defining movers of their own; the new sources are in the
    build list. What the movers compute is held bit for bit by the GPU append tests."""
    from flash_attention_cute_amd import _build

    definition = re.compile(r"\bvoid\s+(move_vec|move_pair)\s*\(")
    shared = (_build.CSRC / "fa_kvcache_move.h").read_text()
    assert sorted(definition.findall(shared)) == ["move_pair", "move_vec"]
    assert 'asm volatile("" : "+v"(a), "+v"(bb));' in shared  # (the pin test_kvcache_abi.py once found in fa_kvcache.hip)
    for name in ("fa_kvcache.hip", "fa_kvcache_varlen.hip"):
        src = (_build.CSRC / name).read_text()
        assert '#include "fa_kvcache_move.h"' in src and not definition.search(src), name
    build = Path(_build.__file__).read_text()
    assert '"fa_kvcache_varlen.hip"' in build and '"fa_paged_varlen_gfx950.hip"' in build
    # the public headers (two more now) are inputs of every kernel object, not only of the dispatchers
    assert re.search(r"inst_deps = \(.*?sorted\(INCLUDE\.glob\(\"\*\.h\"\)\)\)", build, flags=re.S)


def test_kvcache_varlen_host_validation_under_asan_ubsan(tmp_path):
    """The ragged append's host code (csrc/fa_kvcache_varlen.hip, with csrc/fa_fwd_gfx950.hip for the error
    channel) built with AddressSanitizer + UBSan on the host side only and linked with the host-only stub
    instantiations, run as a stand-alone program (tests/asan/kvcache_varlen_validation_driver.cpp): only the check
    entry, and the launch entry with parameters that fail validation or launch nothing."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    csrc = ROOT / "flash_attention_cute_amd" / "csrc"
    inc = [f"-I{ROOT / 'include'}", f"-I{csrc}"]
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined"]
    base = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fPIC", *san, *inc, "-c"]
    objs = []
    for src in (csrc / "fa_fwd_gfx950.hip", csrc / "fa_kvcache.hip", csrc / "fa_kvcache_varlen.hip",
                ROOT / "tests" / "asan" / "stub_instances.hip",
                ROOT / "tests" / "asan" / "kvcache_varlen_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "kvcache_varlen_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "kvcache varlen validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
