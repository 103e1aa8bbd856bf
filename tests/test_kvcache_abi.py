"""The KV-cache append addition to the C-ABI boundary (include/fa_gfx950_kvcache.h): the header declares
its three functions beside the unchanged fa_gfx950.h and fa_gfx950_paged.h, both libraries export them,
and the description of the new tokens, the tables, the cache and the lengths is validated with the
documented codes -- host-only calls, no GPU needed."""
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
HEADER = ROOT / "include" / "fa_gfx950_kvcache.h"
LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950.so"
DEBUG_LIB = ROOT / "flash_attention_cute_amd" / "lib" / "libfa_gfx950_debug.so"
KVCACHE = {"fa_kvcache_append_gfx950", "fa_kvcache_append_gfx950_check", "fa_kvcache_version"}


def params_type():
    from flash_attention_cute_amd._debug import FaKvcacheParams

    return FaKvcacheParams


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists():
        pytest.skip("libfa_gfx950.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  -- same process layout as the product (torch's HIP runtime first)

    lib = ctypes.CDLL(str(LIB))
    lib.fa_last_error.restype = ctypes.c_char_p
    lib.fa_kvcache_append_gfx950.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.fa_kvcache_append_gfx950_check.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return lib


def kv_params(b=32, hq=32, hkv=8, sn=1, sq=1, d=128, max_pages=32, page_size=128, num_pages=2048, rope=True,
              dense=False, pshd=False, **kw):
    """A decode step's append on a [num_pages, Hkv, page_size, D] pool (pshd: flash-attn's [P, page, Hkv,
    D] view; dense: [B, Hkv, page_size, D] and no table), as the torch binding passes it."""
    p = params_type()()
    if sn:
        p.k_new, p.v_new = 0x10000, 0x20000
        for t in "kv":
            setattr(p, f"{t}n_batch_stride", hkv * sn * d)
            setattr(p, f"{t}n_head_stride", sn * d)
            setattr(p, f"{t}n_seqlen_stride", d)
    if sq:
        p.q, p.q_out = 0x30000, 0x40000
        for t in ("q", "qo"):
            setattr(p, f"{t}_batch_stride", hq * sq * d)
            setattr(p, f"{t}_head_stride", sq * d)
            setattr(p, f"{t}_seqlen_stride", d)
    if rope:
        p.cos, p.sin, p.cs_row_stride, p.max_pos = 0x50000, 0x60000, d, 8192
    p.k_cache, p.v_cache = 0x100000, 0x200000
    for t in "kv":
        setattr(p, f"{t}_page_stride", hkv * page_size * d)
        setattr(p, f"{t}_head_stride", d if pshd else page_size * d)
        setattr(p, f"{t}_row_stride", hkv * d if pshd else d)
    if dense:
        max_pages, num_pages = 1, b
    else:
        p.block_table, p.block_table_stride = 0x70000, max_pages
    p.max_pages, p.num_pages, p.page_size = max_pages, num_pages, page_size
    p.seqlens_k, p.seqlens_out = 0x80000, 0x90000
    p.batch_size, p.num_heads_q, p.num_heads_kv = b, hq if sq else 0, hkv
    p.seqlen_new, p.seqlen_q, p.headdim = sn, sq, d
    for key, val in kw.items():
        assert hasattr(p, key), key
        setattr(p, key, val)
    return p


def check(lib, p, dtype=1):
    rc = lib.fa_kvcache_append_gfx950_check(ctypes.byref(p), dtype)
    return rc, lib.fa_last_error().decode()


def test_kvcache_header_declares_its_functions_and_leaves_the_old_headers_alone():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(fa_\w+)\s*\(", text)) == KVCACHE
    assert '#include "fa_gfx950.h"' in text and re.search(r"#define FA_GFX950_KVCACHE_VERSION 1\b", text)
    import test_abi
    import test_paged_abi

    test_abi.test_header_declares_the_boundary()  # include/fa_gfx950.h: the same set as before
    test_paged_abi.test_paged_header_declares_its_four_functions_and_leaves_the_old_header_alone()
    for old in ("fa_gfx950.h", "fa_gfx950_paged.h"):
        assert "fa_kvcache" not in (ROOT / "include" / old).read_text()
    # the write rule and the aliasing rule are part of the contract
    doc = HEADER.read_text()
    assert "DROPPED, never redirected" in doc and "must not overlap seqlens_k" in doc


@pytest.mark.parametrize("path", [LIB, DEBUG_LIB], ids=["product", "debug"])
def test_both_libraries_export_the_kvcache_entry_points(path):
    if not path.exists():
        pytest.skip(f"{path.name} not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
    assert KVCACHE <= set(re.findall(r" T (fa_\w+)$", out, flags=re.M))


def test_kvcache_version_and_the_other_versions(lib):
    assert lib.fa_kvcache_version() == 1
    assert lib.fa_abi_version() == 8  # the dense boundary did not move
    assert lib.fa_paged_version() == 1  # nor the paged one
    from flash_attention_cute_amd import flash_attention as fam

    if fam.flash_attention_cuda is not None:
        assert fam.flash_attention_cuda.kvcache_version() == 1


def test_kvcache_struct_layout():
    t = params_type()
    assert ctypes.sizeof(t) == 41 * 8  # 11 pointers + 30 int64, no padding
    names = [n for n, _ in t._fields_]
    assert [getattr(t, n).offset for n in names] == [8 * i for i in range(41)]
    # the order of the header's struct
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct fa_kvcache_params \{(.*?)\} fa_kvcache_params;", text, flags=re.S).group(1)
    declared = [m for stmt in body.split(";") for m in re.findall(r"[\*\s,](\w+)\s*(?=,|$)", stmt.strip())]
    assert declared == names


def test_kvcache_check_accepts_valid(lib):
    assert check(lib, kv_params()) == (FA_OK, "")
    assert check(lib, kv_params(page_size=32, max_pages=128), dtype=0)[0] == FA_OK
    assert check(lib, kv_params(dense=True, page_size=100))[0] == FA_OK  # a dense cache: Smax is not a multiple of 32
    assert check(lib, kv_params(pshd=True))[0] == FA_OK  # flash-attn's [P, page, Hkv, D] view
    assert check(lib, kv_params(b=4, sn=4096, sq=0, rope=False))[0] == FA_OK  # prefill append, no rotation
    assert check(lib, kv_params(sn=0))[0] == FA_OK  # q rotation alone
    assert check(lib, kv_params(d=72, sn=3, sq=3))[0] == FA_OK  # the element path
    assert check(lib, kv_params(d=71, sq=0, rope=False))[0] == FA_OK  # an odd D without tables
    assert check(lib, kv_params(seqlens_out=None))[0] == FA_OK
    assert check(lib, kv_params(b=0))[0] == FA_OK
    # every alignment works: the element path takes odd bases and strides
    assert check(lib, kv_params(k_cache=0x100002, k_row_stride=130, kn_seqlen_stride=129))[0] == FA_OK
    # nothing to do is no launch and no error, without a stream or a device
    assert lib.fa_kvcache_append_gfx950(ctypes.byref(kv_params(b=0)), 1, None) == FA_OK
    assert lib.fa_kvcache_append_gfx950(ctypes.byref(kv_params(sn=0, sq=0, rope=False)), 1, None) == FA_OK


@pytest.mark.parametrize("kw,code,msg", [
    ({"seqlens_k": None}, FA_ERR_INVALID_ARGUMENT, "non-NULL"),
    ({"seqlens_k": 0x80002}, FA_ERR_INVALID_ARGUMENT, "4-byte aligned"),
    ({"seqlens_out": 0x90001}, FA_ERR_INVALID_ARGUMENT, "4-byte aligned"),
    ({"block_table": 0x70002}, FA_ERR_INVALID_ARGUMENT, "4-byte aligned"),
    ({"batch_size": -1}, FA_ERR_INVALID_ARGUMENT, "non-negative"),
    ({"seqlen_new": -1}, FA_ERR_INVALID_ARGUMENT, "non-negative"),
    ({"num_heads_kv": 0}, FA_ERR_INVALID_ARGUMENT, "at least 1"),
    ({"headdim": 0}, FA_ERR_INVALID_ARGUMENT, "at least 1"),
    ({"num_heads_q": 12}, FA_ERR_INVALID_ARGUMENT, "multiple of num_heads_kv"),
    ({"num_heads_q": 0}, FA_ERR_INVALID_ARGUMENT, "multiple of num_heads_kv"),
    ({"page_size": 48}, FA_ERR_INVALID_ARGUMENT, "multiple of 32"),
    ({"page_size": 0}, FA_ERR_INVALID_ARGUMENT, "multiple of 32"),
    ({"num_pages": 0}, FA_ERR_INVALID_ARGUMENT, "at least 1"),
    ({"max_pages": 0}, FA_ERR_INVALID_ARGUMENT, "at least 1"),
    ({"block_table_stride": 16}, FA_ERR_INVALID_ARGUMENT, "block_table_stride"),
    ({"num_pages": 1 << 40}, FA_ERR_UNSUPPORTED, "too large"),
    ({"max_pages": 1 << 40, "block_table_stride": 1 << 40}, FA_ERR_UNSUPPORTED, "too large"),
    ({"batch_size": 1 << 40}, FA_ERR_UNSUPPORTED, "too large"),
    ({"cos": None, "sin": None}, FA_ERR_INVALID_ARGUMENT, "needs the cos / sin tables"),
    ({"sin": None}, FA_ERR_INVALID_ARGUMENT, "given together"),
    ({"headdim": 71}, FA_ERR_INVALID_ARGUMENT, "even head dim"),
    ({"max_pos": 0}, FA_ERR_INVALID_ARGUMENT, "max_pos"),
    ({"v_new": None}, FA_ERR_INVALID_ARGUMENT, "k_new and v_new"),
    ({"q_out": None}, FA_ERR_INVALID_ARGUMENT, "q and q_out"),
    ({"k_cache": None}, FA_ERR_INVALID_ARGUMENT, "k_cache and v_cache"),
    ({"seqlens_out": 0x80000}, FA_ERR_INVALID_ARGUMENT, "must not overlap"),
    ({"seqlens_out": 0x80000 + 31 * 4}, FA_ERR_INVALID_ARGUMENT, "must not overlap"),
    ({"seqlens_out": 0x80000 - 31 * 4}, FA_ERR_INVALID_ARGUMENT, "must not overlap"),
])
def test_kvcache_check_and_launch_reject_without_touching_the_device(lib, kw, code, msg):
    p = kv_params(**kw)
    rc, err = check(lib, p)
    assert rc == code and msg in err, err
    # the launch entry validates first: NULL stream, bogus pointers, nothing is launched
    assert lib.fa_kvcache_append_gfx950(ctypes.byref(p), 1, None) == code


def test_kvcache_check_more(lib):
    rc, err = check(lib, kv_params(), dtype=7)
    assert rc == FA_ERR_UNSUPPORTED and "fp16 / bf16" in err
    assert lib.fa_kvcache_append_gfx950_check(None, 1) == FA_ERR_INVALID_ARGUMENT
    assert lib.fa_kvcache_append_gfx950(None, 1, None) == FA_ERR_INVALID_ARGUMENT
    # adjacent length arrays do not overlap
    assert check(lib, kv_params(seqlens_out=0x80000 + 32 * 4))[0] == FA_OK
    assert check(lib, kv_params(seqlens_out=0x80000 - 32 * 4))[0] == FA_OK
    # a dense cache has one "page" per sequence, and no page-size rule
    p = kv_params(dense=True)
    p.max_pages = 2
    rc, err = check(lib, p)
    assert rc == FA_ERR_INVALID_ARGUMENT and "max_pages 1" in err
    assert check(lib, kv_params(dense=True, page_size=48))[0] == FA_OK
    p = kv_params(dense=True)
    p.num_pages = 1 << 40  # ignored without a table, as the header says
    assert check(lib, p)[0] == FA_OK


def test_kvcache_source_is_a_translation_unit_of_its_own():
    """One more dispatcher-style source in the build list, outside the AGPR / spill gate's file list; the
    rotation's fp32 pin is fa_rope.hip's."""
    from flash_attention_cute_amd import _build

    src = (_build.CSRC / "fa_kvcache.hip").read_text()
    assert '"fa_kvcache.hip"' in Path(_build.__file__).read_text()
    assert 'asm volatile("" : "+v"(a), "+v"(bb));' in src
    assert 'asm volatile("" : "+v"(a), "+v"(bb));' in (_build.CSRC / "fa_rope.hip").read_text()
    assert "contiguous()" not in src and "hipMalloc" not in src and "Synchronize" not in src


def test_kvcache_host_validation_under_asan_ubsan(tmp_path):
    """The append's host code (csrc/fa_kvcache.hip, with csrc/fa_fwd_gfx950.hip for the error channel) built
    with AddressSanitizer + UBSan on the host side only and linked with the host-only stub instantiations,
    run as a stand-alone program (tests/asan/kvcache_validation_driver.cpp): only the check entry, and the
    launch entry with parameters that fail validation or launch nothing."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    csrc = ROOT / "flash_attention_cute_amd" / "csrc"
    inc = [f"-I{ROOT / 'include'}", f"-I{csrc}"]
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined"]
    base = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fPIC", *san, *inc, "-c"]
    objs = []
    for src in (csrc / "fa_fwd_gfx950.hip", csrc / "fa_kvcache.hip", ROOT / "tests" / "asan" / "stub_instances.hip",
                ROOT / "tests" / "asan" / "kvcache_validation_driver.cpp"):
        obj = tmp_path / (src.stem + ".o")
        subprocess.run([*base, str(src), "-o", str(obj)], check=True, capture_output=True)
        objs.append(str(obj))
    exe = tmp_path / "kvcache_asan"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fsanitize=address", "-fsanitize=undefined", "-fno-gpu-sanitize",
                    *objs, "-o", str(exe)], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and "kvcache validation ok" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
