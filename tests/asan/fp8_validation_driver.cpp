// Host-side validation of the FP8 KV-cache entry points (include/fa_gfx950_fp8.h) under AddressSanitizer +
// UBSan (tests/test_fp8_abi.py::test_fp8_host_validation_under_asan_ubsan builds and runs it; CPU only).
// Every entry point is called with valid and invalid descriptions and must return the right code with no
// sanitizer report. Paged launches that pass validation reach the host-only stubs (fp8_stub_instances.hip),
// never a device; the append's launch entry is only called with parameters that fail validation or launch
// nothing; the device arrays are never read on the host.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_fp8.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// a decode step (Sq == 1 packed: rows = the group) on a [num_pages, Hkv, page_size, D] byte pool
static fa_paged_fp8_params good(int64_t b, int64_t hkv, int64_t g, int64_t max_pages, int64_t page, int64_t d) {
    fa_paged_fp8_params f;
    memset(&f, 0, sizeof(f));
    fa_paged_params &v = f.paged;
    fa_fwd_params &p = v.base;
    p.q_ptr = (const void *)0x10000;
    p.k_ptr = (const void *)0x20000;
    p.v_ptr = (const void *)0x30000;
    p.o_ptr = (void *)0x40000;
    p.batch_size = b;
    p.num_heads_q = p.num_heads_kv = hkv;
    p.seqlen_q = g;
    p.seqlen_kv = max_pages * page;
    p.headdim = d;
    p.head_q_per_group = 1;
    p.q_batch_stride = p.o_batch_stride = hkv * g * d;
    p.q_head_stride = p.o_head_stride = g * d;
    p.k_batch_stride = p.v_batch_stride = hkv * page * d;
    p.k_head_stride = p.v_head_stride = page * d;
    p.q_seqlen_stride = p.k_seqlen_stride = p.v_seqlen_stride = p.o_seqlen_stride = d;
    p.softmax_scale = 0.1275f;
    v.block_table = (const int32_t *)0x50000;
    v.block_table_stride = max_pages;
    v.max_pages = max_pages;
    v.num_pages = 4096;
    v.page_size = page;
    v.seqlens_k = (const int32_t *)0x60000;
    f.k_descale = (const float *)0x70000;
    f.v_descale = (const float *)0x71000;
    f.descale_batch_stride = hkv;
    f.descale_head_stride = 1;
    return f;
}

static fa_kvcache_fp8_params good_append(int64_t b, int64_t hkv, int64_t g, int64_t sn, int64_t max_pages,
                                         int64_t page, int64_t d) {
    fa_kvcache_fp8_params f;
    memset(&f, 0, sizeof(f));
    fa_kvcache_params &p = f.base;
    p.k_new = (const void *)0x10000;
    p.v_new = (const void *)0x20000;
    p.kn_batch_stride = p.vn_batch_stride = hkv * sn * d;
    p.kn_head_stride = p.vn_head_stride = sn * d;
    p.kn_seqlen_stride = p.vn_seqlen_stride = d;
    p.q = (const void *)0x30000;
    p.q_out = (void *)0x40000;
    p.q_batch_stride = p.qo_batch_stride = hkv * g * d;
    p.q_head_stride = p.qo_head_stride = d;
    p.q_seqlen_stride = p.qo_seqlen_stride = d;
    p.cos = (const void *)0x50000;
    p.sin = (const void *)0x60000;
    p.cs_row_stride = d;
    p.max_pos = 8192;
    p.k_cache = (void *)0x100000;
    p.v_cache = (void *)0x200000;
    p.k_page_stride = p.v_page_stride = hkv * page * d;
    p.k_head_stride = p.v_head_stride = page * d;
    p.k_row_stride = p.v_row_stride = d;
    p.block_table = (const int32_t *)0x70000;
    p.block_table_stride = max_pages;
    p.max_pages = max_pages;
    p.num_pages = 4096;
    p.page_size = page;
    p.seqlens_k = (const int32_t *)0x80000;
    p.seqlens_out = (int32_t *)0x90000;
    p.batch_size = b;
    p.num_heads_q = hkv * g;
    p.num_heads_kv = hkv;
    p.seqlen_new = sn;
    p.seqlen_q = 1;
    p.headdim = d;
    f.k_descale = (const float *)0xa0000;
    f.v_descale = (const float *)0xa1000;
    f.descale_batch_stride = hkv;
    f.descale_head_stride = 1;
    return f;
}

int main() {
    EXPECT(fa_fp8_version() == FA_GFX950_FP8_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);
    EXPECT(fa_paged_version() == FA_GFX950_PAGED_VERSION);
    EXPECT(fa_kvcache_version() == FA_GFX950_KVCACHE_VERSION);
    fa_paged_fp8_params v = good(32, 8, 4, 32, 128, 128);
    EXPECT(fa_fwd_gfx950_paged_fp8_check(&v, FA_DTYPE_BF16, 0) == FA_OK);
    EXPECT(fa_fwd_gfx950_paged_fp8_check(NULL, FA_DTYPE_BF16, 0) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_fp8_check(&v, 7, 0) == FA_ERR_UNSUPPORTED);
    EXPECT(fa_fwd_gfx950_paged_fp8(NULL, FA_DTYPE_BF16, 0, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_fp8_workspace_size(NULL, FA_DTYPE_BF16, 0) == -1);
    v.k_descale = v.v_descale = NULL;  // NULL descales: 1.0
    v.descale_batch_stride = v.descale_head_stride = 0;
    EXPECT(fa_fwd_gfx950_paged_fp8_check(&v, FA_DTYPE_F16, 1) == FA_OK);
    struct Case { int field; int64_t value; int code; } cases[] = {
        {0, 48, FA_ERR_INVALID_ARGUMENT},          // page_size not a multiple of 32
        {0, 0, FA_ERR_INVALID_ARGUMENT},
        {1, 0, FA_ERR_INVALID_ARGUMENT},           // num_pages
        {1, INT64_C(1) << 40, FA_ERR_UNSUPPORTED},
        {2, 0, FA_ERR_INVALID_ARGUMENT},           // max_pages
        {2, INT64_MAX, FA_ERR_UNSUPPORTED},        // (no overflow in max_pages * page_size)
        {3, 16, FA_ERR_INVALID_ARGUMENT},          // table rows overlap
        {4, 136, FA_ERR_INVALID_ARGUMENT},         // K row stride a multiple of 8 but not of 16
        {4, INT64_C(1) << 33, FA_ERR_UNSUPPORTED}, // 32-bit tile offsets overflow
        {5, 144, FA_ERR_UNSUPPORTED},              // head dim
        {5, 72, FA_ERR_INVALID_ARGUMENT},          // a multiple of 8 but not of 16
        {5, 0, FA_ERR_INVALID_ARGUMENT},
        {6, 65, FA_ERR_UNSUPPORTED},               // more than 64 rows per kv-head: not a decode shape
        {7, 4096 + 32, FA_ERR_INVALID_ARGUMENT},   // seqlen_kv is not the table's capacity
        {8, -1, FA_ERR_INVALID_ARGUMENT},          // descale strides
        {9, -8, FA_ERR_INVALID_ARGUMENT},
        {10, 8 * 128 * 128 + 8, FA_ERR_INVALID_ARGUMENT},  // V page stride not a multiple of 16
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        fa_paged_fp8_params b = good(32, 8, 4, 32, 128, 128);
        switch (cases[i].field) {
            case 0: b.paged.page_size = cases[i].value; break;
            case 1: b.paged.num_pages = cases[i].value; break;
            case 2: b.paged.max_pages = cases[i].value; break;
            case 3: b.paged.block_table_stride = cases[i].value; break;
            case 4: b.paged.base.k_seqlen_stride = cases[i].value; break;
            case 5: b.paged.base.headdim = cases[i].value; break;
            case 6: b.paged.base.seqlen_q = cases[i].value; break;
            case 7: b.paged.base.seqlen_kv = cases[i].value; break;
            case 8: b.descale_batch_stride = cases[i].value; break;
            case 9: b.descale_head_stride = cases[i].value; break;
            case 10: b.paged.base.v_batch_stride = cases[i].value; break;
        }
        const int rc = fa_fwd_gfx950_paged_fp8_check(&b, FA_DTYPE_BF16, 1);
        if (rc != cases[i].code) fprintf(stderr, "case %zu: rc %d\n", i, rc);
        EXPECT(rc == cases[i].code);
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);
        // the launch and sizing entries validate before touching the device
        EXPECT(fa_fwd_gfx950_paged_fp8(&b, FA_DTYPE_BF16, 1, NULL, 0, NULL) == cases[i].code);
        EXPECT(fa_fwd_gfx950_paged_fp8_workspace_size(&b, FA_DTYPE_BF16, 1) == -1);
    }
    fa_paged_fp8_params m = good(32, 8, 4, 32, 128, 128);
    m.paged.block_table = NULL;
    EXPECT(fa_fwd_gfx950_paged_fp8_check(&m, FA_DTYPE_F16, 0) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 8, 4, 32, 128, 128);
    m.paged.base.k_ptr = (const void *)0x20008;
    EXPECT(fa_fwd_gfx950_paged_fp8_check(&m, FA_DTYPE_F16, 0) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 8, 4, 32, 128, 128);
    m.k_descale = (const float *)0x70002;
    EXPECT(fa_fwd_gfx950_paged_fp8_check(&m, FA_DTYPE_F16, 0) == FA_ERR_INVALID_ARGUMENT);
    // valid parameters reach the (stub) instantiation: plan + dispatch for every dtype / causal / D tile
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int causal = 0; causal < 2; ++causal)
            for (int64_t d = 16; d <= 128; d += 16) {
                fa_paged_fp8_params ok = good(3, 2, 4, 8, 32, d);
                EXPECT(fa_fwd_gfx950_paged_fp8(&ok, dtype, causal, NULL, 0, NULL) == FA_ERR_UNSUPPORTED);
                EXPECT(strstr(fa_last_error(), "stub") != NULL);
            }
    // the split plan: B1 Hkv8 over 32768 keys aims at 256 workgroups: 32 splits of 8 units, 32 rows each
    fa_paged_fp8_params big = good(1, 8, 4, 256, 128, 128);
    const int64_t ws = fa_fwd_gfx950_paged_fp8_workspace_size(&big, FA_DTYPE_BF16, 0);
    EXPECT(ws == INT64_C(8) * 32 * 32 * (128 * 4 + 4));
    EXPECT(ws > fa_fwd_gfx950_paged_workspace_size(&big.paged, FA_DTYPE_BF16, 0));
    // where the target does not bind (the length does) the plan, hence the workspace, is the 16-bit one's
    fa_paged_fp8_params mid = good(2, 2, 4, 64, 32, 128);
    EXPECT(fa_fwd_gfx950_paged_fp8_workspace_size(&mid, FA_DTYPE_BF16, 0) ==
           fa_fwd_gfx950_paged_workspace_size(&mid.paged, FA_DTYPE_BF16, 0));
    EXPECT(fa_fwd_gfx950_paged_fp8(&big, FA_DTYPE_BF16, 0, (void *)0x100000, ws - 16, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_fp8(&big, FA_DTYPE_BF16, 0, (void *)0x100008, ws, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_fp8(&big, FA_DTYPE_BF16, 0, (void *)0x100000, ws, NULL) == FA_ERR_UNSUPPORTED);  // stub
    fa_paged_fp8_params small = good(1, 8, 4, 2, 128, 128);
    EXPECT(fa_fwd_gfx950_paged_fp8_workspace_size(&small, FA_DTYPE_BF16, 0) == 0);

    // ---- the quantizing append ------------------------------------------------------------------
    fa_kvcache_fp8_params a = good_append(32, 8, 4, 1, 32, 128, 128);
    EXPECT(fa_kvcache_append_fp8_gfx950_check(&a, FA_DTYPE_BF16) == FA_OK);
    EXPECT(fa_kvcache_append_fp8_gfx950_check(&a, FA_DTYPE_F16) == FA_OK);
    EXPECT(fa_kvcache_append_fp8_gfx950_check(NULL, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_kvcache_append_fp8_gfx950(NULL, FA_DTYPE_F16, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_kvcache_append_fp8_gfx950_check(&a, 7) == FA_ERR_UNSUPPORTED);
    struct ACase { int field; int64_t value; int code; } acases[] = {
        {0, 72, FA_ERR_INVALID_ARGUMENT},    // head dim a multiple of 8 but not of 16
        {0, 144, FA_ERR_UNSUPPORTED},
        {1, 48, FA_ERR_INVALID_ARGUMENT},    // page size
        {2, 136, FA_ERR_INVALID_ARGUMENT},   // K row stride not a multiple of 16
        {3, 0x100008, FA_ERR_INVALID_ARGUMENT},  // cache base
        {4, 0x80004, FA_ERR_INVALID_ARGUMENT},   // seqlens_out overlaps seqlens_k
        {5, 132, FA_ERR_INVALID_ARGUMENT},   // k_new row stride not a multiple of 8
        {6, -1, FA_ERR_INVALID_ARGUMENT},    // descale stride
        {7, 0, FA_ERR_INVALID_ARGUMENT},     // num_pages
    };
    for (size_t i = 0; i < sizeof(acases) / sizeof(acases[0]); ++i) {
        fa_kvcache_fp8_params b = good_append(32, 8, 4, 1, 32, 128, 128);
        switch (acases[i].field) {
            case 0: b.base.headdim = acases[i].value; break;
            case 1: b.base.page_size = acases[i].value; break;
            case 2: b.base.k_row_stride = acases[i].value; break;
            case 3: b.base.k_cache = (void *)(uintptr_t)acases[i].value; break;
            case 4: b.base.seqlens_out = (int32_t *)(uintptr_t)acases[i].value; break;
            case 5: b.base.kn_seqlen_stride = acases[i].value; break;
            case 6: b.descale_batch_stride = acases[i].value; break;
            case 7: b.base.num_pages = acases[i].value; break;
        }
        const int rc = fa_kvcache_append_fp8_gfx950_check(&b, FA_DTYPE_BF16);
        if (rc != acases[i].code) fprintf(stderr, "append case %zu: rc %d\n", i, rc);
        EXPECT(rc == acases[i].code);
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);
        EXPECT(fa_kvcache_append_fp8_gfx950(&b, FA_DTYPE_BF16, NULL) == acases[i].code);
    }
    // nothing to launch: an empty batch, or neither a new token nor a query
    fa_kvcache_fp8_params e = good_append(0, 8, 4, 1, 32, 128, 128);
    EXPECT(fa_kvcache_append_fp8_gfx950(&e, FA_DTYPE_BF16, NULL) == FA_OK);
    // a dense cache: no table, max_pages 1, any positive length
    fa_kvcache_fp8_params dn = good_append(4, 8, 4, 1, 1, 1000, 64);
    dn.base.block_table = NULL;
    EXPECT(fa_kvcache_append_fp8_gfx950_check(&dn, FA_DTYPE_F16) == FA_OK);
    dn.base.max_pages = 2;
    EXPECT(fa_kvcache_append_fp8_gfx950_check(&dn, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("fp8 validation ok\n");
    return failures ? 1 : 0;
}
