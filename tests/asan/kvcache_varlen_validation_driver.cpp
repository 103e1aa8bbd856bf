// Host-side validation of the ragged KV-cache append (include/fa_gfx950_kvcache_varlen.h) under
// AddressSanitizer + UBSan (tests/test_kvcache_varlen_abi.py::test_kvcache_varlen_host_validation_under_asan_ubsan
// builds and runs it; CPU only): only the check entry, and the launch entry with parameters that fail validation
// or launch nothing. The device arrays are never read.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_kvcache.h"
#include "fa_gfx950_kvcache_varlen.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static fa_kvcache_varlen_params good(int64_t b, int64_t hkv, int64_t g, int64_t total_new, int64_t total_q,
                                     int64_t max_pages, int64_t page, int64_t d) {
    fa_kvcache_varlen_params p;
    memset(&p, 0, sizeof(p));
    if (total_new > 0) {
        p.k_new = (const void *)0x10000;
        p.v_new = (const void *)0x20000;
    }
    p.kn_row_stride = p.vn_row_stride = hkv * d;
    p.kn_head_stride = p.vn_head_stride = d;
    p.cu_seqlens_new = (const int32_t *)0x30000;
    p.total_new = total_new;
    if (total_q > 0) {
        p.q = (const void *)0x40000;
        p.q_out = (void *)0x50000;
        p.cu_seqlens_q = (const int32_t *)0x60000;
    }
    p.q_row_stride = p.qo_row_stride = hkv * g * d;
    p.q_head_stride = p.qo_head_stride = d;
    p.total_q = total_q;
    p.cos = (const void *)0x70000;
    p.sin = (const void *)0x80000;
    p.cs_row_stride = d;
    p.max_pos = max_pages * page;
    p.k_cache = (void *)0x90000;
    p.v_cache = (void *)0xa0000;
    p.k_page_stride = p.v_page_stride = hkv * page * d;
    p.k_head_stride = p.v_head_stride = page * d;
    p.k_row_stride = p.v_row_stride = d;
    p.block_table = (const int32_t *)0xb0000;
    p.block_table_stride = max_pages;
    p.max_pages = max_pages;
    p.num_pages = 4096;
    p.page_size = page;
    p.seqlens_k = (const int32_t *)0xc0000;
    p.seqlens_out = (int32_t *)0xd0000;
    p.batch_size = b;
    p.num_heads_q = hkv * g;
    p.num_heads_kv = hkv;
    p.headdim = d;
    return p;
}

int main() {
    EXPECT(fa_kvcache_varlen_version() == FA_GFX950_KVCACHE_VARLEN_VERSION);
    EXPECT(fa_kvcache_version() == FA_GFX950_KVCACHE_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);

    for (int dtype = 0; dtype < 2; ++dtype)
        for (int64_t d = 2; d <= 128; d += 14)
            for (int64_t tn = 0; tn <= 4096; tn = tn ? tn * 64 : 1)
                for (int64_t tq = 0; tq <= 4096; tq = tq ? tq * 64 : 1) {
                    fa_kvcache_varlen_params ok = good(7, 2, 4, tn, tq, 8, 64, d);
                    EXPECT(fa_kvcache_append_varlen_gfx950_check(&ok, dtype) == FA_OK);
                    EXPECT(strlen(fa_last_error()) == 0);
                }
    EXPECT(fa_kvcache_append_varlen_gfx950_check(NULL, FA_DTYPE_BF16) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_kvcache_append_varlen_gfx950(NULL, FA_DTYPE_BF16, NULL) == FA_ERR_INVALID_ARGUMENT);
    {   // batch_size 0 launches nothing
        fa_kvcache_varlen_params none = good(0, 2, 4, 0, 0, 8, 64, 128);
        EXPECT(fa_kvcache_append_varlen_gfx950(&none, FA_DTYPE_F16, NULL) == FA_OK);
    }

    struct Case { int field; int64_t value; int want; } cases[] = {
        {0, 0, FA_ERR_INVALID_ARGUMENT},  {0, 48, FA_ERR_INVALID_ARGUMENT}, {0, -32, FA_ERR_INVALID_ARGUMENT},  // page_size
        {1, 0, FA_ERR_INVALID_ARGUMENT},  {1, INT64_C(1) << 40, FA_ERR_UNSUPPORTED},                          // num_pages
        {2, 0, FA_ERR_INVALID_ARGUMENT},  {2, INT64_MAX, FA_ERR_UNSUPPORTED},                                   // max_pages
        {3, 4, FA_ERR_INVALID_ARGUMENT},  {3, -1, FA_ERR_INVALID_ARGUMENT},                                     // table stride
        {4, -1, FA_ERR_INVALID_ARGUMENT}, {4, INT64_C(1) << 31, FA_ERR_UNSUPPORTED},                          // total_new
        {5, -1, FA_ERR_INVALID_ARGUMENT}, {5, INT64_MAX, FA_ERR_UNSUPPORTED},                                   // total_q
        {6, -1, FA_ERR_INVALID_ARGUMENT}, {6, INT64_C(0x7fffffff), FA_ERR_UNSUPPORTED},                       // batch_size
        {7, 0, FA_ERR_INVALID_ARGUMENT},  {7, 127, FA_ERR_INVALID_ARGUMENT},                                    // headdim (RoPE: even)
        {8, 0, FA_ERR_INVALID_ARGUMENT},                                                                        // num_heads_kv
        {9, 3, FA_ERR_INVALID_ARGUMENT},  {9, 0, FA_ERR_INVALID_ARGUMENT},                                      // num_heads_q
        {10, 0, FA_ERR_INVALID_ARGUMENT},                                                                       // max_pos
        {11, 0, FA_ERR_UNSUPPORTED},      {11, 0xb0002, FA_ERR_INVALID_ARGUMENT},                               // block_table
        {12, 0, FA_ERR_INVALID_ARGUMENT}, {12, 0xc0001, FA_ERR_INVALID_ARGUMENT},                               // seqlens_k
        {13, 0xc0004, FA_ERR_INVALID_ARGUMENT}, {13, 0xd0003, FA_ERR_INVALID_ARGUMENT},                         // seqlens_out
        {14, 0, FA_ERR_INVALID_ARGUMENT}, {14, 0x30002, FA_ERR_INVALID_ARGUMENT},                               // cu_seqlens_new
        {15, 0, FA_ERR_INVALID_ARGUMENT}, {15, 0x60001, FA_ERR_INVALID_ARGUMENT},                               // cu_seqlens_q
        {16, 0, FA_ERR_INVALID_ARGUMENT},                                                                       // k_new
        {17, 0, FA_ERR_INVALID_ARGUMENT},                                                                       // q_out
        {18, 0, FA_ERR_INVALID_ARGUMENT},                                                                       // sin
        {19, 0, FA_ERR_INVALID_ARGUMENT},                                                                       // k_cache
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        fa_kvcache_varlen_params b = good(7, 2, 4, 341, 341, 8, 64, 128);
        const int64_t v = cases[i].value;
        switch (cases[i].field) {
            case 0: b.page_size = v; break;
            case 1: b.num_pages = v; break;
            case 2: b.max_pages = v; break;
            case 3: b.block_table_stride = v; break;
            case 4: b.total_new = v; break;
            case 5: b.total_q = v; break;
            case 6: b.batch_size = v; break;
            case 7: b.headdim = v; break;
            case 8: b.num_heads_kv = v; break;
            case 9: b.num_heads_q = v; break;
            case 10: b.max_pos = v; break;
            case 11: b.block_table = (const int32_t *)(uintptr_t)v; break;
            case 12: b.seqlens_k = (const int32_t *)(uintptr_t)v; break;
            case 13: b.seqlens_out = (int32_t *)(uintptr_t)v; break;
            case 14: b.cu_seqlens_new = (const int32_t *)(uintptr_t)v; break;
            case 15: b.cu_seqlens_q = (const int32_t *)(uintptr_t)v; break;
            case 16: b.k_new = NULL; break;
            case 17: b.q_out = NULL; break;
            case 18: b.sin = NULL; break;
            case 19: b.k_cache = NULL; break;
        }
        const int rc = fa_kvcache_append_varlen_gfx950_check(&b, FA_DTYPE_BF16);
        if (rc != cases[i].want) fprintf(stderr, "case %zu: field %d value %lld\n", i, cases[i].field, (long long)v);
        EXPECT(rc == cases[i].want);
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);
        EXPECT(fa_kvcache_append_varlen_gfx950(&b, FA_DTYPE_BF16, NULL) == cases[i].want);  // validates first
    }
    {
        fa_kvcache_varlen_params b = good(7, 2, 4, 341, 341, 8, 64, 128);
        EXPECT(fa_kvcache_append_varlen_gfx950_check(&b, 2) == FA_ERR_UNSUPPORTED);  // an FP8 dtype code
        b.cos = b.sin = NULL;  // q is rotated only
        EXPECT(fa_kvcache_append_varlen_gfx950_check(&b, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
        b = good(7, 2, 4, 341, 0, 8, 64, 127);  // no tables, no q: any head dim
        b.cos = b.sin = NULL;
        EXPECT(fa_kvcache_append_varlen_gfx950_check(&b, FA_DTYPE_F16) == FA_OK);
    }

    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("kvcache varlen validation ok\n");
    return failures ? 1 : 0;
}
