// Host-side validation of the KV-cache append entry points (include/fa_gfx950_kvcache.h) under
// AddressSanitizer + UBSan (tests/test_kvcache_abi.py::test_kvcache_host_validation_under_asan_ubsan builds
// and runs it; CPU only). The check entry is called with valid and invalid descriptions of the new tokens,
// the tables, the cache and the lengths and must return the right code with no sanitizer report. The
// launch entry is called only with parameters that fail validation or that launch nothing: no device is
// touched, and the device arrays are never read on the host.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_kvcache.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// one step's append (sn new tokens, sq query rows, RoPE tables) on a [num_pages, Hkv, page, D] pool
static fa_kvcache_params good(int64_t b, int64_t hq, int64_t hkv, int64_t sn, int64_t sq, int64_t max_pages,
                              int64_t page, int64_t d) {
    fa_kvcache_params p;
    memset(&p, 0, sizeof(p));
    if (sn > 0) {
        p.k_new = (const void *)0x10000;
        p.v_new = (const void *)0x20000;
        p.kn_batch_stride = p.vn_batch_stride = hkv * sn * d;
        p.kn_head_stride = p.vn_head_stride = sn * d;
        p.kn_seqlen_stride = p.vn_seqlen_stride = d;
    }
    if (sq > 0) {
        p.q = (const void *)0x30000;
        p.q_out = (void *)0x40000;
        p.q_batch_stride = p.qo_batch_stride = hq * sq * d;
        p.q_head_stride = p.qo_head_stride = sq * d;
        p.q_seqlen_stride = p.qo_seqlen_stride = d;
        p.num_heads_q = hq;
    }
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
    p.num_heads_kv = hkv;
    p.seqlen_new = sn;
    p.seqlen_q = sq;
    p.headdim = d;
    return p;
}

int main() {
    EXPECT(fa_kvcache_version() == FA_GFX950_KVCACHE_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);
    fa_kvcache_params v = good(32, 32, 8, 1, 1, 32, 128, 128);
    EXPECT(fa_kvcache_append_gfx950_check(&v, FA_DTYPE_BF16) == FA_OK);
    EXPECT(strlen(fa_last_error()) == 0);
    EXPECT(fa_kvcache_append_gfx950_check(&v, FA_DTYPE_F16) == FA_OK);
    EXPECT(fa_kvcache_append_gfx950_check(NULL, FA_DTYPE_BF16) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_kvcache_append_gfx950_check(&v, 7) == FA_ERR_UNSUPPORTED);
    EXPECT(fa_kvcache_append_gfx950(NULL, FA_DTYPE_BF16, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_kvcache_append_gfx950(&v, -1, NULL) == FA_ERR_UNSUPPORTED);
    struct Case { int field; int64_t value; int code; } cases[] = {
        {0, 48, FA_ERR_INVALID_ARGUMENT},          // page_size not a multiple of 32
        {0, 0, FA_ERR_INVALID_ARGUMENT},
        {0, -32, FA_ERR_INVALID_ARGUMENT},
        {1, 0, FA_ERR_INVALID_ARGUMENT},           // num_pages
        {1, -5, FA_ERR_INVALID_ARGUMENT},
        {1, INT64_C(1) << 40, FA_ERR_UNSUPPORTED},
        {2, 0, FA_ERR_INVALID_ARGUMENT},           // max_pages
        {2, INT64_C(1) << 40, FA_ERR_UNSUPPORTED},
        {2, INT64_MAX, FA_ERR_UNSUPPORTED},        // (no overflow in max_pages * page_size)
        {3, 16, FA_ERR_INVALID_ARGUMENT},          // table rows overlap
        {3, -32, FA_ERR_INVALID_ARGUMENT},
        {4, 0, FA_ERR_INVALID_ARGUMENT},           // head dim
        {4, 127, FA_ERR_INVALID_ARGUMENT},         // odd with tables
        {4, INT64_MAX, FA_ERR_UNSUPPORTED},
        {5, -1, FA_ERR_INVALID_ARGUMENT},          // batch
        {5, INT64_MAX, FA_ERR_UNSUPPORTED},
        {6, 0, FA_ERR_INVALID_ARGUMENT},           // num_heads_kv
        {6, 5, FA_ERR_INVALID_ARGUMENT},           // Hq % Hkv
        {6, INT64_MAX, FA_ERR_UNSUPPORTED},
        {7, -1, FA_ERR_INVALID_ARGUMENT},          // seqlen_new
        {7, 0, FA_ERR_INVALID_ARGUMENT},           // k_new given with no rows
        {7, INT64_MAX, FA_ERR_UNSUPPORTED},
        {8, -1, FA_ERR_INVALID_ARGUMENT},          // seqlen_q
        {8, INT64_MAX, FA_ERR_UNSUPPORTED},
        {9, 0, FA_ERR_INVALID_ARGUMENT},           // max_pos
        {9, INT64_MIN, FA_ERR_INVALID_ARGUMENT},
        {10, 0x3fffffff, FA_ERR_UNSUPPORTED},      // every size at its bound: too many rows for one launch
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        fa_kvcache_params b = good(32, 32, 8, 1, 1, 32, 128, 128);
        switch (cases[i].field) {
            case 0: b.page_size = cases[i].value; break;
            case 1: b.num_pages = cases[i].value; break;
            case 2: b.max_pages = cases[i].value; break;
            case 3: b.block_table_stride = cases[i].value; break;
            case 4: b.headdim = cases[i].value; break;
            case 5: b.batch_size = cases[i].value; break;
            case 6: b.num_heads_kv = cases[i].value; break;
            case 7: b.seqlen_new = cases[i].value; break;
            case 8: b.seqlen_q = cases[i].value; break;
            case 9: b.max_pos = cases[i].value; break;
            case 10:
                b.batch_size = b.num_heads_kv = b.num_heads_q = 0x7fffffff;
                b.seqlen_new = b.seqlen_q = cases[i].value;
                b.seqlens_out = NULL;  // (2^31 lengths would overlap any nearby array)
                break;
        }
        const int rc = fa_kvcache_append_gfx950_check(&b, FA_DTYPE_BF16);
        if (rc != cases[i].code) fprintf(stderr, "case %zu: rc %d\n", i, rc);
        EXPECT(rc == cases[i].code);
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);
        // the launch entry validates before touching the device
        EXPECT(fa_kvcache_append_gfx950(&b, FA_DTYPE_BF16, NULL) == cases[i].code);
    }
    // pointers: NULL and misaligned int32 arrays, halves of a pair, q without tables, overlapping lengths
    fa_kvcache_params m = good(32, 32, 8, 1, 1, 32, 128, 128);
    m.seqlens_k = NULL;
    EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 32, 8, 1, 1, 32, 128, 128);
    m.seqlens_k = (const int32_t *)0x80002;
    EXPECT(fa_kvcache_append_gfx950(&m, FA_DTYPE_F16, NULL) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 32, 8, 1, 1, 32, 128, 128);
    m.block_table = (const int32_t *)0x70001;
    EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 32, 8, 1, 1, 32, 128, 128);
    m.v_new = NULL;
    EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 32, 8, 1, 1, 32, 128, 128);
    m.q_out = NULL;
    EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 32, 8, 1, 1, 32, 128, 128);
    m.cos = m.sin = NULL;
    EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 32, 8, 1, 1, 32, 128, 128);
    m.sin = NULL;
    EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 32, 8, 1, 1, 32, 128, 128);
    m.v_cache = NULL;
    EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    for (int64_t off = -32; off <= 32; ++off) {  // [B] int32 ranges: overlap iff |distance| < B
        m = good(32, 32, 8, 1, 1, 32, 128, 128);
        m.seqlens_out = (int32_t *)(0x80000 + off * 4);
        const int want = (off > -32 && off < 32) ? FA_ERR_INVALID_ARGUMENT : FA_OK;
        EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_BF16) == want);
    }
    m = good(1, 32, 8, 1, 1, 32, 128, 128);  // at the ends of the address space: no wrap-around in the range test
    m.seqlens_k = (const int32_t *)(UINTPTR_MAX - 3);
    m.seqlens_out = (int32_t *)4;
    EXPECT(fa_kvcache_append_gfx950_check(&m, FA_DTYPE_BF16) == FA_OK);
    // a dense cache: no table, one "page" per batch row of any positive size
    fa_kvcache_params dn = good(4, 32, 8, 3, 3, 1, 100, 72);
    dn.block_table = NULL;
    dn.block_table_stride = 0;
    dn.num_pages = 0;
    EXPECT(fa_kvcache_append_gfx950_check(&dn, FA_DTYPE_F16) == FA_OK);
    dn.num_pages = INT64_MAX;  // ignored without a table
    EXPECT(fa_kvcache_append_gfx950_check(&dn, FA_DTYPE_F16) == FA_OK);
    dn.max_pages = 2;
    EXPECT(fa_kvcache_append_gfx950_check(&dn, FA_DTYPE_F16) == FA_ERR_INVALID_ARGUMENT);
    // nothing to do: no launch, no error, no device
    fa_kvcache_params none = good(0, 32, 8, 1, 1, 32, 128, 128);
    EXPECT(fa_kvcache_append_gfx950(&none, FA_DTYPE_BF16, NULL) == FA_OK);
    none = good(32, 32, 8, 0, 0, 32, 128, 128);
    EXPECT(fa_kvcache_append_gfx950(&none, FA_DTYPE_BF16, NULL) == FA_OK);
    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("kvcache validation ok\n");
    return failures ? 1 : 0;
}
