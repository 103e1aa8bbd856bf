// Host-side validation of the paged entry points (include/fa_gfx950_paged.h) under AddressSanitizer +
// UBSan (tests/test_paged_abi.py::test_paged_host_validation_under_asan_ubsan builds and runs it; CPU
// only). Every entry point is called with valid and invalid descriptions of the page pool, the block
// table and the lengths and must return the right code with no sanitizer report. Launches that pass
// validation reach the host-only stubs (paged_stub_instances.hip), never a device; the device arrays
// are never read on the host.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_paged.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// a decode step (Sq == 1 packed: rows = the group) on a [num_pages, Hkv, page_size, D] pool
static fa_paged_params good(int64_t b, int64_t hkv, int64_t g, int64_t max_pages, int64_t page, int64_t d) {
    fa_paged_params v;
    memset(&v, 0, sizeof(v));
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
    return v;
}

int main() {
    EXPECT(fa_paged_version() == FA_GFX950_PAGED_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);
    fa_paged_params v = good(32, 8, 4, 32, 128, 128);
    EXPECT(fa_fwd_gfx950_paged_check(&v, FA_DTYPE_BF16, 0) == FA_OK);
    EXPECT(fa_fwd_gfx950_paged_check(NULL, FA_DTYPE_BF16, 0) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_check(&v, 7, 0) == FA_ERR_UNSUPPORTED);
    EXPECT(fa_fwd_gfx950_paged(NULL, FA_DTYPE_BF16, 0, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_workspace_size(NULL, FA_DTYPE_BF16, 0) == -1);
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
        {4, 132, FA_ERR_INVALID_ARGUMENT},         // K row stride not a multiple of 8
        {4, INT64_C(1) << 33, FA_ERR_UNSUPPORTED}, // 32-bit tile offsets overflow
        {5, 136, FA_ERR_UNSUPPORTED},              // head dim
        {5, 100, FA_ERR_INVALID_ARGUMENT},
        {6, 65, FA_ERR_UNSUPPORTED},               // more than 64 rows per kv-head: not a decode shape
        {7, 4096 + 32, FA_ERR_INVALID_ARGUMENT},   // seqlen_kv is not the table's capacity
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        fa_paged_params b = good(32, 8, 4, 32, 128, 128);
        switch (cases[i].field) {
            case 0: b.page_size = cases[i].value; break;
            case 1: b.num_pages = cases[i].value; break;
            case 2: b.max_pages = cases[i].value; break;
            case 3: b.block_table_stride = cases[i].value; break;
            case 4: b.base.k_seqlen_stride = cases[i].value; break;
            case 5: b.base.headdim = cases[i].value; break;
            case 6: b.base.seqlen_q = cases[i].value; break;
            case 7: b.base.seqlen_kv = cases[i].value; break;
        }
        const int rc = fa_fwd_gfx950_paged_check(&b, FA_DTYPE_BF16, 1);
        if (rc != cases[i].code) fprintf(stderr, "case %zu: rc %d\n", i, rc);
        EXPECT(rc == cases[i].code);
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);
        // the launch and sizing entries validate before touching the device
        EXPECT(fa_fwd_gfx950_paged(&b, FA_DTYPE_BF16, 1, NULL, 0, NULL) == cases[i].code);
        EXPECT(fa_fwd_gfx950_paged_workspace_size(&b, FA_DTYPE_BF16, 1) == -1);
    }
    fa_paged_params m = good(32, 8, 4, 32, 128, 128);
    m.block_table = NULL;
    EXPECT(fa_fwd_gfx950_paged_check(&m, FA_DTYPE_F16, 0) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 8, 4, 32, 128, 128);
    m.block_table = (const int32_t *)0x50002;
    EXPECT(fa_fwd_gfx950_paged_check(&m, FA_DTYPE_F16, 0) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 8, 4, 32, 128, 128);
    m.seqlens_k = NULL;
    EXPECT(fa_fwd_gfx950_paged(&m, FA_DTYPE_F16, 0, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    m = good(32, 8, 4, 32, 128, 128);
    m.base.k_ptr = (const void *)0x20008;
    EXPECT(fa_fwd_gfx950_paged_check(&m, FA_DTYPE_F16, 0) == FA_ERR_INVALID_ARGUMENT);
    // valid parameters reach the (stub) instantiation: plan + dispatch for every dtype / causal / D tile
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int causal = 0; causal < 2; ++causal)
            for (int64_t d = 56; d <= 128; d += 8) {
                fa_paged_params ok = good(3, 2, 4, 8, 32, d);
                EXPECT(fa_fwd_gfx950_paged(&ok, dtype, causal, NULL, 0, NULL) == FA_ERR_UNSUPPORTED);
                EXPECT(strstr(fa_last_error(), "stub") != NULL);
            }
    // the split plan: B1 Hkv8 over 32768 keys wants a workspace, 256 keys none
    fa_paged_params big = good(1, 8, 4, 256, 128, 128);
    const int64_t ws = fa_fwd_gfx950_paged_workspace_size(&big, FA_DTYPE_BF16, 0);
    EXPECT(ws > 0 && ws % (8 * 32 * (128 * 4 + 4)) == 0);
    EXPECT(fa_fwd_gfx950_paged(&big, FA_DTYPE_BF16, 0, (void *)0x100000, ws - 16, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged(&big, FA_DTYPE_BF16, 0, (void *)0x100008, ws, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged(&big, FA_DTYPE_BF16, 0, (void *)0x100000, ws, NULL) == FA_ERR_UNSUPPORTED);  // stub
    fa_paged_params small = good(1, 8, 4, 2, 128, 128);
    EXPECT(fa_fwd_gfx950_paged_workspace_size(&small, FA_DTYPE_BF16, 0) == 0);
    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("paged validation ok\n");
    return failures ? 1 : 0;
}
