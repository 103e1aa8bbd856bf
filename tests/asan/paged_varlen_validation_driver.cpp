// Host-side validation of the ragged paged-prefill entry points (include/fa_gfx950_paged_varlen.h) under
// AddressSanitizer + UBSan (tests/test_paged_varlen_abi.py::test_varlen_host_validation_under_asan_ubsan builds
// and runs it; CPU only). The check, sizing and launch entries are called with valid and invalid descriptions
// and every kind of window, and must return the paged prefill check's codes (plus the rules of the cumulative
// array that are new here) with no sanitizer report. Launches that pass validation reach the host-only stubs
// (paged_prefill_stub_instances.hip), never a device; the device arrays are never read.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_paged_prefill.h"
#include "fa_gfx950_paged_varlen.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// b sequences of at most max_q packed rows (total_q in all), g q-heads per kv-head, over a
// [num_pages, Hkv, page_size, D] pool
static fa_paged_varlen_params good(int64_t b, int64_t hkv, int64_t g, int64_t max_q, int64_t total_q,
                                   int64_t max_pages, int64_t page, int64_t d) {
    fa_paged_varlen_params v;
    memset(&v, 0, sizeof(v));
    fa_fwd_params &p = v.paged.base;
    p.q_ptr = (const void *)0x10000;
    p.k_ptr = (const void *)0x20000;
    p.v_ptr = (const void *)0x30000;
    p.o_ptr = (void *)0x40000;
    p.batch_size = b;
    p.num_heads_q = hkv * g;
    p.num_heads_kv = hkv;
    p.seqlen_q = max_q;
    p.seqlen_kv = max_pages * page;
    p.headdim = d;
    p.head_q_per_group = g;
    p.q_batch_stride = p.o_batch_stride = 12345;  // ignored: not even a multiple of 8
    p.q_head_stride = p.o_head_stride = d;
    p.q_seqlen_stride = p.o_seqlen_stride = hkv * g * d;
    p.k_batch_stride = p.v_batch_stride = hkv * page * d;
    p.k_head_stride = p.v_head_stride = page * d;
    p.k_seqlen_stride = p.v_seqlen_stride = d;
    p.softmax_scale = 0.1275f;
    v.paged.block_table = (const int32_t *)0x50000;
    v.paged.block_table_stride = max_pages;
    v.paged.max_pages = max_pages;
    v.paged.num_pages = 4096;
    v.paged.page_size = page;
    v.paged.seqlens_k = (const int32_t *)0x60000;
    v.cu_seqlens_q = (const int32_t *)0x70000;
    v.total_q = total_q;
    return v;
}

static const int64_t kWindows[] = {-1, INT64_MIN, 0, 1, 63, 64, 4095, INT64_C(1) << 30, (INT64_C(1) << 30) + 1,
                                   INT64_C(1) << 40, INT64_MAX};
static const size_t kNumWindows = sizeof(kWindows) / sizeof(kWindows[0]);

int main() {
    EXPECT(fa_paged_varlen_version() == FA_GFX950_PAGED_VARLEN_VERSION);
    EXPECT(fa_paged_prefill_version() == FA_GFX950_PAGED_PREFILL_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);
    EXPECT(fa_paged_version() == FA_GFX950_PAGED_VERSION);

    // ---- what is wrong with the pool, the table or q / o: the paged prefill check's code on the packed layout --
    struct Case { int field; int64_t value; } cases[] = {
        {-1, 0},                            // valid
        {0, 48}, {0, 96}, {0, 0}, {0, -64},  // page_size
        {1, 0}, {1, INT64_C(1) << 40},      // num_pages
        {2, 0}, {2, INT64_MAX},             // max_pages
        {3, 16},                            // table rows overlap
        {4, INT64_C(1) << 33},              // 32-bit tile offsets overflow
        {5, 144}, {5, 0}, {5, 68},          // head dim
        {6, 132},                           // q row stride
        {7, 4096 + 64},                     // seqlen_kv is not the table's capacity
        {8, 0}, {8, INT64_C(1) << 31},      // max_seqlen_q
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        fa_paged_varlen_params b = good(8, 8, 4, 512, 3000, 32, 128, 128);
        switch (cases[i].field) {
            case 0: b.paged.page_size = cases[i].value; break;
            case 1: b.paged.num_pages = cases[i].value; break;
            case 2: b.paged.max_pages = cases[i].value; break;
            case 3: b.paged.block_table_stride = cases[i].value; break;
            case 4: b.paged.base.k_seqlen_stride = cases[i].value; break;
            case 5: b.paged.base.headdim = cases[i].value; break;
            case 6: b.paged.base.q_seqlen_stride = cases[i].value; break;
            case 7: b.paged.base.seqlen_kv = cases[i].value; break;
            case 8: b.paged.base.seqlen_q = cases[i].value; break;
        }
        fa_paged_params same = b.paged;  // the same description as a uniform launch over packed rows
        same.base.q_batch_stride = same.base.o_batch_stride = 0;
        const int want = fa_fwd_gfx950_paged_prefill_check(&same, FA_DTYPE_BF16, 1);
        EXPECT((want == FA_OK) == (cases[i].field < 0));
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, FA_DTYPE_BF16, 1) == want);
        if (want != FA_OK) {
            EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);
            for (size_t w = 0; w < kNumWindows; ++w) {  // the launch and sizing entries validate first
                EXPECT(fa_fwd_gfx950_paged_varlen(&b, FA_DTYPE_BF16, 1, kWindows[w], NULL, 0, NULL) == want);
                EXPECT(fa_fwd_gfx950_paged_varlen_workspace_size(&b, FA_DTYPE_BF16, 1, kWindows[w]) == -1);
            }
        }
    }
    EXPECT(fa_fwd_gfx950_paged_varlen_check(NULL, FA_DTYPE_BF16, 0) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_varlen(NULL, FA_DTYPE_BF16, 0, 7, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_varlen_workspace_size(NULL, FA_DTYPE_BF16, 0, 7) == -1);

    // ---- new here: the cumulative array and total_q -----------------------------------------------------
    {
        fa_paged_varlen_params b = good(8, 8, 4, 512, 3000, 32, 128, 128);
        b.cu_seqlens_q = NULL;
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, FA_DTYPE_BF16, 1) == FA_ERR_INVALID_ARGUMENT);
        EXPECT(strstr(fa_last_error(), "cu_seqlens_q") != NULL);
        EXPECT(fa_fwd_gfx950_paged_varlen(&b, FA_DTYPE_BF16, 1, -1, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
        EXPECT(fa_fwd_gfx950_paged_varlen_workspace_size(&b, FA_DTYPE_BF16, 1, -1) == -1);
        b.cu_seqlens_q = (const int32_t *)0x70002;
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, FA_DTYPE_BF16, 1) == FA_ERR_INVALID_ARGUMENT);
        EXPECT(strstr(fa_last_error(), "aligned") != NULL);
        b = good(8, 8, 4, 512, -1, 32, 128, 128);
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, FA_DTYPE_BF16, 1) == FA_ERR_INVALID_ARGUMENT);
        EXPECT(strstr(fa_last_error(), "total_q") != NULL);
        b = good(8, 8, 4, 512, INT64_MIN, 32, 128, 128);
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, FA_DTYPE_BF16, 1) == FA_ERR_INVALID_ARGUMENT);
        b = good(8, 8, 4, 512, INT64_C(1) << 31, 32, 128, 128);
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, FA_DTYPE_BF16, 1) == FA_ERR_UNSUPPORTED);
        b = good(8, 8, 4, 512, INT64_MAX, 32, 128, 128);
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, FA_DTYPE_BF16, 1) == FA_ERR_UNSUPPORTED);
        b = good(INT64_C(0x7fffffff), 8, 4, 512, 3000, 32, 128, 128);
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, FA_DTYPE_BF16, 1) == FA_ERR_UNSUPPORTED);
        b = good(8, 8, 4, 512, 3000, 32, 128, 128);
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, 2, 1) == FA_ERR_UNSUPPORTED);  // an FP8 dtype code
        EXPECT(fa_fwd_gfx950_paged_varlen_check(&b, -1, 1) == FA_ERR_UNSUPPORTED);
    }

    // ---- valid parameters reach the (stub) instantiation for every dtype / causal / D / window ------------
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int causal = 0; causal < 2; ++causal)
            for (int64_t d = 16; d <= 128; d += 16)
                for (int64_t mq = 1; mq <= 2048; mq *= 8)
                    for (size_t w = 0; w < kNumWindows; ++w) {
                        fa_paged_varlen_params ok = good(3, 2, 4, mq, 3 * mq, 8, 64, d);
                        EXPECT(fa_fwd_gfx950_paged_varlen_check(&ok, dtype, causal) == FA_OK);
                        EXPECT(fa_fwd_gfx950_paged_varlen_workspace_size(&ok, dtype, causal, kWindows[w]) == 0);
                        EXPECT(fa_fwd_gfx950_paged_varlen(&ok, dtype, causal, kWindows[w], NULL, 0, NULL) ==
                               FA_ERR_UNSUPPORTED);
                        EXPECT(strstr(fa_last_error(), "stub") != NULL);
                        // one byte less than the entry asks for
                        EXPECT(fa_fwd_gfx950_paged_varlen(&ok, dtype, causal, kWindows[w], NULL, -1, NULL) ==
                               FA_ERR_INVALID_ARGUMENT);
                        EXPECT(strstr(fa_last_error(), "workspace") != NULL);
                        ok.total_q = 0;  // no row: valid, and nothing is launched
                        EXPECT(fa_fwd_gfx950_paged_varlen(&ok, dtype, causal, kWindows[w], NULL, 0, NULL) == FA_OK);
                    }

    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("paged varlen validation ok\n");
    return failures ? 1 : 0;
}
