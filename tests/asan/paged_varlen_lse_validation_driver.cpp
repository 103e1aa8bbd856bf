// Host-side validation of the ragged paged-prefill entry points that write the LSE
// (include/fa_gfx950_paged_varlen_lse.h) under AddressSanitizer + UBSan (tests/test_paged_varlen_lse_abi.py builds
// and runs it; CPU only). The check, sizing and launch entries are called with valid and invalid descriptions and
// every kind of window, and must return the ragged entry's codes (plus the rules that are new here: the LSE array,
// its strides, an optional sinks array) with no sanitizer report. Launches that
// pass validation reach the host-only stubs (paged_varlen_lse_stub_instances.hip), never a device; the device
// arrays are never read.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_paged_varlen.h"
#include "fa_gfx950_paged_varlen_lse.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// b sequences of at most max_q packed rows (total_q in all), g q-heads per kv-head, over a
// [num_pages, Hkv, page_size, D] pool, with a sinks array and an LSE destination [Hq, total_q]
static fa_paged_varlen_lse_params good(int64_t b, int64_t hkv, int64_t g, int64_t max_q, int64_t total_q,
                                        int64_t max_pages, int64_t page, int64_t d) {
    fa_paged_varlen_lse_params s;
    memset(&s, 0, sizeof(s));
    fa_paged_varlen_params &v = s.varlen;
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
    s.sinks = (const float *)0x90000;
    s.lse_ptr = (float *)0xa0000;
    s.lse_head_stride = total_q;
    s.lse_row_stride = 1;
    return s;
}

static const int64_t kWindows[] = {-1, INT64_MIN, 0, 1, 127, 4095, INT64_C(1) << 30, (INT64_C(1) << 30) + 1,
                                   INT64_C(1) << 40, INT64_MAX};
static const size_t kNumWindows = sizeof(kWindows) / sizeof(kWindows[0]);

int main() {
    EXPECT(fa_paged_varlen_lse_version() == FA_GFX950_PAGED_VARLEN_LSE_VERSION);
    EXPECT(fa_paged_varlen_version() == FA_GFX950_PAGED_VARLEN_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);

    // ---- what is wrong below the new rules: the ragged check's code --------------------------------------------
    struct Case { int field; int64_t value; } cases[] = {
        {-1, 0},                            // valid
        {0, 48}, {0, 32}, {0, 0}, {0, -64},  // page_size
        {1, 0}, {1, INT64_C(1) << 40},      // num_pages
        {2, 0}, {2, INT64_MAX},             // max_pages
        {3, 16},                            // table rows overlap
        {5, 144}, {5, 0}, {5, 68},          // head dim
        {6, 132},                           // q row stride
        {7, 4096 + 64},                     // seqlen_kv is not the table's capacity
        {8, 0}, {8, INT64_C(1) << 31},      // max_seqlen_q
        {9, -1}, {9, INT64_C(1) << 31}, {9, INT64_MIN},  // total_q
        {10, 0}, {10, 0x70002},             // cu_seqlens_q
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        fa_paged_varlen_lse_params b = good(8, 8, 4, 512, 3000, 32, 128, 128);
        switch (cases[i].field) {
            case 0: b.varlen.paged.page_size = cases[i].value; break;
            case 1: b.varlen.paged.num_pages = cases[i].value; break;
            case 2: b.varlen.paged.max_pages = cases[i].value; break;
            case 3: b.varlen.paged.block_table_stride = cases[i].value; break;
            case 5: b.varlen.paged.base.headdim = cases[i].value; break;
            case 6: b.varlen.paged.base.q_seqlen_stride = cases[i].value; break;
            case 7: b.varlen.paged.base.seqlen_kv = cases[i].value; break;
            case 8: b.varlen.paged.base.seqlen_q = cases[i].value; break;
            case 9: b.varlen.total_q = cases[i].value; break;
            case 10: b.varlen.cu_seqlens_q = (const int32_t *)(uintptr_t)cases[i].value; break;
        }
        const int want = fa_fwd_gfx950_paged_varlen_check(&b.varlen, FA_DTYPE_BF16, 1);
        char msg[512];
        strncpy(msg, fa_last_error(), sizeof(msg) - 1);
        msg[sizeof(msg) - 1] = 0;
        EXPECT((want == FA_OK) == (cases[i].field < 0));
        EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&b, FA_DTYPE_BF16, 1) == want);
        EXPECT(strcmp(fa_last_error(), msg) == 0);
        if (want != FA_OK) {
            for (size_t w = 0; w < kNumWindows; ++w) {  // the launch and sizing entries validate first
                EXPECT(fa_fwd_gfx950_paged_varlen_lse(&b, FA_DTYPE_BF16, 1, kWindows[w], NULL, 0, NULL) == want);
                EXPECT(fa_fwd_gfx950_paged_varlen_lse_workspace_size(&b, FA_DTYPE_BF16, 1, kWindows[w]) == -1);
            }
        }
    }
    EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(NULL, FA_DTYPE_BF16, 0) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_varlen_lse(NULL, FA_DTYPE_BF16, 0, 7, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_varlen_lse_workspace_size(NULL, FA_DTYPE_BF16, 0, 7) == -1);

    // ---- new here: the LSE array, its strides, and sinks that may be NULL ------------------------------------
    {
        fa_paged_varlen_lse_params b = good(8, 8, 4, 512, 3000, 32, 128, 128);
        b.sinks = NULL;  // no sinks: valid
        EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&b, FA_DTYPE_BF16, 1) == FA_OK);
        EXPECT(fa_fwd_gfx950_paged_varlen_lse_workspace_size(&b, FA_DTYPE_BF16, 1, 127) == 0);
        EXPECT(fa_fwd_gfx950_paged_varlen_lse(&b, FA_DTYPE_BF16, 1, -1, NULL, 0, NULL) == FA_ERR_UNSUPPORTED);
        EXPECT(strstr(fa_last_error(), "stub") != NULL);
        b.sinks = (const float *)0x90002;
        EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&b, FA_DTYPE_F16, 0) == FA_ERR_INVALID_ARGUMENT);
        EXPECT(strstr(fa_last_error(), "sinks must be NULL or a 4-byte aligned") != NULL);
        EXPECT(fa_fwd_gfx950_paged_varlen_lse(&b, FA_DTYPE_F16, 0, 127, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
        struct Bad { int field; int64_t value; const char *word; } bads[] = {
            {0, 0, "lse_ptr is NULL"}, {0, 0xa0002, "lse_ptr must be a 4-byte aligned"},
            {1, -1, "lse strides must be non-negative"}, {1, INT64_MIN, "lse strides must be non-negative"},
            {2, -1, "lse strides must be non-negative"}, {2, INT64_MIN, "lse strides must be non-negative"},
            {2, (INT64_C(1) << 20) + 1, "lse_row_stride"}, {2, INT64_MAX, "lse_row_stride"},
        };
        for (size_t i = 0; i < sizeof(bads) / sizeof(bads[0]); ++i) {
            b = good(8, 8, 4, 512, 3000, 32, 128, 128);
            if (bads[i].field == 0) b.lse_ptr = (float *)(uintptr_t)bads[i].value;
            if (bads[i].field == 1) b.lse_head_stride = bads[i].value;
            if (bads[i].field == 2) b.lse_row_stride = bads[i].value;
            EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&b, FA_DTYPE_BF16, 1) == FA_ERR_INVALID_ARGUMENT);
            EXPECT(strstr(fa_last_error(), bads[i].word) != NULL);
            EXPECT(fa_fwd_gfx950_paged_varlen_lse(&b, FA_DTYPE_BF16, 1, -1, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
            EXPECT(fa_fwd_gfx950_paged_varlen_lse_workspace_size(&b, FA_DTYPE_BF16, 1, 127) == -1);
        }
        b = good(8, 8, 4, 512, 3000, 32, 128, 128);
        b.lse_head_stride = INT64_MAX;  // (any non-negative head stride; 0 and 2^20 row strides)
        b.lse_row_stride = INT64_C(1) << 20;
        EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&b, FA_DTYPE_BF16, 1) == FA_OK);
        b.lse_head_stride = b.lse_row_stride = 0;
        EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&b, FA_DTYPE_BF16, 1) == FA_OK);
        EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&b, 2, 1) == FA_ERR_UNSUPPORTED);  // an FP8 dtype code
        EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&b, -1, 1) == FA_ERR_UNSUPPORTED);
    }

    // ---- valid parameters reach the (stub) instantiation for every dtype / causal / D / window ------------
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int causal = 0; causal < 2; ++causal)
            for (int64_t d = 16; d <= 128; d += 16)
                for (int64_t mq = 1; mq <= 2048; mq *= 8)
                    for (size_t w = 0; w < kNumWindows; ++w) {
                        fa_paged_varlen_lse_params ok = good(3, 2, 4, mq, 3 * mq, 8, 64, d);
                        if (w & 1) ok.sinks = NULL;
                        EXPECT(fa_fwd_gfx950_paged_varlen_lse_check(&ok, dtype, causal) == FA_OK);
                        EXPECT(fa_fwd_gfx950_paged_varlen_lse_workspace_size(&ok, dtype, causal, kWindows[w]) == 0);
                        EXPECT(fa_fwd_gfx950_paged_varlen_lse(&ok, dtype, causal, kWindows[w], NULL, 0, NULL) ==
                               FA_ERR_UNSUPPORTED);
                        EXPECT(strstr(fa_last_error(), "stub") != NULL);
                        // one byte less than the entry asks for
                        EXPECT(fa_fwd_gfx950_paged_varlen_lse(&ok, dtype, causal, kWindows[w], NULL, -1, NULL) ==
                               FA_ERR_INVALID_ARGUMENT);
                        EXPECT(strstr(fa_last_error(), "workspace") != NULL);
                        ok.varlen.total_q = 0;  // no row: valid, and nothing is launched
                        EXPECT(fa_fwd_gfx950_paged_varlen_lse(&ok, dtype, causal, kWindows[w], NULL, 0, NULL) == FA_OK);
                    }

    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("paged varlen lse validation ok\n");
    return failures ? 1 : 0;
}
