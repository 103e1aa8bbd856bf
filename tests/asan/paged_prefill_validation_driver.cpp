// Host-side validation of the paged-prefill entry points (include/fa_gfx950_paged_prefill.h) under
// AddressSanitizer + UBSan (tests/test_paged_prefill_abi.py::test_prefill_host_validation_under_asan_ubsan builds
// and runs it; CPU only). The check, sizing and launch entries are called with valid and invalid descriptions,
// decode- and prefill-shaped, and every kind of window, and must return the paged decode check's codes (plus
// the page-size rule that is new here) with no sanitizer report. Launches that pass validation reach the
// host-only stubs (paged_prefill_stub_instances.hip), never a device; the device arrays are never read.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_paged_prefill.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// sq positions of g q-heads per kv-head over a [num_pages, Hkv, page_size, D] pool
static fa_paged_params good(int64_t b, int64_t hkv, int64_t g, int64_t sq, int64_t max_pages, int64_t page,
                            int64_t d) {
    fa_paged_params v;
    memset(&v, 0, sizeof(v));
    fa_fwd_params &p = v.base;
    p.q_ptr = (const void *)0x10000;
    p.k_ptr = (const void *)0x20000;
    p.v_ptr = (const void *)0x30000;
    p.o_ptr = (void *)0x40000;
    p.batch_size = b;
    p.num_heads_q = hkv * g;
    p.num_heads_kv = hkv;
    p.seqlen_q = sq;
    p.seqlen_kv = max_pages * page;
    p.headdim = d;
    p.head_q_per_group = g;
    p.q_batch_stride = p.o_batch_stride = hkv * g * sq * d;
    p.q_head_stride = p.o_head_stride = sq * d;
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

static const int64_t kWindows[] = {-1, INT64_MIN, 0, 1, 63, 64, 4095, INT64_C(1) << 30, (INT64_C(1) << 30) + 1,
                                   INT64_C(1) << 40, INT64_MAX};
static const size_t kNumWindows = sizeof(kWindows) / sizeof(kWindows[0]);

int main() {
    EXPECT(fa_paged_prefill_version() == FA_GFX950_PAGED_PREFILL_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);
    EXPECT(fa_paged_version() == FA_GFX950_PAGED_VERSION);

    // ---- a decode-shaped description: the codes are the paged decode check's ---------------------------
    struct Case { int field; int64_t value; } cases[] = {
        {-1, 0},                   // valid
        {0, 48}, {0, 0}, {0, -64}, // page_size
        {1, 0}, {1, INT64_C(1) << 40},  // num_pages
        {2, 0}, {2, INT64_MAX},    // max_pages (no overflow in max_pages * page_size)
        {3, 16},                   // table rows overlap
        {4, INT64_C(1) << 33},     // 32-bit tile offsets overflow
        {5, 144}, {5, 0},          // head dim
        {7, 4096 + 64},            // seqlen_kv is not the table's capacity
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        for (int64_t sq = 1; sq <= 512; sq *= 512) {  // a decode step, and a 512-position chunk
            fa_paged_params b = good(32, 8, 4, sq, 32, 128, 128);
            switch (cases[i].field) {
                case 0: b.page_size = cases[i].value; break;
                case 1: b.num_pages = cases[i].value; break;
                case 2: b.max_pages = cases[i].value; break;
                case 3: b.block_table_stride = cases[i].value; break;
                case 4: b.base.k_seqlen_stride = cases[i].value; break;
                case 5: b.base.headdim = cases[i].value; break;
                case 7: b.base.seqlen_kv = cases[i].value; break;
            }
            fa_paged_params step = b;  // the same pool under a decode step: the paged decode check's verdict
            step.base.seqlen_q = 1;
            step.base.q_batch_stride = step.base.o_batch_stride = 8 * 4 * 128;
            step.base.q_head_stride = step.base.o_head_stride = 128;
            const int want = fa_fwd_gfx950_paged_check(&step, FA_DTYPE_BF16, 1);
            EXPECT((want == FA_OK) == (cases[i].field < 0));
            EXPECT(fa_fwd_gfx950_paged_prefill_check(&b, FA_DTYPE_BF16, 1) == want);
            if (want != FA_OK) {
                EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);
                for (size_t w = 0; w < kNumWindows; ++w) {  // the launch and sizing entries validate first
                    EXPECT(fa_fwd_gfx950_paged_prefill(&b, FA_DTYPE_BF16, 1, kWindows[w], NULL, 0, NULL) == want);
                    EXPECT(fa_fwd_gfx950_paged_prefill_workspace_size(&b, FA_DTYPE_BF16, 1, kWindows[w]) == -1);
                }
            }
        }
    }
    EXPECT(fa_fwd_gfx950_paged_prefill_check(NULL, FA_DTYPE_BF16, 0) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_prefill(NULL, FA_DTYPE_BF16, 0, 7, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_prefill_workspace_size(NULL, FA_DTYPE_BF16, 0, 7) == -1);

    // ---- new here: a page holds whole 64-key tiles, and its rows stay inside 32-bit offsets -------------
    for (int64_t page = 32; page <= 96; page += 64) {  // valid pools for the decode entries
        fa_paged_params b = good(4, 8, 4, 1, 32, page, 128);
        EXPECT(fa_fwd_gfx950_paged_check(&b, FA_DTYPE_F16, 0) == FA_OK);
        EXPECT(fa_fwd_gfx950_paged_prefill_check(&b, FA_DTYPE_F16, 0) == FA_ERR_UNSUPPORTED);
        EXPECT(strstr(fa_last_error(), "multiple of 64") != NULL);
        EXPECT(fa_fwd_gfx950_paged_prefill(&b, FA_DTYPE_F16, 0, -1, NULL, 0, NULL) == FA_ERR_UNSUPPORTED);
        EXPECT(fa_fwd_gfx950_paged_prefill_workspace_size(&b, FA_DTYPE_F16, 0, -1) == -1);
    }
    {   // a pool past 2^31 elements is fine (the page term is 64-bit) ...
        fa_paged_params b = good(2, 8, 4, 512, 64, 256, 128);
        b.num_pages = INT64_C(1) << 20;  // 2^20 pages x 8 heads x 256 rows x 128: 2^38 elements
        EXPECT(fa_fwd_gfx950_paged_prefill_check(&b, FA_DTYPE_BF16, 1) == FA_OK);
        // ... a page whose rows span 2^31 bytes is not: 2^14 rows x a row stride of 2^16 elements x 2 bytes
        fa_paged_params wide = good(1, 1, 1, 512, 2, INT64_C(1) << 14, 128);
        wide.base.k_seqlen_stride = wide.base.v_seqlen_stride = INT64_C(1) << 16;
        wide.base.k_head_stride = wide.base.v_head_stride = 128;
        wide.base.k_batch_stride = wide.base.v_batch_stride = INT64_C(1) << 30;
        EXPECT(fa_fwd_gfx950_paged_prefill_check(&wide, FA_DTYPE_BF16, 1) == FA_ERR_UNSUPPORTED);
        EXPECT(strstr(fa_last_error(), "2^31") != NULL);
    }

    // ---- any g * Sq; valid parameters reach the (stub) instantiation for every dtype / causal / D / window --
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int causal = 0; causal < 2; ++causal)
            for (int64_t d = 16; d <= 128; d += 16)
                for (int64_t sq = 1; sq <= 2048; sq *= 8)
                    for (size_t w = 0; w < kNumWindows; ++w) {
                        fa_paged_params ok = good(3, 2, 4, sq, 8, 64, d);
                        EXPECT(fa_fwd_gfx950_paged_prefill_check(&ok, dtype, causal) == FA_OK);
                        EXPECT(fa_fwd_gfx950_paged_prefill_workspace_size(&ok, dtype, causal, kWindows[w]) == 0);
                        EXPECT(fa_fwd_gfx950_paged_prefill(&ok, dtype, causal, kWindows[w], NULL, 0, NULL) ==
                               FA_ERR_UNSUPPORTED);
                        EXPECT(strstr(fa_last_error(), "stub") != NULL);
                        // one byte less than the entry asks for
                        EXPECT(fa_fwd_gfx950_paged_prefill(&ok, dtype, causal, kWindows[w], NULL, -1, NULL) ==
                               FA_ERR_INVALID_ARGUMENT);
                        EXPECT(strstr(fa_last_error(), "workspace") != NULL);
                    }
    // the decode entry refuses a chunk that this one takes
    fa_paged_params chunk = good(8, 8, 4, 512, 64, 64, 128);
    EXPECT(fa_fwd_gfx950_paged_check(&chunk, FA_DTYPE_BF16, 1) == FA_ERR_UNSUPPORTED);
    EXPECT(fa_fwd_gfx950_paged_prefill_check(&chunk, FA_DTYPE_BF16, 1) == FA_OK);
    // q / o are still checked as given
    chunk.base.q_seqlen_stride = 132;
    EXPECT(fa_fwd_gfx950_paged_prefill_check(&chunk, FA_DTYPE_BF16, 1) != FA_OK);

    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("paged prefill validation ok\n");
    return failures ? 1 : 0;
}
