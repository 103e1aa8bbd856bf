// Host-side validation of the sliding-window paged decode entry points (include/fa_gfx950_paged_window.h)
// under AddressSanitizer + UBSan (tests/test_paged_window_abi.py::test_window_host_validation_under_asan_ubsan
// builds and runs it; CPU only). The check, sizing and launch entries are called with valid and invalid
// descriptions and every kind of window and must return the unwindowed entries' codes and the window plan's
// sizes with no sanitizer report. Launches that pass validation reach the host-only stubs
// (paged_window_stub_instances.hip; with window_left < 0 the unwindowed entries' paged_stub_instances.hip and
// fp8_stub_instances.hip), never a device; the device arrays are never read.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_paged_window.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// a decode step on a [num_pages, Hkv, page_size, D] pool: g q-heads per kv-head, sq positions, unpacked (the
// form a windowed launch takes)
static fa_paged_fp8_params good(int64_t b, int64_t hkv, int64_t g, int64_t sq, int64_t max_pages, int64_t page,
                                int64_t d) {
    fa_paged_fp8_params f;
    memset(&f, 0, sizeof(f));
    fa_paged_params &v = f.paged;
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
    f.k_descale = (const float *)0x70000;
    f.v_descale = (const float *)0x71000;
    f.descale_batch_stride = hkv;
    f.descale_head_stride = 1;
    return f;
}

static const int64_t kWindows[] = {-1, INT64_MIN, 0, 1, 31, 32, 4095, INT64_C(1) << 30, (INT64_C(1) << 30) + 1,
                                   INT64_C(1) << 40, INT64_MAX};
static const size_t kNumWindows = sizeof(kWindows) / sizeof(kWindows[0]);

int main() {
    EXPECT(fa_paged_window_version() == FA_GFX950_PAGED_WINDOW_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);
    EXPECT(fa_paged_version() == FA_GFX950_PAGED_VERSION);
    EXPECT(fa_fp8_version() == FA_GFX950_FP8_VERSION);

    // ---- every window is valid; the codes are the unwindowed checks' ---------------------------------
    struct Case { int field; int64_t value; } cases[] = {
        {-1, 0},                   // valid
        {0, 48}, {0, 0},           // page_size
        {1, 0}, {1, INT64_C(1) << 40},  // num_pages
        {2, 0}, {2, INT64_MAX},    // max_pages (no overflow in max_pages * page_size)
        {3, 16},                   // table rows overlap
        {4, INT64_C(1) << 33},     // 32-bit tile offsets overflow
        {5, 144}, {5, 0},          // head dim
        {6, 17},                   // 4 heads x 17 positions: not a decode shape
        {7, 4096 + 32},            // seqlen_kv is not the table's capacity
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        fa_paged_fp8_params b = good(32, 8, 4, 1, 32, 128, 128);
        switch (cases[i].field) {
            case 0: b.paged.page_size = cases[i].value; break;
            case 1: b.paged.num_pages = cases[i].value; break;
            case 2: b.paged.max_pages = cases[i].value; break;
            case 3: b.paged.block_table_stride = cases[i].value; break;
            case 4: b.paged.base.k_seqlen_stride = cases[i].value; break;
            case 5: b.paged.base.headdim = cases[i].value; break;
            case 6: b.paged.base.seqlen_q = cases[i].value; break;
            case 7: b.paged.base.seqlen_kv = cases[i].value; break;
        }
        const int want16 = fa_fwd_gfx950_paged_check(&b.paged, FA_DTYPE_BF16, 1);
        const int want8 = fa_fwd_gfx950_paged_fp8_check(&b, FA_DTYPE_BF16, 1);
        EXPECT((want16 == FA_OK) == (cases[i].field < 0) && (want8 == FA_OK) == (cases[i].field < 0));
        for (size_t w = 0; w < kNumWindows; ++w) {
            EXPECT(fa_fwd_gfx950_paged_window_check(&b.paged, FA_DTYPE_BF16, 1, kWindows[w]) == want16);
            EXPECT(fa_fwd_gfx950_paged_window_fp8_check(&b, FA_DTYPE_BF16, 1, kWindows[w]) == want8);
            if (want16 != FA_OK) {
                EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);
                // the launch and sizing entries validate before touching the device
                EXPECT(fa_fwd_gfx950_paged_window(&b.paged, FA_DTYPE_BF16, 1, kWindows[w], NULL, 0, NULL) == want16);
                EXPECT(fa_fwd_gfx950_paged_window_fp8(&b, FA_DTYPE_BF16, 1, kWindows[w], NULL, 0, NULL) == want8);
                EXPECT(fa_fwd_gfx950_paged_window_workspace_size(&b.paged, FA_DTYPE_BF16, 1, kWindows[w]) == -1);
                EXPECT(fa_fwd_gfx950_paged_window_fp8_workspace_size(&b, FA_DTYPE_BF16, 1, kWindows[w]) == -1);
            }
        }
    }
    EXPECT(fa_fwd_gfx950_paged_window_check(NULL, FA_DTYPE_BF16, 0, 7) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_window_fp8_check(NULL, FA_DTYPE_BF16, 0, 7) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_window(NULL, FA_DTYPE_BF16, 0, 7, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_window_fp8(NULL, FA_DTYPE_BF16, 0, 7, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_window_workspace_size(NULL, FA_DTYPE_BF16, 0, 7) == -1);
    EXPECT(fa_fwd_gfx950_paged_window_fp8_workspace_size(NULL, FA_DTYPE_BF16, 0, 7) == -1);

    // ---- valid parameters reach the (stub) instantiation for every dtype / causal / D tile / window --
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int causal = 0; causal < 2; ++causal)
            for (int64_t d = 16; d <= 128; d += 16)
                for (size_t w = 0; w < kNumWindows; ++w) {
                    fa_paged_fp8_params ok = good(3, 2, 4, 3, 8, 32, d);
                    EXPECT(fa_fwd_gfx950_paged_window(&ok.paged, dtype, causal, kWindows[w], NULL, 0, NULL) ==
                           FA_ERR_UNSUPPORTED);
                    EXPECT(strstr(fa_last_error(), "stub") != NULL);
                    EXPECT(fa_fwd_gfx950_paged_window_fp8(&ok, dtype, causal, kWindows[w], NULL, 0, NULL) ==
                           FA_ERR_UNSUPPORTED);
                    EXPECT(strstr(fa_last_error(), "stub") != NULL);
                }

    // ---- the workspace follows the window's plan -----------------------------------------------------
    // B1 Hkv8 g4 over 131072 keys: the unwindowed plans split (8 units: 20 / 32 splits for 160 / 256 workgroups)
    fa_paged_fp8_params big = good(1, 8, 4, 1, 1024, 128, 128);
    const int64_t full16 = fa_fwd_gfx950_paged_workspace_size(&big.paged, FA_DTYPE_BF16, 0);
    const int64_t full8 = fa_fwd_gfx950_paged_fp8_workspace_size(&big, FA_DTYPE_BF16, 0);
    EXPECT(full16 == INT64_C(8) * 20 * 32 * (128 * 4 + 4) && full8 == INT64_C(8) * 32 * 32 * (128 * 4 + 4));
    for (size_t w = 0; w < kNumWindows; ++w) {
        const int64_t n16 = fa_fwd_gfx950_paged_window_workspace_size(&big.paged, FA_DTYPE_BF16, 0, kWindows[w]);
        const int64_t n8 = fa_fwd_gfx950_paged_window_fp8_workspace_size(&big, FA_DTYPE_BF16, 0, kWindows[w]);
        EXPECT(n16 >= 0 && n16 <= full16 && n8 >= 0 && n8 <= full8);
        if (kWindows[w] < 0 || kWindows[w] >= 131072) EXPECT(n16 == full16 && n8 == full8);
        if (kWindows[w] >= 0 && kWindows[w] <= 32) EXPECT(n16 == 0 && n8 == 0);  // 2-3 tiles: no split
    }
    // window_left 4095, Sq 1: 32 * (128 + 1) keys = 129 tiles, at most 8 splits of 4 waves x 4 tiles: 8 of 17
    const int64_t w16 = fa_fwd_gfx950_paged_window_workspace_size(&big.paged, FA_DTYPE_BF16, 0, 4095);
    EXPECT(w16 == INT64_C(8) * 8 * 32 * (128 * 4 + 4));
    EXPECT(fa_fwd_gfx950_paged_window_fp8_workspace_size(&big, FA_DTYPE_BF16, 0, 4095) == w16);
    EXPECT(fa_fwd_gfx950_paged_window_workspace_size(&big.paged, FA_DTYPE_BF16, 0, 255) == 0);
    EXPECT(fa_fwd_gfx950_paged_window(&big.paged, FA_DTYPE_BF16, 0, 4095, (void *)0x100000, w16 - 16, NULL) ==
           FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_window(&big.paged, FA_DTYPE_BF16, 0, 4095, (void *)0x100008, w16, NULL) ==
           FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_window(&big.paged, FA_DTYPE_BF16, 0, 4095, (void *)0x100000, w16, NULL) ==
           FA_ERR_UNSUPPORTED);  // stub
    EXPECT(fa_fwd_gfx950_paged_window_fp8(&big, FA_DTYPE_BF16, 0, 4095, (void *)0x100000, w16 - 16, NULL) ==
           FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_window_fp8(&big, FA_DTYPE_BF16, 0, 4095, (void *)0x100000, w16, NULL) ==
           FA_ERR_UNSUPPORTED);  // stub
    // a workspace sized for the window is too small for the unwindowed plan of the same launch
    EXPECT(fa_fwd_gfx950_paged_window(&big.paged, FA_DTYPE_BF16, 0, -1, (void *)0x100000, w16, NULL) ==
           FA_ERR_INVALID_ARGUMENT);
    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("paged window validation ok\n");
    return failures ? 1 : 0;
}
