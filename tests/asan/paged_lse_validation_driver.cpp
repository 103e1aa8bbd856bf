// Host-side validation of the LSE entry points (include/fa_gfx950_lse.h) under AddressSanitizer + UBSan
// (tests/test_lse_abi.py::test_lse_host_validation_under_asan_ubsan builds and runs it; CPU only). The check,
// sizing and launch entries of the 16-bit and the FP8 pool are called with valid and invalid descriptions and
// must return the paged decode check's codes, plus the rules that are new here (the LSE array, seqlen_offset,
// no window, seqlens_k may be NULL), with no sanitizer report. Launches that pass validation reach the
// host-only stubs (paged_lse_stub_instances.hip), never a device; the device arrays are never read. The merge
// entry's check is host code of a kernel file and is covered by tests/test_lse_abi.py on the built library.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_lse.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// sq positions of g q-heads per kv-head over a [num_pages, Hkv, page_size, D] pool (elem: bytes of a K / V element
// only matter to the caller; the strides are in elements)
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

static fa_paged_lse_params good16(int64_t b, int64_t hkv, int64_t g, int64_t sq, int64_t max_pages, int64_t page,
                                  int64_t d) {
    fa_paged_lse_params v;
    memset(&v, 0, sizeof(v));
    v.paged = good(b, hkv, g, sq, max_pages, page, d);
    v.lse_ptr = (float *)0x70000;
    v.lse_batch_stride = hkv * g * sq;
    v.lse_head_stride = sq;
    v.lse_seqlen_stride = 1;
    return v;
}

static fa_paged_fp8_lse_params good8(int64_t b, int64_t hkv, int64_t g, int64_t sq, int64_t max_pages, int64_t page,
                                     int64_t d) {
    fa_paged_fp8_lse_params v;
    memset(&v, 0, sizeof(v));
    v.fp8.paged = good(b, hkv, g, sq, max_pages, page, d);
    v.fp8.k_descale = (const float *)0x80000;
    v.fp8.v_descale = (const float *)0x81000;
    v.fp8.descale_batch_stride = hkv;
    v.fp8.descale_head_stride = 1;
    v.lse_ptr = (float *)0x70000;
    v.lse_batch_stride = hkv * g * sq;
    v.lse_head_stride = sq;
    v.lse_seqlen_stride = 1;
    return v;
}

// the three entries of a pool agree on a description: `want` from the check, the launch validates first, the
// sizing entry answers -1 for anything invalid
#define ALL16(v, dtype, causal, w, want)                                                                 \
    do {                                                                                                 \
        EXPECT(fa_fwd_gfx950_paged_lse_check(&(v), dtype, causal, w) == (want));                          \
        EXPECT(fa_fwd_gfx950_paged_lse(&(v), dtype, causal, w, NULL, 0, NULL) == (want));                 \
        EXPECT(fa_fwd_gfx950_paged_lse_workspace_size(&(v), dtype, causal, w) == -1);                     \
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);                            \
    } while (0)
#define ALL8(v, dtype, causal, w, want)                                                                  \
    do {                                                                                                 \
        EXPECT(fa_fwd_gfx950_paged_lse_fp8_check(&(v), dtype, causal, w) == (want));                      \
        EXPECT(fa_fwd_gfx950_paged_lse_fp8(&(v), dtype, causal, w, NULL, 0, NULL) == (want));             \
        EXPECT(fa_fwd_gfx950_paged_lse_fp8_workspace_size(&(v), dtype, causal, w) == -1);                 \
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);                            \
    } while (0)

int main() {
    EXPECT(fa_lse_version() == FA_GFX950_LSE_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);
    EXPECT(fa_paged_version() == FA_GFX950_PAGED_VERSION);
    EXPECT(fa_fp8_version() == FA_GFX950_FP8_VERSION);

    // ---- the base description: the codes are the paged decode checks' ------------------------------------
    struct Case { int field; int64_t value; } cases[] = {
        {0, 48}, {0, 0}, {0, -64},        // page_size
        {1, 0}, {1, INT64_C(1) << 40},    // num_pages
        {2, 0}, {2, INT64_MAX},           // max_pages (no overflow in max_pages * page_size)
        {3, 16},                          // table rows overlap
        {4, INT64_C(1) << 33},            // 32-bit tile offsets overflow
        {5, 144}, {5, 0},                 // head dim
        {6, 17},                          // 65 rows: past the decode rule
        {7, 4096 + 64},                   // seqlen_kv is not the table's capacity
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
        fa_paged_lse_params a = good16(32, 8, 4, 1, 32, 128, 128);
        fa_paged_fp8_lse_params b = good8(32, 8, 4, 1, 32, 128, 128);
        fa_paged_params *both[2] = {&a.paged, &b.fp8.paged};
        for (int k = 0; k < 2; ++k) {
            fa_paged_params &g = *both[k];
            switch (cases[i].field) {
                case 0: g.page_size = cases[i].value; break;
                case 1: g.num_pages = cases[i].value; break;
                case 2: g.max_pages = cases[i].value; break;
                case 3: g.block_table_stride = cases[i].value; break;
                case 4: g.base.k_seqlen_stride = cases[i].value; break;
                case 5: g.base.headdim = cases[i].value; break;
                case 6: g.base.seqlen_q = cases[i].value; break;
                case 7: g.base.seqlen_kv = cases[i].value; break;
            }
        }
        const int want16 = fa_fwd_gfx950_paged_check(&a.paged, FA_DTYPE_BF16, 1);
        const int want8 = fa_fwd_gfx950_paged_fp8_check(&b.fp8, FA_DTYPE_BF16, 1);
        EXPECT(want16 != FA_OK && want8 != FA_OK);
        ALL16(a, FA_DTYPE_BF16, 1, -1, want16);
        ALL8(b, FA_DTYPE_BF16, 1, -1, want8);
    }
    EXPECT(fa_fwd_gfx950_paged_lse_check(NULL, FA_DTYPE_BF16, 0, -1) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_lse(NULL, FA_DTYPE_BF16, 0, -1, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_lse_workspace_size(NULL, FA_DTYPE_BF16, 0, -1) == -1);
    EXPECT(fa_fwd_gfx950_paged_lse_fp8_check(NULL, FA_DTYPE_BF16, 0, -1) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_lse_fp8(NULL, FA_DTYPE_BF16, 0, -1, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    EXPECT(fa_fwd_gfx950_paged_lse_fp8_workspace_size(NULL, FA_DTYPE_BF16, 0, -1) == -1);

    // ---- new here: the LSE array, seqlen_offset, the window, a NULL seqlens_k ------------------------------
    {
        fa_paged_lse_params a = good16(4, 8, 4, 1, 32, 64, 128);
        fa_paged_fp8_lse_params b = good8(4, 8, 4, 1, 32, 64, 128);
        EXPECT(fa_fwd_gfx950_paged_lse_check(&a, FA_DTYPE_F16, 0, -1) == FA_OK);
        EXPECT(fa_fwd_gfx950_paged_lse_fp8_check(&b, FA_DTYPE_F16, 0, -1) == FA_OK);
        a.lse_ptr = b.lse_ptr = NULL;
        ALL16(a, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
        ALL8(b, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
        a.lse_ptr = b.lse_ptr = (float *)0x70002;  // misaligned
        ALL16(a, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
        ALL8(b, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
        a.lse_ptr = b.lse_ptr = (float *)0x70000;
        const int64_t bad_strides[] = {-1, INT64_MIN};
        for (int f = 0; f < 3; ++f)
            for (int s = 0; s < 2; ++s) {
                fa_paged_lse_params a2 = a;
                fa_paged_fp8_lse_params b2 = b;
                (f == 0 ? a2.lse_batch_stride : f == 1 ? a2.lse_head_stride : a2.lse_seqlen_stride) = bad_strides[s];
                (f == 0 ? b2.lse_batch_stride : f == 1 ? b2.lse_head_stride : b2.lse_seqlen_stride) = bad_strides[s];
                ALL16(a2, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
                ALL8(b2, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
            }
        const int64_t bad_offsets[] = {(INT64_C(1) << 30) + 1, -(INT64_C(1) << 30) - 1, INT64_MAX, INT64_MIN};
        for (int s = 0; s < 4; ++s) {
            fa_paged_lse_params a2 = a;
            fa_paged_fp8_lse_params b2 = b;
            a2.seqlen_offset = b2.seqlen_offset = bad_offsets[s];
            ALL16(a2, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
            ALL8(b2, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
        }
        const int64_t windows[] = {0, 1, 4095, INT64_C(1) << 30, INT64_MAX};
        for (int s = 0; s < 5; ++s) {
            ALL16(a, FA_DTYPE_F16, 0, windows[s], FA_ERR_UNSUPPORTED);
            EXPECT(strstr(fa_last_error(), "window") != NULL);
            ALL8(b, FA_DTYPE_F16, 0, windows[s], FA_ERR_UNSUPPORTED);
        }
        // every offset in range, with and without seqlens_k, and any negative window_left
        const int64_t offsets[] = {0, 1, -1, 2048, -2048, INT64_C(1) << 30, -(INT64_C(1) << 30)};
        for (int s = 0; s < 7; ++s)
            for (int null_lens = 0; null_lens < 2; ++null_lens) {
                fa_paged_lse_params a2 = a;
                fa_paged_fp8_lse_params b2 = b;
                a2.seqlen_offset = b2.seqlen_offset = offsets[s];
                if (null_lens) a2.paged.seqlens_k = b2.fp8.paged.seqlens_k = NULL;
                EXPECT(fa_fwd_gfx950_paged_lse_check(&a2, FA_DTYPE_BF16, 1, s ? -1 : INT64_MIN) == FA_OK);
                EXPECT(fa_fwd_gfx950_paged_lse_fp8_check(&b2, FA_DTYPE_BF16, 1, s ? -1 : INT64_MIN) == FA_OK);
            }
        // a NULL block_table is still refused (the stand-in for seqlens_k needs it, and so does the kernel)
        a.paged.block_table = NULL;
        a.paged.seqlens_k = NULL;
        ALL16(a, FA_DTYPE_F16, 0, -1, FA_ERR_INVALID_ARGUMENT);
    }

    // ---- valid parameters reach the (stub) instantiation for every dtype / causal / D; the workspace rules -----
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int causal = 0; causal < 2; ++causal)
            for (int64_t d = 16; d <= 128; d += 16)
                for (int64_t sq = 1; sq <= 16; sq *= 4) {
                    fa_paged_lse_params a = good16(2, 2, 4, sq, 64, 64, d);
                    fa_paged_fp8_lse_params b = good8(2, 2, 4, sq, 64, 64, d);
                    // the view of a shared-prefix group: zero / permuted LSE strides are fine
                    a.lse_batch_stride = sq * 8;
                    a.lse_head_stride = 1;
                    a.lse_seqlen_stride = 8;
                    EXPECT(fa_fwd_gfx950_paged_lse_check(&a, dtype, causal, -1) == FA_OK);
                    EXPECT(fa_fwd_gfx950_paged_lse_fp8_check(&b, dtype, causal, -1) == FA_OK);
                    // the plan, and so the workspace, is the one of the entry without the LSE
                    const int64_t n16 = fa_fwd_gfx950_paged_lse_workspace_size(&a, dtype, causal, -1);
                    const int64_t n8 = fa_fwd_gfx950_paged_lse_fp8_workspace_size(&b, dtype, causal, -1);
                    EXPECT(n16 == fa_fwd_gfx950_paged_workspace_size(&a.paged, dtype, causal));
                    EXPECT(n8 == fa_fwd_gfx950_paged_fp8_workspace_size(&b.fp8, dtype, causal));
                    EXPECT(n16 > 0 && n8 > 0);
                    EXPECT(fa_fwd_gfx950_paged_lse(&a, dtype, causal, -1, NULL, 0, NULL) == FA_ERR_UNSUPPORTED);
                    EXPECT(strstr(fa_last_error(), "stub") != NULL);
                    EXPECT(fa_fwd_gfx950_paged_lse_fp8(&b, dtype, causal, -1, NULL, 0, NULL) == FA_ERR_UNSUPPORTED);
                    EXPECT(strstr(fa_last_error(), "stub") != NULL);
                    // one byte less than the entry asks for, and a misaligned workspace
                    EXPECT(fa_fwd_gfx950_paged_lse(&a, dtype, causal, -1, (void *)0x100000, n16 - 1, NULL) ==
                           FA_ERR_INVALID_ARGUMENT);
                    EXPECT(strstr(fa_last_error(), "workspace") != NULL);
                    EXPECT(fa_fwd_gfx950_paged_lse_fp8(&b, dtype, causal, -1, (void *)0x100000, n8 - 1, NULL) ==
                           FA_ERR_INVALID_ARGUMENT);
                    EXPECT(fa_fwd_gfx950_paged_lse(&a, dtype, causal, -1, (void *)0x100008, n16, NULL) ==
                           FA_ERR_INVALID_ARGUMENT);
                }

    if (failures) fprintf(stderr, "%d failures\n", failures);
    else printf("paged lse validation ok\n");
    return failures ? 1 : 0;
}
