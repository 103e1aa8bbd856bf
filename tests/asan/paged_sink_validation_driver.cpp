// Host-side validation of the attention-sink entry points (include/fa_gfx950_sink.h) under AddressSanitizer +
// UBSan (tests/test_sink_abi.py::test_sink_host_validation_under_asan_ubsan builds and runs it; CPU only). The
// check, sizing and launch entries of the 16-bit and the FP8 pool are called with valid and invalid descriptions
// and must return the paged decode check's codes, plus the rule that is new here (the sinks array), for every
// window_left, with no sanitizer report. Launches that pass validation reach the host-only stubs
// (paged_sink_stub_instances.hip), never a device; the device arrays are never read.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fa_gfx950_sink.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, fa_last_error()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// sq positions of g q-heads per kv-head over a [num_pages, Hkv, page_size, D] pool (strides in elements)
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

static fa_paged_sink_params good16(int64_t b, int64_t hkv, int64_t g, int64_t sq, int64_t max_pages, int64_t page,
                                   int64_t d) {
    fa_paged_sink_params v;
    memset(&v, 0, sizeof(v));
    v.paged = good(b, hkv, g, sq, max_pages, page, d);
    v.sinks = (const float *)0x70000;
    return v;
}

static fa_paged_fp8_sink_params good8(int64_t b, int64_t hkv, int64_t g, int64_t sq, int64_t max_pages, int64_t page,
                                      int64_t d) {
    fa_paged_fp8_sink_params v;
    memset(&v, 0, sizeof(v));
    v.fp8.paged = good(b, hkv, g, sq, max_pages, page, d);
    v.fp8.k_descale = (const float *)0x80000;
    v.fp8.v_descale = (const float *)0x81000;
    v.fp8.descale_batch_stride = hkv;
    v.fp8.descale_head_stride = 1;
    v.sinks = (const float *)0x70000;
    return v;
}

static const int64_t kWindows[] = {-1, -(INT64_C(1) << 40), 0, 1, 127, 4095, INT64_C(1) << 40};

// the three entries of a pool agree on a description, for every window: `want` from the check, the launch
// validates first, the sizing entry answers -1 for anything invalid
#define ALL16(v, dtype, causal, want)                                                                    \
    for (int64_t w : kWindows) {                                                                         \
        EXPECT(fa_fwd_gfx950_paged_sink_check(&(v), dtype, causal, w) == (want));                         \
        EXPECT(fa_fwd_gfx950_paged_sink(&(v), dtype, causal, w, NULL, 0, NULL) == (want));                \
        EXPECT(fa_fwd_gfx950_paged_sink_workspace_size(&(v), dtype, causal, w) == -1);                    \
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);                            \
    }
#define ALL8(v, dtype, causal, want)                                                                     \
    for (int64_t w : kWindows) {                                                                         \
        EXPECT(fa_fwd_gfx950_paged_sink_fp8_check(&(v), dtype, causal, w) == (want));                     \
        EXPECT(fa_fwd_gfx950_paged_sink_fp8(&(v), dtype, causal, w, NULL, 0, NULL) == (want));            \
        EXPECT(fa_fwd_gfx950_paged_sink_fp8_workspace_size(&(v), dtype, causal, w) == -1);                \
        EXPECT(strlen(fa_last_error()) > 0 && strlen(fa_last_error()) < 512);                            \
    }

int main() {
    EXPECT(fa_sink_version() == FA_GFX950_SINK_VERSION);
    EXPECT(fa_abi_version() == FA_GFX950_ABI_VERSION);
    EXPECT(fa_paged_version() == FA_GFX950_PAGED_VERSION);
    EXPECT(fa_fp8_version() == FA_GFX950_FP8_VERSION);
    EXPECT(fa_paged_window_version() == FA_GFX950_PAGED_WINDOW_VERSION);

    // ---- the rule that is new here ----------------------------------------------------------------------
    {
        fa_paged_sink_params a = good16(32, 8, 4, 1, 32, 128, 128);
        fa_paged_fp8_sink_params f = good8(32, 8, 4, 1, 32, 128, 128);
        a.sinks = NULL;
        f.sinks = NULL;
        ALL16(a, 1, 0, FA_ERR_INVALID_ARGUMENT);
        ALL8(f, 1, 0, FA_ERR_INVALID_ARGUMENT);
        a.sinks = (const float *)0x70002;
        f.sinks = (const float *)0x70001;
        ALL16(a, 0, 1, FA_ERR_INVALID_ARGUMENT);
        ALL8(f, 0, 1, FA_ERR_INVALID_ARGUMENT);
    }
    // ---- the base description: the codes are the paged decode checks' -------------------------------------
    {
        fa_paged_sink_params a = good16(32, 8, 4, 1, 32, 128, 128);
        a.paged.page_size = 48;
        ALL16(a, 1, 0, FA_ERR_INVALID_ARGUMENT);
        a = good16(32, 8, 4, 17, 32, 128, 128);  // g 4 x Sq 17: past the decode rule
        ALL16(a, 1, 1, FA_ERR_UNSUPPORTED);
        a = good16(32, 8, 4, 1, 32, 128, 128);
        a.paged.block_table = NULL;
        ALL16(a, 1, 0, FA_ERR_INVALID_ARGUMENT);
        a = good16(32, 8, 4, 1, 32, 128, 128);
        ALL16(a, 7, 0, FA_ERR_UNSUPPORTED);  // dtype
        fa_paged_fp8_sink_params f = good8(32, 8, 4, 1, 32, 128, 72);  // an fp8 pool needs D % 16 == 0
        ALL8(f, 1, 0, FA_ERR_INVALID_ARGUMENT);
        f = good8(32, 8, 4, 17, 32, 128, 128);
        ALL8(f, 1, 1, FA_ERR_UNSUPPORTED);
        f = good8(32, 8, 4, 1, 32, 128, 128);
        f.fp8.k_descale = (const float *)0x80002;
        ALL8(f, 1, 0, FA_ERR_INVALID_ARGUMENT);
        EXPECT(fa_fwd_gfx950_paged_sink_check(NULL, 1, 0, -1) == FA_ERR_INVALID_ARGUMENT);
        EXPECT(fa_fwd_gfx950_paged_sink_fp8_check(NULL, 1, 0, 5) == FA_ERR_INVALID_ARGUMENT);
        EXPECT(fa_fwd_gfx950_paged_sink_workspace_size(NULL, 1, 0, -1) == -1);
        EXPECT(fa_fwd_gfx950_paged_sink_fp8(NULL, 1, 0, -1, NULL, 0, NULL) == FA_ERR_INVALID_ARGUMENT);
    }
    // ---- valid descriptions: the workspace is the entry's without sinks, a smaller one is refused, and a ----
    // ---- launch that passes every check reaches the stub ---------------------------------------------------
    const int64_t shapes[][7] = {{1, 8, 8, 1, 256, 64, 64}, {32, 8, 4, 1, 32, 128, 128}, {2, 2, 4, 3, 64, 32, 128},
                                 {4, 8, 8, 5, 16, 256, 64}};
    for (const auto &s : shapes) {
        for (int dtype = 0; dtype < 2; ++dtype) {
            for (int64_t w : kWindows) {
                fa_paged_sink_params a = good16(s[0], s[1], s[2], s[3], s[4], s[5], s[6]);
                fa_paged_fp8_sink_params f = good8(s[0], s[1], s[2], s[3], s[4], s[5], s[6]);
                const int c = s[3] > 1;
                EXPECT(fa_fwd_gfx950_paged_sink_check(&a, dtype, c, w) == FA_OK);
                EXPECT(fa_fwd_gfx950_paged_sink_fp8_check(&f, dtype, c, w) == FA_OK);
                const int64_t n16 = fa_fwd_gfx950_paged_sink_workspace_size(&a, dtype, c, w);
                const int64_t n8 = fa_fwd_gfx950_paged_sink_fp8_workspace_size(&f, dtype, c, w);
                EXPECT(n16 == fa_fwd_gfx950_paged_window_workspace_size(&a.paged, dtype, c, w) && n16 >= 0);
                EXPECT(n8 == fa_fwd_gfx950_paged_window_fp8_workspace_size(&f.fp8, dtype, c, w) && n8 >= 0);
                if (w < 0) {
                    EXPECT(n16 == fa_fwd_gfx950_paged_workspace_size(&a.paged, dtype, c));
                    EXPECT(n8 == fa_fwd_gfx950_paged_fp8_workspace_size(&f.fp8, dtype, c));
                }
                if (n16 > 0)
                    EXPECT(fa_fwd_gfx950_paged_sink(&a, dtype, c, w, (void *)0x100000, n16 - 1, NULL) ==
                           FA_ERR_INVALID_ARGUMENT);
                if (n8 > 0)
                    EXPECT(fa_fwd_gfx950_paged_sink_fp8(&f, dtype, c, w, (void *)0x100000, n8 - 1, NULL) ==
                           FA_ERR_INVALID_ARGUMENT);
                EXPECT(fa_fwd_gfx950_paged_sink(&a, dtype, c, w, (void *)0x100008, n16, NULL) == FA_ERR_INVALID_ARGUMENT);
                // unsplit (no workspace): validation passes, the stub answers
                EXPECT(fa_fwd_gfx950_paged_sink(&a, dtype, c, w, NULL, 0, NULL) == FA_ERR_UNSUPPORTED);
                EXPECT(strstr(fa_last_error(), "stub") != NULL);
                EXPECT(fa_fwd_gfx950_paged_sink_fp8(&f, dtype, c, w, NULL, 0, NULL) == FA_ERR_UNSUPPORTED);
                EXPECT(strstr(fa_last_error(), "stub") != NULL);
            }
        }
    }
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("paged sink validation ok\n");
    return 0;
}
