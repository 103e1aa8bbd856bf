/*
 * fa_gfx950_sink.h -- attention sinks on the paged split-KV decode (16-bit and FP8 e4m3 pools, with or without a
 * sliding window) for the MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no existing version macro moves and no existing entry changes.
 * No reference counterpart; a sink is flash-attn's `s_aux` / `sinks`, vLLM's `sinks`, the learned per-head
 * logit of the gpt-oss models (whose layers alternate a 128-key window with full attention).
 *
 * `sinks` holds one fp32 value per q-head, [num_heads_q], on the device, in FINAL-LOGIT units: it is NOT
 * multiplied by softmax_scale and, for an FP8 pool, NOT by k_descale (the column is concatenated to the already
 * scaled, masked scores). With s_n = scale * q . k_n over the row's visible keys (scale = softmax_scale as the
 * caller means it, times k_descale[b, h] for an FP8 pool; causal and window rules unchanged), row (b, h, m) is
 *
 *     out = v_descale * sum_n exp(s_n - mu) v_n / (sum_n exp(s_n - mu) + exp(sinks[h] - mu)),
 *     mu  = max(max_n s_n, sinks[h]),
 *
 * the softmax with one extra key of logit sinks[h] and value 0 (v_descale: FP8 pools only).
 *
 *   - A row without a visible key stays 0.
 *   - sinks[h] == -inf, or any value at or below -1e30, means "no sink on this head": the row then has the
 *     BITS of the entry without sinks. Values above 1e30 count as 1e30 (such a row is 0). NaN is unspecified.
 *   - The sink is applied once per row: in a split launch the partial results are the unsinked ones and the
 *     sink enters in the final merge. The split plan and the workspace are those of the entry without sinks
 *     (fa_fwd_gfx950_paged / _paged_fp8 for window_left < 0, fa_fwd_gfx950_paged_window / _window_fp8 otherwise).
 *
 * window_left < 0 is no window; every non-negative value is the window of fa_gfx950_paged_window.h (what is
 * read and what is never read is stated there). As there, seqlen_q is taken AS PASSED: pass a decode step as
 * seqlen_q 1 with head_q_per_group = the group size, never as the q-head pack -- the pack would also lose the
 * q-head a row belongs to, which selects its sink. Everything else is fa_gfx950_paged.h's and fa_gfx950_fp8.h's
 * (clamping, the decode rule head_q_per_group * seqlen_q <= 64, the workspace rules).
 *
 * Not built: sinks in the dense, padded, varlen, paged-prefill and ragged entries, and the LSE of a sinked row.
 */
#ifndef FA_GFX950_SINK_H
#define FA_GFX950_SINK_H

#include "fa_gfx950.h"
#include "fa_gfx950_fp8.h"
#include "fa_gfx950_paged.h"
#include "fa_gfx950_paged_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_SINK_VERSION 1

typedef struct fa_paged_sink_params {
    fa_paged_params paged;      /* as for fa_fwd_gfx950_paged / _paged_window */
    const float *sinks;         /* [num_heads_q] fp32, device, 4-byte aligned, non-NULL */
} fa_paged_sink_params;

typedef struct fa_paged_fp8_sink_params {
    fa_paged_fp8_params fp8;    /* as for fa_fwd_gfx950_paged_fp8 / _paged_window_fp8 */
    const float *sinks;
} fa_paged_fp8_sink_params;

/*
 * The paged decode with sinks. Asynchronous, no host synchronisation, safe under hipGraph capture.
 * Validation is the entry's without sinks (its codes and messages; decode shapes only: FA_ERR_UNSUPPORTED)
 * plus: sinks NULL or not 4-byte aligned is FA_ERR_INVALID_ARGUMENT. Workspace as for the entry without sinks
 * (NULL: unsplit; 16-byte aligned; smaller than _workspace_size: FA_ERR_INVALID_ARGUMENT).
 */
int fa_fwd_gfx950_paged_sink(const fa_paged_sink_params *params, int dtype, int causal, int64_t window_left,
                             void *workspace, int64_t workspace_bytes, void *stream);

/* Workspace bytes fa_fwd_gfx950_paged_sink wants (0: no split; -1: invalid parameters). */
int64_t fa_fwd_gfx950_paged_sink_workspace_size(const fa_paged_sink_params *params, int dtype, int causal,
                                                int64_t window_left);

/* Validate exactly as fa_fwd_gfx950_paged_sink does (every window_left is valid), without touching the device. */
int fa_fwd_gfx950_paged_sink_check(const fa_paged_sink_params *params, int dtype, int causal, int64_t window_left);

/* The same three over an FP8 (e4m3) pool. */
int fa_fwd_gfx950_paged_sink_fp8(const fa_paged_fp8_sink_params *params, int dtype, int causal, int64_t window_left,
                                 void *workspace, int64_t workspace_bytes, void *stream);
int64_t fa_fwd_gfx950_paged_sink_fp8_workspace_size(const fa_paged_fp8_sink_params *params, int dtype, int causal,
                                                    int64_t window_left);
int fa_fwd_gfx950_paged_sink_fp8_check(const fa_paged_fp8_sink_params *params, int dtype, int causal,
                                       int64_t window_left);

/* FA_GFX950_SINK_VERSION of the loaded library. */
int fa_sink_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_SINK_H */
