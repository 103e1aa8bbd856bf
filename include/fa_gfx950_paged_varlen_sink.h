/*
 * fa_gfx950_paged_varlen_sink.h -- attention sinks on the ragged paged prefill (fa_gfx950_paged_varlen.h) for the
 * MI355X (gfx950 / CDNA4) FlashAttention-2 forward operator: the prompt chunks of a continuous batch for a model
 * whose heads carry a learned sink (gpt-oss), in ONE launch of the paged prefill kernel with the pool read in place.
 *
 * An addition to the boundary of fa_gfx950.h (same library, same conventions, error codes and
 * fa_last_error()), versioned on its own: no existing version macro moves and no existing entry changes.
 * The query side, the pool, the table, the lengths, the masks and the never-read guarantees are
 * fa_gfx950_paged_varlen.h's, per sequence; the sink is fa_gfx950_sink.h's:
 *
 * `sinks` holds one fp32 value per q-head, [num_heads_q], on the device, in FINAL-LOGIT units: it is NOT
 * multiplied by softmax_scale (the column is concatenated to the already scaled, masked scores). With
 * s_n = softmax_scale * q . k_n over the row's visible keys (causal and window rules unchanged), row m of q-head h is
 *
 *     out = sum_n exp(s_n - mu) v_n / (sum_n exp(s_n - mu) + exp(sinks[h] - mu)),
 *     mu  = max(max_n s_n, sinks[h]),
 *
 * the softmax with one extra key of logit sinks[h] and value 0.
 *
 *   - A row without a visible key stays 0.
 *   - sinks[h] == -inf, or any value at or below -1e30, means "no sink on this head": the row then has the
 *     BITS of fa_fwd_gfx950_paged_varlen. Values above 1e30 count as 1e30 (such a row is 0). NaN is unspecified.
 *   - The sink is applied once per row, when the row's sum is final: the key loop is the unsinked one.
 *   - The array is read at [0, num_heads_q) only.
 *
 * 16-bit pools and page sizes that are multiples of 64 only, as the entry without sinks. Not built: sinks in the
 * dense, padded and varlen entries and in the uniform paged prefill (fa_gfx950_paged_prefill.h: pass a uniform
 * chunk here with a uniform cu_seqlens_q), FP8 pools in this kernel, and the LSE of a sinked row.
 */
#ifndef FA_GFX950_PAGED_VARLEN_SINK_H
#define FA_GFX950_PAGED_VARLEN_SINK_H

#include "fa_gfx950.h"
#include "fa_gfx950_paged_varlen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_GFX950_PAGED_VARLEN_SINK_VERSION 1

typedef struct fa_paged_varlen_sink_params {
    fa_paged_varlen_params varlen; /* as for fa_fwd_gfx950_paged_varlen */
    const float *sinks;            /* [num_heads_q] fp32, device, 4-byte aligned, non-NULL */
} fa_paged_varlen_sink_params;

/*
 * The ragged paged prefill with sinks. Asynchronous, no host synchronisation, safe under hipGraph capture (sinks
 * is read when the kernel runs, as cu_seqlens_q, the table, the lengths and the pool are). Validation is
 * fa_fwd_gfx950_paged_varlen's (its codes and messages) plus: sinks NULL or not 4-byte aligned is
 * FA_ERR_INVALID_ARGUMENT. The launch keeps nothing in the workspace (_workspace_size is 0 and `workspace` may be
 * NULL); workspace_bytes below _workspace_size, a negative one included, is FA_ERR_INVALID_ARGUMENT.
 * total_q == 0 launches nothing.
 */
int fa_fwd_gfx950_paged_varlen_sink(const fa_paged_varlen_sink_params *params, int dtype, int causal,
                                    int64_t window_left, void *workspace, int64_t workspace_bytes, void *stream);

/* Workspace bytes fa_fwd_gfx950_paged_varlen_sink wants (0; -1: invalid parameters). Host-only. */
int64_t fa_fwd_gfx950_paged_varlen_sink_workspace_size(const fa_paged_varlen_sink_params *params, int dtype,
                                                       int causal, int64_t window_left);

/* Validate exactly as fa_fwd_gfx950_paged_varlen_sink does, without touching the device:
 * fa_fwd_gfx950_paged_varlen_check (called, not copied), then the sinks rule. */
int fa_fwd_gfx950_paged_varlen_sink_check(const fa_paged_varlen_sink_params *params, int dtype, int causal);

/* FA_GFX950_PAGED_VARLEN_SINK_VERSION of the loaded library. */
int fa_paged_varlen_sink_version(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_GFX950_PAGED_VARLEN_SINK_H */
