"""MI355X-native FlashAttention-2 forward (drop-in for izmttk/flash_attention_cute)."""
from .flash_attention import (apply_rope, flash_attention_forward, flash_attention_padded_forward,  # noqa: F401
                              flash_attention_paged_forward, flash_attn_paged_func,
                              flash_attention_kvcache_append, flash_attn_kvcache_append, flash_attn_with_kvcache,
                              flash_attention_kvcache_append_fp8, flash_attention_paged_forward_fp8,
                              flash_attention_paged_window_forward, flash_attention_paged_window_forward_fp8,
                              flash_attention_varlen_forward, flash_attention_window_forward, flash_attn_func,
                              flash_attn_padded_func, flash_attn_rope_func, flash_attn_varlen_func,
                              flash_attn_window_func, split_errors,
                              flash_attention_paged_forward_lse, flash_attention_paged_forward_lse_fp8,
                              flash_attention_merge_states, flash_attn_merge_states,
                              flash_attn_paged_shared_prefix_func,
                              flash_attention_paged_varlen_forward, flash_attn_paged_varlen_func,
                              flash_attention_kvcache_append_varlen, flash_attn_kvcache_append_varlen,
                              flash_attn_varlen_with_kvcache,
                              flash_attention_paged_forward_sink, flash_attention_paged_forward_sink_fp8)

__all__ = ["flash_attn_func", "flash_attention_forward", "flash_attn_varlen_func", "flash_attention_varlen_forward",
           "flash_attn_rope_func", "apply_rope", "flash_attn_window_func", "flash_attention_window_forward",
           "flash_attn_padded_func", "flash_attention_padded_forward", "flash_attn_paged_func",
           "flash_attention_paged_forward", "flash_attn_kvcache_append", "flash_attn_with_kvcache",
           "flash_attention_kvcache_append", "flash_attention_paged_forward_fp8",
           "flash_attention_kvcache_append_fp8", "flash_attention_paged_window_forward",
           "flash_attention_paged_window_forward_fp8", "split_errors", "flash_attention_paged_forward_lse",
           "flash_attention_paged_forward_lse_fp8", "flash_attention_merge_states", "flash_attn_merge_states",
           "flash_attn_paged_shared_prefix_func", "flash_attention_paged_varlen_forward",
           "flash_attn_paged_varlen_func", "flash_attention_kvcache_append_varlen",
           "flash_attn_kvcache_append_varlen", "flash_attn_varlen_with_kvcache",
           "flash_attention_paged_forward_sink", "flash_attention_paged_forward_sink_fp8"]
