"""Drop-in import name of the reference package (reference flash_attention/__init__.py:1).

``from flash_attention import flash_attn_func`` resolves to the gfx950 implementation, and so do
the reference's submodule paths ``flash_attention.flash_attention`` and
``flash_attention.load_cpp_extention``.
"""
from .flash_attention import flash_attn_func  # noqa: F401
from .flash_attention import flash_attn_varlen_func  # noqa: F401  (beyond the reference: varlen)
from .flash_attention import flash_attn_paged_func  # noqa: F401  (beyond the reference: paged KV cache)
from .flash_attention import flash_attn_kvcache_append, flash_attn_with_kvcache  # noqa: F401  (beyond the reference)
from .flash_attention import flash_attention_kvcache_append  # noqa: F401  (the custom op's function)
from .flash_attention import flash_attention_kvcache_append_fp8, flash_attention_paged_forward_fp8  # noqa: F401  (FP8 cache)
from .flash_attention import flash_attention_paged_window_forward, flash_attention_paged_window_forward_fp8  # noqa: F401  (windowed paged decode)
from .flash_attention import flash_attn_paged_varlen_func, flash_attn_kvcache_append_varlen, flash_attn_varlen_with_kvcache  # noqa: F401  (ragged step on the paged cache)
