"""The decode half of the V1 MLA backend: mirror of TritonMLAImpl._forward_decode
(vllm/v1/attention/backends/mla/triton_mla.py:124-171) up to, and not including, `_v_up_proj`, over
the HIP kernels behind `decode_attention_fwd`.  MLACommonImpl is not mirrored.  Beyond the reference,
which raises for an fp8 cache: kv_cache_dtype "fp8" / "fp8_e4m3" runs when the cache's scale is passed
as `k_scale` (the tensor `concat_and_cache_mla` took)."""
from __future__ import annotations

import torch

from .....attention.ops.triton_decode_attention import decode_attention_fwd


def forward_decode(q_nope: torch.Tensor, q_pe: torch.Tensor, kv_c_and_k_pe_cache: torch.Tensor,
                   block_table: torch.Tensor, seq_lens: torch.Tensor, scale: float, kv_lora_rank: int = 512,
                   kv_cache_dtype: str = "auto", k_scale: torch.Tensor | None = None) -> torch.Tensor:
    """q_nope [B, H, kv_lora_rank], q_pe [B, H, rope]; kv_c_and_k_pe_cache [num_blocks, page_size,
    kv_lora_rank + rope]; returns o [B, H, kv_lora_rank] (the input of `_v_up_proj`)."""
    assert kv_c_and_k_pe_cache.numel() > 0
    if kv_cache_dtype.startswith("fp8") and k_scale is None:
        raise NotImplementedError("FP8 Triton MLA not yet supported")   # :134-135
    B, num_heads = q_nope.shape[0], q_nope.shape[1]
    q = torch.cat([q_nope, q_pe], dim=-1)
    o = torch.zeros(B, num_heads, kv_lora_rank, dtype=q.dtype, device=q.device)
    num_kv_splits = 4   # :146
    attn_logits = torch.empty((B, num_heads, num_kv_splits, kv_lora_rank + 1), dtype=torch.float32,
                              device=q.device)
    kv_c_and_k_pe_cache = kv_c_and_k_pe_cache.unsqueeze(2)   # a head dimension of 1
    kv_c_cache = kv_c_and_k_pe_cache[..., :kv_lora_rank]
    page_size = kv_c_and_k_pe_cache.size(1)
    decode_attention_fwd(q, kv_c_and_k_pe_cache, kv_c_cache, o, block_table, seq_lens, attn_logits,
                         num_kv_splits, scale, page_size, k_scale=k_scale)
    return o
