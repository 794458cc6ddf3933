"""The prefill half of the V1 MLA backend: mirrors of MLACommonImpl._flash_attn_varlen_diff_headdims
(vllm/v1/attention/backends/mla/common.py:821-857) and _forward_prefill / _compute_prefill_context (:1017-1127) over
the HIP kernels `vllm_amd_mla_prefill_attention`, `vllm_amd_merge_attn_states` (csrc/mla_prefill.hip) and
`gather_cache` (csrc/cache_kernels.hip).  Nothing else of MLACommonImpl is mirrored (no metadata builder, no
kv_b_proj, no rope): the up-projection of a context chunk is passed in as a callable.

Where the reference concatenates k_nope with the expanded k_pe, pads v from 128 to 192 columns and calls
flash_attn_varlen_func, the kernel here takes K in split form and v at its own width: no copy is made."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import torch

from ....._custom_ops import gather_cache
from ....._lib import check, lib
from ....._torch_ops import _dev, _dt, _ptr, _stream
from .....attention.ops.merge_attn_states import merge_attn_states

QK_NOPE, QK_ROPE, V_DIM = 128, 64, 128


@dataclass
class ChunkedContext:
    """MLACommonPrefillMetadata.ChunkedContextMetadata (:266-279) with what _compute_prefill_context takes from
    `self` and the prefill metadata beside it."""
    kv_c_and_k_pe_cache: torch.Tensor          # [num_blocks, page_size, kv_lora_rank + 64]
    block_table: torch.Tensor                  # int32 [B, max_blocks]
    cu_seq_lens: Sequence[torch.Tensor]        # per chunk: int32 [B + 1]
    starts: Sequence[torch.Tensor]             # per chunk: int32 [B], multiples of the page size
    seq_tot: Sequence[int]                     # per chunk: tokens gathered
    max_seq_lens: Sequence[int]                # per chunk: longest piece
    workspace: torch.Tensor                    # [>= max(seq_tot), kv_lora_rank + 64], q's dtype
    kv_b_proj: Callable[[torch.Tensor], torch.Tensor]   # [toks, kv_lora_rank] -> [toks, H * 256]
    kv_lora_rank: int = 512
    scale: Optional[torch.Tensor] = None       # the fp8 cache's scale (float32, one element); None: a 16-bit cache


@torch.inference_mode()
def flash_attn_varlen_diff_headdims(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale,
                                    causal, return_softmax_lse=False, k_pe=None):
    """q [Tq, H, 192]; k [Tk, H, 192], or k [Tk, H, 128] with k_pe [Tk, 1 | H, 64]; v [Tk, H, 128] (never padded).
    Returns out [Tq, H, 128], with return_softmax_lse also lse float32 [H, Tq].  causal is bottom-right aligned."""
    Tq, H, Dq = q.shape
    if k_pe is None:
        if k.dim() != 3 or k.shape[2] != QK_NOPE + QK_ROPE:
            raise RuntimeError(f"flash_attn_varlen_diff_headdims: without k_pe, k must be [Tk, H, 192]; got {tuple(k.shape)}")
        kp_ptr, kp_st, kp_sh, kp_ok = k.data_ptr() + QK_NOPE * k.element_size(), k.stride(0), k.stride(1), True
    else:
        k_pe = k_pe.unsqueeze(1) if k_pe.dim() == 2 else k_pe
        kp_ok = (k_pe.dim() == 3 and k_pe.shape[0] == k.shape[0] and k_pe.shape[1] in (1, H) and k_pe.shape[2] == QK_ROPE
                 and k_pe.stride(2) == 1 and k_pe.dtype == q.dtype and k_pe.device == q.device and k.shape[2] == QK_NOPE)
        kp_ptr, kp_st, kp_sh = k_pe.data_ptr(), k_pe.stride(0), (0 if k_pe.shape[1] == 1 else k_pe.stride(1))
    ok = (kp_ok and k.dim() == 3 and v.dim() == 3 and k.shape[:2] == v.shape[:2] and k.shape[1] == H
          and v.shape[2] == V_DIM and q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
          and k.dtype == q.dtype and v.dtype == q.dtype and k.device == q.device and v.device == q.device
          and cu_seqlens_q.dtype == torch.int32 and cu_seqlens_k.dtype == torch.int32
          and cu_seqlens_q.is_contiguous() and cu_seqlens_k.is_contiguous()
          and cu_seqlens_q.shape == cu_seqlens_k.shape and cu_seqlens_q.device == q.device
          and cu_seqlens_k.device == q.device)
    if not ok:
        raise RuntimeError("flash_attn_varlen_diff_headdims: q [Tq, H, 192], k [Tk, H, 192] or k [Tk, H, 128] with k_pe "
                           "[Tk, 1 | H, 64], v [Tk, H, 128] of one 16-bit dtype with contiguous last dimensions and "
                           "int32 cu_seqlens_q / cu_seqlens_k [B + 1] on q's device are required")
    out = torch.empty((Tq, H, V_DIM), dtype=q.dtype, device=q.device)
    lse = torch.empty((H, Tq), dtype=torch.float32, device=q.device) if return_softmax_lse else None
    with _dev(q):
        check(lib.vllm_amd_mla_prefill_attention(
            _ptr(out), _ptr(lse), _ptr(q), _ptr(k), kp_ptr, _ptr(v), _ptr(cu_seqlens_q), _ptr(cu_seqlens_k),
            cu_seqlens_q.numel() - 1, Tq, H, Dq, v.shape[2], QK_ROPE, int(max_seqlen_q), float(softmax_scale),
            int(bool(causal)), q.stride(0), q.stride(1), out.stride(0), out.stride(1), k.stride(0), k.stride(1),
            kp_st, kp_sh, v.stride(0), v.stride(1), Tq, _dt(q), _stream(q)))
    return (out, lse) if return_softmax_lse else out


def _split(kv_nope: torch.Tensor, H: int):
    kv_nope = kv_nope.view(-1, H, QK_NOPE + V_DIM)
    return kv_nope[..., :QK_NOPE], kv_nope[..., QK_NOPE:]   # views: the kernel reads them where they are


@torch.inference_mode()
def forward_prefill(q: torch.Tensor, kv_nope: torch.Tensor, k_pe: torch.Tensor, query_start_loc: torch.Tensor,
                    max_query_len: int, scale: float, context: Optional[ChunkedContext] = None) -> torch.Tensor:
    """q [T, H, 192], kv_nope = kv_b_proj(kv_c_normed) [T, H * 256] (or [T, H, 256]), k_pe [T, 1, 64] or [T, 64] of
    the new tokens; query_start_loc int32 [B + 1].  Returns [T, H * 128]."""
    H = q.shape[1]
    k_nope, v = _split(kv_nope, H)
    output = flash_attn_varlen_diff_headdims(q, k_nope, v, query_start_loc, query_start_loc, max_query_len,
                                             max_query_len, scale, True, return_softmax_lse=context is not None,
                                             k_pe=k_pe)
    if context is not None:
        suffix_output, suffix_lse = output
        ctx_out = ctx_lse = None
        c, rank = context, context.kv_lora_rank
        for i, toks in enumerate(c.seq_tot):           # _compute_prefill_context (:1017-1081)
            gather_cache(c.kv_c_and_k_pe_cache, c.workspace, c.block_table, c.cu_seq_lens[i],
                         query_start_loc.numel() - 1, c.starts[i], **({} if c.scale is None else {"scale": c.scale}))
            rows = c.workspace[:toks]
            ck_nope, cv = _split(c.kv_b_proj(rows[..., :rank]), H)
            o, l = flash_attn_varlen_diff_headdims(q, ck_nope, cv, query_start_loc, c.cu_seq_lens[i], max_query_len,
                                                   c.max_seq_lens[i], scale, False, return_softmax_lse=True,
                                                   k_pe=rows[..., rank:].unsqueeze(1))
            if ctx_out is None:
                ctx_out, ctx_lse = o, l
            else:
                merged, merged_lse = torch.empty_like(ctx_out), torch.empty_like(ctx_lse)
                merge_attn_states(merged, ctx_out, ctx_lse, o, l, merged_lse)
                ctx_out, ctx_lse = merged, merged_lse
        output = suffix_output
        if ctx_out is not None:
            output = torch.empty_like(suffix_output)
            merge_attn_states(output, ctx_out, ctx_lse, suffix_output, suffix_lse)
    return output.flatten(start_dim=-2)
