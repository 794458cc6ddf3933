"""Python op surface of the hot path: same names, arguments and error behaviour
as the reference's ``vllm/_custom_ops.py`` (file:line cited per function), so a
caller written against the reference runs unchanged:

    from vllm_amd import _custom_ops as ops

Every function dispatches through ``torch.ops.<ns>.<op>`` (registered in
``vllm_amd/_torch_ops.py``) into the hand-written HIP kernels; there is no
eager / Triton / CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _torch_ops  # noqa: F401  (registers torch.ops._C / _C_cache_ops / _rocm_C)

# vllm/platforms/rocm.py:387-397 -- gfx950 uses OCP e4m3fn (gfx94x used fnuz)
FP8_DTYPE = torch.float8_e4m3fn


# vllm/_custom_ops.py:39-65
def paged_attention_v1(
    out: torch.Tensor,
    query: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    num_kv_heads: int,
    scale: float,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    block_size: int,
    max_seq_len: int,
    alibi_slopes: Optional[torch.Tensor],
    kv_cache_dtype: str,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    tp_rank: int = 0,
    blocksparse_local_blocks: int = 0,
    blocksparse_vert_stride: int = 0,
    blocksparse_block_size: int = 64,
    blocksparse_head_sliding_step: int = 0,
) -> None:
    torch.ops._C.paged_attention_v1(
        out, query, key_cache, value_cache, num_kv_heads, scale, block_tables, seq_lens,
        block_size, max_seq_len, alibi_slopes, kv_cache_dtype, k_scale, v_scale, tp_rank,
        blocksparse_local_blocks, blocksparse_vert_stride, blocksparse_block_size,
        blocksparse_head_sliding_step)


# vllm/_custom_ops.py:68-97
def paged_attention_v2(
    out: torch.Tensor,
    exp_sum: torch.Tensor,
    max_logits: torch.Tensor,
    tmp_out: torch.Tensor,
    query: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    num_kv_heads: int,
    scale: float,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    block_size: int,
    max_seq_len: int,
    alibi_slopes: Optional[torch.Tensor],
    kv_cache_dtype: str,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    tp_rank: int = 0,
    blocksparse_local_blocks: int = 0,
    blocksparse_vert_stride: int = 0,
    blocksparse_block_size: int = 64,
    blocksparse_head_sliding_step: int = 0,
) -> None:
    torch.ops._C.paged_attention_v2(
        out, exp_sum, max_logits, tmp_out, query, key_cache, value_cache, num_kv_heads, scale,
        block_tables, seq_lens, block_size, max_seq_len, alibi_slopes, kv_cache_dtype, k_scale,
        v_scale, tp_rank, blocksparse_local_blocks, blocksparse_vert_stride,
        blocksparse_block_size, blocksparse_head_sliding_step)


# vllm/_custom_ops.py:100-126
def paged_attention_rocm(
    out: torch.Tensor,
    exp_sum: torch.Tensor,
    max_logits: torch.Tensor,
    tmp_out: torch.Tensor,
    query: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    num_kv_heads: int,
    scale: float,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    query_start_loc: Optional[torch.Tensor],
    block_size: int,
    max_seq_len: int,
    alibi_slopes: Optional[torch.Tensor],
    kv_cache_dtype: str,
    k_scale: torch.Tensor,
    v_scale: torch.Tensor,
    fp8_out_scale: Optional[torch.Tensor] = None,
) -> None:
    torch.ops._rocm_C.paged_attention(out, exp_sum, max_logits, tmp_out, query, key_cache,
                                      value_cache, num_kv_heads, scale, block_tables, seq_lens,
                                      query_start_loc, block_size, max_seq_len, alibi_slopes,
                                      kv_cache_dtype, k_scale, v_scale, fp8_out_scale)


# vllm/_custom_ops.py:1617-1629
def reshape_and_cache(key, value, key_cache, value_cache, slot_mapping, kv_cache_dtype: str,
                      k_scale: torch.Tensor, v_scale: torch.Tensor) -> None:
    torch.ops._C_cache_ops.reshape_and_cache(key, value, key_cache, value_cache, slot_mapping,
                                             kv_cache_dtype, k_scale, v_scale)


# vllm/_custom_ops.py:1632-1645
def reshape_and_cache_flash(key, value, key_cache, value_cache, slot_mapping,
                            kv_cache_dtype: str, k_scale: torch.Tensor,
                            v_scale: torch.Tensor) -> None:
    torch.ops._C_cache_ops.reshape_and_cache_flash(key, value, key_cache, value_cache,
                                                   slot_mapping, kv_cache_dtype, k_scale, v_scale)


# vllm/_custom_ops.py:1648-1658
def concat_and_cache_mla(kv_c: torch.Tensor, k_pe: torch.Tensor, kv_cache: torch.Tensor,
                         slot_mapping: torch.Tensor, kv_cache_dtype: str,
                         scale: torch.Tensor) -> None:
    torch.ops._C_cache_ops.concat_and_cache_mla(kv_c, k_pe, kv_cache, slot_mapping,
                                                kv_cache_dtype, scale)


# vllm/_custom_ops.py:1661-1664
def copy_blocks(key_caches: list[torch.Tensor], value_caches: list[torch.Tensor],
                block_mapping: torch.Tensor) -> None:
    torch.ops._C_cache_ops.copy_blocks(key_caches, value_caches, block_mapping)


# vllm/_custom_ops.py:1672-1674
def swap_blocks(src: torch.Tensor, dst: torch.Tensor, block_mapping: torch.Tensor) -> None:
    torch.ops._C_cache_ops.swap_blocks(src, dst, block_mapping)


# vllm/_custom_ops.py:1677-1681
def convert_fp8(output: torch.Tensor, input: torch.Tensor, scale: float = 1.0,
                kv_dtype: str = "fp8") -> None:
    torch.ops._C_cache_ops.convert_fp8(output, input, scale, kv_dtype)


# vllm/_custom_ops.py:1684-1691.  Beyond the reference: with the keyword `scale` (float32, one element, on the
# cache's device) src_cache is the fp8 (e4m3fn) latent cache and dst, float16 / bfloat16, gets float(byte) * scale --
# the value the fp8 MLA decode reads.  That form goes through the C ABI; the torch op keeps the same-dtype contract.
def gather_cache(src_cache: torch.Tensor, dst: torch.Tensor, block_table: torch.Tensor,
                 cu_seq_lens: torch.Tensor, batch_size: int,
                 seq_starts: Optional[torch.Tensor] = None, *, scale: Optional[torch.Tensor] = None) -> None:
    if scale is None:
        torch.ops._C_cache_ops.gather_cache(src_cache, dst, block_table, cu_seq_lens, batch_size, seq_starts)
        return
    from ._lib import KV_FP8_E4M3, check, lib
    from ._torch_ops import _dev, _dt, _ptr, _stream
    if (src_cache.dtype not in (torch.uint8, torch.float8_e4m3fn) or src_cache.dim() != 3 or dst.dim() != 2
            or src_cache.stride(2) != 1 or dst.stride(1) != 1 or dst.shape[1] != src_cache.shape[2]
            or block_table.dtype != torch.int32 or cu_seq_lens.dtype != torch.int32 or block_table.stride(1) != 1
            or not cu_seq_lens.is_contiguous() or cu_seq_lens.numel() <= batch_size
            or (seq_starts is not None and (seq_starts.dtype != torch.int32 or not seq_starts.is_contiguous()))
            or scale.dtype != torch.float32 or scale.numel() != 1
            or any(t.device != src_cache.device for t in (dst, block_table, cu_seq_lens, scale))):
        raise RuntimeError("gather_cache with scale: src_cache [NUM_BLOCKS, BLOCK_SIZE, ENTRY] uint8 / float8_e4m3fn, dst "
                           "[TOT_TOKENS, ENTRY] float16 / bfloat16, int32 block_table / cu_seq_lens / seq_starts and a "
                           "float32 scale of one element, all on one device, are required")
    with _dev(src_cache):
        check(lib.vllm_amd_gather_cache(
            _ptr(src_cache), _ptr(dst), _ptr(block_table), _ptr(cu_seq_lens), _ptr(seq_starts), batch_size,
            dst.shape[0], src_cache.shape[1], src_cache.shape[2], block_table.stride(0), src_cache.stride(0),
            src_cache.stride(1), dst.stride(0), 2, _dt(dst), KV_FP8_E4M3, _ptr(scale), _stream(src_cache)))


# vllm/_custom_ops.py:1244-1304
def scaled_fp8_quant(
    input: torch.Tensor,
    scale: Optional[torch.Tensor] = None,
    num_token_padding: Optional[int] = None,
    scale_ub: Optional[torch.Tensor] = None,
    use_per_token_if_dynamic: bool = False,
    output: Optional[torch.Tensor] = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Quantize ``input`` [num_tokens, hidden] to fp8 e4m3fn; returns (output, scale).

    scale given -> static per-tensor; else dynamic per-tensor, or per-token when
    ``use_per_token_if_dynamic``.  ``num_token_padding`` pads the first output
    dimension (rows beyond num_tokens are left uninitialised, as in the reference).
    """
    assert input.ndim == 2
    shape: Union[tuple[int, int], torch.Size] = input.shape
    out_dtype = FP8_DTYPE
    if num_token_padding:
        shape = (max(num_token_padding, input.shape[0]), shape[1])
    if output is None:
        output = torch.empty(shape, device=input.device, dtype=out_dtype)
    else:
        assert num_token_padding is None, "padding not supported if output passed in"
        assert output.dtype == out_dtype

    if scale is None:
        if use_per_token_if_dynamic:
            scale = torch.empty((shape[0], 1), device=input.device, dtype=torch.float32)
            torch.ops._C.dynamic_per_token_scaled_fp8_quant(output, input.contiguous(), scale,
                                                            scale_ub)
        else:
            scale = torch.zeros(1, device=input.device, dtype=torch.float32)
            torch.ops._C.dynamic_scaled_fp8_quant(output, input.contiguous(), scale)
    else:
        assert scale.numel() == 1, f"{scale.shape}"
        torch.ops._C.static_scaled_fp8_quant(output, input.contiguous(), scale)
    return output, scale


# csrc/torch_bindings.cpp:623-627 (the reference calls the op directly from fp8_utils.py)
def per_token_group_fp8_quant(input: torch.Tensor, output_q: torch.Tensor, output_s: torch.Tensor,
                              group_size: int, eps: float, fp8_min: float, fp8_max: float,
                              scale_ue8m0: bool) -> None:
    """Quantize every ``group_size`` consecutive elements of a row with a scale of their own;
    writes ``output_q`` (fp8, contiguous) and ``output_s`` (fp32 [tokens, hidden / group_size],
    any strides)."""
    torch.ops._C.per_token_group_fp8_quant(input, output_q, output_s, group_size, eps, fp8_min,
                                           fp8_max, scale_ue8m0)


# vllm/_custom_ops.py:697-742
def cutlass_scaled_mm(a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor,
                      scale_b: torch.Tensor, out_dtype: torch.dtype,
                      bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """output = torch.mm((scale_a * a), (scale_b * b)).to(out_dtype) (+ bias), with
    scale_a per-tensor [1] or per-token [M,1], scale_b per-tensor or per-channel [N,1].
    a: fp8 [M,K] row-major; b: fp8 [K,N] column-major (``weight.t()``).

    Group broadcast (blockwise scaling as in DeepSeek V3): 2-D scales with
    ``scale_a.shape * [1, 128] == a.shape`` and ``scale_b.shape * [128, 128] == b.shape``
    (the last block of N may be ragged), fp32, any strides: every 128-wide slice of the
    reduction is weighted by ``scale_a[m, k // 128] * scale_b[k // 128, n // 128]``.
    K must be a multiple of 128."""
    assert out_dtype is torch.bfloat16 or out_dtype is torch.float16
    assert bias is None or (bias.shape[0] == b.shape[1] and bias.dtype == out_dtype)
    m, n = a.shape[0], b.shape[1]
    out = torch.empty((m, n), dtype=out_dtype, device=a.device)
    torch.ops._C.cutlass_scaled_mm(out, a, b, scale_a, scale_b, bias)
    return out


#: the name BASELINE.json / the north star use for the same operator
scaled_mm = cutlass_scaled_mm


# vllm/_custom_ops.py:1501-1508
def wvSplitKQ(a: torch.Tensor, b: torch.Tensor, out_dtype: torch.dtype, scale_a: torch.Tensor,
              scale_b: torch.Tensor, cu_count: int) -> torch.Tensor:
    out = torch.empty((b.shape[0], a.shape[0]), dtype=out_dtype, device=b.device)
    torch.ops._rocm_C.wvSplitKQ(a, b, out, scale_a, scale_b, cu_count)
    return out


# ---- fused neighbours of the GEMM (vllm/_custom_ops.py:283-293, 368-384) -----------------
def scaled_rms_norm(out: torch.Tensor, input: torch.Tensor, weight: torch.Tensor,
                    scale: torch.Tensor, epsilon: float) -> None:
    torch.ops._C.rms_norm_static_fp8_quant(out, input, weight, scale, epsilon)


def scaled_fused_add_rms_norm(out: torch.Tensor, input: torch.Tensor, residual: torch.Tensor,
                              weight: torch.Tensor, scale: torch.Tensor, epsilon: float) -> None:
    torch.ops._C.fused_add_rms_norm_static_fp8_quant(out, input, residual, weight, scale, epsilon)


def rms_norm_dynamic_per_token_quant(
        input: torch.Tensor, weight: torch.Tensor, epsilon: float, quant_dtype: torch.dtype,
        scale_ub: Optional[torch.Tensor] = None,
        residual: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    output = torch.empty_like(input, dtype=quant_dtype)
    scales = torch.empty((input.numel() // input.shape[-1], 1), device=input.device,
                         dtype=torch.float32)
    torch.ops._C.rms_norm_dynamic_per_token_quant(output, input, weight, scales, epsilon,
                                                  scale_ub, residual)
    return output, scales


def silu_and_mul_quant(out: torch.Tensor, input: torch.Tensor, scale: torch.Tensor) -> None:
    torch.ops._C.silu_and_mul_quant(out, input, scale)


# ---- fused MoE (vllm/_custom_ops.py:1512-1522) ---------------------------------------------
def moe_sum(input: torch.Tensor, output: torch.Tensor):
    torch.ops._moe_C.moe_sum(input, output)


def moe_align_block_size(topk_ids: torch.Tensor, num_experts: int, block_size: int,
                         sorted_token_ids: torch.Tensor, experts_ids: torch.Tensor,
                         num_tokens_post_pad: torch.Tensor) -> None:
    torch.ops._moe_C.moe_align_block_size(topk_ids, num_experts, block_size, sorted_token_ids,
                                          experts_ids, num_tokens_post_pad)


def topk_softmax(topk_weights: torch.Tensor, topk_ids: torch.Tensor, token_expert_indices: torch.Tensor,
                 gating_output: torch.Tensor) -> None:
    torch.ops._moe_C.topk_softmax(topk_weights, topk_ids, token_expert_indices, gating_output)


# no reference counterparts: there fused_topk divides by the sum in torch and grouped_topk is torch code
def fused_topk(topk_weights: torch.Tensor, topk_ids: torch.Tensor, token_expert_indices: torch.Tensor,
               gating_output: torch.Tensor, renormalize: bool) -> None:
    """topk_softmax with the optional division by the weights' sum inside the same launch."""
    torch.ops._moe_C.fused_topk(topk_weights, topk_ids, token_expert_indices, gating_output, renormalize)


def grouped_topk(topk_weights: torch.Tensor, topk_ids: torch.Tensor, gating_output: torch.Tensor,
                 e_score_correction_bias: Optional[torch.Tensor], num_expert_group: int, topk_group: int,
                 renormalize: bool, scoring_func: str) -> None:
    """Group-limited routing in one launch: fp32 ``topk_weights`` and int32 ``topk_ids`` [tokens, topk]."""
    torch.ops._moe_C.grouped_topk(topk_weights, topk_ids, gating_output, e_score_correction_bias,
                                  num_expert_group, topk_group, renormalize, scoring_func)


# no reference counterpart: the grouped GEMM there is Triton (fused_moe.py:268-475)
def moe_block_fp8_gemm(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor, a_scales: torch.Tensor,
                       b_scales: torch.Tensor, topk_weights: Optional[torch.Tensor],
                       sorted_token_ids: torch.Tensor, expert_ids: torch.Tensor,
                       num_tokens_post_padded: torch.Tensor, mul_routed_weight: bool, top_k: int,
                       block_size_m: int) -> None:
    """c[t] = (topk_weights[t] *) a[t // top_k] @ b[expert of t].T with 1 x 128 / 128 x 128 block
    scales, for the flat (token, k) slots t that ``sorted_token_ids`` lists; ``block_size_m`` 16 or 64 (the
    weight-streaming kernel) or 128 (the tile kernel)."""
    torch.ops._C.moe_block_fp8_gemm(c, a, b, a_scales, b_scales, topk_weights, sorted_token_ids,
                                    expert_ids, num_tokens_post_padded, mul_routed_weight, top_k,
                                    block_size_m)


def silu_and_mul_group_quant(output_q: torch.Tensor, output_s: torch.Tensor,
                             input: torch.Tensor) -> None:
    """silu_and_mul of ``input`` [rows, 2 d], quantised in 128-wide groups: fp8 ``output_q``
    [rows, d] and fp32 ``output_s`` [rows, d / 128] (any strides)."""
    torch.ops._C.silu_and_mul_group_quant(output_q, output_s, input)


# ---- MXFP4 (w4a4) experts: no reference counterparts (its quantiser raises on gfx95 and its GEMM
# ---- runs on weights dequantised to bf16, quark_moe.py:284-291) ------------------------------------
def mxfp4_quant(output_q: torch.Tensor, output_s: torch.Tensor, input: torch.Tensor) -> None:
    """``input`` [rows, K] bf16 / f16 (K contiguous, any row stride) as MXFP4: uint8 e2m1 codes
    ``output_q`` [rows, K / 2] (element 2 j in the low nibble of byte j) and uint8 e8m0 scales
    ``output_s`` [rows, K / 32]; round-to-nearest-even, K % 32 == 0."""
    torch.ops._C.mxfp4_quant(output_q, output_s, input)


def silu_and_mul_mxfp4_quant(output_q: torch.Tensor, output_s: torch.Tensor, input: torch.Tensor) -> None:
    """silu_and_mul of ``input`` [rows, 2 d] quantised as by ``mxfp4_quant``: ``output_q`` [rows, d / 2],
    ``output_s`` [rows, d / 32]."""
    torch.ops._C.silu_and_mul_mxfp4_quant(output_q, output_s, input)


def moe_mxfp4_gemm(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor, a_scales: torch.Tensor,
                   b_scales: torch.Tensor, topk_weights: Optional[torch.Tensor],
                   sorted_token_ids: torch.Tensor, expert_ids: torch.Tensor,
                   num_tokens_post_padded: torch.Tensor, mul_routed_weight: bool, top_k: int,
                   block_size_m: int) -> None:
    """``moe_block_fp8_gemm`` over MXFP4 operands: a [rows, K / 2] and b [E, N, K / 2] uint8 codes, a_scales
    [rows, K / 32] and b_scales [E, N, K / 32] uint8 e8m0; K % 128 == 0."""
    torch.ops._C.moe_mxfp4_gemm(c, a, b, a_scales, b_scales, topk_weights, sorted_token_ids, expert_ids,
                                num_tokens_post_padded, mul_routed_weight, top_k, block_size_m)
