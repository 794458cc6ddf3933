"""Fused MoE over block-scaled fp8 weights, routing included, with the names and arguments of the
reference's ``vllm/model_executor/layers/fused_moe/fused_moe.py`` (fused_topk :882-915, grouped_topk
:920-975, fused_experts :1253-1346, fused_experts_impl :1349-1563, invoke_fused_moe_kernel :478-640,
fused_moe :1566-1689).

Routing: ``fused_topk`` (softmax, top-k, optional renormalisation) and ``grouped_topk`` (softmax or
sigmoid scores, optional correction bias, group-limited top-k) are ONE launch each of the routing
kernel of libvllm_amd.so (csrc/moe_routing.hip), which reads the logits in their own dtype and scores
them in fp32: no torch arithmetic, no host synchronisation.  Ties go to the lower expert / group
index and the ids come in descending order of the selecting score (the reference asks torch.topk
for ``sorted=False``).  ``fused_moe`` is routing followed by ``fused_experts``.

Supported: ``use_fp8_w8a8=True`` with ``block_shape == [128, 128]``, or ``use_mxfp4_w4a4=True`` (OCP MXFP4
weights AND activations, e8m0 scales per 32 values, on the fp4 scaled MFMA; csrc/moe_mxfp4.hip); silu with
mul, dynamic activation scales, bf16 / f16 hidden states.  One layer is five launches and a sum, all HIP
kernels of libvllm_amd.so, plus the zero fill of the second GEMM's output, with no host
synchronisation (graph-capturable):

  per_token_group_fp8_quant -> moe_align_block_size -> moe_block_fp8_gemm (w1)
  -> silu_and_mul_group_quant -> moe_block_fp8_gemm (w2, routed weights) -> moe_sum

  mxfp4_quant -> moe_align_block_size -> moe_mxfp4_gemm (w1)
  -> silu_and_mul_mxfp4_quant -> moe_mxfp4_gemm (w2, routed weights) -> moe_sum

Anything else raises NotImplementedError naming the argument: there is no eager or Triton
fallback."""
from __future__ import annotations

from typing import Any, Callable, Optional

import torch

from .... import _custom_ops as ops
from ....quantization.fp8_utils import per_token_group_quant_fp8
from .moe_align_block_size import moe_align_block_size

#: tokens per pass (VLLM_FUSED_MOE_CHUNK_SIZE's default in the reference, fused_moe.py:1402)
CHUNK_SIZE = 32768
#: average slots per expert from which the fp8 grouped GEMM runs its 128-row tile kernel
TILE_MIN_SLOTS = 64


def _block_size_m(num_tokens: int, top_k: int, num_experts: int) -> int:
    # 16 sorted rows per workgroup while an expert sees 16 slots or fewer on average (padding to 64
    # would then stream every touched expert's weights for mostly empty MFMA tiles), 64 above.
    # Measured at E 256, top-k 8 (tools/bench_moe.py, profiles/moe_block_fp8.txt): 16 is 1.5 - 2.2 x
    # faster than 64 from 1 to 256 tokens, 64 is 1.06 - 1.32 x faster at 4096 tokens; the crossover
    # itself (between 256 and 4096 tokens) is not measured, the rule puts it at 512.
    # 128 (the grouped tile kernel: LDS-staged 128 x 128 tiles, the weights read once per 128 rows) from
    # TILE_MIN_SLOTS slots per expert on.  Measured at E 256, top-k 8 (tools/bench_moe.py --tile,
    # profiles/moe_block_fp8_tile.txt), the whole fused_experts call with 128 against this rule without it:
    # 0.86 - 0.89 x at 256 tokens, 1.16 - 1.30 x at 512, 1.9 - 2.1 x at 1024, 2.6 - 3.3 x at 2048, 2.9 - 3.8 x
    # at 4096, 3.4 - 4.6 x at 16384.  128 wins from 512 tokens = 16 slots per expert on; the threshold stays
    # at 64 (2048 tokens there), the lowest value this rule allows itself: every batch below it keeps the
    # kernel, and the bits, it had.
    slots = num_tokens * top_k
    if slots >= TILE_MIN_SLOTS * num_experts:
        return 128
    return 16 if slots <= 16 * num_experts else 64


def _gating_2d(name: str, hidden_states: torch.Tensor, gating_output: torch.Tensor) -> None:
    assert hidden_states.size(0) == gating_output.size(0), "Number of tokens mismatch"
    if gating_output.dim() != 2 or (gating_output.size(1) > 1 and gating_output.stride(1) != 1):
        raise NotImplementedError(f"{name}: gating_output must be [num_tokens, num_experts] with contiguous experts")
    if gating_output.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{name}: gating_output dtype {gating_output.dtype} is not implemented")


def fused_topk(hidden_states: torch.Tensor, gating_output: torch.Tensor, topk: int, renormalize: bool,
               indices_type: Optional[torch.dtype] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The ``topk`` largest softmax probabilities of every row of ``gating_output`` (fp32, bf16 or f16; no fp32
    copy is made), divided by their sum with ``renormalize``: fp32 weights, ids of ``indices_type`` (int32 by
    default, or int64) and token_expert_indices[t, k] = k * num_tokens + t, all [num_tokens, topk]."""
    _gating_2d("fused_topk", hidden_states, gating_output)
    if indices_type not in (None, torch.int32, torch.int64):
        raise NotImplementedError(f"fused_topk: indices_type {indices_type} is not implemented (int32 or int64)")
    M, dev = hidden_states.size(0), hidden_states.device
    topk_weights = torch.empty((M, topk), dtype=torch.float32, device=dev)
    topk_ids = torch.empty((M, topk), dtype=torch.int32 if indices_type is None else indices_type, device=dev)
    token_expert_indices = torch.empty((M, topk), dtype=torch.int32, device=dev)
    ops.fused_topk(topk_weights, topk_ids, token_expert_indices, gating_output, renormalize)
    return topk_weights, topk_ids, token_expert_indices


def grouped_topk(hidden_states: torch.Tensor, gating_output: torch.Tensor, topk: int, renormalize: bool,
                 num_expert_group: int = 0, topk_group: int = 0, scoring_func: str = "softmax",
                 e_score_correction_bias: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """DeepSeek-V2 / V3 routing: scores = softmax or sigmoid of the logits; the experts are selected by
    scores + ``e_score_correction_bias`` (fp32, one entry per expert) among the ``topk_group`` best of
    ``num_expert_group`` groups, a group scoring the sum of its two best with a bias and its best without;
    the weights are the unbiased scores of the selected experts, divided by their sum with ``renormalize``.
    Returns fp32 weights and int32 ids, [num_tokens, topk]."""
    _gating_2d("grouped_topk", hidden_states, gating_output)
    if scoring_func not in ("softmax", "sigmoid"):
        raise ValueError(f"Unsupported scoring function: {scoring_func}")
    if e_score_correction_bias is not None and e_score_correction_bias.dtype != torch.float32:
        raise NotImplementedError(
            f"grouped_topk: e_score_correction_bias dtype {e_score_correction_bias.dtype} is not implemented (float32)")
    M, dev = hidden_states.size(0), hidden_states.device
    topk_weights = torch.empty((M, topk), dtype=torch.float32, device=dev)
    topk_ids = torch.empty((M, topk), dtype=torch.int32, device=dev)
    ops.grouped_topk(topk_weights, topk_ids, gating_output, e_score_correction_bias, num_expert_group, topk_group,
                     renormalize, scoring_func)
    return topk_weights, topk_ids


def invoke_fused_moe_kernel(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor,
                            A_scale: Optional[torch.Tensor], B_scale: Optional[torch.Tensor],
                            B_zp: Optional[torch.Tensor], topk_weights: Optional[torch.Tensor],
                            sorted_token_ids: torch.Tensor, expert_ids: torch.Tensor,
                            num_tokens_post_padded: torch.Tensor, mul_routed_weight: bool, top_k: int,
                            config: dict[str, Any], compute_type: Any = None,
                            use_fp8_w8a8: bool = False, use_int8_w8a8: bool = False,
                            use_int8_w8a16: bool = False, use_int4_w4a16: bool = False,
                            per_channel_quant: bool = False,
                            block_shape: Optional[list[int]] = None) -> None:
    """The grouped GEMM: C[t] = (topk_weights[t] *) A[t // top_k] @ B[expert of slot t].T for the
    slots ``sorted_token_ids`` lists; ``config["BLOCK_SIZE_M"]`` is the block size the ids were
    aligned to (16 or 64: the weight-streaming kernel; 128: the tile kernel).  ``compute_type`` is implied by
    C's dtype."""
    for name, flag in (("use_int8_w8a8", use_int8_w8a8), ("use_int8_w8a16", use_int8_w8a16),
                       ("use_int4_w4a16", use_int4_w4a16), ("per_channel_quant", per_channel_quant)):
        if flag:
            raise NotImplementedError(f"invoke_fused_moe_kernel: {name} is not implemented on gfx950")
    if not use_fp8_w8a8:
        raise NotImplementedError("invoke_fused_moe_kernel: only use_fp8_w8a8=True is implemented")
    if block_shape is None or list(block_shape) != [128, 128]:
        raise NotImplementedError("invoke_fused_moe_kernel: block_shape must be [128, 128]")
    if B_zp is not None:
        raise NotImplementedError("invoke_fused_moe_kernel: B_zp is not implemented")
    assert topk_weights is not None or not mul_routed_weight
    assert topk_weights is None or topk_weights.stride(-1) == 1
    assert sorted_token_ids.stride(0) == 1
    assert A_scale is not None and B_scale is not None
    assert -(-B.size(-2) // 128) == B_scale.size(-2) and -(-B.size(-1) // 128) == B_scale.size(-1)
    tw = None
    if topk_weights is not None:
        tw = topk_weights.reshape(-1)
        if tw.dtype != torch.float32:
            tw = tw.float()
    ops.moe_block_fp8_gemm(C, A, B, A_scale, B_scale, tw, sorted_token_ids, expert_ids,
                           num_tokens_post_padded, mul_routed_weight, top_k, config["BLOCK_SIZE_M"])


def fused_experts(hidden_states: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
                  topk_weights: torch.Tensor, topk_ids: torch.Tensor, inplace: bool = False,
                  activation: str = "silu", is_act_and_mul: bool = True,
                  apply_router_weight_on_input: bool = False, use_fp8_w8a8: bool = False,
                  use_int8_w8a8: bool = False, use_int8_w8a16: bool = False,
                  use_int4_w4a16: bool = False, use_mxfp4_w4a4: bool = False,
                  per_channel_quant: bool = False, global_num_experts: int = -1,
                  expert_map: Optional[torch.Tensor] = None,
                  w1_scale: Optional[torch.Tensor] = None, w2_scale: Optional[torch.Tensor] = None,
                  w1_zp: Optional[torch.Tensor] = None, w2_zp: Optional[torch.Tensor] = None,
                  a1_scale: Optional[torch.Tensor] = None, a2_scale: Optional[torch.Tensor] = None,
                  block_shape: Optional[list[int]] = None, allow_deep_gemm: bool = False,
                  allow_cutlass_block_scaled_grouped_gemm: bool = False) -> torch.Tensor:
    """hidden_states [M, K]; w1 [E, 2 I, K] and w2 [E, K, I] fp8 e4m3 with w1_scale
    [E, ceil(2 I / 128), K / 128] and w2_scale [E, ceil(K / 128), I / 128]; topk_weights / topk_ids
    [M, top_k].  With ``use_mxfp4_w4a4``: w1 [E, 2 I, K / 2] and w2 [E, K, I / 2] uint8 (two e2m1 codes per
    byte, the even element in the low nibble) with w1_scale [E, 2 I, K / 32] and w2_scale [E, K, I / 32]
    uint8 e8m0, K and I multiples of 128, no ``block_shape``.
    Returns sum_k topk_weights[m, k] * expert_{topk_ids[m, k]}(hidden_states[m]), written
    into ``hidden_states`` with ``inplace``.  A slot whose id is outside [0, global_num_experts) adds
    nothing; with ``expert_map`` (global -> local index, -1 = absent) w1 / w2 hold the local experts."""
    for name, flag in (("use_int8_w8a8", use_int8_w8a8), ("use_int8_w8a16", use_int8_w8a16),
                       ("use_int4_w4a16", use_int4_w4a16), ("per_channel_quant", per_channel_quant)):
        if flag:
            raise NotImplementedError(f"fused_experts: {name} is not implemented on gfx950")
    if use_mxfp4_w4a4:
        if use_fp8_w8a8:
            raise NotImplementedError("fused_experts: use_fp8_w8a8 cannot be combined with use_mxfp4_w4a4")
        if block_shape is not None:
            raise NotImplementedError("fused_experts: block_shape is not implemented with use_mxfp4_w4a4 "
                                      "(MXFP4 scales are one per 32 values)")
    elif not use_fp8_w8a8:
        raise NotImplementedError("fused_experts: only use_fp8_w8a8=True and use_mxfp4_w4a4=True are implemented")
    elif block_shape is None or list(block_shape) != [128, 128]:
        raise NotImplementedError("fused_experts: block_shape must be [128, 128]")
    if activation != "silu" or not is_act_and_mul:
        raise NotImplementedError(
            f"fused_experts: activation={activation!r}, is_act_and_mul={is_act_and_mul}: only silu "
            "with mul is implemented")
    for name, val in (("a1_scale", a1_scale), ("a2_scale", a2_scale), ("w1_zp", w1_zp), ("w2_zp", w2_zp)):
        if val is not None:
            raise NotImplementedError(f"fused_experts: {name} is not implemented (activation scales are dynamic)")
    if hidden_states.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"fused_experts: hidden_states dtype {hidden_states.dtype} is not implemented")
    assert w1_scale is not None and w2_scale is not None, "block-scaled weights need their scales"
    pack = 2 if use_mxfp4_w4a4 else 1                     # values per weight byte
    if use_mxfp4_w4a4 and (hidden_states.size(1) % 128 or w2.size(2) * 2 % 128):
        raise NotImplementedError(f"fused_experts: use_mxfp4_w4a4 needs K = {hidden_states.size(1)} and I = "
                                  f"{w2.size(2) * 2} to be multiples of 128")
    assert hidden_states.size(1) == w1.size(2) * pack, \
        f"Hidden size mismatch {hidden_states.size(1)} != {w1.size(2) * pack}"
    assert topk_weights.size() == topk_ids.size(), "topk shape mismatch"
    assert hidden_states.is_contiguous(), "Hidden_states must be contiguous"
    assert w1.stride(-1) == 1 and w2.stride(-1) == 1, "Stride of last dimension must be 1"

    num_tokens = hidden_states.size(0)
    E, N, _ = w1.size()
    K = w2.size(1)
    assert w2.size(2) * pack * 2 == N, "w1 holds gate and up: [E, 2 I, K] against w2 [E, K, I]"
    if global_num_experts == -1:
        global_num_experts = E
    top_k = topk_ids.size(1)
    if apply_router_weight_on_input:
        assert top_k == 1, "apply_router_weight_on_input is only implemented for topk=1"
    out = hidden_states if inplace else torch.empty_like(hidden_states)
    if topk_ids.dtype != torch.int32:
        topk_ids = topk_ids.to(torch.int32)
    if topk_weights.dtype != torch.float32:
        topk_weights = topk_weights.float()
    dev, dtype = hidden_states.device, hidden_states.dtype

    for begin in range(0, num_tokens, CHUNK_SIZE):
        end = min(begin + CHUNK_SIZE, num_tokens)
        m = end - begin
        ids, weights = topk_ids[begin:end], topk_weights[begin:end].contiguous()
        config = {"BLOCK_SIZE_M": _block_size_m(m, top_k, global_num_experts)}
        cache1 = torch.empty((m * top_k, N), device=dev, dtype=dtype)
        # zeros: a slot whose id is outside [0, global_num_experts) is in no expert's run, so neither GEMM
        # writes its row, and moe_sum must add nothing for it (cache1 / q2 rows of such slots are never read)
        cache3 = torch.zeros((m, top_k, K), device=dev, dtype=dtype)
        bm = config["BLOCK_SIZE_M"]
        if use_mxfp4_w4a4:
            bm = min(bm, 64)                                  # the MXFP4 GEMM has no tile form
            q1 = torch.empty((m, K // 2), device=dev, dtype=torch.uint8)
            s1 = torch.empty((m, K // 32), device=dev, dtype=torch.uint8)
            q2 = torch.empty((m * top_k, N // 4), device=dev, dtype=torch.uint8)
            s2 = torch.empty((m * top_k, N // 64), device=dev, dtype=torch.uint8)
            ops.mxfp4_quant(q1, s1, hidden_states[begin:end])
            sorted_ids, expert_ids, num_post = moe_align_block_size(ids, bm, global_num_experts, expert_map)
            ops.moe_mxfp4_gemm(cache1, q1, w1, s1, w1_scale, weights.view(-1), sorted_ids, expert_ids, num_post,
                               apply_router_weight_on_input, top_k, bm)
            ops.silu_and_mul_mxfp4_quant(q2, s2, cache1)
            ops.moe_mxfp4_gemm(cache3, q2, w2, s2, w2_scale, weights.view(-1), sorted_ids, expert_ids, num_post,
                               not apply_router_weight_on_input, 1, bm)
        else:
            q2 = torch.empty((m * top_k, N // 2), device=dev, dtype=ops.FP8_DTYPE)
            s2 = torch.empty((m * top_k, N // 256), device=dev, dtype=torch.float32)
            q1, s1 = per_token_group_quant_fp8(hidden_states[begin:end], 128)
            sorted_ids, expert_ids, num_post = moe_align_block_size(ids, bm, global_num_experts, expert_map)
            invoke_fused_moe_kernel(q1, w1, cache1, s1, w1_scale, None, weights, sorted_ids, expert_ids, num_post,
                                    apply_router_weight_on_input, top_k, config, use_fp8_w8a8=True,
                                    block_shape=block_shape)
            ops.silu_and_mul_group_quant(q2, s2, cache1)
            invoke_fused_moe_kernel(q2, w2, cache3, s2, w2_scale, None, weights, sorted_ids, expert_ids, num_post,
                                    not apply_router_weight_on_input, 1, config, use_fp8_w8a8=True,
                                    block_shape=block_shape)
        ops.moe_sum(cache3, out[begin:end])
    return out


def fused_moe(hidden_states: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, gating_output: torch.Tensor,
              topk: int, renormalize: bool, inplace: bool = False, activation: str = "silu",
              is_act_and_mul: bool = True, use_grouped_topk: bool = False,
              num_expert_group: Optional[int] = None, topk_group: Optional[int] = None,
              custom_routing_function: Optional[Callable] = None, use_fp8_w8a8: bool = False,
              use_int8_w8a8: bool = False, use_int8_w8a16: bool = False, use_int4_w4a16: bool = False,
              use_mxfp4_w4a4: bool = False, per_channel_quant: bool = False, global_num_experts: int = -1,
              expert_map: Optional[torch.Tensor] = None, w1_scale: Optional[torch.Tensor] = None,
              w2_scale: Optional[torch.Tensor] = None, w1_zp: Optional[torch.Tensor] = None,
              w2_zp: Optional[torch.Tensor] = None, a1_scale: Optional[torch.Tensor] = None,
              a2_scale: Optional[torch.Tensor] = None, block_shape: Optional[list[int]] = None) -> torch.Tensor:
    """A whole MoE layer: routing of ``gating_output`` [M, E] (``grouped_topk`` with ``use_grouped_topk``, else
    ``custom_routing_function(hidden_states, gating_output, topk, renormalize)`` when given, else ``fused_topk``),
    then ``fused_experts`` with the remaining arguments."""
    if use_grouped_topk:
        assert num_expert_group is not None and topk_group is not None
        topk_weights, topk_ids = grouped_topk(hidden_states, gating_output, topk, renormalize, num_expert_group,
                                              topk_group)
    elif custom_routing_function is None:
        topk_weights, topk_ids, _ = fused_topk(hidden_states, gating_output, topk, renormalize)
    else:
        topk_weights, topk_ids = custom_routing_function(hidden_states, gating_output, topk, renormalize)
    return fused_experts(hidden_states, w1, w2, topk_weights, topk_ids, inplace=inplace, activation=activation,
                         is_act_and_mul=is_act_and_mul, use_fp8_w8a8=use_fp8_w8a8, use_int8_w8a8=use_int8_w8a8,
                         use_int8_w8a16=use_int8_w8a16, use_int4_w4a16=use_int4_w4a16,
                         use_mxfp4_w4a4=use_mxfp4_w4a4, per_channel_quant=per_channel_quant,
                         global_num_experts=global_num_experts, expert_map=expert_map, w1_scale=w1_scale,
                         w2_scale=w2_scale, w1_zp=w1_zp, w2_zp=w2_zp, a1_scale=a1_scale, a2_scale=a2_scale,
                         block_shape=block_shape)
