"""moe_align_block_size with the reference's signature and buffer sizes
(vllm/model_executor/layers/fused_moe/moe_align_block_size.py:12-87) over the HIP kernel
(csrc/moe_block_fp8.hip)."""
from __future__ import annotations

from typing import Optional

import torch

from .... import _custom_ops as ops


def moe_align_block_size(
    topk_ids: torch.Tensor,
    block_size: int,
    num_experts: int,
    expert_map: Optional[torch.Tensor] = None,
    pad_sorted_ids: bool = False,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Sorts the flat (token, k) slots of ``topk_ids`` by expert and pads every expert's run to a
    multiple of ``block_size`` with the sentinel ``topk_ids.numel()``.

    Returns (sorted_token_ids, expert_ids, num_tokens_post_padded): the slot list, the expert of
    every ``block_size`` entries of it, and the padded total (a device scalar; entries past it are
    not meaningful).  With ``expert_map`` (global -> local expert index, -1 = on another rank)
    ``expert_ids`` is mapped to local indices, so that the grouped GEMM writes zeros for the blocks of
    absent experts; ``num_experts`` is then the global count.  The order inside an expert's run is
    unspecified.  Ids outside [0, num_experts) are left out."""
    max_num_tokens_padded = topk_ids.numel() + num_experts * (block_size - 1)
    if pad_sorted_ids:
        max_num_tokens_padded = -(-max_num_tokens_padded // block_size) * block_size
    sorted_ids = torch.empty((max_num_tokens_padded, ), dtype=torch.int32, device=topk_ids.device)
    if pad_sorted_ids:   # the kernel writes the unrounded length; the rounding tail is padding too
        sorted_ids.fill_(topk_ids.numel())
    max_num_m_blocks = -(-max_num_tokens_padded // block_size)
    expert_ids = torch.empty((max_num_m_blocks, ), dtype=torch.int32, device=topk_ids.device)
    num_tokens_post_pad = torch.empty((1), dtype=torch.int32, device=topk_ids.device)
    if topk_ids.dtype != torch.int32:
        topk_ids = topk_ids.to(torch.int32)
    ops.moe_align_block_size(topk_ids.contiguous().view(-1), num_experts, block_size, sorted_ids,
                             expert_ids, num_tokens_post_pad)
    if expert_map is not None:
        expert_ids = expert_map[expert_ids.long()].to(torch.int32)
    return sorted_ids, expert_ids, num_tokens_post_pad
