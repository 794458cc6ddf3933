"""merge_attn_states: mirror of vllm/attention/ops/triton_merge_attn_states.py:12-36 (same arguments) over
`vllm_amd_merge_attn_states` (HIP, csrc/mla_prefill.hip) instead of the Triton kernel.

One stated difference: a row whose prefix and suffix lse are both -inf gets output 0 and lse -inf (the reference
computes NaN, which the next merge inherits).  float16 / bfloat16 outputs with a head size that is a multiple of 8 up
to 512; anything else raises: there is no Triton or eager path behind this module."""
from __future__ import annotations

from typing import Optional

import torch

from ..._lib import check, lib
from ..._torch_ops import _dev, _dt, _ptr, _stream


@torch.inference_mode()
def merge_attn_states(output: torch.Tensor, prefix_output: torch.Tensor, prefix_lse: torch.Tensor,
                      suffix_output: torch.Tensor, suffix_lse: torch.Tensor,
                      output_lse: Optional[torch.Tensor] = None) -> None:
    T, H, D = output.shape
    lses = [prefix_lse, suffix_lse] + ([] if output_lse is None else [output_lse])
    for o in (output, prefix_output, suffix_output):
        if tuple(o.shape) != (T, H, D) or o.dtype != output.dtype or o.stride(2) != 1 or o.device != output.device:
            raise RuntimeError(f"merge_attn_states: outputs must be [{T}, {H}, {D}] {output.dtype} with a contiguous "
                               f"last dimension; got {tuple(o.shape)} {o.dtype} strides {o.stride()}")
    for l in lses:
        if tuple(l.shape) != (H, T) or l.dtype != torch.float32 or not l.is_contiguous() or l.device != output.device:
            raise RuntimeError(f"merge_attn_states: every lse must be a contiguous float32 [{H}, {T}]; got "
                               f"{tuple(l.shape)} {l.dtype}")
    with _dev(output):
        check(lib.vllm_amd_merge_attn_states(
            _ptr(output), _ptr(output_lse), _ptr(prefix_output), _ptr(prefix_lse), _ptr(suffix_output),
            _ptr(suffix_lse), T, H, D, output.stride(0), output.stride(1), prefix_output.stride(0),
            prefix_output.stride(1), suffix_output.stride(0), suffix_output.stride(1), T, _dt(output),
            _stream(output)))
