"""Block-scaled fp8 linear path (DeepSeek-V3 style checkpoints), host side, with the names and
arguments of the reference's ``quantization/utils/fp8_utils.py``:

  per_token_group_quant_fp8    1 x group_size activation scales
  w8a8_block_fp8_matmul        128 x 128 weight scales, 1 x 128 activation scales
  apply_w8a8_block_fp8_linear  quantise, then multiply

Both steps are HIP kernels of libvllm_amd.so (csrc/group_quant.hip, csrc/scaled_mm_block.hip);
there is no eager or Triton fallback."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _custom_ops as ops


def per_token_group_quant_fp8(x: torch.Tensor, group_size: int, eps: float = 1e-10,
                              dtype: Optional[torch.dtype] = None,
                              column_major_scales: bool = False,
                              out_q: Optional[torch.Tensor] = None,
                              use_ue8m0: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """Returns (x_q, x_s): fp8 codes of the shape of ``x`` and fp32 scales
    ``x.shape[:-1] + (x.shape[-1] // group_size,)``; with ``column_major_scales`` the scales of
    one group index are contiguous over the tokens (the same logical shape, other strides)."""
    dtype = ops.FP8_DTYPE if dtype is None else dtype
    assert dtype == ops.FP8_DTYPE, "gfx950 quantises to float8_e4m3fn only"
    assert x.shape[-1] % group_size == 0, (
        f"the last dimension of `x` {x.shape[-1]} must be divisible by `group_size` {group_size}")
    assert x.stride(-1) == 1, "`x` groups must be contiguous"
    x = x.contiguous()
    finfo = torch.finfo(dtype)
    if out_q is None:
        out_q = torch.empty(x.shape, device=x.device, dtype=dtype)
    else:
        assert out_q.shape == x.shape and out_q.dtype == dtype and out_q.is_contiguous()
    groups = x.shape[-1] // group_size
    tokens = x.numel() // x.shape[-1] if x.shape[-1] else 0
    if column_major_scales:
        x_s = torch.empty((groups, tokens), device=x.device, dtype=torch.float32).t()
    else:
        x_s = torch.empty((tokens, groups), device=x.device, dtype=torch.float32)
    ops.per_token_group_fp8_quant(x, out_q, x_s, group_size, eps, finfo.min, finfo.max, use_ue8m0)
    if x.dim() != 2:   # scales of an n-d input: a view of the row-major buffer only
        assert not column_major_scales, "column-major scales need a 2-D input"
        x_s = x_s.view(*x.shape[:-1], groups)
    return out_q, x_s


def w8a8_block_fp8_matmul(A: torch.Tensor, B: torch.Tensor, As: torch.Tensor, Bs: torch.Tensor,
                          block_size: list[int],
                          output_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """A [..., K] fp8 with As [..., K / 128]; B [N, K] fp8 with Bs [ceil(N / 128), K / 128];
    returns [..., N].  The weight and its scales are passed on as transposed views."""
    assert len(block_size) == 2 and tuple(block_size) == (128, 128), "block size is 128 x 128"
    assert A.shape[-1] == B.shape[-1] and B.dim() == 2 and Bs.dim() == 2
    assert A.shape[:-1] == As.shape[:-1]
    K, N = A.shape[-1], B.shape[0]
    a2 = A.reshape(-1, K)
    as2 = As.reshape(-1, As.shape[-1]) if As.dim() != 2 else As
    out = ops.cutlass_scaled_mm(a2, B.t(), as2, Bs.t(), output_dtype)
    return out.view(*A.shape[:-1], N)


def apply_w8a8_block_fp8_linear(input: torch.Tensor, weight: torch.Tensor, block_size: list[int],
                                weight_scale: torch.Tensor,
                                input_scale: Optional[torch.Tensor] = None,
                                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dynamic 1 x 128 activation quantisation, then the block-scaled GEMM against ``weight``
    [N, K] fp8 with ``weight_scale`` [ceil(N / 128), K / 128]; output in ``input.dtype``."""
    assert input_scale is None, "activation scales are dynamic"
    assert tuple(block_size) == (128, 128), "block size is 128 x 128"
    input_2d = input.reshape(-1, input.shape[-1])
    q, s = per_token_group_quant_fp8(input_2d, block_size[1])
    out = ops.cutlass_scaled_mm(q, weight.t(), s, weight_scale.t(), input.dtype, bias)
    return out.view(*input.shape[:-1], weight.shape[0])
