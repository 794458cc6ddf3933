"""MLA decode attention over the latent KV cache: mirror of
vllm/attention/ops/triton_decode_attention.py:629-674 (`decode_attention_fwd`, same arguments) over
`vllm_amd_mla_decode` / `vllm_amd_mla_decode_fp8` (HIP, csrc/mla_decode.hip) instead of the Triton kernels.

Only the form the MLA backend calls (vllm/v1/attention/backends/mla/triton_mla.py:124-171) is served:
one kv head, `k_buffer[..., 576]`, `v_buffer` the 512-wide view of the same storage, no logit cap.
Beyond the reference: with the keyword `k_scale` (float32, one element, on q's device) `k_buffer` is the
fp8 (e4m3fn) cache `concat_and_cache_mla` writes for kv_cache_dtype "fp8", row = float(byte) * k_scale.
Anything else raises NotImplementedError: there is no Triton or eager path behind this module."""
from __future__ import annotations

import torch

from ... import _lib
from ..._lib import check, lib
from ..._torch_ops import _dev, _ptr, _stream

_DT = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
_FP8 = (torch.uint8, torch.float8_e4m3fn)
MLA_FORM = ("the MLA form: q [B, H, 576], k_buffer [num_blocks, page_size, 1, 576] (one kv head; bfloat16 / float16 "
            "like q without k_scale, uint8 / float8_e4m3fn with k_scale = a float32 tensor of one element on q's "
            "device), v_buffer = k_buffer[..., :512] (a view of the same storage), logit_cap == 0")


def _code(dtype: torch.dtype) -> int:
    return _DT.get(dtype, -1)


@torch.inference_mode()
def decode_attention_fwd(q, k_buffer, v_buffer, o, req_to_token, b_seq_len, attn_logits, num_kv_splits,
                         sm_scale, page_size=1, logit_cap=0.0, *, k_scale: torch.Tensor | None = None) -> None:
    assert num_kv_splits == attn_logits.shape[2]
    if logit_cap > 0:
        raise NotImplementedError(f"decode_attention_fwd: logit_cap is not supported; only {MLA_FORM}")
    if k_buffer.dim() == 3:   # [tokens, kv heads, width]: page_size 1
        k_buffer, v_buffer = k_buffer.unsqueeze(1), v_buffer.unsqueeze(1)
    mla = (q.dim() == 3 and k_buffer.dim() == 4 and v_buffer.dim() == 4 and k_buffer.shape[2] == 1
           and v_buffer.shape[:3] == k_buffer.shape[:3] and v_buffer.data_ptr() == k_buffer.data_ptr()
           and v_buffer.stride()[:2] == k_buffer.stride()[:2] and k_buffer.shape[1] == page_size
           and k_buffer.stride(3) == 1 and v_buffer.stride(3) == 1 and q.stride(2) == 1 and o.stride(2) == 1
           and o.dtype == q.dtype and tuple(o.shape) == (q.shape[0], q.shape[1], v_buffer.shape[3]))
    if not mla:
        raise NotImplementedError(f"decode_attention_fwd: only {MLA_FORM} is implemented")
    kv_dtype = _lib.KV_FP8_E4M3 if k_buffer.dtype in _FP8 else _lib.KV_AUTO
    assert attn_logits.dtype == torch.float32 and attn_logits.is_contiguous()
    assert req_to_token.stride(1) == 1 and b_seq_len.is_contiguous() and req_to_token.dtype == b_seq_len.dtype
    args = (_ptr(o), _ptr(q), _ptr(k_buffer), _ptr(req_to_token), _ptr(b_seq_len), _ptr(attn_logits),
            attn_logits.numel(), q.shape[0], q.shape[1], k_buffer.shape[3], v_buffer.shape[3], page_size,
            req_to_token.shape[1], num_kv_splits, float(sm_scale), q.stride(0), q.stride(1), o.stride(0),
            o.stride(1), k_buffer.stride(0), k_buffer.stride(1), req_to_token.stride(0), _code(q.dtype),
            _code(k_buffer.dtype), kv_dtype, 8 * req_to_token.element_size())
    if k_scale is None:   # an fp8 cache without its scale is refused there
        with _dev(q):
            check(lib.vllm_amd_mla_decode(*args, _stream(q)))
        return
    if kv_dtype != _lib.KV_FP8_E4M3:
        raise RuntimeError(f"decode_attention_fwd: k_scale with a {k_buffer.dtype} cache; the supported form is "
                           f"{MLA_FORM}")
    if k_scale.dtype != torch.float32 or k_scale.numel() != 1 or k_scale.device != q.device:
        raise RuntimeError(f"decode_attention_fwd: k_scale is {k_scale.dtype} with {k_scale.numel()} element(s) on "
                           f"{k_scale.device}; the supported form is {MLA_FORM}")
    with _dev(q):   # the strides of a byte cache are bytes
        check(lib.vllm_amd_mla_decode_fp8(*args, _ptr(k_scale), _stream(q)))
