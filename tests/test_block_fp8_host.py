"""CPU tests (no GPU) of the block-scaled fp8 entry points: host-side validation decides from
shapes and enums only (dummy pointers are never dereferenced, nothing is launched)."""
import os
import re

from vllm_amd import _lib

L = _lib.lib
P = 0x1000  # aligned, never touched


def _err(rc):
    assert rc != 0
    return rc, L.vllm_amd_last_error().decode()


def _mm(M=4, N=256, K=256, out_dtype=_lib.BF16):
    return L.vllm_amd_scaled_mm_blockwise(P, P, P, P, P, None, M, N, K, K, K, N, K // 128, 1,
                                          (N + 127) // 128, 1, out_dtype, None)


def _quant(tokens=4, hidden=256, group=128, dtype=_lib.BF16):
    return L.vllm_amd_per_token_group_fp8_quant(P, P, P, tokens, hidden, group, 1e-10, -448.0, 448.0,
                                                0, hidden // max(group, 1), 1, dtype, None)


def test_blockwise_gemm_validation():
    rc, msg = _err(_mm(K=192))
    assert rc == -2 and "K" in msg and "128" in msg          # VLLM_AMD_EUNSUPPORTED
    rc, msg = _err(_mm(M=-1))
    assert rc == -1 and "negative dimension" in msg          # VLLM_AMD_EINVAL
    assert "bfloat16 or float16" in _err(_mm(out_dtype=_lib.F32))[1]
    assert _mm(M=0) == 0 and _mm(N=0) == 0                   # empty: nothing to do, no launch


def test_group_quant_validation():
    assert "not a multiple of the group size" in _err(_quant(hidden=200, group=128))[1]
    assert _err(_quant(hidden=240, group=12))[0] == -2       # not a multiple of 8
    assert "unsupported dtype" in _err(_quant(dtype=9))[1]
    assert _quant(tokens=0) == 0


def test_new_symbols_declared_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vllm_amd.h")).read(), flags=re.S)
    for sym in ("vllm_amd_per_token_group_fp8_quant", "vllm_amd_scaled_mm_blockwise"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert hasattr(L, sym) and sym in _lib.SIGNATURES
    assert L.vllm_amd_set_tuning(b"mm_block_kernel", 0) == 0
