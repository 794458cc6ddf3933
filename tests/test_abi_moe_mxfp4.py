"""CPU test (no GPU): the three MXFP4 entry points are exported, carry ctypes signatures and decide their refusals
on the host (dummy pointers are never dereferenced, nothing is launched)."""


def test_mxfp4_validation_without_launch():
    from vllm_amd import _lib
    L, p = _lib.lib, 0x1000              # aligned, never touched
    for name in ("vllm_amd_mxfp4_quant", "vllm_amd_silu_and_mul_mxfp4_quant", "vllm_amd_moe_mxfp4_gemm"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name

    def err(rc):
        assert rc != 0
        return L.vllm_amd_last_error().decode()

    def gemm(c=p, w=p, ws=p, nvt=8, top_k=2, bm=16, N=208, K=256, dtype=_lib.BF16, lda=None, as_sm=None, pad=60):
        lda = K // 2 if lda is None else lda
        as_sm = K // 32 if as_sm is None else as_sm
        return L.vllm_amd_moe_mxfp4_gemm(c, p, w, p, ws, p, p, p, p, nvt, top_k, 1, bm, nvt + pad, 4, N, K, lda,
                                         N * K // 2, K // 2, N, as_sm, N * K // 32, K // 32, dtype, None)

    assert gemm(nvt=0, c=None) == 0                               # empty: nothing to do, no launch
    assert "K = 192 must be a positive multiple of 128" in err(gemm(K=192))
    assert "block_size_m = 32 must be 16 or 64" in err(gemm(bm=32))
    assert "bfloat16 or float16" in err(gemm(dtype=_lib.F32))
    assert "null pointer" in err(gemm(c=None))
    assert "multiples of 16" in err(gemm(lda=136))
    assert "multiples of 4" in err(gemm(as_sm=10))

    quant = lambda rows=4, K=256, ld=None, dtype=_lib.BF16, q=p, x=p: L.vllm_amd_mxfp4_quant(
        q, p, x, rows, K, K if ld is None else ld, dtype, None)
    assert quant(rows=0, q=None) == 0
    assert "row length 48 is not a multiple of the 32-wide MX block" in err(quant(K=48))
    assert "multiple of 8 elements" in err(quant(ld=260))

    silu = lambda rows=4, d=128, dtype=_lib.F16, q=p: L.vllm_amd_silu_and_mul_mxfp4_quant(q, p, p, rows, d, dtype, None)
    assert silu(rows=0, q=None) == 0
    assert "row length 80 is not a multiple" in err(silu(d=80))
    assert "4-byte" in err(silu(q=p + 2))
