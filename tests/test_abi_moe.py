"""CPU test (no GPU): the four fused-MoE entry points are exported, carry ctypes signatures and decide their
refusals on the host from shapes, enums, strides and pointer values (dummy pointers are never dereferenced,
nothing is launched)."""


def test_moe_validation_without_launch():
    from vllm_amd import _lib
    L, p = _lib.lib, 0x1000              # aligned, never touched
    for name in ("vllm_amd_moe_blockwise_gemm", "vllm_amd_moe_align_block_size",
                 "vllm_amd_silu_and_mul_group_quant", "vllm_amd_moe_sum"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name

    def gemm(c=p, w=p, nvt=8, top_k=2, bm=16, E=4, N=256, K=256, dtype=_lib.BF16, lda=None, pad=60):
        lda = K if lda is None else lda
        return L.vllm_amd_moe_blockwise_gemm(c, p, w, p, p, p, p, p, w, nvt, top_k, 1, bm, nvt + pad, E, N, K, lda, N * K, K, N,
                                             K // 128, 1, 2 * (K // 128), K // 128, 1, dtype, None)

    def err(rc):
        assert rc != 0
        return L.vllm_amd_last_error().decode()

    assert gemm(nvt=0, c=None) == 0                               # empty: nothing to do, no launch
    assert gemm(N=0, c=None) == 0
    assert "K = 200 must be a positive multiple of the 128-wide scale block" in err(gemm(K=200, lda=208))
    assert "block_size_m = 24 must be 16 or 64" in err(gemm(bm=24))
    assert "bfloat16 or float16" in err(gemm(dtype=_lib.F32))
    assert "not a multiple of top_k" in err(gemm(nvt=7))
    assert "null pointer" in err(gemm(c=None))
    assert "max_num_tokens_padded 7 < num_valid_tokens 8" in err(gemm(pad=-1))
    assert "null pointer" in err(gemm(w=None))                    # weights
    assert "multiples of 16" in err(gemm(lda=264))

    align = lambda numel=8, E=4, ids=p, out=p: L.vllm_amd_moe_align_block_size(ids, numel, E, 16, out, p, p, None)
    assert align(numel=0, ids=None, out=None) == 0
    assert "num_experts 2000 > 1024" in err(align(E=2000))
    assert "null pointer" in err(align(out=None))

    silu = lambda rows=4, d=256, dtype=_lib.BF16, q=p: L.vllm_amd_silu_and_mul_group_quant(q, p, p, rows, d, d // 128,
                                                                                          1, dtype, None)
    assert silu(rows=0, q=None) == 0
    assert "intermediate size 192 is not a multiple of 128" in err(silu(d=192))
    assert "float16 or bfloat16" in err(silu(dtype=_lib.F32))
    assert "null pointer" in err(silu(q=None))
    assert "8-byte aligned" in err(silu(q=p + 4))

    msum = lambda nt=4, dtype=_lib.F16, out=p: L.vllm_amd_moe_sum(out, p, nt, 2, 128, dtype, None)
    assert msum(nt=0, out=None) == 0
    assert "float16 or bfloat16" in err(msum(dtype=_lib.F32))
    assert "null pointer" in err(msum(out=None))

    for ks in (8, 2, 0):
        assert L.vllm_amd_set_tuning(b"moe_ks", ks) == 0
