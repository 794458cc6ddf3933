"""CPU test (no GPU): the three MLA prefill entry points are exported, carry ctypes signatures and decide their
refusals on the host (dummy pointers are never dereferenced, nothing is launched)."""


def test_mla_prefill_validation_without_launch():
    from vllm_amd import _lib
    L, p = _lib.lib, 0x1000              # aligned, never touched
    for name in ("vllm_amd_mla_prefill_attention", "vllm_amd_merge_attn_states", "vllm_amd_gather_cache"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name

    def err(rc):
        assert rc != 0
        return L.vllm_amd_last_error().decode()

    def attn(out=p, B=2, Tq=300, H=4, qk=192, dtype=_lib.BF16, kn_st=1024):
        return L.vllm_amd_mla_prefill_attention(out, None, p, p, p, p, p, p, B, Tq, H, qk, 128, 64, 256, 0.1, 1,
                                                H * 192, 192, H * 128, 128, kn_st, 256, 64, 0, 1024, 256, Tq, dtype, None)

    assert attn(B=0, out=None) == 0 and attn(Tq=0, out=None) == 0      # empty: nothing to do, no launch
    assert "only 192 / 128 / 64 is implemented" in err(attn(qk=256))
    assert "bfloat16 or float16" in err(attn(dtype=_lib.F32))
    assert "multiples of 8 elements" in err(attn(kn_st=1028))
    assert "null pointer" in err(attn(out=None))

    def merge(T=37, D=128, out=p):
        return L.vllm_amd_merge_attn_states(out, None, p, p, p, p, T, 3, D, 3 * D, D, 3 * D, D, 3 * D, D, T, _lib.F16, None)

    assert merge(T=0, out=None) == 0
    assert "head size 100 is not a multiple of 8" in err(merge(D=100))

    def gather(B=2, rows=64, dst=p, kv=_lib.KV_AUTO, entry=576):
        return L.vllm_amd_gather_cache(p, dst, p, p, None, B, rows, 16, entry, 8, 16 * entry, entry, entry, 2, _lib.BF16,
                                       kv, None, None)

    assert gather(B=0, dst=None) == 0 and gather(rows=0, dst=None) == 0
    assert "null pointer" in err(gather(kv=_lib.KV_FP8_E4M3))          # an fp8 cache without its scale
