"""CPU test (no GPU): vllm_amd_mla_decode_fp8 decides its refusals on the host from shapes, enums, strides
and pointer values (dummy pointers are never dereferenced, nothing is launched), and vllm_amd_mla_decode
points an fp8 cache at it."""


def test_mla_decode_fp8_validation_without_launch():
    from vllm_amd import _lib
    L, p = _lib.lib, 0x1000              # aligned, never touched

    def call(fn=L.vllm_amd_mla_decode_fp8, batch=2, H=16, widths=(576, 512), splits=4, floats=2 * 16 * 4 * 513,
             entry=576, dtype=_lib.BF16, kv=_lib.KV_FP8_E4M3, bits=32, cache=p, scale=(p,)):
        return fn(p, p, cache, p, p, p, floats, batch, H, *widths, 16, 4, splits, 0.04, H * 576, 576, H * 512, 512,
                  16 * entry, entry, 4, dtype, dtype, kv, bits, *scale, None)

    def err(rc):
        assert rc != 0
        return L.vllm_amd_last_error().decode()

    assert call(batch=0, cache=None, scale=(None,)) == 0          # empty batch: nothing to do, no launch
    assert "row width 512 / 448" in err(call(widths=(512, 448)))
    assert "16-bit latent cache goes through vllm_amd_mla_decode;" in err(call(kv=_lib.KV_AUTO))
    assert "q must be bfloat16 or float16" in err(call(dtype=_lib.F32))
    assert "must be int32" in err(call(bits=64))
    assert "num_kv_splits 0 < 1" in err(call(splits=0))
    assert "num_heads 129 > 128" in err(call(H=129, floats=1 << 30))
    assert "scratch too small" in err(call(floats=2 * 16 * 4 * 512))
    assert "null pointer" in err(call(scale=(None,)))
    for bad in (dict(entry=584), dict(entry=560), dict(cache=p + 8)):
        assert "multiples of 16" in err(call(**bad)) and "supported form" in err(call(**bad))
    assert "vllm_amd_mla_decode_fp8" in err(call(fn=L.vllm_amd_mla_decode, scale=()))
