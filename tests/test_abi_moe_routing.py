"""CPU test (no GPU): the two MoE routing entry points are exported, carry ctypes signatures and decide their
refusals on the host (dummy pointers are never dereferenced, nothing is launched)."""


def test_moe_routing_validation_without_launch():
    from vllm_amd import _lib
    L, p = _lib.lib, 0x1000              # aligned, never touched
    for name in ("vllm_amd_topk_softmax", "vllm_amd_grouped_topk"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name

    def soft(w=p, g=p, T=4, E=64, topk=6, stride=None, dtype=_lib.BF16, ids64=0):
        return L.vllm_amd_topk_softmax(w, p, p, g, T, E, topk, E if stride is None else stride, 1, dtype, ids64, None)

    def grouped(w=p, bias=None, T=4, E=256, topk=8, G=8, kept=4, scoring=1, dtype=_lib.F32):
        return L.vllm_amd_grouped_topk(w, p, p, bias, T, E, topk, G, kept, scoring, 1, E, dtype, None)

    def err(rc):
        assert rc != 0
        return L.vllm_amd_last_error().decode()

    assert soft(T=0, w=None, g=None) == 0                         # empty: nothing to do, no launch
    assert grouped(T=0, w=None) == 0
    for call in (soft, grouped):
        assert "num_experts 2000 > 1024" in err(call(E=2000))
        assert "topk 0 is outside [1, min(num_experts, 64)]" in err(call(topk=0))
        assert "gating dtype 9 must be float32, float16 or bfloat16" in err(call(dtype=9))
        assert "null pointer" in err(call(w=None))
    assert "topk 9 is outside" in err(soft(E=8, topk=9))
    assert "topk 65 is outside" in err(soft(E=128, topk=65))
    assert "gating stride 60 < num_experts 64" in err(soft(stride=60))
    assert "ids dtype 2 must be" in err(soft(ids64=2))
    assert "null pointer" in err(soft(g=None))
    assert "num_expert_group 3 does not divide num_experts 256" in err(grouped(G=3))
    assert "num_expert_group 0 does not divide" in err(grouped(G=0))
    assert "topk_group 9 is outside [1, num_expert_group 8]" in err(grouped(kept=9))
    assert "topk_group 0 is outside" in err(grouped(kept=0))
    assert "topk 8 > topk_group 1 x 4 experts per group" in err(grouped(E=32, kept=1))
    assert "needs groups of at least 2 experts, got 1" in err(grouped(E=8, topk=2, bias=p))
    assert "unknown scoring function 7" in err(grouped(scoring=7))
    assert "num_expert_group 65 > 64" in err(grouped(E=130, G=65, kept=8))   # 2 experts per group, 4 per lane
