"""MoE routing on the GPU (csrc/moe_routing.hip): fused_topk / topk_softmax and grouped_topk against the reference's
formulas (fused_moe.py:882-975) evaluated in fp64, fused_moe against fused_experts over the same routing, and opcheck.

Data: per token logits = (randperm(E) - E // 2) / 32, exact in bf16 and f16 and without ties, bias = rand(E) * 0.2.
Every case first asserts that the fp64 reference decides by a margin of at least 1e-5 (a property of the data:
about a hundred fp32 roundings of a score), so the ids must agree as sets.  Weights: rtol 1e-5 (about twenty fp32
roundings and two 2-ulp expf give 1.5e-6), atol 0."""
import functools

import pytest
import torch

from test_gpu_opcheck import opcheck
from test_gpu_parity_moe import block_quant

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GROUPED = [(1, 256, 8, 4, 8, "sigmoid", True), (33, 256, 8, 4, 8, "sigmoid", True), (33, 256, 8, 4, 8, "sigmoid", False),
           (7, 160, 8, 3, 6, "softmax", False), (5, 64, 1, 1, 6, "softmax", False), (19, 16, 4, 2, 4, "sigmoid", True)]
SOFTMAX = [(1, 8, 2), (33, 64, 6), (70, 128, 8), (5, 256, 8), (3, 60, 4)]


def gap(values, k):
    """smallest distance between the k-th and (k+1)-th largest entry of a row; inf when all are taken"""
    if k >= values.shape[1]:
        return float("inf")
    top = values.topk(k + 1, dim=-1).values
    return (top[:, k - 1] - top[:, k]).min().item()


@functools.lru_cache(maxsize=None)
def case(T, E, topk, G=0, kept=0, scoring="softmax", bias=False):
    """(logits fp32, bias fp32 or None, ids sorted per row, unnormalised fp64 weights of those ids), on the CPU"""
    g = torch.Generator().manual_seed(T * 1000 + E)
    logits = torch.stack([(torch.randperm(E, generator=g) - E // 2) / 32 for _ in range(T)])
    b = torch.rand(E, generator=g) * 0.2 if bias else None
    scores = logits.double().softmax(-1) if scoring == "softmax" else logits.double().sigmoid()
    sel = scores + b.double() if bias else scores
    if G:
        per_group = sel.view(T, G, -1)
        group_scores = per_group.topk(2, dim=-1).values.sum(-1) if bias else per_group.amax(-1)
        assert gap(group_scores, kept) >= 1e-5
        alive = torch.zeros(T, G, dtype=torch.bool).scatter_(1, group_scores.topk(kept, dim=-1).indices, True)
        sel = sel.masked_fill(~alive.repeat_interleave(E // G, 1), float("-inf"))
    assert gap(sel, topk) >= 1e-5
    ids = sel.topk(topk, dim=-1).indices.sort(-1).values
    return logits, b, ids, scores.gather(1, ids)


def check(weights, ids, ref_ids, ref_w, renormalize):
    order = ids.long().cpu().argsort(-1)
    assert torch.equal(ids.long().cpu().gather(1, order), ref_ids)
    if renormalize:
        ref_w = ref_w / ref_w.sum(-1, keepdim=True)
    torch.testing.assert_close(weights.cpu().gather(1, order).double(), ref_w, rtol=1e-5, atol=0)


@pytest.mark.parametrize("renormalize", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,E,G,kept,topk,scoring,bias", GROUPED)
def test_grouped_topk_vs_fp64(ops, T, E, G, kept, topk, scoring, bias, dtype, renormalize):
    from vllm_amd.model_executor.layers.fused_moe import grouped_topk
    logits, b, ref_ids, ref_w = case(T, E, topk, G, kept, scoring, bias)
    x = torch.empty((T, 1), device="cuda")
    w, ids = grouped_topk(x, logits.to(dtype).cuda(), topk, renormalize, G, kept, scoring, b.cuda() if bias else None)
    assert w.dtype == torch.float32 and ids.dtype == torch.int32
    check(w, ids, ref_ids, ref_w, renormalize)


@pytest.mark.parametrize("renormalize", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,E,topk", SOFTMAX)
def test_fused_topk_vs_fp64(ops, T, E, topk, dtype, renormalize):
    from vllm_amd.model_executor.layers.fused_moe import fused_topk
    logits, _, ref_ids, ref_w = case(T, E, topk)
    x = torch.empty((T, 1), device="cuda")
    for indices_type in (None, torch.int64) if (T, E) == (33, 64) else (None,):
        w, ids, tei = fused_topk(x, logits.to(dtype).cuda(), topk, renormalize, indices_type)
        assert ids.dtype == (indices_type or torch.int32)
        check(w, ids, ref_ids, ref_w, renormalize)
        assert (w[:, 1:] <= w[:, :-1]).all()
        assert torch.equal(tei.cpu(), (torch.arange(topk) * T)[None, :].int() + torch.arange(T)[:, None].int())
    if not renormalize:     # the reference's op itself, on a row-strided view
        wide = torch.zeros((T, E + 8), dtype=dtype, device="cuda")
        wide[:, :E] = logits.to(dtype)
        w2, ids2 = torch.empty_like(w), torch.empty((T, topk), dtype=torch.int32, device="cuda")
        ops.topk_softmax(w2, ids2, tei, wide[:, :E])
        assert torch.equal(w2, w) and torch.equal(ids2.long(), ids.long())
    with pytest.raises(NotImplementedError, match="indices_type"):
        fused_topk(x, logits.cuda(), topk, renormalize, torch.int16)


@pytest.mark.parametrize("E,G,kept,topk", [(64, 0, 0, 6), (256, 8, 4, 8), (16, 4, 2, 6), (160, 8, 3, 50)])
def test_ties_go_to_the_lower_index(ops, E, G, kept, topk):
    """All logits equal, constant bias: experts 0 .. topk-1 with equal weights; in the last two cases topk exceeds a
    group, so the ids also show that groups 0 .. kept-1 were the ones kept."""
    from vllm_amd.model_executor.layers.fused_moe import fused_topk, grouped_topk
    x, logits = torch.empty((1, 1), device="cuda"), torch.full((1, E), 0.25, device="cuda")
    if G:
        w, ids = grouped_topk(x, logits, topk, False, G, kept, "sigmoid", torch.full((E,), 0.1, device="cuda"))
    else:
        w, ids, _ = fused_topk(x, logits, topk, False)
    assert ids[0].tolist() == list(range(topk)) and (w == w[0, 0]).all()
    with pytest.raises(ValueError, match="Unsupported scoring function: tanh"):
        grouped_topk(x, logits, topk, False, G, kept, "tanh")


@pytest.mark.parametrize("use_grouped", [False, True])
def test_fused_moe(ops, use_grouped):
    """Routing + experts equals the experts over the same routing bit for bit, eagerly and from one graph replayed
    with gating_output changed in place (shapes of test_fused_experts' second case)."""
    from vllm_amd.model_executor.layers.fused_moe import fused_experts, fused_moe, fused_topk, grouped_topk
    M, N, K, E, topk = 33, 512, 384, 8, 2
    torch.manual_seed(0)
    a = torch.randn((M, K), dtype=torch.bfloat16, device="cuda") / 10
    w1, w1_s = block_quant(torch.randn((E, 2 * N, K), dtype=torch.bfloat16, device="cuda") / 15)
    w2, w2_s = block_quant(torch.randn((E, K, N), dtype=torch.bfloat16, device="cuda") / 15)
    gatings = [torch.randn((M, E), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    kw = dict(use_fp8_w8a8=True, w1_scale=w1_s, w2_scale=w2_s, block_shape=[128, 128])
    route = dict(use_grouped_topk=True, num_expert_group=4, topk_group=2) if use_grouped else {}
    eager = []
    for g in gatings:
        tw, ids = grouped_topk(a, g, topk, True, 4, 2) if use_grouped else fused_topk(a, g, topk, True)[:2]
        eager.append(fused_experts(a, w1, w2, tw, ids, **kw))
        assert torch.equal(fused_moe(a, w1, w2, g, topk, True, **route, **kw), eager[-1])
    assert not torch.equal(eager[0], eager[1])
    gating = gatings[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = fused_moe(a, w1, w2, gating, topk, True, **route, **kw)
    for want, src in zip(eager, gatings):
        gating.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, want)


def test_opcheck_routing_ops(ops):
    T, E, topk = 5, 256, 8
    logits = torch.randn((T, E), device="cuda", dtype=torch.bfloat16)
    w = torch.zeros((T, topk), device="cuda")
    ids, tei = torch.zeros((T, topk), dtype=torch.int32, device="cuda"), torch.zeros((T, topk), dtype=torch.int32, device="cuda")
    opcheck(torch.ops._moe_C.topk_softmax, (w, ids, tei, logits))
    opcheck(torch.ops._moe_C.fused_topk, (w, ids, tei, logits, True))
    opcheck(torch.ops._moe_C.grouped_topk, (w, ids, logits, torch.rand(E, device="cuda"), 8, 4, True, "sigmoid"))
    opcheck(torch.ops._moe_C.grouped_topk, (w, ids, logits, None, 8, 4, False, "softmax"))
