"""The 128-row tile kernel of the fp8 grouped MoE GEMM (block_size_m = 128) on the GPU: against fp64 with the
bound of test_gpu_parity_block_fp8.py, bit-exact on integer data with a dropped block and under an expert_map,
fused_experts end to end above the threshold (eager and one captured graph), and opcheck."""
import pytest
import torch

from test_gpu_opcheck import opcheck
from test_gpu_parity_block_fp8 import FP8, check_bound
from test_gpu_parity_moe import block_quant, moe_gemm_case, rand_ids, ref_moe, run_gemm, slot_refs

pytestmark = pytest.mark.gpu

BM = 128


@pytest.mark.parametrize("dtype,mul", [(torch.bfloat16, True), (torch.float16, False)])
@pytest.mark.parametrize("tokens,E,top_k", [(1, 4, 1), (70, 8, 6), (150, 4, 3)])
@pytest.mark.parametrize("N", [128, 204, 328])
@pytest.mark.parametrize("K", [128, 256, 384, 512, 1152])
def test_moe_tile_gemm_vs_fp64(ops, K, N, tokens, E, top_k, mul, dtype):
    """1, 2, 3, 4 and 9 K blocks around the 4-stage ring; N 204: a partial tile with 8-byte aligned rows (scalar
    stores), 328: three scale columns; one valid row among 127 padding rows, several experts of one partial block
    each plus the -1 slot, and expert 0 with two m-blocks."""
    a, b, As, Bs, ids, w, (ref, R) = moe_gemm_case(tokens, E, top_k, N, K)
    c, _ = run_gemm(ops, a, b, As, Bs, ids, w, BM, mul, dtype)
    routed = (ids.view(-1) >= 0)
    assert (c[~routed] == 7.0).all()                     # rows no entry names keep their prefill
    scale = w.double().view(-1, 1) if mul else 1.0
    check_bound(c[routed], (ref * scale)[routed], (R * scale)[routed], dtype)


def test_moe_tile_gemm_integer_exact_and_dropped_block(ops):
    """The recipe of test_moe_gemm_integer_exact_and_dropped_block (every partial, scale product, running sum and
    routed product exact in fp32, below 3 x 768 x 4 x 2): the f16 output equals the rounded fp64 result bit for bit.
    Then expert_ids[0] = -1: the valid rows of block 0 are zero, every other row is unchanged."""
    tokens, E, top_k, N, K = 150, 4, 3, 208, 384
    g = torch.Generator(device="cuda").manual_seed(BM)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, device="cuda", generator=g)
    a, b = ri(-3, 3, tokens, K).float().to(FP8), ri(-2, 2, E, N, K).float().to(FP8)
    As = (2.0 ** ri(-2, 1, K // 128, tokens).float()).t()          # token-contiguous
    Bs = 2.0 ** ri(-2, 1, E, 2, K // 128).float()
    ids, w = rand_ids(g, tokens, E, top_k), 2.0 ** ri(-2, 1, tokens, top_k).float()
    want = (slot_refs(a, b, As, Bs, ids)[0] * w.double().view(-1, 1)).to(torch.float16)
    c, _ = run_gemm(ops, a, b, As, Bs, ids, w, BM, True, torch.float16)
    assert torch.equal(c, want)
    c, sorted_ids = run_gemm(ops, a, b, As, Bs, ids, w, BM, True, torch.float16, drop_block=0)
    rows = sorted_ids[:BM][sorted_ids[:BM] < ids.numel()].long()
    assert rows.numel() and not c[rows].any()
    want[rows] = 0
    assert torch.equal(c, want)


def test_moe_tile_gemm_full_bound_under_expert_map(ops):
    """The recipe of test_moe_gemm_full_bound_under_expert_map: one slot per global expert, so the padded total
    E x 128 is the whole length of sorted_token_ids; experts 5 and 7 are local.  Bit-exact."""
    from vllm_amd.model_executor.layers.fused_moe import moe_align_block_size
    E, local, N, K = 8, [5, 7], 208, 384
    g = torch.Generator(device="cuda").manual_seed(BM)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, device="cuda", generator=g)
    a, b = ri(-3, 3, E, K).float().to(FP8), ri(-2, 2, E, N, K).float().to(FP8)
    As, Bs = 2.0 ** ri(-2, 1, E, K // 128).float(), 2.0 ** ri(-2, 1, E, 2, K // 128).float()
    ids, w = torch.randperm(E, device="cuda", generator=g).to(torch.int32).view(E, 1), 2.0 ** ri(-2, 1, E).float()
    emap = torch.full((E,), -1, device="cuda", dtype=torch.int32)
    emap[local] = torch.arange(2, device="cuda", dtype=torch.int32)
    sorted_ids, expert_ids, post = moe_align_block_size(ids, BM, E, emap)
    assert post.item() == E * BM == sorted_ids.numel()
    c = torch.full((E, N), 7.0, dtype=torch.float16, device="cuda")
    ops.moe_block_fp8_gemm(c, a, b[local], As, Bs[local], w, sorted_ids, expert_ids, post, True, 1, BM)
    want = slot_refs(a, b, As, Bs, ids)[0] * w.double().view(-1, 1)
    want[~torch.isin(ids.view(-1), torch.tensor(local, device="cuda", dtype=torch.int32))] = 0
    assert torch.equal(c, want.to(torch.float16))


def test_fused_experts_tile(ops):
    """256 slots per expert: fused_experts takes the tile kernel.  The recipe and tolerance of test_fused_experts;
    then the call captured in one graph, replayed twice with topk_ids changed in place, against eager bit for bit."""
    from vllm_amd.model_executor.layers.fused_moe import fused_experts
    from vllm_amd.model_executor.layers.fused_moe.fused_moe import _block_size_m
    M, N, K, E, topk = 512, 256, 384, 4, 2
    assert _block_size_m(M, topk, E) == BM
    torch.manual_seed(0)
    dt = torch.bfloat16
    a = torch.randn((M, K), dtype=dt, device="cuda") / 10
    w1, w1_s = block_quant(torch.randn((E, 2 * N, K), dtype=dt, device="cuda") / 15)
    w2, w2_s = block_quant(torch.randn((E, K, N), dtype=dt, device="cuda") / 15)
    topk_w, topk_ids = torch.randn((M, E), device="cuda").softmax(-1).topk(topk, dim=-1)
    topk_ids = topk_ids.to(torch.int32)
    kw = dict(use_fp8_w8a8=True, w1_scale=w1_s, w2_scale=w2_s, block_shape=[128, 128])
    out = fused_experts(a, w1, w2, topk_w, topk_ids, **kw)
    torch.testing.assert_close(out, ref_moe(a, w1, w2, w1_s, w2_s, topk_w, topk_ids), atol=0.035, rtol=0.035)
    other = topk_ids.flip(0).contiguous()
    eager = [out, fused_experts(a, w1, w2, topk_w, other, **kw)]
    ids = topk_ids.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = fused_experts(a, w1, w2, topk_w, ids, **kw)
    for want, src in zip(eager, (topk_ids, other)):
        ids.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, want)


def test_opcheck_moe_tile_gemm(ops):
    E, top_k, N, K = 8, 2, 256, 256
    ids = torch.tensor([[0, 5], [3, 1], [6, 2]], dtype=torch.int32, device="cuda")   # one slot per expert: one order
    n = ids.numel() + E * (BM - 1)
    sorted_ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    expert_ids = torch.zeros(-(-n // BM), dtype=torch.int32, device="cuda")
    post = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.moe_align_block_size(ids.view(-1), E, BM, sorted_ids, expert_ids, post)
    a = torch.randn((3, K), device="cuda").to(FP8)
    b = torch.randn((E, N, K), device="cuda").to(FP8)
    As, Bs = torch.rand((3, K // 128), device="cuda"), torch.rand((E, N // 128, K // 128), device="cuda")
    c = torch.zeros((6, N), dtype=torch.bfloat16, device="cuda")
    w = torch.rand(6, device="cuda")
    opcheck(torch.ops._C.moe_block_fp8_gemm, (c, a, b, As, Bs, w, sorted_ids, expert_ids, post, True, top_k, BM))
    opcheck(torch.ops._C.moe_block_fp8_gemm, (c, a, b, As, Bs, None, sorted_ids, expert_ids, post, False, top_k, BM))
