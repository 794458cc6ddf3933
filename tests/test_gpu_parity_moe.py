"""Fused MoE experts over block-scaled fp8 weights on the GPU: moe_align_block_size (contract as set
equalities), the grouped GEMM against fp64 (the bound of test_gpu_parity_block_fp8.py; the routed weight
multiplies ref and R, its fp32 multiply adds one 2^-24 term that the 2^-16 R slack covers for K <= 16384),
silu_and_mul_group_quant, moe_sum, fused_experts end to end against the torch restatement of the reference's
test (tests/kernels/moe/test_block_fp8.py:100-133, its data recipe and its tolerance 0.035), and opcheck."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_opcheck import opcheck
from test_gpu_parity_block_fp8 import FP8, check_bound, ref_gemm

pytestmark = pytest.mark.gpu


@pytest.fixture
def moe_ks(request):
    from vllm_amd import _lib
    _lib.set_tuning("moe_ks", request.param)
    yield request.param
    _lib.set_tuning("moe_ks", 0)


def rand_ids(g, tokens, E, top_k):
    """top_k distinct experts per token, expert 0 first for every token (so it gets `tokens` rows: more than one
    m-block from 17 / 65 tokens on) and expert E - 1 for nobody."""
    score = torch.rand((tokens, max(E - 1, 1)), device="cuda", generator=g)
    score[:, 0] -= 1
    return score.argsort(1)[:, :top_k].to(torch.int32)


@pytest.mark.parametrize("numel,E,block", [(1, 4, 16), (48, 8, 16), (330, 8, 64), (4096, 256, 16)])
def test_align_contract(ops, numel, E, block):
    from vllm_amd.model_executor.layers.fused_moe import moe_align_block_size
    g = torch.Generator(device="cuda").manual_seed(numel)
    ids = torch.randint(0, E - 1, (numel,), device="cuda", generator=g, dtype=torch.int32)
    if numel > 1:
        ids[numel // 2] = -1
    sorted_ids, expert_ids, post = (t.cpu() for t in moe_align_block_size(ids.view(-1, 1), block, E))
    ids = ids.cpu()
    assert sorted_ids.numel() == numel + E * (block - 1) and expert_ids.numel() == -(-sorted_ids.numel() // block)
    cnt = torch.bincount(ids[ids >= 0], minlength=E)
    pad = (cnt + block - 1) // block * block
    assert post.item() == pad.sum().item()
    assert torch.equal(expert_ids[:post.item() // block], torch.arange(E).repeat_interleave(pad // block).int())
    start = 0
    for e in range(E):
        seg = sorted_ids[start:start + pad[e]]
        assert torch.equal(seg[seg < numel].sort().values, torch.nonzero(ids == e).view(-1).int())
        assert (seg[seg >= numel] == numel).all()
        start += pad[e].item()


@functools.lru_cache(maxsize=None)
def moe_gemm_case(tokens, E, top_k, N, K):
    """Data as gemm_case of test_gpu_parity_block_fp8.py, with an expert axis; one slot is routed nowhere (-1).
    Returns the operands and, per flat slot, the fp64 (ref, R) without the routed weight."""
    g = torch.Generator(device="cuda").manual_seed(tokens * 7919 + N * 31 + K + E)
    rnd = lambda *shape: torch.rand(shape, device="cuda", generator=g)
    a = ((rnd(tokens, K) - 0.5) * 2 * 448).clamp(-448, 448).to(FP8)
    b = ((rnd(E, N, K) - 0.5) * 2 * 448).clamp(-448, 448).to(FP8)
    As, Bs = rnd(tokens, K // 128) * 1e-2, rnd(E, (N + 127) // 128, K // 128) * 1e-2
    ids, w = rand_ids(g, tokens, E, top_k), rnd(tokens, top_k) + 0.25
    if tokens > 1:
        ids[tokens // 2, 0] = -1
    return a, b, As, Bs, ids, w, slot_refs(a, b, As, Bs, ids)


def slot_refs(a, b, As, Bs, ids):
    top_k, flat = ids.shape[1], ids.view(-1)
    ref = torch.zeros((flat.numel(), b.shape[1]), dtype=torch.float64, device="cuda")
    R = torch.zeros_like(ref)
    for e in flat.unique().tolist():
        if e >= 0:
            t = torch.nonzero(flat == e).view(-1)
            ref[t], R[t] = ref_gemm(a[t // top_k], b[e], As[t // top_k], Bs[e])
    return ref, R


def run_gemm(ops, a, b, As, Bs, ids, w, bm, mul, dtype, drop_block=None):
    from vllm_amd.model_executor.layers.fused_moe import moe_align_block_size
    sorted_ids, expert_ids, post = moe_align_block_size(ids, bm, b.shape[0])
    if drop_block is not None:
        expert_ids[drop_block] = -1
    c = torch.full((ids.numel(), b.shape[1]), 7.0, dtype=dtype, device="cuda")
    ops.moe_block_fp8_gemm(c, a, b, As, Bs, w.view(-1) if mul else None, sorted_ids, expert_ids, post, mul, ids.shape[1], bm)
    return c, sorted_ids


@pytest.mark.parametrize("dtype,mul", [(torch.bfloat16, True), (torch.float16, False)])
@pytest.mark.parametrize("moe_ks", [8, 2], indirect=True)
@pytest.mark.parametrize("bm", [16, 64])
@pytest.mark.parametrize("tokens,E,top_k", [(1, 4, 1), (5, 8, 2), (70, 8, 6)])
@pytest.mark.parametrize("N", [128, 208])
@pytest.mark.parametrize("K", [128, 384, 1152])
def test_moe_gemm_vs_fp64(ops, K, N, tokens, E, top_k, bm, moe_ks, mul, dtype):
    """Every (dtype, block_size_m, moe_ks) instantiation at every shape; the routed weight goes with bf16 here and
    with f16 in the integer-exact tests."""
    a, b, As, Bs, ids, w, (ref, R) = moe_gemm_case(tokens, E, top_k, N, K)
    c, _ = run_gemm(ops, a, b, As, Bs, ids, w, bm, mul, dtype)
    routed = (ids.view(-1) >= 0)
    assert (c[~routed] == 7.0).all()                     # rows no entry names keep their prefill
    scale = w.double().view(-1, 1) if mul else 1.0
    check_bound(c[routed], (ref * scale)[routed], (R * scale)[routed], dtype)


@pytest.mark.parametrize("bm,moe_ks", [(16, 8), (16, 2), (64, 8), (64, 2)], indirect=["moe_ks"])
def test_moe_gemm_integer_exact_and_dropped_block(ops, bm, moe_ks):
    """Small integers, power-of-two scales and routed weights: every partial, scale product, running sum and the
    routed product is exact in fp32 and below 65504 (3 blocks x 768 x 4 x 2), so the f16 output equals the rounded
    fp64 result bit for bit -- a scale or row from the wrong expert, token or stride shows.  Then the same
    call with expert_ids[0] = -1: the valid rows of block 0 are zero, every other row is unchanged."""
    tokens, E, top_k, N, K = 37, 4, 3, 208, 384
    g = torch.Generator(device="cuda").manual_seed(bm)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, device="cuda", generator=g)
    a, b = ri(-3, 3, tokens, K).float().to(FP8), ri(-2, 2, E, N, K).float().to(FP8)
    As = (2.0 ** ri(-2, 1, K // 128, tokens).float()).t()          # token-contiguous
    Bs = 2.0 ** ri(-2, 1, E, 2, K // 128).float()
    ids, w = rand_ids(g, tokens, E, top_k), 2.0 ** ri(-2, 1, tokens, top_k).float()
    want = (slot_refs(a, b, As, Bs, ids)[0] * w.double().view(-1, 1)).to(torch.float16)
    c, _ = run_gemm(ops, a, b, As, Bs, ids, w, bm, True, torch.float16)
    assert torch.equal(c, want)
    c, sorted_ids = run_gemm(ops, a, b, As, Bs, ids, w, bm, True, torch.float16, drop_block=0)
    rows = sorted_ids[:bm][sorted_ids[:bm] < ids.numel()].long()
    assert rows.numel() and not c[rows].any()
    want[rows] = 0
    assert torch.equal(c, want)


@pytest.mark.parametrize("bm", [16, 64])
def test_moe_gemm_full_bound_under_expert_map(ops, bm):
    """One slot per global expert: the padded total E bm IS the host-side bound (the length of sorted_token_ids),
    and the last blocks are those of the last experts.  Only experts 5 and 7 are local (b holds 2), so a bound
    taken from b's expert count (8 + 2 (bm - 1) entries) would cut them.  Integer data as above: bit-exact."""
    from vllm_amd.model_executor.layers.fused_moe import moe_align_block_size
    E, local, N, K = 8, [5, 7], 208, 384
    g = torch.Generator(device="cuda").manual_seed(bm)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, device="cuda", generator=g)
    a, b = ri(-3, 3, E, K).float().to(FP8), ri(-2, 2, E, N, K).float().to(FP8)
    As, Bs = 2.0 ** ri(-2, 1, E, K // 128).float(), 2.0 ** ri(-2, 1, E, 2, K // 128).float()
    ids, w = torch.randperm(E, device="cuda", generator=g).to(torch.int32).view(E, 1), 2.0 ** ri(-2, 1, E).float()
    emap = torch.full((E,), -1, device="cuda", dtype=torch.int32)
    emap[local] = torch.arange(2, device="cuda", dtype=torch.int32)
    sorted_ids, expert_ids, post = moe_align_block_size(ids, bm, E, emap)
    assert post.item() == E * bm == sorted_ids.numel()
    c = torch.full((E, N), 7.0, dtype=torch.float16, device="cuda")
    ops.moe_block_fp8_gemm(c, a, b[local], As, Bs[local], w, sorted_ids, expert_ids, post, True, 1, bm)
    want = slot_refs(a, b, As, Bs, ids)[0] * w.double().view(-1, 1)
    want[~torch.isin(ids.view(-1), torch.tensor(local, device="cuda", dtype=torch.int32))] = 0
    assert torch.equal(c, want.to(torch.float16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,d", [(1, 128), (7, 384)])
def test_silu_and_mul_group_quant(ops, rows, d, dtype):
    """Against the fp32 formula on the host: v = T(T(silu(x)) y), s = max(1e-10, max|v|) / 448 per 128-group,
    q = e4m3(v / s).  The device's expf / reciprocal differ from the host's by an ulp or two of fp32, which can
    move T(silu(x)) or v by one step of T, so v_dev = v (1 + d), |d| <= u = one step of T (2^-7 bf16, 2^-10 f16)
    -- the same for the group maximum: |s - s_ref| <= u s_ref.  The dequantised value q s is one e4m3 rounding
    from v_dev / s: half a step of a 3-bit mantissa, bound 2^-4 |v| with the step of T inside, or half a
    subnormal step, 2^-10 s, below the normal range."""
    u = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    g = torch.Generator().manual_seed(rows * d)
    x = (torch.randn((rows, 2 * d), generator=g) * 3).to(dtype)
    zero = rows * d > 128
    if zero:
        x[0, :128], x[0, d:d + 128] = 0.0, 1.0                          # an all-zero group: scale 1e-10 / 448
    x[-1, d - 128:d], x[-1, -128:] = 20.0, (448.0 * torch.randint(-3, 4, (128,), generator=g) / 20).to(dtype)
    q = torch.empty((rows, d), dtype=FP8, device="cuda")
    s = torch.empty((d // 128, rows), device="cuda").t()               # row-contiguous strides
    ops.silu_and_mul_group_quant(q, s, x.cuda())
    xf, yf = x[:, :d].float(), x[:, d:].float()
    v = ((xf / (1 + torch.exp(-xf))).to(dtype).float() * yf).to(dtype).float()
    s_ref = v.view(rows, -1, 128).abs().amax(-1).clamp(min=1e-10) / 448.0
    s = s.cpu()
    assert ((s - s_ref).abs() <= u * s_ref).all()
    assert not zero or (s[0, 0] == s_ref[0, 0] and not q[0, :128].float().any())
    se = s.repeat_interleave(128, 1)
    err = (q.cpu().float() * se - v).abs()
    assert (err <= torch.maximum(2.0 ** -4 * v.abs(), 2.0 ** -10 * se)).all()


@pytest.mark.parametrize("hidden", [256, 100])
@pytest.mark.parametrize("top_k", [1, 2, 6])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_moe_sum(ops, dtype, top_k, hidden):
    x = torch.randn((5, top_k, hidden), device="cuda", generator=torch.Generator(device="cuda").manual_seed(top_k)).to(dtype)
    out = torch.empty((5, hidden), dtype=dtype, device="cuda")
    ops.moe_sum(x, out)
    acc = torch.zeros((5, hidden), device="cuda")
    for k in range(top_k):
        acc += x[:, k].float()
    assert torch.equal(out, acc.to(dtype))


def block_quant(w):
    """per_block_cast_to_fp8 of the reference's tests (tests/kernels/quant_utils.py:225-241), batched over experts."""
    E, n, k = w.shape
    v = w.view(E, n // 128, 128, k // 128, 128)
    amax = v.abs().float().amax(dim=(2, 4), keepdim=True).clamp(1e-4)
    return (v * (448.0 / amax)).to(FP8).view(E, n, k), (amax / 448.0).view(E, n // 128, k // 128)


def group_quant(x):
    v = x.reshape(-1, 128)
    s = v.abs().amax(-1, keepdim=True).clamp(min=1e-10).float() / 448.0
    return (v / s).clamp(-448, 448).to(FP8).float().view(x.shape), s.view(*x.shape[:-1], -1)


def block_matmul(aq, As, w, ws, dtype):
    """native_w8a8_block_matmul: fp32 product of the dequantised blocks, cast once."""
    ad = aq.view(aq.shape[0], -1, 128) * As[..., None]
    wd = w.float().view(w.shape[0] // 128, 128, -1, 128) * ws[:, None, :, None]
    return (ad.view(aq.shape[0], -1) @ wd.view(w.shape[0], -1).t()).to(dtype)


def ref_moe(a, w1, w2, w1_s, w2_s, topk_w, topk_ids, expert_map=None):
    """torch_w8a8_block_fp8_moe of the reference's test, in plain torch; an expert the map drops, and an id
    outside the global experts, add nothing."""
    B, topk = topk_ids.shape
    flat = topk_ids.view(-1).long()
    n = w1.shape[0] if expert_map is None else expert_map.numel()
    ok = (flat >= 0) & (flat < n)
    flat = flat.clamp(0, n - 1)
    flat = torch.where(ok, flat if expert_map is None else expert_map[flat].long(), -1)
    rep = a.repeat_interleave(topk, 0)
    out = torch.zeros((B * topk, w2.shape[1]), dtype=a.dtype, device=a.device)
    aq, a_s = group_quant(rep)
    for e in range(w1.shape[0]):
        m = flat == e
        if m.any():
            h = block_matmul(aq[m], a_s[m], w1[e], w1_s[e], a.dtype)
            d = h.shape[1] // 2
            hq, h_s = group_quant(F.silu(h[:, :d]) * h[:, d:])
            out[m] = block_matmul(hq, h_s, w2[e], w2_s[e], a.dtype)
    return (out.view(B, topk, -1) * topk_w.view(B, topk, 1).to(a.dtype)).sum(1)


@pytest.mark.parametrize("M,N,K,E,topk,inplace,local", [
    (1, 256, 128, 2, 1, False, None), (33, 512, 384, 8, 2, True, None), (83, 256, 1152, 8, 6, False, (1, 2, 3, 4, 5, 6, 7)),
    (9, 256, 384, 8, 2, False, (5, 7))])
def test_fused_experts(ops, M, N, K, E, topk, inplace, local):
    """The reference test's recipe (randn / 10 activations, randn / 15 weights quantised per 128 x 128 block, softmax
    top-k routing without renormalisation) and its tolerance.  `local`: the experts of this rank under an
    expert_map; with 2 of 8 the ids are aligned for 8 experts (up to 8 x 16 padded entries) while the weights show 2
    (18 + 2 x 15 = 48 entries would cut real work), and one id there is outside the global experts.  The third case
    also captures the whole call in one graph and replays it twice, with topk_ids changed in place, against eager
    bit for bit."""
    from vllm_amd.model_executor.layers.fused_moe import fused_experts
    torch.manual_seed(0)
    dt = torch.bfloat16
    a = torch.randn((M, K), dtype=dt, device="cuda") / 10
    w1, w1_s = block_quant(torch.randn((E, 2 * N, K), dtype=dt, device="cuda") / 15)
    w2, w2_s = block_quant(torch.randn((E, K, N), dtype=dt, device="cuda") / 15)
    topk_w, topk_ids = torch.randn((M, E), device="cuda").softmax(-1).topk(topk, dim=-1)
    topk_ids = topk_ids.to(torch.int32)
    emap = None
    if local:
        emap = torch.full((E,), -1, device="cuda", dtype=torch.int32)
        emap[list(local)] = torch.arange(len(local), device="cuda", dtype=torch.int32)
        w1, w1_s, w2, w2_s = (t[list(local)] for t in (w1, w1_s, w2, w2_s))
        if len(local) == 2:
            topk_ids[0, 0] = E
    drop = local is not None and len(local) > 2
    kw = dict(use_fp8_w8a8=True, w1_scale=w1_s, w2_scale=w2_s, block_shape=[128, 128], global_num_experts=E,
              expert_map=emap)
    ref = ref_moe(a, w1, w2, w1_s, w2_s, topk_w, topk_ids, emap)
    x = a.clone()
    out = fused_experts(x, w1, w2, topk_w, topk_ids, inplace=inplace, **kw)
    assert (out.data_ptr() == x.data_ptr()) == inplace
    torch.testing.assert_close(out, ref, atol=0.035, rtol=0.035)
    if not drop:
        return
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


def test_fused_experts_refusals(ops):
    from vllm_amd.model_executor.layers.fused_moe import fused_experts
    t = torch.zeros((1, 128), dtype=torch.bfloat16, device="cuda")
    for bad in (dict(use_fp8_w8a8=False), dict(block_shape=[64, 64]), dict(activation="gelu"), dict(a1_scale=t),
                dict(use_int8_w8a8=True)):
        with pytest.raises(NotImplementedError, match=next(iter(bad))):
            fused_experts(t, t, t, t, t, **{"use_fp8_w8a8": True, "block_shape": [128, 128], **bad})


def test_opcheck_moe_ops(ops):
    E, bm, top_k, N, K = 8, 16, 2, 256, 256
    ids = torch.tensor([[0, 5], [3, 1], [6, 2]], dtype=torch.int32, device="cuda")   # one slot per expert: one order
    n = ids.numel() + E * (bm - 1)
    sorted_ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    expert_ids = torch.zeros(-(-n // bm), dtype=torch.int32, device="cuda")
    post = torch.zeros(1, dtype=torch.int32, device="cuda")
    opcheck(torch.ops._moe_C.moe_align_block_size, (ids.view(-1), E, bm, sorted_ids, expert_ids, post))
    ops.moe_align_block_size(ids.view(-1), E, bm, sorted_ids, expert_ids, post)
    a = torch.randn((3, K), device="cuda").to(FP8)
    b = torch.randn((E, N, K), device="cuda").to(FP8)
    As, Bs = torch.rand((3, K // 128), device="cuda"), torch.rand((E, N // 128, K // 128), device="cuda")
    c = torch.zeros((6, N), dtype=torch.bfloat16, device="cuda")
    w = torch.rand(6, device="cuda")
    opcheck(torch.ops._C.moe_block_fp8_gemm, (c, a, b, As, Bs, w, sorted_ids, expert_ids, post, True, top_k, bm))
    opcheck(torch.ops._C.moe_block_fp8_gemm, (c, a, b, As, Bs, None, sorted_ids, expert_ids, post, False, top_k, bm))
    q = torch.zeros((6, N // 2), dtype=torch.uint8, device="cuda")
    opcheck(torch.ops._C.silu_and_mul_group_quant, (q, torch.zeros((6, 1), device="cuda"), c))
    opcheck(torch.ops._moe_C.moe_sum, (c.view(3, 2, N), torch.zeros((3, N), dtype=torch.bfloat16, device="cuda")))
