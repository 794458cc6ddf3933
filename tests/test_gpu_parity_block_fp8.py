"""Block-scaled fp8 linear path on the GPU: per-token-group quantiser (bit-exact against the fp32
formula) and the 128 x 128 / 1 x 128 block-scaled GEMM (both launch forms) against fp64.

GEMM bound, derived: |out - ref| <= u |ref| + 2^-16 R, R = the same sum over |A|, |B|; u = one output
ulp (2^-8 bf16, 2^-11 f16).  Products of e4m3 values are exact in fp32; a block's 128-term fp32 sum,
the scale product, one FMA per block (and the fp32 bias add) cost at most (128 + K/128 + 5) 2^-24 R
<= 2^-16 R for K <= 16384."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def ref_gemm(a, b, As, Bs, bias=None):
    """fp64 (ref, R) from the exact fp8 values; a [M, K], b [N, K], As [M, K/128], Bs [ceil(N/128), K/128]."""
    M, K = a.shape
    N = b.shape[0]
    a3 = a.double().view(M, K // 128, 128).permute(1, 0, 2)                      # [kb, M, 128]
    b3 = b.double().view(N, K // 128, 128).permute(1, 2, 0)                      # [kb, 128, N]
    s = As.double().t()[:, :, None] * Bs.double().t().repeat_interleave(128, 1)[:, None, :N]   # [kb, M, N]
    ref = (s * (a3 @ b3)).sum(0)
    R = (s.abs() * (a3.abs() @ b3.abs())).sum(0)
    return (ref if bias is None else ref + bias.double()), R


def check_bound(out, ref, R, dtype):
    err = (out.double() - ref).abs()
    bound = U[dtype] * ref.abs() + 2.0 ** -16 * R
    worst = (err - bound).max().item()
    print(f"max err {err.max().item():.3e}, max err - bound {worst:.3e}")
    assert worst <= 0


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K):
    """Data as in the reference's test_block_fp8.py: fp8 values over the whole e4m3 range, scales rand * 1e-2."""
    g = torch.Generator(device="cuda").manual_seed(M * 7919 + N * 31 + K)
    rnd = lambda *shape: torch.rand(shape, device="cuda", generator=g)
    a = ((rnd(M, K) - 0.5) * 2 * 448).clamp(-448, 448).to(FP8)
    b = ((rnd(N, K) - 0.5) * 2 * 448).clamp(-448, 448).to(FP8)
    As, Bs = rnd(M, K // 128) * 1e-2, rnd((N + 127) // 128, K // 128) * 1e-2
    bias = (rnd(N) - 0.5) * 100 if N == 576 else None
    return a, b, As, Bs, bias, ref_gemm(a, b, As, Bs, bias)


@pytest.mark.parametrize("as_col_major", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", [(128, 128), (576, 384), (200, 1024), (1536, 2304)])
@pytest.mark.parametrize("M", [1, 16, 17, 32, 33, 129, 300])
def test_block_gemm_vs_fp64(ops, M, N, K, dtype, as_col_major):
    a, b, As, Bs, bias, (ref, R) = gemm_case(M, N, K)
    if as_col_major:
        As = As.t().contiguous().t()
    bias_d = None if bias is None else bias.to(dtype)
    if bias is not None:
        ref = ref - bias.double() + bias_d.double()
    out = ops.cutlass_scaled_mm(a, b.t(), As, Bs.t(), dtype, bias_d)
    assert out.shape == (M, N) and out.dtype == dtype
    check_bound(out, ref, R, dtype)


@pytest.fixture
def tile_form(request):
    """Tuning key mm_block_kernel: 0 = the form the launcher picks by M, 2 / 3 = the 128- / 256-row tile kernel (the
    launcher takes 256-row tiles from 190 of them on: M 4096 at N >= 768)."""
    from vllm_amd import _lib
    _lib.set_tuning("mm_block_kernel", request.param)
    yield request.param
    _lib.set_tuning("mm_block_kernel", 0)


@pytest.mark.parametrize("tile_form", [2, 3], indirect=True)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,K", [(576, 384), (204, 256), (1536, 2304)])
@pytest.mark.parametrize("M", [70, 300])
def test_block_gemm_tile_forms_vs_fp64(ops, tile_form, M, N, K, dtype):
    """Both tile kernels forced, at sizes with partial and several 128- and 256-row tiles; N 204 ends in a
    4-element piece (element-wise store tail), and the second call writes rows of an odd stride (no
    16-byte stores at all)."""
    a, b, As, Bs, bias, (ref, R) = gemm_case(M, N, K)
    bias_d = None if bias is None else bias.to(dtype)
    if bias is not None:
        ref = ref - bias.double() + bias_d.double()
    check_bound(ops.cutlass_scaled_mm(a, b.t(), As, Bs.t(), dtype, bias_d), ref, R, dtype)
    wide = torch.zeros((M, N + 1), dtype=dtype, device="cuda")
    torch.ops._C.cutlass_scaled_mm(wide[:, :N], a, b.t(), As, Bs.t(), bias_d)
    check_bound(wide[:, :N], ref, R, dtype)
    assert not wide[:, N].any()


@pytest.mark.parametrize("M,tile_form", [(7, 0), (160, 0), (160, 3), (300, 3)], indirect=["tile_form"])
def test_block_gemm_integer_exact(ops, M, tile_form):
    """Small integers and power-of-two scales: every partial, scale product and running sum is exact in
    fp32 and below 65504, so the f16 output equals the rounded fp64 result bit for bit -- a scale read
    from the wrong row, block or stride shows.  Streaming, 128-row and (forced) 256-row kernels."""
    N, K = 384, 512
    g = torch.Generator(device="cuda").manual_seed(M)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, device="cuda", generator=g)
    a, b = ri(-3, 3, M, K).float().to(FP8), ri(-2, 2, N, K).float().to(FP8)
    As = (2.0 ** ri(-2, 1, K // 128, M).float()).t()          # token-contiguous
    Bs = 2.0 ** ri(-2, 1, N // 128, K // 128).float()
    ref, _ = ref_gemm(a, b, As, Bs)
    out = ops.cutlass_scaled_mm(a, b.t(), As, Bs.t(), torch.float16)
    assert torch.equal(out, ref.to(torch.float16))


def ref_group_quant(x, g, ue8m0, eps=1e-10):
    """The formula in fp32 on the host: (codes as uint8, scales)."""
    x3 = x.float().cpu().view(x.shape[0], -1, g)
    s = x3.abs().amax(-1).clamp(min=eps) / 448.0
    if ue8m0:
        m, e = torch.frexp(s.abs().clamp(min=1e-10))                    # s = m 2^e, m in [0.5, 1)
        s = torch.ldexp(torch.ones_like(s), torch.where(m == 0.5, e - 1, e))
    q = (x3 / s[..., None]).clamp(-448.0, 448.0).to(FP8)
    return q.view(x.shape).view(torch.uint8), s


@pytest.mark.parametrize("ue8m0", [False, True])
@pytest.mark.parametrize("col_major", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("g", [64, 128])
@pytest.mark.parametrize("tokens,hidden", [(1, 128), (7, 512), (33, 1536)])
def test_group_quant_bit_exact(ops, tokens, hidden, g, dtype, col_major, ue8m0):
    from vllm_amd.quantization.fp8_utils import per_token_group_quant_fp8
    gen = torch.Generator().manual_seed(tokens * hidden + g)
    x = torch.randn((tokens, hidden), generator=gen) * torch.rand((tokens, 1), generator=gen) * 8
    x[0, :g] = 0.0                                                       # scale eps / 448
    x[-1, -g:] = 448.0 * torch.randint(-3, 4, (g,), generator=gen)       # +-448 k: must saturate
    x = x.to(dtype).cuda()
    q, s = per_token_group_quant_fp8(x, g, column_major_scales=col_major, use_ue8m0=ue8m0)
    assert s.shape == (tokens, hidden // g) and (not col_major or s.stride(0) == 1)
    q_ref, s_ref = ref_group_quant(x, g, ue8m0)
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(q.cpu().view(torch.uint8), q_ref)


def test_linear_plumbing(ops):
    from vllm_amd.quantization.fp8_utils import (apply_w8a8_block_fp8_linear, per_token_group_quant_fp8,
                                                 w8a8_block_fp8_matmul)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((2, 5, 512), device="cuda", generator=g).to(torch.bfloat16)
    w = ((torch.rand((384, 512), device="cuda", generator=g) - 0.5) * 896).to(FP8)
    ws = torch.rand((3, 4), device="cuda", generator=g) * 1e-2
    bias = torch.randn(384, device="cuda", generator=g).to(torch.bfloat16)
    out = apply_w8a8_block_fp8_linear(x, w, [128, 128], ws, bias=bias)
    assert out.shape == (2, 5, 384) and out.dtype == torch.bfloat16
    q, s = per_token_group_quant_fp8(x.view(10, 512), 128)
    ref, R = ref_gemm(q, w, s, ws, bias)
    check_bound(out.view(10, 384), ref, R, torch.bfloat16)
    # the reference's [N, K] / [N/128, K/128] argument order == the op on the transposed views
    y = w8a8_block_fp8_matmul(q.view(2, 5, 512), w, s.view(2, 5, 4), ws, [128, 128], torch.float16)
    assert torch.equal(y.view(10, 384), ops.cutlass_scaled_mm(q, w.t(), s, ws.t(), torch.float16))


def test_contract(ops):
    M, N, K = 40, 256, 512
    a, b, As, Bs, _, _ = gemm_case(M, N, K)
    with pytest.raises(RuntimeError, match="per-tensor.*per-token.*blockwise"):
        ops.cutlass_scaled_mm(a, b.t(), As[:, :3].contiguous(), Bs.t(), torch.bfloat16)
    # empty inputs
    assert ops.cutlass_scaled_mm(a[:0], b.t(), As[:0], Bs.t(), torch.bfloat16).shape == (0, N)
    from vllm_amd.quantization.fp8_utils import per_token_group_quant_fp8
    q, s = per_token_group_quant_fp8(torch.empty((0, 256), device="cuda", dtype=torch.bfloat16), 128)
    assert q.shape == (0, 256) and s.shape == (0, 2)
    # one GEMM captured in a graph (a single linear chain), replayed twice == eager, bit for bit
    eager = ops.cutlass_scaled_mm(a, b.t(), As, Bs.t(), torch.bfloat16)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        torch.ops._C.cutlass_scaled_mm(out, a, b.t(), As, Bs.t(), None)
    for _ in range(2):
        out.fill_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    # opcheck; the codes go to a uint8 tensor (the op takes either), which opcheck can compare
    x = torch.randn((5, 256), device="cuda", dtype=torch.bfloat16)
    torch.library.opcheck(
        torch.ops._C.per_token_group_fp8_quant,
        (x, torch.zeros((5, 256), dtype=torch.uint8, device="cuda"), torch.zeros((5, 2), device="cuda"), 128, 1e-10,
         -448.0, 448.0, False),
        test_utils=("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic"),
        raise_exception=True)
