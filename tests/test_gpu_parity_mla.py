"""MLA decode (csrc/mla_decode.hip through decode_attention_fwd) against an fp64 reference computed from the
same 16-bit inputs: rows gathered through the block table, a plain softmax over each sequence's tokens,
the weighted sum of the rows' first 512 columns.

Bound, per element: |out - ref| <= u |ref| + (u + eps) A, with A = sum_t softmax_t |v_t| (fp64) and u one
output ulp (2^-8 bf16, 2^-11 fp16).  u |ref| is the output rounding; u A the probabilities' round-to-nearest
to the data type (the kernel, like the reference implementation, sums them BEFORE rounding and keeps every
probability <= 1 by subtracting the running maximum before the exponential: half an ulp in the numerator,
the other half is slack); eps = 2 delta + 2^-16 with delta = 578 * 2^-24 * sm_scale * max_t sum_i |q_i k_ti|
the worst fp32 logit error (it enters numerator and denominator through the exponential) and 2^-16 for the
fp32 accumulation over tiles and splits and the hardware exp2."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

T = 32                                   # the kernel's token tile
LENS = [0, 1, 3, T - 1, T, T + 1, 2 * T + 5, 4 * T]
SCALE = 576 ** -0.5
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def make_case(dtype, H, page, lens=LENS, seed=0, strided=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    B, nb = len(lens), max(-(-max(lens) // page), 1)
    pool = B * nb * 2 + 3                # more blocks than needed: a wrong page index reads a wrong row
    if strided:
        q = torch.randn(B, H + 1, 640, generator=g, device="cuda").to(dtype)[:, 1:, 32:608]
        cache = torch.randn(pool, page + 1, 576, generator=g, device="cuda").to(dtype)[:, :page]
    else:
        q = torch.randn(B, H, 576, generator=g, device="cuda").to(dtype)
        cache = torch.randn(pool, page, 576, generator=g, device="cuda").to(dtype)
    bt = torch.randperm(pool, generator=g, device="cuda")[:B * nb].view(B, nb).to(torch.int32)
    return q, cache, bt, torch.tensor(lens, dtype=torch.int32, device="cuda")


def reference(q, cache, bt, sl, scale=SCALE):
    """fp64 output, A and eps per (sequence, head[, column])"""
    page, B, H = cache.shape[1], q.shape[0], q.shape[1]
    ref = torch.zeros(B, H, 512, dtype=torch.float64, device="cuda")
    A, eps = torch.zeros_like(ref), torch.zeros(B, H, 1, dtype=torch.float64, device="cuda")
    for b, n in enumerate(sl.tolist()):
        if n == 0:
            continue
        tok = torch.arange(n, device="cuda")
        rows = cache[bt[b, tok // page].long(), tok % page].double()
        qb = q[b].double()
        p = torch.softmax(qb @ rows.T * scale, dim=-1)
        ref[b], A[b] = p @ rows[:, :512], p @ rows[:, :512].abs()
        delta = 578 * 2.0 ** -24 * scale * (qb.abs() @ rows.abs().T).amax(dim=-1, keepdim=True)
        eps[b] = 2 * delta + 2.0 ** -16
    return ref, A, eps


def check(out, ref, A, eps):
    u = ULP[out.dtype]
    err, bound = (out.double() - ref).abs(), u * ref.abs() + (u + eps) * A
    assert bool((err <= bound).all()), f"worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"


def run(q, cache, bt, sl, splits, scale=SCALE, o=None, logits=None):
    from vllm_amd.attention.ops.triton_decode_attention import decode_attention_fwd
    B, H = q.shape[0], q.shape[1]
    o = torch.full((B, H, 512), float("nan"), dtype=q.dtype, device="cuda") if o is None else o
    if logits is None:                   # poisoned: a read of an unwritten split shows
        logits = torch.full((B, H, splits, 513), float("nan"), dtype=torch.float32, device="cuda")
    kv = cache.unsqueeze(2)
    decode_attention_fwd(q, kv, kv[..., :512], o, bt, sl, logits, splits, scale, cache.shape[1])
    return o


@functools.lru_cache(maxsize=None)
def shared(dtype, H, page):
    case = make_case(dtype, H, page)
    return case, reference(*case)


@pytest.mark.parametrize("splits", [1, 4, 7])
@pytest.mark.parametrize("page", [1, 16, 64])
@pytest.mark.parametrize("H", [1, 16, 17, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_decode(dtype, H, page, splits):
    case, ref = shared(dtype, H, page)
    out = run(*case, splits)
    assert not bool(out[0].any()), "a sequence of length 0 gets a zero row"
    check(out, *ref)


@pytest.mark.parametrize("hpw", [16, 32])
def test_forced_heads_per_workgroup(hpw):
    from vllm_amd import _lib
    case, ref = shared(torch.bfloat16, 128, 16)
    _lib.set_tuning("mla_hpw", hpw)
    try:
        check(run(*case, 4), *ref)
    finally:
        _lib.set_tuning("mla_hpw", 0)


@pytest.mark.parametrize("splits", [1, 4])
def test_strided_q_and_cache(splits):
    case = make_case(torch.bfloat16, 17, 16, seed=1, strided=True)
    assert case[0].stride(1) == 640 and case[1].stride(0) == 17 * 576
    check(run(*case, splits), *reference(*case))


@pytest.mark.parametrize("kind", ["dominant", "equal"])
def test_extreme_logits(kind):
    q, cache, bt, sl = make_case(torch.float16, 16, 16, seed=2)
    if kind == "dominant":               # one key row far above the others, late in the longest sequence
        blk, off = int(bt[7, (3 * T + 7) // 16]), (3 * T + 7) % 16
        cache[blk, off] = (q[7, 3].float() * 4).to(cache.dtype)
    else:                                # all logits equal: ref is the mean of the latent rows
        q.zero_()
    check(run(q, cache, bt, sl, 4), *reference(q, cache, bt, sl))


def test_graph_replay_follows_lengths_and_table():
    q, cache, bt, sl = make_case(torch.bfloat16, 17, 16, seed=3)
    o = torch.zeros(len(LENS), 17, 512, dtype=q.dtype, device="cuda")
    logits = torch.empty(len(LENS), 17, 4, 513, dtype=torch.float32, device="cuda")
    run(q, cache, bt, sl, 4, o=o, logits=logits)   # warm up outside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(q, cache, bt, sl, 4, o=o, logits=logits)
    for shift in (1, 3, 1):
        sl.copy_(sl.roll(shift))
        bt.copy_(bt.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, run(q, cache, bt, sl, 4))


def test_backend_mirror_equals_the_op():
    from vllm_amd.v1.attention.backends.mla.triton_mla import forward_decode
    q, cache, bt, sl = make_case(torch.bfloat16, 16, 16, lens=[5, 70, 33], seed=4)
    o = forward_decode(q[..., :512], q[..., 512:], cache, bt, sl, SCALE)
    assert torch.equal(o, run(q, cache, bt, sl, 4))


def test_refused_forms_name_the_supported_one():
    from vllm_amd.attention.ops.triton_decode_attention import decode_attention_fwd
    q, cache, bt, sl = make_case(torch.bfloat16, 16, 16, lens=[5, 9])
    kv, o = cache.unsqueeze(2), torch.empty(2, 16, 512, dtype=q.dtype, device="cuda")
    lg = torch.empty(2, 16, 4, 513, dtype=torch.float32, device="cuda")
    with pytest.raises(NotImplementedError, match="MLA form"):
        decode_attention_fwd(q, kv, kv[..., :512], o, bt, sl, lg, 4, SCALE, 16, logit_cap=30.0)
    with pytest.raises(NotImplementedError, match="MLA form"):       # v is not a view of k
        decode_attention_fwd(q, kv, kv[..., :512].clone(), o, bt, sl, lg, 4, SCALE, 16)
    with pytest.raises(RuntimeError, match="row width 512 / 448.*supported form"):
        decode_attention_fwd(q[..., :512], kv[..., :512], kv[..., :448], o[..., :448], bt, sl, lg, 4, SCALE, 16)
    with pytest.raises(RuntimeError, match="dtype mismatch.*supported form"):
        decode_attention_fwd(q.half(), kv, kv[..., :512], o.half(), bt, sl, lg, 4, SCALE, 16)
    with pytest.raises(RuntimeError, match="must be int32"):
        decode_attention_fwd(q, kv, kv[..., :512], o, bt.long(), sl.long(), lg, 4, SCALE, 16)
    with pytest.raises(RuntimeError, match="num_kv_splits 0 < 1"):
        decode_attention_fwd(q, kv, kv[..., :512], o, bt, sl, lg[:, :, :0], 0, SCALE, 16)
    with pytest.raises(RuntimeError, match="scratch too small"):
        decode_attention_fwd(q, kv, kv[..., :512], o, bt, sl, lg[..., :512].contiguous(), 4, SCALE, 16)
    k8 = kv.view(torch.uint8)[..., :576]
    with pytest.raises(RuntimeError, match="fp8 latent cache.*supported form"):
        decode_attention_fwd(q, k8, k8[..., :512], o, bt, sl, lg, 4, SCALE, 16)
