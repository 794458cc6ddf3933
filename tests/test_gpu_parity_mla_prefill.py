"""MLA prefill (csrc/mla_prefill.hip, gather_cache in csrc/cache_kernels.hip) against fp64 references computed on the
GPU from the same 16-bit inputs: a plain masked softmax per (sequence, head).

The kernel's tiles are 256 query rows by 64 keys; the lengths below sit on both edges.  Bound, per element, the
derived form of test_gpu_parity_mla.py: |out - ref| <= u |ref| + (u + eps) A with A = sum_j p_j |v_j| (fp64), u one
output ulp, eps = 2 delta + 2^-16, delta = 194 * 2^-24 * scale * max_j sum_i |q_i k_ji| (the fp32 error of a
192-term logit); |lse - ref| <= eps + 2^-23 |ref|.  The end-to-end test keeps that bound: each partial output is
rounded once more before the merge, (u / 2) sum_parts w_part |o_part| <= (u / 2) A, which is the half of u A that the
single-pass derivation leaves as slack."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EDGE = [1, 63, 64, 65, 255, 256, 257, 300]
SK = [0, 1, 64, 65, 130]
BATCHES = {"causal": (EDGE, EDGE, True), "context": (EDGE, [SK[i % len(SK)] for i in range(len(EDGE))], False),
           "bottom_right": ([65], [130], True)}
SCALE = 192 ** -0.5
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.bfloat16, torch.float16]


def cu(lens):
    return torch.tensor([0] + lens, device="cuda").cumsum(0).to(torch.int32)


def attention_ref(q, k, v, sq, sk, causal, scale=SCALE):
    """fp64 out [Tq, H, 128], A, eps [Tq, H, 1], lse [H, Tq]; k [Tk, H, 192]"""
    Tq, H = q.shape[:2]
    ref = torch.zeros(Tq, H, 128, dtype=torch.float64, device="cuda")
    A, eps = torch.zeros_like(ref), torch.zeros(Tq, H, 1, dtype=torch.float64, device="cuda")
    lse = torch.full((H, Tq), float("-inf"), dtype=torch.float64, device="cuda")
    q0 = k0 = 0
    for nq, nk in zip(sq, sk):
        qb, kb, vb = (t.double().transpose(0, 1) for t in (q[q0:q0 + nq], k[k0:k0 + nk], v[k0:k0 + nk]))
        vis = torch.ones(nq, nk, dtype=torch.bool, device="cuda")
        if causal:                           # bottom-right aligned
            vis = torch.arange(nk, device="cuda")[None, :] <= torch.arange(nq, device="cuda")[:, None] + (nk - nq)
        s = (qb @ kb.transpose(1, 2) * scale).masked_fill(~vis, float("-inf"))
        l = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - l.masked_fill(l == float("-inf"), 0)[..., None])
        ref[q0:q0 + nq], A[q0:q0 + nq] = (p @ vb).transpose(0, 1), (p @ vb.abs()).transpose(0, 1)
        lse[:, q0:q0 + nq] = l
        if nk:
            worst = (qb.abs() @ kb.abs().transpose(1, 2)).masked_fill(~vis, 0).amax(dim=-1)
            eps[q0:q0 + nq] = (2 * 194 * 2.0 ** -24 * scale * worst + 2.0 ** -16).transpose(0, 1)[..., None]
        q0, k0 = q0 + nq, k0 + nk
    return ref, A, eps, lse


def check(out, lse, ref, A, eps, ref_lse):
    u = ULP[out.dtype]
    err, bound = (out.double() - ref).abs(), u * ref.abs() + (u + eps) * A
    assert bool((err <= bound).all()), f"worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
    if lse is not None:
        empty = ref_lse == float("-inf")
        assert bool((lse[empty] == float("-inf")).all()) and not bool(out[empty.T].any())
        lerr = (lse.double() - ref_lse)[~empty].abs()
        assert bool((lerr <= (eps[..., 0].T + 2.0 ** -23 * ref_lse.abs())[~empty]).all()), float(lerr.max())


@functools.lru_cache(maxsize=None)
def shared(dtype, H, batch):
    sq, sk, causal = BATCHES[batch]
    g = torch.Generator(device="cuda").manual_seed(len(batch) + H)
    q = torch.randn(sum(sq), H, 192, generator=g, device="cuda").to(dtype)
    kv = torch.randn(sum(sk), H, 256, generator=g, device="cuda").to(dtype)     # kv_b_proj's output: [k_nope | v]
    k_pe = torch.randn(sum(sk), 1, 64, generator=g, device="cuda").to(dtype)
    k = torch.cat([kv[..., :128], k_pe.expand(-1, H, -1)], dim=-1)
    return (q, kv, k_pe, k), attention_ref(q, k, kv[..., 128:], sq, sk, causal)


@pytest.mark.parametrize("form", ["concatenated", "split"])
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention(dtype, H, batch, form):
    from vllm_amd import _lib
    (q, kv, k_pe, k), ref = shared(dtype, H, batch)
    sq, sk, causal = BATCHES[batch]
    out = torch.full((q.shape[0], H, 128), float("nan"), dtype=dtype, device="cuda")
    lse = torch.full((H, q.shape[0]), float("nan"), dtype=torch.float32, device="cuda")
    kn, kp, kp_sh = (k, k[..., 128:], k.stride(1)) if form == "concatenated" else (kv, k_pe, 0)
    v, cq, ck = kv[..., 128:], cu(sq), cu(sk)
    _lib.check(_lib.lib.vllm_amd_mla_prefill_attention(
        out.data_ptr(), lse.data_ptr(), q.data_ptr(), kn.data_ptr(), kp.data_ptr(), v.data_ptr(), cq.data_ptr(),
        ck.data_ptr(), len(sq), q.shape[0], H, 192, 128, 64, max(sq), SCALE, int(causal), q.stride(0), q.stride(1),
        out.stride(0), out.stride(1), kn.stride(0), kn.stride(1), kp.stride(0), kp_sh, v.stride(0), v.stride(1),
        q.shape[0], _lib.F16 if dtype == torch.float16 else _lib.BF16, torch.cuda.current_stream().cuda_stream))
    check(out, lse, *ref)


@pytest.mark.parametrize("D", [128, 200])
@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_attn_states(dtype, D):
    from vllm_amd.attention.ops.merge_attn_states import merge_attn_states
    T, H, inf = 37, 3, float("inf")
    g = torch.Generator(device="cuda").manual_seed(D)
    po, so = (torch.randn(T, H, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    # lse in [3, 9], the range of a log-sum over some tens to thousands of keys: the fp32 error of log(s) + m is at most
    # 2^-24 (|m| + 2 ln 2 + |lse|) < 2^-24 * 20.1, inside 2^-20 |lse| for |lse| >= 3 (near 0 no fp32 result could be)
    pl, sl = (torch.rand(H, T, generator=g, device="cuda") * 6 + 3 for _ in range(2))
    pl[:, 3], sl[:, 5], pl[:, 7], sl[:, 7] = -inf, inf, -inf, -inf      # empty prefix, FA2's empty suffix, both empty
    out = torch.full_like(po, float("nan"))
    lse = torch.full_like(pl, float("nan"))
    merge_attn_states(out, po, pl, so, sl, lse)
    p64, s64 = pl.double(), sl.double().masked_fill(sl == inf, -inf)
    ref_lse = torch.logaddexp(p64, s64)
    both = ref_lse == -inf
    wp, ws = (torch.exp(x - ref_lse.masked_fill(both, 0)).T[..., None] for x in (p64, s64))
    ref = po.double() * wp + so.double() * ws
    bound = ULP[dtype] * ref.abs() + 2.0 ** -20 * (po.double().abs() + so.double().abs())
    assert bool(((out.double() - ref).abs() <= bound).all())
    assert not bool(out[both.T].any()) and bool((lse[both] == -inf).all())
    assert bool(((lse.double() - ref_lse)[~both].abs() <= 2.0 ** -20 * ref_lse[~both].abs()).all())


@pytest.mark.parametrize("starts", [False, True])
@pytest.mark.parametrize("page", [1, 16, 64])
def test_gather_cache(ops, page, starts):
    lens = [0, 1, page - 1, page, page + 1, 5 * page + 3]
    B, first, tot = len(lens), [0, 2, 1, 0, 3, 1], sum(lens)
    g = torch.Generator(device="cuda").manual_seed(page)
    nb = max(f + -(-n // page) for f, n in zip(first, lens))
    pool = B * nb * 2 + 3                # larger than needed and permuted: a wrong block index reads a wrong row
    cache = torch.randn(pool, page, 576, generator=g, device="cuda").to(torch.bfloat16)
    bt = torch.randperm(pool, generator=g, device="cuda")[:B * nb].view(B, nb).to(torch.int32)
    ss = torch.tensor([f * page for f in first], dtype=torch.int32, device="cuda") if starts else None
    rows = torch.cat([bt[b, (first[b] if starts else 0) + torch.arange(n, device="cuda") // page].long() * page
                      + torch.arange(n, device="cuda") % page for b, n in enumerate(lens)])
    dst = torch.full((tot + 5, 640), 7.0, dtype=torch.bfloat16, device="cuda")[:, :576]   # a row stride above the entry
    ops.gather_cache(cache, dst, bt, cu(lens), B, ss)
    assert torch.equal(dst[:tot], cache.view(-1, 576)[rows]) and bool((dst[tot:] == 7).all())
    c8 = torch.randn(pool, page, 576, generator=g, device="cuda").to(torch.float8_e4m3fn)
    scale = torch.tensor([0.37], device="cuda")
    for dtype in DTYPES:
        d16 = torch.full((tot + 5, 576), 7.0, dtype=dtype, device="cuda")
        ops.gather_cache(c8, d16, bt, cu(lens), B, ss, scale=scale)
        want = (c8.view(torch.uint8).view(-1, 576)[rows].view(torch.float8_e4m3fn).float() * scale).to(dtype)
        assert torch.equal(d16[:tot], want) and bool((d16[tot:] == 7).all())
    if page == 16 and starts:
        odd = torch.full((tot, 571), 7.0, dtype=torch.bfloat16, device="cuda")   # no 16-byte vectors: the element path
        ops.gather_cache(cache[..., :571], odd, bt, cu(lens), B, ss)
        assert torch.equal(odd, cache.view(-1, 576)[rows, :571])
        torch.library.opcheck(torch.ops._C_cache_ops.gather_cache, (cache, dst, bt, cu(lens), B, ss), raise_exception=True,
                              test_utils=("test_schema", "test_autograd_registration", "test_faketensor",
                                          "test_aot_dispatch_dynamic"))


def test_forward_prefill_with_chunked_context():
    from vllm_amd.v1.attention.backends.mla.common import ChunkedContext, forward_prefill
    dtype, H, page, ctx, new, chunk = torch.bfloat16, 2, 16, [0, 70], [65, 33], 48
    g = torch.Generator(device="cuda").manual_seed(11)
    W = torch.randn(512, H * 256, generator=g, device="cuda", dtype=torch.float64) / 512 ** 0.5
    kv_b_proj = lambda x: (x.double() @ W).to(dtype)     # fp64: the rows do not depend on how they are batched
    latent = torch.randn(sum(ctx) + sum(new), 576, generator=g, device="cuda").to(dtype)   # seq 1's context, then the new tokens
    q = torch.randn(sum(new), H, 192, generator=g, device="cuda").to(dtype)
    cache = torch.zeros(9, page, 576, dtype=dtype, device="cuda")
    bt = torch.tensor([[0, 0, 0, 0, 0], [7, 2, 5, 1, 8]], dtype=torch.int32, device="cuda")
    cache[bt[1].long()] = torch.cat([latent[:70], latent[:10]]).view(5, page, 576)
    pieces = [[min(max(c - i * chunk, 0), chunk) for c in ctx] for i in range(2)]
    context = ChunkedContext(cache, bt, [cu(p) for p in pieces],
                             [torch.full((2,), i * chunk, dtype=torch.int32, device="cuda") for i in range(2)],
                             [sum(p) for p in pieces], [max(p) for p in pieces],
                             torch.empty(chunk + 3, 576, dtype=dtype, device="cuda"), kv_b_proj)
    fresh = latent[70:]
    out = forward_prefill(q, kv_b_proj(fresh[:, :512]), fresh[:, None, 512:], cu(new), max(new), SCALE, context)
    # reference: every sequence's keys are its context followed by its new tokens, causal bottom-right
    order = torch.cat([latent[70:135], latent[:70], latent[135:]])
    kv = kv_b_proj(order[:, :512]).view(-1, H, 256)
    k = torch.cat([kv[..., :128], order[:, None, 512:].expand(-1, H, -1)], dim=-1)
    ref, A, eps, _ = attention_ref(q, k, kv[..., 128:], new, [c + n for c, n in zip(ctx, new)], True)
    check(out.view(-1, H, 128), None, ref, A, eps, None)
