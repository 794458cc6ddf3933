"""MLA decode over the fp8 (e4m3fn) latent cache (mla_decode_fp8_kernel through decode_attention_fwd with
k_scale) against the fp64 reference of test_gpu_parity_mla.py on the cache's exact values, float(byte) *
kv_scale.  The bound is that test's, u |ref| + (u + eps) A: the widening is exact and the arithmetic is the
same, except that its delta takes 580 in place of 578 for the two fp32 roundings of the folded scale."""
import functools

import pytest
import torch

from test_gpu_parity_mla import SCALE, ULP, check, make_case, reference

pytestmark = pytest.mark.gpu

T = 64                                   # the fp8 kernel's token tile
LENS = [0, 1, 3, T - 1, T, T + 1, 2 * T + 5, 4 * T]
KV_SCALE = {1: 1.0, 16: 0.037, 64: 0.037}   # by page size


def make_case8(dtype, H, page, kv_scale, lens=LENS, seed=0, strided=False):
    """q, block table and lengths of make_case; a byte cache of quantised randn / kv_scale rows (no NaN byte)"""
    q, cache, bt, sl = make_case(dtype, H, page, lens, seed, strided)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    pool = cache.shape[0]
    rows = (torch.randn(pool, page, 576, generator=g, device="cuda") / kv_scale).to(torch.float8_e4m3fn)
    if strided:                          # entry stride 592 bytes, block stride (page + 1) * 592
        c8 = torch.zeros(pool, page + 1, 592, dtype=torch.uint8, device="cuda")[:, :page, :576]
        c8.copy_(rows.view(torch.uint8))
    else:
        c8 = rows.view(torch.uint8)
    return q, c8, bt, sl, torch.tensor([kv_scale], dtype=torch.float32, device="cuda")


def reference8(q, c8, bt, sl, ks):
    values = c8.contiguous().view(torch.float8_e4m3fn).float().double() * ks.double()
    ref, A, eps = reference(q, values, bt, sl)
    return ref, A, (eps - 2.0 ** -16) * (580 / 578) + 2.0 ** -16


def run8(q, c8, bt, sl, ks, splits, o=None, logits=None):
    from vllm_amd.attention.ops.triton_decode_attention import decode_attention_fwd
    B, H = q.shape[0], q.shape[1]
    o = torch.full((B, H, 512), float("nan"), dtype=q.dtype, device="cuda") if o is None else o
    if logits is None:                   # poisoned: a read of an unwritten split shows
        logits = torch.full((B, H, splits, 513), float("nan"), dtype=torch.float32, device="cuda")
    kv = c8.unsqueeze(2)
    decode_attention_fwd(q, kv, kv[..., :512], o, bt, sl, logits, splits, SCALE, c8.shape[1], k_scale=ks)
    return o


@functools.lru_cache(maxsize=None)
def shared(dtype, H, page):
    case = make_case8(dtype, H, page, KV_SCALE[page])
    return case, reference8(*case)


@pytest.mark.parametrize("splits", [1, 4, 7])
@pytest.mark.parametrize("page", [1, 16, 64])
@pytest.mark.parametrize("H", [1, 16, 17, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_decode(dtype, H, page, splits):
    case, ref = shared(dtype, H, page)
    out = run8(*case, splits)
    assert not bool(out[0].any()), "a sequence of length 0 gets a zero row"
    check(out, *ref)


@pytest.mark.parametrize("hpw", [16, 32])
def test_forced_heads_per_workgroup(hpw):
    from vllm_amd import _lib
    case, ref = shared(torch.bfloat16, 128, 16)
    _lib.set_tuning("mla_hpw", hpw)
    try:
        check(run8(*case, 4), *ref)
    finally:
        _lib.set_tuning("mla_hpw", 0)


@pytest.mark.parametrize("splits", [1, 4])
def test_strided_q_and_padded_rows(splits):
    case = make_case8(torch.bfloat16, 17, 16, 0.037, seed=1, strided=True)
    assert case[0].stride(1) == 640 and case[1].stride(1) == 592 and case[1].stride(0) == 17 * 592
    check(run8(*case, splits), *reference8(*case))


def test_written_cache_is_what_decode_reads(ops):
    q, cache, bt, sl = make_case(torch.bfloat16, 16, 16, lens=[40, 7, 64], seed=5)
    ks = torch.tensor([0.037], device="cuda")
    direct = torch.empty(cache.shape, dtype=torch.uint8, device="cuda")
    ops.convert_fp8(direct, cache, 0.037, "fp8")
    written = torch.zeros_like(direct)
    for b, n in enumerate(sl.tolist()):  # the tokens of every sequence, through its block table
        tok = torch.arange(n, device="cuda")
        slots = bt[b, tok // 16].long() * 16 + tok % 16
        rows = cache.view(-1, 576)[slots]
        ops.concat_and_cache_mla(rows[:, :512], rows[:, 512:], written, slots, "fp8", ks)
    assert torch.equal(run8(q, written, bt, sl, ks, 4), run8(q, direct, bt, sl, ks, 4))


def test_graph_replay_follows_lengths_and_table():
    q, c8, bt, sl, ks = make_case8(torch.bfloat16, 17, 16, 0.037, seed=3)
    o = torch.zeros(len(LENS), 17, 512, dtype=q.dtype, device="cuda")
    logits = torch.empty(len(LENS), 17, 4, 513, dtype=torch.float32, device="cuda")
    run8(q, c8, bt, sl, ks, 4, o=o, logits=logits)   # warm up outside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run8(q, c8, bt, sl, ks, 4, o=o, logits=logits)
    for shift in (1, 3, 1):
        sl.copy_(sl.roll(shift))
        bt.copy_(bt.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, run8(q, c8, bt, sl, ks, 4))


def test_backend_mirror_equals_the_op():
    from vllm_amd.v1.attention.backends.mla.triton_mla import forward_decode
    q, c8, bt, sl, ks = make_case8(torch.bfloat16, 16, 16, 0.037, lens=[5, 70, 33], seed=4)
    o = forward_decode(q[..., :512], q[..., 512:], c8, bt, sl, SCALE, kv_cache_dtype="fp8", k_scale=ks)
    assert torch.equal(o, run8(q, c8, bt, sl, ks, 4))
    with pytest.raises(NotImplementedError, match="FP8"):
        forward_decode(q[..., :512], q[..., 512:], c8, bt, sl, SCALE, kv_cache_dtype="fp8")


def test_refused_forms_name_the_supported_one():
    q, c8, bt, sl, ks = make_case8(torch.bfloat16, 16, 16, 1.0, lens=[5, 9])
    with pytest.raises(RuntimeError, match="k_scale with a torch.bfloat16 cache.*supported form"):
        run8(q, c8.to(torch.bfloat16), bt, sl, ks, 4)
    odd = torch.zeros(c8.shape[0], 16, 584, dtype=torch.uint8, device="cuda")[..., :576]
    with pytest.raises(RuntimeError, match="multiples of 16.*supported form"):
        run8(q, odd, bt, sl, ks, 4)
    for bad in (ks.double(), ks.repeat(2)):
        with pytest.raises(RuntimeError, match="k_scale is.*supported form"):
            run8(q, c8, bt, sl, bad, 4)
