"""concat_and_cache_mla (csrc/cache_kernels.hip): bit-exact against the inputs ("auto") or against
ops.convert_fp8 of the concatenated inputs (fp8; that op is pinned bit-exact in
test_gpu_parity_cache_quant.py), untouched rows keep a sentinel, and the layout is the one
decode_attention_fwd reads."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


def make_inputs(dtype, tokens, widths, strided, scale, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rank, pe = widths
    rows = tokens + 3                    # kv_c / k_pe are longer than slot_mapping (graph padding)
    x = torch.randn(rows, rank + pe + 8, generator=g, device="cuda") * (100 * scale)
    x[0, :6] = torch.tensor([0.0, -0.0, 1e4 * scale, -1e4 * scale, 2.0 ** -8 * scale, -2.0 ** -9 * scale])
    x = x.to(dtype)                      # +-0, beyond +-448 scale, subnormal fp8 results
    if strided:                          # slices of one fused projection output
        return x[:, :rank], x[:, rank:rank + pe]
    return x[:, :rank].contiguous(), x[:, rank:rank + pe].contiguous()


def make_slots(tokens, block_size, num_blocks, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    slots = torch.randperm(num_blocks * block_size, generator=g, device="cuda")[:tokens]
    if tokens > 2:
        slots[tokens // 2] = -1          # a padded token
    return slots


@pytest.mark.parametrize("kv,scale", [("auto", 1.0), ("fp8", 1.0), ("fp8_e4m3", 0.037)])
@pytest.mark.parametrize("widths", [(512, 64), (64, 8)])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("block_size", [1, 16, 64])
@pytest.mark.parametrize("tokens", [1, 7, 130])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_concat_and_cache_mla(ops, dtype, tokens, block_size, strided, widths, kv, scale):
    kv_c, k_pe = make_inputs(dtype, tokens, widths, strided, scale)
    width, num_blocks = sum(widths), -(-tokens // block_size) + 2
    cdt = dtype if kv == "auto" else torch.uint8
    cache = torch.empty(num_blocks, block_size, width, dtype=cdt, device="cuda")
    cache.view(torch.uint8).fill_(SENTINEL)
    slots = make_slots(tokens, block_size, num_blocks)
    ops.concat_and_cache_mla(kv_c, k_pe, cache, slots, kv, torch.tensor([scale], device="cuda"))

    want = torch.cat([kv_c, k_pe], dim=-1)[:tokens].contiguous()
    if kv != "auto":
        q8 = torch.empty(want.shape, dtype=torch.uint8, device="cuda")
        ops.convert_fp8(q8, want, scale, "fp8")
        want = q8
    expect = torch.empty_like(cache)
    expect.view(torch.uint8).fill_(SENTINEL)
    keep = slots >= 0
    expect.view(-1, width)[slots[keep]] = want[keep]
    assert torch.equal(cache.view(torch.uint8), expect.view(torch.uint8))


def test_written_rows_are_what_decode_reads(ops):
    from test_gpu_parity_mla import SCALE, make_case, run
    q, cache, bt, sl = make_case(torch.bfloat16, 16, 16, lens=[40, 7, 64], seed=5)
    written = torch.zeros_like(cache)
    for b, n in enumerate(sl.tolist()):  # the tokens of every sequence, through its block table
        tok = torch.arange(n, device="cuda")
        slots = bt[b, tok // 16].long() * 16 + tok % 16
        rows = cache.view(-1, 576)[slots]
        ops.concat_and_cache_mla(rows[:, :512], rows[:, 512:], written, slots, "auto", torch.ones(1, device="cuda"))
    assert torch.equal(run(q, written, bt, sl, 4, SCALE), run(q, cache, bt, sl, 4, SCALE))


def test_opcheck_concat_and_cache_mla(ops):
    from test_gpu_opcheck import opcheck
    kv_c, k_pe = make_inputs(torch.bfloat16, 7, (512, 64), True, 1.0)
    for kv, cdt in (("auto", torch.bfloat16), ("fp8", torch.uint8)):
        cache = torch.zeros(3, 16, 576, dtype=cdt, device="cuda")
        opcheck(torch.ops._C_cache_ops.concat_and_cache_mla,
                (kv_c, k_pe, cache, make_slots(7, 16, 3), kv, torch.ones(1, device="cuda")))
