#!/usr/bin/env python3
"""MLA prefill (csrc/mla_prefill.hip, gather_cache) on the GPU:
    python tools/bench_mla_prefill.py [--out FILE] [--iters 5] [--heads 16,128]

Attention, bf16, DeepSeek-V3 head dims (q.k 192, v 128), K in split form (views of one [Tk, H, 256] tensor and a
shared k_pe): one sequence of 4096 and of 16384 tokens, causal; 8 x 2048 ragged, causal; one non-causal context pass of
4096 queries over 16384 keys.  Per row: us (device events around `iters` eager calls, after warm-up; every call
runs for hundreds of us at least) and TFLOP/s over 2 * (192 + 128) flops per visible (q, k) pair, with the share of
the bf16 MFMA peak.  Beside it, in the same run, what a caller without the kernel runs: torch.cat of k, the zero-padded
v and torch's scaled_dot_product_attention per sequence (skipped where its score matrix could not be held).
Two alternated rounds: the spread between a column's two numbers is what a difference has to exceed.
Then merge_attn_states and gather_cache as GB/s over the bytes read + written (HIP graph replays, rotating buffers
larger than the Infinity Cache)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2500.0
SCALE = 192 ** -0.5


def time_eager(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def torch_path(q, kv, k_pe, sq, sk, causal):
    """cat + pad + SDPA per sequence (bottom-right causal is the plain causal mask here: Sq == Sk in the causal rows)"""
    H = q.shape[1]
    k = torch.cat([kv[..., :128], k_pe.expand(-1, H, -1)], dim=-1)
    v = F.pad(kv[..., 128:], (0, 64))
    outs, q0, k0 = [], 0, 0
    for nq, nk in zip(sq, sk):
        o = F.scaled_dot_product_attention(q[q0:q0 + nq].transpose(0, 1)[None], k[k0:k0 + nk].transpose(0, 1)[None],
                                           v[k0:k0 + nk].transpose(0, 1)[None], is_causal=causal, scale=SCALE)
        outs.append(o[0].transpose(0, 1)[..., :128])
        q0, k0 = q0 + nq, k0 + nk
    return torch.cat(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--heads", default="16,128")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_mla_prefill: no GPU", file=sys.stderr)
        return 2
    from vllm_amd import _custom_ops as ops
    from vllm_amd.attention.ops.merge_attn_states import merge_attn_states
    from vllm_amd.v1.attention.backends.mla.common import flash_attn_varlen_diff_headdims
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    def cu(lens):
        return torch.tensor([0] + lens, device=dev).cumsum(0).to(torch.int32)

    g = torch.Generator(device="cpu").manual_seed(0)
    ragged = torch.randint(256, 3841, (8,), generator=g).tolist()
    shapes = [("1 x 4096 causal", [4096], [4096], True), ("1 x 16384 causal", [16384], [16384], True),
              ("8 x 2048 causal", [2048] * 8, [2048] * 8, True), ("8 x U[256,3840] causal", ragged, ragged, True),
              ("4096 x 16384 context", [4096], [16384], False)]
    emit("# MLA prefill attention, bf16, q.k 192 / v 128, split K; us per call (round 1, round 2), TFLOP/s of the better")
    emit("# shape                    H |   kernel us (r1, r2)  TFLOP/s  of 2500 | cat + pad + SDPA us (r1, r2) | speed-up")
    for name, sq, sk, causal in shapes:
        pairs = sum(nq * nk - (nq * (nq - 1) // 2 if causal else 0) for nq, nk in zip(sq, sk))
        for H in [int(h) for h in a.heads.split(",")]:
            q = torch.randn(sum(sq), H, 192, device=dev, dtype=dt)
            kv = torch.randn(sum(sk), H, 256, device=dev, dtype=dt)
            k_pe = torch.randn(sum(sk), 1, 64, device=dev, dtype=dt)
            cq, ck = cu(sq), cu(sk)
            ours = lambda: flash_attn_varlen_diff_headdims(q, kv[..., :128], kv[..., 128:], cq, ck, max(sq), max(sk), SCALE,
                                                           causal, k_pe=k_pe)
            base = lambda: torch_path(q, kv, k_pe, sq, sk, causal)
            base_ok = H * max(sq) * max(sk) * 4 <= 48 << 30     # an fp32 score matrix, should SDPA fall to its math path
            if base_ok:
                err = (ours().float() - base().float()).abs().max().item()
                assert err < 0.05, f"{name} H {H}: kernel and torch path differ by {err}"
            t, tb = [], []
            for _ in range(2):
                t.append(time_eager(ours, a.iters))
                tb.append(time_eager(base, max(a.iters // 2, 1)) if base_ok else float("nan"))
            tf = pairs * H * 2.0 * (192 + 128) / min(t) / 1e12
            emit(f"  {name:24s} {H:3d} | {t[0] * 1e6:9.1f} {t[1] * 1e6:9.1f}  {tf:7.1f}  {tf / BF16_DENSE_PEAK_TFLOPS:6.3f} | "
                 f"{tb[0] * 1e6:11.1f} {tb[1] * 1e6:11.1f}   | {min(tb) / min(t):6.2f}")
            del q, kv, k_pe
            torch.cuda.empty_cache()

    emit("# merge_attn_states, bf16, 8192 tokens x 128 heads x 128: us, GB/s over 2 outputs read + 1 written (+ lse)")
    T, H, D = 8192, 128, 128
    copies = max(2, -(-int(1.25 * bench.MALL_BYTES) // (3 * T * H * D * 2)))
    bufs = [[torch.randn(T, H, D, device=dev, dtype=dt) for _ in range(3)] for _ in range(copies)]
    pl, sl, ol = (torch.randn(H, T, device=dev) for _ in range(3))
    st = {"i": 0}

    def merge():
        o, p, s = bufs[st["i"] % copies]
        st["i"] += 1
        merge_attn_states(o, p, pl, s, sl, ol)
    for r in (1, 2):
        t = bench.time_gpu_graph(merge, copies * 2)
        emit(f"  round {r} | {t * 1e6:8.1f} us | {(3 * T * H * D * 2 + 3 * T * H * 4) / t / 1e9:7.0f} GB/s")
    del bufs
    torch.cuda.empty_cache()

    emit("# gather_cache, 16384 tokens x 576, page 64, 8 sequences of 2048: us, GB/s over bytes read + written")
    T, page, B = 16384, 64, 8
    nb = T // page
    bt = torch.randperm(nb, device=dev).view(B, nb // B).to(torch.int32)
    cs = cu([T // B] * B)
    one = torch.full((1,), 0.5, device=dev)
    for kind, cdt, rb in (("bf16 -> bf16", dt, 2), ("fp8 -> bf16", torch.uint8, 1)):
        copies = max(2, -(-int(1.25 * bench.MALL_BYTES) // (T * 576 * (rb + 2))))
        caches = [torch.randint(0, 120, (nb, page, 576 * rb), device=dev, dtype=torch.uint8).view(cdt) for _ in range(copies)]
        dsts = [torch.empty(T, 576, device=dev, dtype=dt) for _ in range(copies)]
        st = {"i": 0}

        def gather():
            i = st["i"] % copies
            st["i"] += 1
            ops.gather_cache(caches[i], dsts[i], bt, cs, B, None, **({"scale": one} if rb == 1 else {}))
        for r in (1, 2):
            t = bench.time_gpu_graph(gather, copies * 2)
            emit(f"  {kind:12s} round {r} | {t * 1e6:8.1f} us | {T * 576 * (rb + 2) / t / 1e9:7.0f} GB/s")
        del caches, dsts
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
