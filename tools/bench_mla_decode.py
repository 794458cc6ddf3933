#!/usr/bin/env python3
"""MLA decode (csrc/mla_decode.hip) and the latent cache write on the GPU:
    python tools/bench_mla_decode.py [--out FILE] [--iters 8] [--fp8]
(--fp8: instead of the tables below, the fp8-cache kernel beside the 16-bit one on the same shapes, see fp8_table)

bf16, page size 64, H in {16, 128}, num_kv_splits in {1, 4, 16}; per row: us, TB/s over the algorithmic
bytes (cache rows once + q + o), PFLOP/s over B * len * H * 2 * (576 + 512), and the share of
min(8 TB/s * arithmetic intensity, 2.5 PF).  Calls are captured in a HIP graph (bench.time_gpu_graph: device
events around replays, warm-up per shape); the cache rotates through copies that together exceed
1.25 x the 256 MiB Infinity Cache, so rows come from HBM.  Beside each shape: the same computation
composed from torch ops on the same GPU (gather the rows through the block table, bmm, softmax, bmm),
eager, device events, which is what a caller without this kernel runs."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

BF16_DENSE_PEAK_PFLOPS = 2.5
PAGE = 64


def torch_composed(q, cache, bt, sl, scale):
    B, Lmax = q.shape[0], int(sl.max())
    tok = torch.arange(Lmax, device=q.device)
    slots = bt[:, tok // PAGE].long() * PAGE + tok % PAGE
    rows = cache.view(-1, 576)[slots]                                   # [B, Lmax, 576]
    logits = torch.bmm(q, rows.transpose(1, 2)).float() * scale
    logits.masked_fill_(tok[None, None, :] >= sl[:, None, None], float("-inf"))
    return torch.bmm(torch.softmax(logits, dim=-1).to(q.dtype), rows[..., :512])


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


def fp8_table(shapes, scale, dev, iters, emit):
    """--fp8: per shape the 16-bit kernel, the fp8 kernel, the 16-bit kernel again (its two times are the
    spread a difference has to exceed), each over its own rotating cache copies; TB/s over the bytes each
    kernel has to move (rows once + q + o)."""
    from vllm_amd.attention.ops.triton_decode_attention import decode_attention_fwd
    emit("# MLA decode, bf16 q, page 64, kv_scale 0.5: 16-bit cache (timed twice) and fp8 cache, same run")
    emit("# shape              H  splits | 16-bit us (1st, 2nd) TB/s | fp8 us   TB/s | fp8 / 16-bit")
    ks = torch.tensor([0.5], device=dev)
    for name, lens in shapes:
        B, tokens = len(lens), sum(lens)
        nb = -(-max(lens) // PAGE)
        blocks = B * nb
        want = int(1.25 * bench.MALL_BYTES)
        c16 = [torch.randn(blocks, PAGE, 576, device=dev, dtype=torch.bfloat16)
               for _ in range(max(2, -(-want // (blocks * PAGE * 1152))))]
        c8 = [(torch.randn(blocks, PAGE, 576, device=dev) * 2).to(torch.float8_e4m3fn).view(torch.uint8)
              for _ in range(max(2, -(-want // (blocks * PAGE * 576))))]
        bt = torch.randperm(blocks, device=dev).view(B, nb).to(torch.int32)
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        for H in (16, 128):
            q = torch.randn(B, H, 576, device=dev, dtype=torch.bfloat16)
            o = torch.empty(B, H, 512, device=dev, dtype=torch.bfloat16)
            for splits in (1, 4, 16):
                lg = torch.empty(B, H, splits, 513, device=dev, dtype=torch.float32)

                def timed(caches, k_scale):
                    st = {"i": 0}

                    def fn():
                        kv = caches[st["i"] % len(caches)].unsqueeze(2)
                        st["i"] += 1
                        decode_attention_fwd(q, kv, kv[..., :512], o, bt, sl, lg, splits, scale, PAGE, k_scale=k_scale)
                    return bench.time_gpu_graph(fn, -(-iters // len(caches)) * len(caches))
                t16a, t8, t16b = timed(c16, None), timed(c8, ks), timed(c16, None)
                qo = B * H * (576 + 512) * 2
                t16 = min(t16a, t16b)
                emit(f"  {name:17s} {H:3d} {splits:5d}   | {t16a * 1e6:7.1f} {t16b * 1e6:7.1f}   {(tokens * 1152 + qo) / t16 / 1e12:5.2f} | "
                     f"{t8 * 1e6:7.1f}  {(tokens * 576 + qo) / t8 / 1e12:5.2f} | {t8 / t16:5.2f}")
        del c16, c8
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fp8", action="store_true", help="the fp8-cache kernel beside the 16-bit one, same shapes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_mla_decode: no GPU", file=sys.stderr)
        return 2
    from vllm_amd import _custom_ops as ops
    from vllm_amd.attention.ops.triton_decode_attention import decode_attention_fwd
    dev = torch.device("cuda", 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    g = torch.Generator(device="cpu").manual_seed(0)
    shapes = [("64 x 4096", [4096] * 64), ("8 x 32768", [32768] * 8), ("1 x 8192", [8192]),
              ("64 x U[512,4096]", torch.randint(512, 4097, (64,), generator=g).tolist())]
    scale = 576 ** -0.5
    if a.fp8:
        fp8_table(shapes, scale, dev, a.iters, emit)
        return 0
    emit("# MLA decode, bf16, page 64; cache copies rotate through > 1.25 x 256 MiB")
    emit("# shape              H  splits |      us |  TB/s | PFLOP/s | roof (bound) share | torch-composed us")
    for name, lens in shapes:
        B, tokens = len(lens), sum(lens)
        nb = -(-max(lens) // PAGE)
        blocks = B * nb
        copies = max(2, -(-int(1.25 * bench.MALL_BYTES) // (blocks * PAGE * 1152)))
        caches = [torch.randn(blocks, PAGE, 576, device=dev, dtype=torch.bfloat16) for _ in range(copies)]
        bt = torch.randperm(blocks, device=dev).view(B, nb).to(torch.int32)
        sl = torch.tensor(lens, dtype=torch.int32, device=dev)
        for H in (16, 128):
            q = torch.randn(B, H, 576, device=dev, dtype=torch.bfloat16)
            o = torch.empty(B, H, 512, device=dev, dtype=torch.bfloat16)
            t_ref = time_eager(lambda: torch_composed(q, caches[0], bt, sl, scale), 3)
            for splits in (1, 4, 16):
                lg = torch.empty(B, H, splits, 513, device=dev, dtype=torch.float32)
                st = {"i": 0}

                def fn():
                    kv = caches[st["i"] % copies].unsqueeze(2)
                    st["i"] += 1
                    decode_attention_fwd(q, kv, kv[..., :512], o, bt, sl, lg, splits, scale, PAGE)
                t = bench.time_gpu_graph(fn, -(-a.iters // copies) * copies)
                nbytes = tokens * 1152 + B * H * (576 + 512) * 2
                flops = tokens * H * 2.0 * (576 + 512)
                ai = flops / nbytes
                t_hbm, t_mfma = nbytes / (bench.HBM_PEAK_GBPS * 1e9), flops / (BF16_DENSE_PEAK_PFLOPS * 1e15)
                bound = "HBM" if t_hbm > t_mfma else "MFMA"
                emit(f"  {name:17s} {H:3d} {splits:5d}   | {t * 1e6:7.1f} | {nbytes / t / 1e12:5.2f} | {flops / t / 1e15:7.3f} | "
                     f"AI {ai:5.0f} {bound:4s} {max(t_hbm, t_mfma) / t:5.3f} | {t_ref * 1e6:9.1f}")
        del caches
        torch.cuda.empty_cache()

    emit("# concat_and_cache_mla, bf16, block 64: us and TB/s over read + written bytes")
    for T, kv, cdt, wb in ((64, "auto", torch.bfloat16, 2), (8192, "auto", torch.bfloat16, 2), (8192, "fp8", torch.uint8, 1)):
        x = torch.randn(T, 576, device=dev, dtype=torch.bfloat16)
        nblk = T // 64 + 1
        copies = max(2, -(-int(1.25 * bench.MALL_BYTES) // (nblk * 64 * 576 * wb)))
        caches = [torch.empty(nblk, 64, 576, device=dev, dtype=cdt) for _ in range(copies)]
        slots = torch.randperm(nblk * 64, device=dev)[:T]
        one = torch.ones(1, device=dev)
        st = {"i": 0}

        def fn():
            ops.concat_and_cache_mla(x[:, :512], x[:, 512:], caches[st["i"] % copies], slots, kv, one)
            st["i"] += 1
        t = bench.time_gpu_graph(fn, -(-a.iters // copies) * copies)
        emit(f"  T {T:5d} {kv:4s} | {t * 1e6:7.2f} us | {T * 576 * (2 + wb) / t / 1e12:5.2f} TB/s")
        del caches
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
