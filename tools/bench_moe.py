#!/usr/bin/env python3
"""Fused MoE experts over block-scaled fp8 weights on the GPU:
    python tools/bench_moe.py [--out FILE] [--tokens 1,16,64,256,4096] [--inter 2048,256] [--iters 4]

DeepSeek-V3 shapes: E 256, top-k 8, hidden 7168, intermediate size I per rank 2048 (TP 1) or 256 (TP 8);
softmax top-k routing of random logits.  For each of the two grouped GEMMs (w1 [E, 2 I, 7168], w2 [E, 7168, I]):
device time per call (graph replays, bench.time_gpu_graph) and TB/s over the TOUCHED experts' weight bytes
against the 8 TB/s HBM peak -- the weights (7.5 + 3.8 GB at I 2048) are far beyond the 256 MiB Infinity Cache,
so every call streams them.  Yardstick, timed in the same process and alternated with the new path: the
per-expert loop of cutlass_scaled_mm calls on the same data (gather of the expert's rows, block-scaled GEMM,
scatter), with the row lists prepared on the host beforehand and the loop captured in a graph too, so its
launch overhead is NOT counted against it.  Then "moe_ks" 8 against 2 for both GEMMs, block_size_m 16 against
64, and the whole fused_experts call.

    python tools/bench_moe.py --mxfp4 [--out FILE] [--tokens 1,16,64,256] [--inter 2048,256] [--iters 4]

The MXFP4 (w4a4) path against the fp8 block-scaled path on the same shapes, alternated in the same process: per
GEMM and for the whole fused_experts call, device time by graph replay and TB/s over the touched experts' weight
bytes (codes and scales), and "moe_ks" 8 against 2 for the MXFP4 GEMM.

    python tools/bench_moe.py --tile [--out FILE] [--tokens 256,512,1024,2048,4096,16384] [--inter 2048,256]

Prefill: block_size_m 128 (the grouped tile kernel) against 64 (the weight-streaming kernel) for both GEMMs, and for
the whole fused_experts call 128 against what _block_size_m picks without the tile kernel (16 or 64), alternated in
the same process, two rounds each.  Achieved TFLOP/s from 2 * valid rows * N * K, and the share of the larger of the
two lower bounds on the time: that work at the fp8 MFMA peak, or the touched experts' weight bytes at the HBM peak."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

FP8 = torch.float8_e4m3fn
E, TOPK, H = 256, 8, 7168


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="1,16,64,256,4096")
    ap.add_argument("--inter", default="2048,256")
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mxfp4", action="store_true", help="MXFP4 (w4a4) against block-scaled fp8")
    ap.add_argument("--tile", action="store_true", help="block_size_m 128 (tile kernel) against 64 at prefill sizes")
    a = ap.parse_args()
    if a.tile and a.tokens == ap.get_default("tokens"):
        a.tokens = "256,512,1024,2048,4096,16384"
    if a.mxfp4 and a.tokens == ap.get_default("tokens"):
        a.tokens = "1,16,64,256"
    if not torch.cuda.is_available():
        print("bench_moe: no GPU", file=sys.stderr)
        return 2
    from vllm_amd import _custom_ops as ops, _lib
    from vllm_amd.model_executor.layers.fused_moe import fused_experts, moe_align_block_size
    from vllm_amd.model_executor.layers.fused_moe.fused_moe import _block_size_m
    dev = torch.device("cuda", 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    def fp8_rand(*shape):   # codes 0 .. 119: finite, positive
        return torch.randint(0, 120, shape, device=dev, dtype=torch.uint8).view(FP8)

    def time_pair(new, old, iters):
        t = [bench.time_gpu_graph(f, iters) * 1e6 for f in (old, new, old, new)]
        return t[1], t[3], t[0], t[2]

    if a.mxfp4:
        return mxfp4_mode(a, dev, emit, fp8_rand, time_pair)
    if a.tile:
        return tile_mode(a, dev, emit, fp8_rand, time_pair)
    emit(f"# E {E}, top-k {TOPK}, hidden {H}; us per call (two alternated rounds); TB/s = touched experts' weight bytes / "
         f"time, share of the {bench.HBM_PEAK_GBPS / 1000:.0f} TB/s HBM peak")
    for inter in (int(x) for x in a.inter.split(",")):
        w1, w2 = fp8_rand(E, 2 * inter, H), fp8_rand(E, H, inter)
        w1_s = torch.rand((E, 2 * inter // 128, H // 128), device=dev) * 1e-2
        w2_s = torch.rand((E, H // 128, inter // 128), device=dev) * 1e-2
        for tokens in (int(x) for x in a.tokens.split(",")):
            g = torch.Generator(device=dev).manual_seed(tokens)
            topk_w, ids = torch.randn((tokens, E), device=dev, generator=g).softmax(-1).topk(TOPK, dim=-1)
            ids = ids.to(torch.int32)
            touched = ids.unique().numel()
            x = torch.randn((tokens, H), device=dev, dtype=torch.bfloat16) / 10
            slots = tokens * TOPK
            rows = [torch.nonzero(ids.view(-1) == e).view(-1) for e in range(E)]   # host-prepared, outside the timing
            rows = [(e, r) for e, r in enumerate(rows) if r.numel()]
            for name, w, ws, top_k, a_rows in (("w1", w1, w1_s, TOPK, tokens), ("w2", w2, w2_s, 1, slots)):
                N, K = w.shape[1], w.shape[2]
                aq, As = fp8_rand(a_rows, K), torch.rand((a_rows, K // 128), device=dev) * 1e-2
                c = torch.zeros((slots, N), dtype=torch.bfloat16, device=dev)
                wbytes = touched * N * K
                tw = topk_w.reshape(-1).contiguous()

                def aligned(bm):
                    return moe_align_block_size(ids, bm, E)

                def new_call(bm, al):
                    return lambda: ops.moe_block_fp8_gemm(c, aq, w, As, ws, tw, al[0], al[1], al[2], True, top_k, bm)

                def loop():
                    for e, r in rows:
                        src = r // top_k
                        o = ops.cutlass_scaled_mm(aq[src], w[e].t(), As[src], ws[e].t(), torch.bfloat16)
                        c[r] = o
                bm = min(_block_size_m(tokens, TOPK, E), 64)   # the tile kernel (128) has its own mode: --tile
                n1, n2, o1, o2 = time_pair(new_call(bm, aligned(bm)), loop, a.iters)
                tn = min(n1, n2)
                emit(f"  I {inter:5d} tokens {tokens:5d} {name} N {N:5d} K {K:5d} bm {bm:2d} touched {touched:3d} | grouped {n1:9.1f} "
                     f"{n2:9.1f} | loop {o1:9.1f} {o2:9.1f} | loop / grouped {min(o1, o2) / tn:6.2f} | "
                     f"{wbytes / tn / 1e6:6.2f} TB/s, {wbytes / tn / 1e3 / bench.HBM_PEAK_GBPS:.3f} of peak")
                t = []
                for ks, b in ((8, bm), (2, bm), (0, 16), (0, 64)) * 2:
                    _lib.set_tuning("moe_ks", ks)
                    t.append(bench.time_gpu_graph(new_call(b, aligned(b)), a.iters) * 1e6)
                _lib.set_tuning("moe_ks", 0)
                emit(f"      moe_ks 8: {t[0]:9.1f} {t[4]:9.1f}  moe_ks 2: {t[1]:9.1f} {t[5]:9.1f} | block_size_m 16: {t[2]:9.1f} "
                     f"{t[6]:9.1f}  64: {t[3]:9.1f} {t[7]:9.1f}")
            full = lambda: fused_experts(x, w1, w2, topk_w, ids, use_fp8_w8a8=True, w1_scale=w1_s, w2_scale=w2_s,
                                         block_shape=[128, 128])
            t = bench.time_gpu_graph(full, a.iters) * 1e6
            allb = touched * 3 * inter * H
            emit(f"  I {inter:5d} tokens {tokens:5d} fused_experts (quant, align, w1, act + quant, w2, sum): {t:9.1f} us, "
                 f"{allb / t / 1e6:6.2f} TB/s over the touched weights")
        del w1, w2
        torch.cuda.empty_cache()
    return 0


def tile_mode(a, dev, emit, fp8_rand, time_pair):
    from vllm_amd import _custom_ops as ops
    from vllm_amd.model_executor.layers.fused_moe import fused_experts, moe_align_block_size
    fm = sys.modules[fused_experts.__module__]   # the module: the package exports a function of the same name
    peak_f, peak_b = bench.FP8_DENSE_PEAK_TFLOPS * 1e12, bench.HBM_PEAK_GBPS * 1e9
    emit(f"# E {E}, top-k {TOPK}, hidden {H}; block_size_m 128 (tile kernel) against 64 (streaming kernel), us per call, two "
         f"alternated rounds each; TFLOP/s = 2 * valid rows * N * K / time of 128; bound = the larger of that work at "
         f"{peak_f / 1e15:.0f} PFLOP/s (mfma) and the touched experts' weight bytes at {peak_b / 1e12:.0f} TB/s (hbm)")
    for inter in (int(x) for x in a.inter.split(",")):
        w1, w2 = fp8_rand(E, 2 * inter, H), fp8_rand(E, H, inter)
        w1_s = torch.rand((E, 2 * inter // 128, H // 128), device=dev) * 1e-2
        w2_s = torch.rand((E, H // 128, inter // 128), device=dev) * 1e-2
        for tokens in (int(x) for x in a.tokens.split(",")):
            g = torch.Generator(device=dev).manual_seed(tokens)
            topk_w, ids = torch.randn((tokens, E), device=dev, generator=g).softmax(-1).topk(TOPK, dim=-1)
            ids = ids.to(torch.int32)
            touched, slots = ids.unique().numel(), tokens * TOPK
            x = torch.randn((tokens, H), device=dev, dtype=torch.bfloat16) / 10
            tw = topk_w.reshape(-1).contiguous()
            al = {bm: moe_align_block_size(ids, bm, E) for bm in (64, 128)}
            for name, w, ws, top_k, a_rows in (("w1", w1, w1_s, TOPK, tokens), ("w2", w2, w2_s, 1, slots)):
                N, K = w.shape[1], w.shape[2]
                aq, As = fp8_rand(a_rows, K), torch.rand((a_rows, K // 128), device=dev) * 1e-2
                c = torch.zeros((slots, N), dtype=torch.bfloat16, device=dev)

                def call(bm):
                    s, e, p = al[bm]
                    return lambda: ops.moe_block_fp8_gemm(c, aq, w, As, ws, tw, s, e, p, True, top_k, bm)
                n1, n2, o1, o2 = time_pair(call(128), call(64), a.iters)
                tn, flop = min(n1, n2) * 1e-6, 2.0 * slots * N * K
                t_f, t_b = flop / peak_f, touched * N * K / peak_b
                emit(f"  I {inter:5d} tokens {tokens:5d} {name} N {N:5d} K {K:5d} touched {touched:3d} | 128: {n1:9.1f} {n2:9.1f} | "
                     f"64: {o1:9.1f} {o2:9.1f} | 64 / 128 {min(o1, o2) / min(n1, n2):5.2f} | {flop / tn / 1e12:7.1f} TFLOP/s, "
                     f"{max(t_f, t_b) / tn:.3f} of the {'mfma' if t_f >= t_b else 'hbm'} bound")
                del aq, As, c

            def full(min_slots):   # the threshold of _block_size_m: 0 -> always 128, out of reach -> 16 / 64
                def run():
                    fm.TILE_MIN_SLOTS = min_slots
                    return fused_experts(x, w1, w2, topk_w, ids, use_fp8_w8a8=True, w1_scale=w1_s, w2_scale=w2_s,
                                         block_shape=[128, 128])
                return run
            keep = fm.TILE_MIN_SLOTS
            try:
                n1, n2, o1, o2 = time_pair(full(0), full(1 << 30), a.iters)
            finally:
                fm.TILE_MIN_SLOTS = keep
            rule = 16 if slots <= 16 * E else 64     # what _block_size_m picks without the tile kernel
            emit(f"  I {inter:5d} tokens {tokens:5d} fused_experts | 128: {n1:9.1f} {n2:9.1f} | {rule}: {o1:9.1f} {o2:9.1f} | "
                 f"{rule} / 128 {min(o1, o2) / min(n1, n2):5.2f}")
        del w1, w2
        torch.cuda.empty_cache()
    return 0


def mxfp4_mode(a, dev, emit, fp8_rand, time_pair):
    from vllm_amd import _custom_ops as ops, _lib
    from vllm_amd.model_executor.layers.fused_moe import fused_experts, moe_align_block_size
    from vllm_amd.model_executor.layers.fused_moe.fused_moe import _block_size_m
    u8 = lambda lo, hi, *shape: torch.randint(lo, hi, shape, device=dev, dtype=torch.uint8)
    emit(f"# E {E}, top-k {TOPK}, hidden {H}; MXFP4 (w4a4) against block-scaled fp8, us per call (two alternated rounds "
         f"each); TB/s = touched experts' weight bytes (codes + scales) / time, peak {bench.HBM_PEAK_GBPS / 1000:.0f} TB/s")
    for inter in (int(x) for x in a.inter.split(",")):
        f8 = dict(w1=fp8_rand(E, 2 * inter, H), w2=fp8_rand(E, H, inter),
                  s1=torch.rand((E, 2 * inter // 128, H // 128), device=dev) * 1e-2,
                  s2=torch.rand((E, H // 128, inter // 128), device=dev) * 1e-2)
        mx = dict(w1=u8(0, 256, E, 2 * inter, H // 2), w2=u8(0, 256, E, H, inter // 2),     # all 16 codes
                  s1=u8(118, 122, E, 2 * inter, H // 32), s2=u8(118, 122, E, H, inter // 32))
        for tokens in (int(x) for x in a.tokens.split(",")):
            g = torch.Generator(device=dev).manual_seed(tokens)
            topk_w, ids = torch.randn((tokens, E), device=dev, generator=g).softmax(-1).topk(TOPK, dim=-1)
            ids = ids.to(torch.int32)
            touched, slots = ids.unique().numel(), tokens * TOPK
            x = torch.randn((tokens, H), device=dev, dtype=torch.bfloat16) / 10
            tw = topk_w.reshape(-1).contiguous()
            bm = min(_block_size_m(tokens, TOPK, E), 64)
            al = moe_align_block_size(ids, bm, E)
            for name, top_k, a_rows in (("w1", TOPK, tokens), ("w2", 1, slots)):
                N, K = f8[name].shape[1], f8[name].shape[2]
                c = torch.zeros((slots, N), dtype=torch.bfloat16, device=dev)
                a8, As8 = fp8_rand(a_rows, K), torch.rand((a_rows, K // 128), device=dev) * 1e-2
                a4, As4 = u8(0, 256, a_rows, K // 2), u8(125, 129, a_rows, K // 32)
                w8, ws8, w4, ws4 = f8[name], f8["s" + name[1]], mx[name], mx["s" + name[1]]
                fp8 = lambda: ops.moe_block_fp8_gemm(c, a8, w8, As8, ws8, tw, al[0], al[1], al[2], True, top_k, bm)
                mx4 = lambda: ops.moe_mxfp4_gemm(c, a4, w4, As4, ws4, tw, al[0], al[1], al[2], True, top_k, bm)
                n1, n2, o1, o2 = time_pair(mx4, fp8, a.iters)
                tn, to = min(n1, n2), min(o1, o2)
                b4, b8 = touched * N * (K // 2 + K // 32), touched * N * K
                emit(f"  I {inter:5d} tokens {tokens:4d} {name} N {N:5d} K {K:5d} bm {bm:2d} touched {touched:3d} | mxfp4 {n1:8.1f} "
                     f"{n2:8.1f} ({b4 / tn / 1e6:5.2f} TB/s) | fp8 {o1:8.1f} {o2:8.1f} ({b8 / to / 1e6:5.2f} TB/s) | "
                     f"fp8 / mxfp4 time {to / tn:5.2f}, bytes {b8 / b4:4.2f}")
                t = []
                for ks in (8, 2) * 2:
                    _lib.set_tuning("moe_ks", ks)
                    t.append(bench.time_gpu_graph(mx4, a.iters) * 1e6)
                _lib.set_tuning("moe_ks", 0)
                emit(f"      mxfp4 moe_ks 8: {t[0]:8.1f} {t[2]:8.1f}  moe_ks 2: {t[1]:8.1f} {t[3]:8.1f}")
            full8 = lambda: fused_experts(x, f8["w1"], f8["w2"], topk_w, ids, use_fp8_w8a8=True, w1_scale=f8["s1"],
                                          w2_scale=f8["s2"], block_shape=[128, 128])
            full4 = lambda: fused_experts(x, mx["w1"], mx["w2"], topk_w, ids, use_mxfp4_w4a4=True, w1_scale=mx["s1"],
                                          w2_scale=mx["s2"])
            n1, n2, o1, o2 = time_pair(full4, full8, a.iters)
            tn, to = min(n1, n2), min(o1, o2)
            b8 = touched * 3 * inter * H
            b4 = b8 // 2 + b8 // 32
            emit(f"  I {inter:5d} tokens {tokens:4d} fused_experts | mxfp4 {n1:8.1f} {n2:8.1f} ({b4 / tn / 1e6:5.2f} TB/s) | fp8 "
                 f"{o1:8.1f} {o2:8.1f} ({b8 / to / 1e6:5.2f} TB/s) | fp8 / mxfp4 time {to / tn:5.2f}, bytes {b8 / b4:4.2f}")
        del f8, mx
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
