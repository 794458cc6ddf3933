#!/usr/bin/env python3
"""Block-scaled fp8 GEMM and per-token-group quantiser on the GPU:
    python tools/bench_block_gemm.py [--out FILE] [--shapes 576x7168,...] [--ms 1,16,...] [--iters 20]

Yardstick: the per-token x per-channel cutlass_scaled_mm at the same (M, N, K), timed in the same
process and alternated with the block-scaled path (two rounds each; the table shows the mean and both
ratios).  It moves the same bytes and issues the same MFMAs, so the ratio is the price of scaling
inside the K loop.  Calls are captured in a HIP graph (bench.time_gpu_graph: device events around
replays, warm-up per shape), weights rotate through a pool larger than the Infinity Cache as in
bench.run_scaled_mm.  M <= 32 rows are bound by the weight bytes (GB/s of N x K), larger M by whichever of
the 5 PF fp8 peak and the 8 TB/s HBM peak gives the longer time; the column `bound` says which.
Because both paths are timed as graph replays, the yardstick is the UNSPLIT per-channel kernel: a captured
cutlass_scaled_mm never takes a split-K workspace slot, so at M <= 64, K >= 12288 (here: 7168 x 18432) an eager
caller of the per-channel path gets a somewhat faster kernel than the one in the table."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

FP8 = torch.float8_e4m3fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="576x7168,1536x7168,4608x7168,7168x2304,7168x18432,4096x4096", help="NxK,...")
    ap.add_argument("--ms", default="1,16,32,64,256,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_block_gemm: no GPU", file=sys.stderr)
        return 2
    from vllm_amd import _custom_ops, _lib  # noqa: F401  (registers the operators)
    dev = torch.device("cuda", 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    def pool(N, K):
        copies = max(3, -(-int(1.25 * bench.MALL_BYTES) // (K * N)))
        ws = [((torch.rand((N, K), device=dev) - 0.5) * 896).to(FP8) for _ in range(copies)]
        return ws, copies

    def timed(call, ws, copies, iters):
        st = {"i": 0}

        def fn():
            call(ws[st["i"] % copies])
            st["i"] += 1
        return bench.time_gpu_graph(fn, -(-iters // copies) * copies)

    def gemm_calls(M, N, K):
        aq = ((torch.rand((M, K), device=dev) - 0.5) * 896).to(FP8)
        out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        sa, sb = torch.rand((M, 1), device=dev) * 1e-2, torch.rand((N, 1), device=dev) * 1e-2
        As = torch.rand((M, K // 128), device=dev) * 1e-2
        Bs = torch.rand((-(-N // 128), K // 128), device=dev) * 1e-2
        chan = lambda w: torch.ops._C.cutlass_scaled_mm(out, aq, w.t(), sa, sb, None)
        block = lambda w: torch.ops._C.cutlass_scaled_mm(out, aq, w.t(), As, Bs.t(), None)
        return chan, block

    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    Ms = [int(m) for m in a.ms.split(",")]
    emit("# block-scaled vs per-channel fp8 GEMM, bf16 out, weights rotating through > 1.25 x 256 MiB")
    emit("#     N      K     M | per-channel us | block us (r1, r2) | ratio r1, r2 | block TFLOP/s | weight GB/s | bound, share")
    for (N, K) in shapes:
        ws, copies = pool(N, K)
        for M in Ms:
            chan, block = gemm_calls(M, N, K)
            t = [timed(f, ws, copies, a.iters) for f in (chan, block, chan, block)]
            tc, tb = (t[0] + t[2]) / 2, (t[1] + t[3]) / 2
            flops, wbytes = 2.0 * M * N * K, float(N) * K
            nbytes = M * K + wbytes + 2 * M * N
            t_mfma, t_hbm = flops / (bench.FP8_DENSE_PEAK_TFLOPS * 1e12), nbytes / (bench.HBM_PEAK_GBPS * 1e9)
            bound = "MFMA" if t_mfma > t_hbm else "HBM"
            emit(f"  {N:5d} {K:6d} {M:5d} | {tc * 1e6:9.2f} | {tb * 1e6:9.2f} ({t[1] * 1e6:.2f}, {t[3] * 1e6:.2f}) | "
                 f"{t[1] / t[0]:.3f}, {t[3] / t[2]:.3f} | {flops / tb / 1e12:8.1f} | {wbytes / tb / 1e9:8.1f} | "
                 f"{bound} {max(t_mfma, t_hbm) / tb:.3f}")
        del ws
        torch.cuda.empty_cache()

    emit("# tile kernel (mm_block_kernel 1) vs streaming kernel (0: what M <= 64 takes), us")
    for (N, K) in ((1536, 7168), (7168, 2304)):
        ws, copies = pool(N, K)
        for M in (16, 32, 48, 64):
            _, block = gemm_calls(M, N, K)
            t = []
            for knob in (1, 0, 1, 0):
                _lib.set_tuning("mm_block_kernel", knob)
                t.append(timed(block, ws, copies, a.iters) * 1e6)
            _lib.set_tuning("mm_block_kernel", 0)
            emit(f"  {N:5d} {K:6d} {M:5d} | tile {t[0]:8.2f} {t[2]:8.2f} | stream {t[1]:8.2f} {t[3]:8.2f}")
        del ws
        torch.cuda.empty_cache()

    emit("# quantisers, bf16 [T, 7168]: us and GB/s of input + codes + scales bytes (HBM peak 8000 GB/s)")
    for T in (1, 256, 8192):
        H = 7168
        pool_x = [torch.randn((T, H), device=dev, dtype=torch.bfloat16) for _ in range(max(3, -(-(320 << 20) // (T * H * 3))) if T > 1 else 3)]
        q = torch.empty((T, H), device=dev, dtype=FP8)
        sg, st_ = torch.empty((T, H // 128), device=dev), torch.empty((T, 1), device=dev)
        grp = lambda x: torch.ops._C.per_token_group_fp8_quant(x, q, sg, 128, 1e-10, -448.0, 448.0, False)
        tok = lambda x: torch.ops._C.dynamic_per_token_scaled_fp8_quant(q, x, st_, None)
        t = [timed(f, pool_x, len(pool_x), a.iters) for f in (tok, grp, tok, grp)]
        bg, bt = T * H * 3 + T * (H // 128) * 4, T * H * 3 + T * 4
        emit(f"  T {T:5d} | per-token {t[0] * 1e6:8.2f} {t[2] * 1e6:8.2f} us, {bt / min(t[0], t[2]) / 1e9:7.1f} GB/s | "
             f"group-128 {t[1] * 1e6:8.2f} {t[3] * 1e6:8.2f} us, {bg / min(t[1], t[3]) / 1e9:7.1f} GB/s")
        del pool_x
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
