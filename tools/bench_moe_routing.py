#!/usr/bin/env python3
"""MoE routing on the GPU:
    python tools/bench_moe_routing.py [--out FILE] [--tokens 1,16,64,256,4096] [--iters 20] [--steps 200]

grouped_topk (E 256, 8 groups, 4 kept, top-8, sigmoid scores with a correction bias: DeepSeek-V3) and fused_topk
(E 128, top-8, renormalised) of csrc/moe_routing.hip, one launch each, against the same functions written in torch
ops as the reference has them (softmax / sigmoid, add, view, top-2, sum, top-k of the groups, scatter, expand,
masked_fill, top-k, gather, sum, divide, casts), on bf16 logits, in the same process and alternated.  Two times
per path: from a replayed graph (bench.time_gpu_graph: device time per call, launch cost excluded) and eagerly
(bench.time_gpu: HIP-event time per call of a loop of calls, which at these sizes is the host's launch path).
The torch grouped_topk is timed as the reference runs it, scoring in the logits' dtype; the new path's outputs are
compared first with the same torch functions on fp32 logits.  Last column: fused_experts (hidden 7168, intermediate 256 per
rank, block-scaled fp8) from a graph at the same token count and the new ids, the work that routing feeds."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

FP8 = torch.float8_e4m3fn
H, INTER = 7168, 256


def torch_grouped_topk(gating, topk, renormalize, groups, kept, bias):
    scores = gating.sigmoid()
    T = scores.size(0)
    sel = scores + bias.unsqueeze(0)
    group_scores = sel.view(T, groups, -1).topk(2, dim=-1)[0].sum(dim=-1)
    group_idx = torch.topk(group_scores, k=kept, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores).scatter_(1, group_idx, 1)
    mask = group_mask.unsqueeze(-1).expand(T, groups, sel.size(-1) // groups).reshape(T, -1)
    ids = torch.topk(sel.masked_fill(~mask.bool(), float("-inf")), k=topk, dim=-1, sorted=False)[1]
    w = scores.gather(1, ids)
    if renormalize:
        w = w / w.sum(dim=-1, keepdim=True)
    return w.to(torch.float32), ids.to(torch.int32)


def torch_fused_topk(gating, topk, renormalize):
    w, ids = gating.float().softmax(-1).topk(topk, dim=-1)
    if renormalize:
        w = w / w.sum(dim=-1, keepdim=True)
    return w, ids.to(torch.int32)


def same(new, old):
    """ids as sets and weights paired by id (random bf16 logits can tie: rows where the id sets differ are counted)"""
    on, oo = new[1].long().argsort(-1), old[1].long().argsort(-1)
    rows = (new[1].long().gather(1, on) == old[1].long().gather(1, oo)).all(-1)
    err = ((new[0].gather(1, on) - old[0].float().gather(1, oo)).abs() / old[0].float().gather(1, oo))[rows]
    return int((~rows).sum()), float(err.max()) if err.numel() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="1,16,64,256,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_moe_routing: no GPU", file=sys.stderr)
        return 2
    from vllm_amd.model_executor.layers.fused_moe import fused_experts, fused_topk, grouped_topk
    dev = torch.device("cuda", 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    def graph_pair(new, old):   # us per call, two alternated rounds each
        t = [bench.time_gpu_graph(f, a.iters) * 1e6 for f in (old, new, old, new)]
        return min(t[1], t[3]), min(t[0], t[2]), abs(t[1] - t[3]) / min(t[1], t[3])

    def eager_pair(new, old):
        t = [bench.time_gpu(f, a.steps, 20)[1] / a.steps * 1e6 for f in (old, new, old, new)]
        return min(t[1], t[3]), min(t[0], t[2])

    w1 = torch.randint(0, 120, (256, 2 * INTER, H), device=dev, dtype=torch.uint8).view(FP8)
    w2 = torch.randint(0, 120, (256, H, INTER), device=dev, dtype=torch.uint8).view(FP8)
    w1_s = torch.rand((256, 2 * INTER // 128, H // 128), device=dev) * 1e-2
    w2_s = torch.rand((256, H // 128, INTER // 128), device=dev) * 1e-2
    emit("# MoE routing, bf16 logits; us per call: new HIP kernel (one launch) / torch ops as in the reference; graph = device "
         "time from a replayed graph, eager = HIP-event time per call of a loop of eager calls (launch path included)")
    emit("# case          tokens | graph new    torch      x | eager new    torch      x | rounds differ | id-set mismatches, "
         "max rel. weight diff | fused_experts I 256 graph us")
    for tokens in (int(x) for x in a.tokens.split(",")):
        g = torch.Generator(device=dev).manual_seed(tokens)
        x = torch.randn((tokens, H), device=dev, dtype=torch.bfloat16) / 10
        for name, E in (("grouped_topk", 256), ("fused_topk", 128)):
            gating = torch.randn((tokens, E), device=dev, generator=g).to(torch.bfloat16)
            bias = torch.rand(E, device=dev, generator=g) * 0.2
            if name == "grouped_topk":
                new = lambda: grouped_topk(x, gating, 8, True, 8, 4, "sigmoid", bias)
                old = lambda: torch_grouped_topk(gating, 8, True, 8, 4, bias)   # as there: scored in the logits' dtype
                check = lambda: torch_grouped_topk(gating.float(), 8, True, 8, 4, bias)
            else:
                new = lambda: fused_topk(x, gating, 8, True)[:2]
                old = check = lambda: torch_fused_topk(gating, 8, True)
            bad, err = same(new(), check())
            gn, go, spread = graph_pair(new, old)
            en, eo = eager_pair(new, old)
            experts = ""
            if name == "grouped_topk":
                tw, ids = new()
                full = lambda: fused_experts(x, w1, w2, tw, ids, use_fp8_w8a8=True, w1_scale=w1_s, w2_scale=w2_s,
                                             block_shape=[128, 128])
                experts = f"{bench.time_gpu_graph(full, 4) * 1e6:9.1f}"
            emit(f"  {name:13s} {tokens:6d} | {gn:9.2f} {go:8.2f} {go / gn:6.2f} | {en:9.2f} {eo:8.2f} {eo / en:6.2f} | "
                 f"{spread:6.3f} | {bad:3d}, {err:.2e} | {experts}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
