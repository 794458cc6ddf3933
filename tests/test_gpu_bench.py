"""GPU test of a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run (in-process, smallest K / W):
the result line carries the headline only, `ms_per_step` and `value` describe the same K steps, and the dumped
array is what `PagedAttention.forward_decode` returns for the benchmark's seeded inputs at the last timed step --
bit for bit, since two builds are compared through these files."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_output(tmp_path, capsys):
    import bench
    from vllm_amd.attention import PagedAttention
    K, W = 3, 1
    bench.main(["--gpus", "1", "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == K and line["warmup"] == W and line["n_gpus"] == 1
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and "fp8" in line["dtype"]
    assert "extra" not in line and "cpu_baseline" not in line and "cold" not in line["roofline"]
    S, ctx, H, KVH, D, BS = 64, 4096, 32, 8, 128, 16
    nbytes = bench.attention_bytes(S, ctx, H, KVH, D, BS, 1)
    # value = bytes / wall and ms_per_step = wall / K of the same K steps; the line rounds ms_per_step to 1e-5 ms
    # and value to 0.1 GB/s
    assert line["ms_per_step"] > 0
    expect = nbytes / (line["ms_per_step"] * 1e-3) / 1e9
    assert abs(line["value"] - expect) <= expect * (1e-5 / line["ms_per_step"]) + 0.1

    assert os.listdir(tmp_path) == ["decode_out.npy"]
    out = np.load(tmp_path / "decode_out.npy")
    assert out.dtype == np.float32 and out.shape == (S, H, D) and np.abs(out).max() > 0
    q, caches, bt, sl, one = bench.make_attention_inputs(S, ctx, H, KVH, D, BS, True, torch.device("cuda", 0))
    kc, vc = caches[(W + K - 1) % len(caches)]      # the two caches alternate; an even number of untimed launches precedes W
    ref = PagedAttention.forward_decode(q, kc, vc, bt, sl, ctx, "fp8", KVH, D ** -0.5, None, one, one)
    assert np.array_equal(out, ref.float().cpu().numpy())
