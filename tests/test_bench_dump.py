"""CPU: bench.py's options and --dump-outputs on host tensors -- which frames are written, in what type, within what size."""
import os

import numpy as np
import torch

import bench


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_frames_fixed_sample_within_budget():
    assert bench.dump_frames(8, 1000) == list(range(8))
    f = bench.dump_frames(256, 7_000_000)
    assert f == bench.dump_frames(256, 7_000_000) and len(f) == 8 and f[0] == 0 and f[-1] == 255 and f == sorted(set(f))
    assert len(bench.dump_frames(256, 7_000_000)) * 7_000_000 <= bench.DUMP_BYTES
    assert bench.dump_frames(5, 10 * bench.DUMP_BYTES) == [0]


def test_dump_outputs_writes_the_parts_frames_in_order(tmp_path):
    g = torch.Generator().manual_seed(0)
    # two parts of 3 frames, inv_dist [B, 1, H, W] and norm_costs [B, D, H, W]
    parts = [(torch.rand(3, 1, 4, 6, generator=g), torch.rand(3, 5, 4, 6, generator=g)) for _ in range(2)]
    shapes, frames = bench.dump_outputs(str(tmp_path), parts, torch, np)
    assert frames == list(range(6)) and shapes == {"inv_dist": [6, 1, 4, 6], "norm_costs": [6, 5, 4, 6]}
    for i, name in enumerate(bench.OUTPUT_NAMES):
        x = np.load(os.path.join(tmp_path, name + ".npy"))
        assert x.dtype == np.float32
        assert np.array_equal(x, torch.cat([p[i] for p in parts]).numpy())


def test_dump_outputs_samples_a_large_step(tmp_path, monkeypatch):
    parts = [(torch.arange(k * 4 * 24, (k + 1) * 4 * 24, dtype=torch.float32).reshape(4, 1, 4, 6), None) for k in range(2)]
    # a step over the budget: dump_frames(8 frames of 24 floats) picks 3 of them, across both parts
    monkeypatch.setattr(bench, "dump_frames", lambda n, b: [0, 5, 7] if (n, b) == (8, 4 * 24) else None)
    shapes, frames = bench.dump_outputs(str(tmp_path), parts, torch, np)
    assert frames == [0, 5, 7] and shapes == {"inv_dist": [3, 1, 4, 6]}
    assert sorted(os.listdir(tmp_path)) == ["inv_dist.npy"]
    x = np.load(os.path.join(tmp_path, "inv_dist.npy"))
    assert np.array_equal(x[:, 0, 0, 0], np.array([0, 5, 7]) * 24.0)
