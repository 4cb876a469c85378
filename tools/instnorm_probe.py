#!/usr/bin/env python3
"""G16V with norm_type='instance' against the batch-norm model on the same device: frames/s of a hipGraph replay at
B = 1, 16, 128, instance-norm launches per frame, and the time / effective bandwidth of the two norm kernels
(mvsgi_instance_norm_f32) on the largest layers.  One JSON line per measurement.

    python tools/instnorm_probe.py [--batches 1,16,128] [--steps 20]
For the kernel trace: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/instnorm_probe.py --batches 1 --steps 5
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mvs_gi_amd import hip_ops as H, synth  # noqa: E402
from mvs_gi_amd.configs import CONFIGS, PathConfig  # noqa: E402
from mvs_gi_amd.pipeline import HotPath  # noqa: E402


def fps(cfg, B, steps, warmup=3):
    inp = synth.make_inputs(cfg, seed=0, batch=1)
    hp = HotPath(cfg, synth.make_weights(cfg, seed=0), inp, device="cuda:0")
    feats = torch.from_numpy(inp["feats"]).to("cuda:0").expand(B, *inp["feats"].shape[1:]).contiguous()
    calls = [0]
    real = H.instance_norm

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    H.instance_norm = counted
    try:
        hp(feats)
        torch.cuda.synchronize()
    finally:
        H.instance_norm = real
    hp.capture(feats)
    for _ in range(warmup):
        hp.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        hp.replay()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    return dict(norm=cfg.norm_type, B=B, ms_per_step=ms, frames_per_s=B * 1000.0 / ms, norm_calls_per_forward=calls[0],
                norm_launches_per_forward=2 * calls[0])


def kernel(B, S, C, reps=50):
    x = torch.randn(B, S, C, device="cuda:0")
    res = torch.randn_like(x)
    for r in (None, res):
        H.instance_norm(x, r, out=x)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            H.instance_norm(x, r, neg_slope=0.01, out=x)
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1000.0 / reps
        passes = 3 + (1 if r is not None else 0)      # statistics read, apply read + write (+ residual read)
        yield dict(kernel="instance_norm(stats+apply)", B=B, S=S, C=C, res=r is not None, us=us,
                   eff_TBps=passes * x.numel() * 4 / (us * 1e-6) / 1e12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,128")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    base = CONFIGS["G16V"]
    inst = PathConfig(**{**base.__dict__, "norm_type": "instance"})
    for B in (int(b) for b in a.batches.split(",")):
        for cfg in (base, inst):
            print(json.dumps(fps(cfg, B, a.steps)), flush=True)
            torch.cuda.empty_cache()
    if not a.no_kernels:
        # post_vol / out_costs.0 output (16 x 80 x 320 x 16) and level 0 (8 x 40 x 160 x 32), one frame and 16 frames
        for B in (1, 16):
            for S, C in ((16 * 80 * 320, 16), (8 * 40 * 160, 32)):
                for row in kernel(B, S, C):
                    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
