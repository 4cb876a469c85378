#!/usr/bin/env python3
"""Generate tests/golden/confidence_*.npz: the REFERENCE's own DistanceRegressorWithFixedCandidates (CPU, fp32, pre_interp=True)
on small seeded cost volumes, its norm_costs, and the four confidence maps derived from that norm_costs in float64.

    MVSGI_REFERENCE=<checkout of the reference> python tools/make_confidence_goldens.py

Only data leaves this script: the inputs, the reference's output and arithmetic on it.  The reference's code is imported, never
copied (import recipe as in tools/make_goldens.py).  Rows and file names come from tests/confidence_cases.py.
Each file: costs [B, 1, D, H, W] fp32, dist_cands [D] float64, bf, factor, norm_costs [B, D, OH, OW] fp32 (the reference's), and from
it in float64 max_prob = max_d p_d, entropy = -sum p_d ln p_d, spread = sqrt(sum p_d (w_d - mu)^2) with w = the module's
inv_dist_idx and mu = sum p_d w_d, argmax = the lowest index of the largest p_d (int32), each [B, 1, OH, OW].
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("MVSGI_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "dsta_mvs")):
    sys.exit("set MVSGI_REFERENCE to a checkout of the reference (the directory that holds dsta_mvs/)")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))

tv, ops = types.ModuleType("torchvision"), types.ModuleType("torchvision.ops")
def _absent(*a, **k):
    raise NotImplementedError("torchvision not installed")
ops.deform_conv2d = _absent
tv.ops = ops
sys.modules.setdefault("torchvision", tv)
sys.modules.setdefault("torchvision.ops", ops)

from dsta_mvs.model.distance_regressor.distance_regressor import DistanceRegressorWithFixedCandidates  # noqa: E402

import confidence_cases as CC  # noqa: E402


def main():
    for i, (shape, f) in enumerate(CC.GOLDEN_ROWS):
        B, D, H, W = shape
        rng = np.random.default_rng(5309 + i)
        costs = (rng.standard_normal((B, 1, D, H, W)) * 4).astype(np.float32)
        cands = np.geomspace(0.5, 100.0, D)
        dr = DistanceRegressorWithFixedCandidates(bf=CC.BF, dist_cands=[float(c) for c in cands], interp_scale_factor=f,
                                                  pre_interp=True).eval()
        with torch.no_grad():
            _, pr = dr(torch.from_numpy(costs))
        p = pr.numpy().astype(np.float64)
        w = dr.inv_dist_idx.numpy().astype(np.float64).reshape(1, -1, 1, 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ent = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(axis=1, keepdims=True)
        mu = (p * w).sum(axis=1, keepdims=True)
        spread = np.sqrt((p * (w - mu) ** 2).sum(axis=1, keepdims=True))
        path = os.path.join(OUT, CC.golden_name(shape, f))
        np.savez_compressed(path, costs=costs, dist_cands=cands, bf=np.asarray(CC.BF), factor=np.asarray(float(f)), norm_costs=pr.numpy(),
                            max_prob=p.max(axis=1, keepdims=True), entropy=ent, spread=spread,
                            argmax=p.argmax(axis=1)[:, None].astype(np.int32))
        print(f"  {path}: x{f} {shape} -> norm_costs {tuple(pr.shape)}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
