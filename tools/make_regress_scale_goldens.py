#!/usr/bin/env python3
"""Generate tests/golden/regress_scales.npz: the REFERENCE's own DistanceRegressorWithFixedCandidates (CPU, fp32,
pre_interp=True) at interp_scale_factor 4, 3, 8, 1.5, 2.5 and 0.5 on small seeded cost volumes.

    MVSGI_REFERENCE=<checkout of the reference> python tools/make_regress_scale_goldens.py

Only data leaves this script: the factors, the inputs and the reference's outputs.  The reference's code is imported, never
copied (import recipe as in tools/make_goldens.py).  norm_costs is stored for the rows where it has at most PR_MAX elements (all but the [2, 16, 40, 160] one), which keeps the file
under half a megabyte.
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

tv, ops = types.ModuleType("torchvision"), types.ModuleType("torchvision.ops")
def _absent(*a, **k):
    raise NotImplementedError("torchvision not installed")
ops.deform_conv2d = _absent
tv.ops = ops
sys.modules.setdefault("torchvision", tv)
sys.modules.setdefault("torchvision.ops", ops)

from dsta_mvs.model.distance_regressor.distance_regressor import DistanceRegressorWithFixedCandidates  # noqa: E402

# (factor, costs shape [B, 1, D, H, W])
ROWS = [(4, (2, 1, 16, 10, 40)),      # product case, vector path (W % 4 == 0)
        (4, (1, 1, 8, 5, 9)),         # odd W, scalar tails, D <= 16
        (4, (1, 1, 32, 6, 12)),       # D <= 32 regime
        (4, (1, 1, 48, 4, 8)),        # D > 32: three passes
        (4, (1, 1, 16, 1, 7)),        # H = 1: both rows clamp to row 0
        (3, (1, 1, 10, 5, 9)),        # other integer factors, odd D
        (8, (1, 1, 10, 5, 9)),
        (1.5, (1, 1, 16, 7, 13)),     # thread-per-pixel path, floor() output sizes 10 x 19, 17 x 32, 3 x 6
        (2.5, (1, 1, 16, 7, 13)),
        (0.5, (1, 1, 16, 7, 13))]
BF = 96.0
PR_MAX = 40000


def main():
    rng = np.random.default_rng(4178)
    out = dict(factors=np.asarray([f for f, _ in ROWS], np.float64), bf=np.asarray(BF))
    for i, (f, shape) in enumerate(ROWS):
        costs = (rng.standard_normal(shape) * 3).astype(np.float32)
        cands = np.geomspace(0.5, 100.0, shape[2])
        dr = DistanceRegressorWithFixedCandidates(bf=BF, dist_cands=[float(c) for c in cands], interp_scale_factor=f,
                                                  pre_interp=True).eval()
        with torch.no_grad():
            inv, pr = dr(torch.from_numpy(costs))
        out[f"costs_{i}"], out[f"dist_cands_{i}"] = costs, cands
        out[f"inv_{i}"] = inv.numpy()
        if pr.numel() <= PR_MAX:
            out[f"pr_{i}"] = pr.numpy()
        print(f"  row {i}: x{f} {shape} -> inv {tuple(inv.shape)} norm_costs {tuple(pr.shape)}")
    path = os.path.join(OUT, "regress_scales.npz")
    np.savez_compressed(path, **out)
    print(f"  {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
