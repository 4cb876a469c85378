#!/usr/bin/env python3
"""Generate tests/golden/wide_rig.npz: the REFERENCE's own SphericalSweepStdMasked(num_cams=N).sweep (CPU, fp32) for rigs of
5, 6, 7 and 8 cameras on the seeded small cases of tests/wide_rig_cases.py.

    MVSGI_REFERENCE=<checkout of the reference> python tools/make_wide_rig_goldens.py

Only data leaves this script: the reference's outputs and the sha256 of the inputs (which the tests regenerate from the seed).
The reference's code is imported, never copied (import recipe as in tools/make_goldens.py).
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
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

from dsta_mvs.model.cost_volume_builder import SphericalSweepStdMasked  # noqa: E402

import wide_rig_cases as W  # noqa: E402


def main():
    out = {}
    for N in W.NS:
        inp = W.small_case(N)
        C = inp["feats"].shape[2]
        cvb = SphericalSweepStdMasked(num_cams=N, feat_chs=C, post_k_sz=3).eval()
        with torch.no_grad():
            vol = cvb.sweep(*(torch.from_numpy(inp[k]) for k in ("feats", "grids", "grid_masks", "masks")))
        out[f"vol_raw_{N}"] = vol.numpy()
        out[f"inputs_sha256_{N}"] = np.asarray(W.digest(inp))
        print(f"  N = {N}: feats {inp['feats'].shape} -> vol_raw {tuple(vol.shape)}")
    path = os.path.join(OUT, "wide_rig.npz")
    np.savez_compressed(path, **out)
    print(f"  {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
