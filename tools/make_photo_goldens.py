#!/usr/bin/env python3
"""Generate tests/golden/photo.npz: the REFERENCE's own SphericalSweepStdMasked.sweep (spherical_sweep_avg.py:38-135; CPU, fp32) on
the camera images as features, for every case of tests/photo_cases.py.

    MVSGI_REFERENCE=<checkout of the reference> python tools/make_photo_goldens.py

Per case the class is given: feats = the images as fp32 [B, N, C, Hr, Wr] (uint8 / 255, as the facade converts), grids = the grids
of the back-projection chain as [B, N, 1, H, W, 2] (one "candidate": the predicted distance), grid_masks = the chain's valid, masks =
ones (the case's camera masks where it has some).  Its output [B, C, 1, H, W] is var_c of the definition.  Only data leaves this
script: that array and the sha256 of the inputs (which the tests regenerate from the seed).  The reference's code is imported, never
copied (import recipe as in tools/make_goldens.py).  Prints, per case, the distance from tests/photo_cases.restate."""
import hashlib
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

import photo_cases as PC  # noqa: E402
import reproject_cases as RC  # noqa: E402


def digest(inp) -> str:
    h = hashlib.sha256()
    for k in ("inv", "imgs", "cam_masks", "mask"):
        if inp[k] is not None:
            h.update(inp[k].numpy().tobytes())
    return h.hexdigest()


def main():
    out = {}
    for name in PC.CASES:
        s = PC.spec(name)
        inp = PC.make_inputs(name)
        ch = PC.chain(name, inp)
        B, N, (H, W) = s["B"], s["N"], s["hw"]
        feats = RC.as_f32_chw(inp["imgs"]).reshape(B, N, s["C"], *s["img"])
        masks = torch.ones((B, N, 1, *s["img"])) if inp["cam_masks"] is None else inp["cam_masks"].unsqueeze(0).repeat(B, 1, 1, 1, 1)
        cvb = SphericalSweepStdMasked(num_cams=N, feat_chs=s["C"], post_k_sz=3).eval()
        with torch.no_grad():
            vol = cvb.sweep(feats, ch["grid"].unsqueeze(2), ch["valid"].unsqueeze(2).unsqueeze(-1), masks)
        var_c = vol[:, :, 0].contiguous()
        out[f"{name}/var_c"] = var_c.numpy()
        out[f"{name}/sha256"] = np.asarray(digest(inp))
        r = PC.restate(ch["warped"], ch["seen"])
        print(f"  {name:14s} var_c {tuple(var_c.shape)}  max |reference - restatement| = {float((var_c - r['var_c']).abs().max()):.3e}")
    path = os.path.join(OUT, "photo.npz")
    np.savez_compressed(path, **out)
    print(f"  {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
