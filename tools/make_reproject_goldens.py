#!/usr/bin/env python3
"""Golden vectors for the back-projection (csrc/reproject.hip), produced by the REFERENCE's own closed forms on the CPU:
dsta_mvs/support/dataset/torch_cuda_sweep.py (RayMaker_UEPanorama, transform_3D_points_torch, DoubleSphereSampleGridMaker,
EquirectangularSampleGridMaker; loaded through the mvs_utils stand-ins of tools/make_grid_goldens.py) and
dsta_mvs/model/backports/backports.py (bilinear_grid_sample).

SphericalSweepStereo._create_warped_inputs (spherical_sweep_stereo.py:417-471) projects through mvs_utils camera models, which
this build cannot load; what is stored is the composition stated in tests/reproject_cases.py evaluated with the reference's
functions.  The division, the multiply by the rays, the |g| <= 1 clause of `valid` and the select of the invalid value are the
definition's own (plain torch here).  Data only.

  python tools/make_reproject_goldens.py      ->  tests/golden/reproject.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_grid_goldens as MG  # noqa: E402
import make_resample_goldens as MR  # noqa: E402
import reproject_cases as RC  # noqa: E402


def main():
    R = MG.load_reference()
    BP = MR.load_backports()
    ds = R.DoubleSphereSampleGridMaker(params=list(RC.DS_PARAMS), calib_shape=list(RC.DS_CALIB))
    eq = R.EquirectangularSampleGridMaker()
    makers = (R.transform_3D_points_torch, lambda q, params, calib: ds.make_grid(q), eq.make_grid)
    out = {}
    for name, c in RC.CASES.items():
        H, W = c["hw"]
        rays = R.RayMaker_UEPanorama(np.ones(1, np.float32), RC.LON, RC.LAT).make_rays_for_candidates((H, W))[:, 0]
        T = torch.stack([p.inverse().to(torch.float32) for p in RC.poses(name)])
        inv, imgs = RC.make_inputs(name)
        r = RC.compose(name, inv, None, ray_table=rays, T=T, makers=makers)
        B, N = c["B"], c["N"]

        def sample(invalid):
            s = BP.bilinear_grid_sample(RC.as_f32_chw(imgs), r["grid"].reshape(B * N, H, W, 2), align_corners=False)
            s = torch.where(r["valid"].reshape(B * N, 1, H, W), s, torch.tensor(invalid, dtype=torch.float32))
            return s.reshape(B, N, -1, H, W)

        arrays = dict(inv=inv, imgs=imgs, rays=rays, T=T, xyz=r["xyz"], grid=r["grid"], in_fov=r["in_fov"], valid=r["valid"],
                      warped=sample(0.0), warped_neg=sample(RC.INVALID_OTHER))
        assert tuple(arrays) == RC.STORED
        for k, t in arrays.items():
            out[f"{name}_{k}"] = t.numpy()
        share = [round(float(r["valid"][:, n].float().mean()), 3) for n in range(N)]
        print(f"{name}: valid share per camera {share}")
    p = os.path.join(ROOT, "tests", "golden", "reproject.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
