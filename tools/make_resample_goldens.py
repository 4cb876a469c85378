#!/usr/bin/env python3
"""Golden vectors for the fisheye -> surrogate-view resampler, produced by the REFERENCE's own closed forms:
dsta_mvs/support/dataset/torch_cuda_sweep.py (transform_3D_points_torch, DoubleSphereSampleGridMaker; loaded through the
mvs_utils stand-ins of tools/make_grid_goldens.py) and dsta_mvs/model/backports/backports.py (bilinear_grid_sample, loaded
by file path: it imports torch only).

The reference's image_sampler package is an empty submodule, so the resampler is defined as the composition stated in
tests/resample_cases.py; what is stored is that composition evaluated with the reference's functions.  The surrogate rays,
the |g| <= 1 clause of `valid` and the select of the invalid value are the definition's own (plain torch here).  Data only.

  python tools/make_resample_goldens.py      ->  tests/golden/resample.npz
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_grid_goldens as MG  # noqa: E402
import resample_cases as RC  # noqa: E402


def load_backports():
    spec = importlib.util.spec_from_file_location(
        "dsta_mvs_ref_backports", os.path.join(MG.REF, "dsta_mvs", "model", "backports", "backports.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    R = MG.load_reference()
    BP = load_backports()
    out = {}
    for name, c in RC.CASES.items():
        H, W = c["out"]
        rays = RC.surrogate_rays(H, W)
        # the rays are pixel centres of the equirect projection the sweep uses: grid_equirect(p) = (u, v)
        uv = R.EquirectangularSampleGridMaker().make_grid(rays.view(1, 3, 1, H, W))[0, 0]
        u = (2 * torch.arange(W) + 1).float() / W - 1
        v = (2 * torch.arange(H) + 1).float() / H - 1
        err = max(float((uv[..., 0] - u.view(1, W)).abs().max()), float((uv[..., 1] - v.view(H, 1)).abs().max()))
        assert err <= 2e-7, err
        rot = RC.rotation(*c["ypr"])
        pts = R.transform_3D_points_torch(RC.transform4(rot), rays.view(1, 3, 1, H, W))
        grid, ds = R.DoubleSphereSampleGridMaker(params=list(c["params"]), calib_shape=list(c["raw"])).make_grid(pts)
        assert bool(torch.isfinite(grid).all())
        g1 = grid[0]                                   # [1, H, W, 2]: the grid of a batch of one image
        ds = ds[0, 0]
        valid = ds & (g1[0, ..., 0].abs() <= 1) & (g1[0, ..., 1].abs() <= 1)

        def sample(img_chw, invalid):
            s = BP.bilinear_grid_sample(img_chw.unsqueeze(0), g1, align_corners=False)
            return torch.where(valid.view(1, 1, H, W), s, torch.tensor(invalid, dtype=torch.float32))

        img, smooth, mask = RC.make_images(name)
        f = img.permute(2, 0, 1).float() / 255.0       # inference_pytorch.py:58-59
        m, _ = sample((mask * 255).unsqueeze(0), 0.0), None          # sample_masks, multi_view_camera_model_dataset.py:431-434
        m[m > 0] = 1.0
        arrays = dict(rays=rays, R=torch.from_numpy(rot), grid=g1[0], ds_mask=ds, valid=valid, img=img, out=sample(f, 0.0),
                      out_neg=sample(f, RC.INVALID_OTHER), smooth=smooth,
                      out_smooth=sample(smooth.permute(2, 0, 1).float() / 255.0, 0.0), mask=mask, out_mask=m.squeeze(0))
        assert tuple(arrays) == RC.STORED
        for k, t in arrays.items():
            out[f"{name}_{k}"] = t.numpy()
        # taps straddling the raw image border among the valid pixels
        x = ((g1[0, ..., 0] + 1) * c["raw"][1] - 1) / 2
        y = ((g1[0, ..., 1] + 1) * c["raw"][0] - 1) / 2
        straddle = valid & ((x < 0) | (x > c["raw"][1] - 1) | (y < 0) | (y > c["raw"][0] - 1))
        print(f"{name}: valid share {float(valid.float().mean()):.2f}, {int(straddle.sum())} valid pixels straddle the border, "
              f"equirect round trip {err:.1e}")
    p = os.path.join(ROOT, "tests", "golden", "resample.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
