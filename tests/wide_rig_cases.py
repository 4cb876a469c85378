"""Seeded inputs of the 5- to 8-camera masked-variance sweep, shared by tools/make_wide_rig_goldens.py (which runs the REFERENCE's
SphericalSweepStdMasked(num_cams=N).sweep on them), tests/test_wide_rig_host.py and tests/test_gpu_wide_rig.py (which regenerate
the bit-identical arrays).  Only the reference's outputs and the inputs' digest are stored (tests/golden/wide_rig.npz).

The grid masks are NOT independent per camera: per voxel a count k in 0 .. N is drawn uniformly and k cameras, chosen by a random
permutation, are set true -- so every count of valid cameras occurs often (independent Bernoulli(0.8) masks would put 99 % of the
voxels at "two or more valid" and leave the n = 0 and n = 1 branches of spherical_sweep_avg.py:108-125 untested)."""
import hashlib

import numpy as np

from mvs_gi_amd.configs import DIST_8L, PathConfig

NS = (5, 6, 7, 8)
GOLDEN_C = {5: 16, 6: 8, 7: 8, 8: 16}          # channels of the golden case per camera count
B, HI, WI, D, HO, WO, HM, WM = 2, 12, 20, 4, 6, 70, 24, 40      # Wo 70: two w-tiles, the second 6 voxels wide


def small_case(N: int, C: int = None, shape=None, seed: int = None) -> dict:
    """feats [B, N, C, Hi, Wi] standard normal, grids [B, N, D, Ho, Wo, 2] uniform in [-1.15, 1.15] (taps outside the image on
    every side), grid_masks [B, N, D, Ho, Wo, 1] bool with a uniformly drawn count of true cameras per voxel, masks
    [B, N, 1, Hm, Wm] Bernoulli(0.9) as fp32.  shape = (B, Hi, Wi, D, Ho, Wo, Hm, Wm) overrides the small shape, `seed` the
    generator's (100 + N)."""
    C = GOLDEN_C[N] if C is None else C
    b, hi, wi, d, ho, wo, hm, wm = shape or (B, HI, WI, D, HO, WO, HM, WM)
    rng = np.random.default_rng(100 + N if seed is None else seed)
    feats = rng.standard_normal((b, N, C, hi, wi)).astype(np.float32)
    grids = rng.uniform(-1.15, 1.15, (b, N, d, ho, wo, 2)).astype(np.float32)
    masks = (rng.random((b, N, 1, hm, wm)) < 0.9).astype(np.float32)
    k = rng.integers(0, N + 1, (b, 1, d, ho, wo))
    rank = np.argsort(np.argsort(rng.random((b, N, d, ho, wo)), axis=1), axis=1)      # a random permutation of the cameras per voxel
    grid_masks = (rank < k)[..., None]
    return dict(feats=feats, grids=grids, grid_masks=np.ascontiguousarray(grid_masks), masks=masks)


def digest(inp: dict) -> str:
    h = hashlib.sha256()
    for key in ("feats", "grids", "grid_masks", "masks"):
        a = np.ascontiguousarray(inp[key])
        h.update(key.encode() + str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def whole_path_cfg(N: int) -> PathConfig:
    return PathConfig("wide", N, "std", 16, 32, DIST_8L, feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32))
