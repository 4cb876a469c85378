"""CPU: the soft-argmin at any interp_scale_factor -- the golden file of the reference's regressor at factors 4, 3, 8, 1.5, 2.5
and 0.5 (tools/make_regress_scale_goldens.py), the coordinate rule the HIP kernels are written from restated in NumPy against
those goldens, and the Python surface (PathConfig, drop-in constructor)."""
import dataclasses
import math
import os

import numpy as np
import pytest

from mvs_gi_amd import dropin
from mvs_gi_amd.configs import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "regress_scales.npz"))


def _axis(n_in: int, n_out: int, rs):
    """F.interpolate(scale_factor=s, bilinear, align_corners=False) along one axis, every step in fp32:
    src = max((dst + 0.5) * (1 / s) - 0.5, 0), i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1."""
    dst = np.arange(n_out, dtype=f32)
    src = np.maximum((dst + f32(0.5)) * rs - f32(0.5), f32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(f32)
    return i0, i1, f32(1) - l1, l1


def soft_argmin_numpy(costs, inv_idx, s: float):
    """costs [B, D, H, W] fp32 -> (inv_dist [B, 1, OH, OW], norm_costs [B, D, OH, OW]); the blend in the order of the kernels'
    sample(): ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11)."""
    B, D, H, W = costs.shape
    OH, OW = math.floor(H * s), math.floor(W * s)
    rs = f32(1.0 / s)                                   # 1 / s in double, rounded to fp32 once
    y0, y1, ly0, ly1 = _axis(H, OH, rs)
    x0, x1, lx0, lx1 = _axis(W, OW, rs)
    ra, rb = costs[:, :, y0], costs[:, :, y1]
    up = ly0[:, None] * (lx0 * ra[..., x0] + lx1 * ra[..., x1]) + ly1[:, None] * (lx0 * rb[..., x0] + lx1 * rb[..., x1])
    e = np.exp(up - up.max(axis=1, keepdims=True))
    pr = e / e.sum(axis=1, keepdims=True)
    return (pr * inv_idx.reshape(1, -1, 1, 1)).sum(axis=1, keepdims=True), pr


def test_golden_file_rows_and_output_sizes(z):
    factors = [float(f) for f in z["factors"]]
    assert factors == [4, 4, 4, 4, 4, 3, 8, 1.5, 2.5, 0.5]
    shapes = [tuple(z[f"costs_{i}"].shape) for i in range(len(factors))]
    assert shapes == [(2, 1, 16, 10, 40), (1, 1, 8, 5, 9), (1, 1, 32, 6, 12), (1, 1, 48, 4, 8), (1, 1, 16, 1, 7), (1, 1, 10, 5, 9),
                      (1, 1, 10, 5, 9), (1, 1, 16, 7, 13), (1, 1, 16, 7, 13), (1, 1, 16, 7, 13)]
    for i, (s, (B, _, D, H, W)) in enumerate(zip(factors, shapes)):
        OH, OW = math.floor(H * s), math.floor(W * s)
        assert tuple(z[f"inv_{i}"].shape) == (B, 1, OH, OW) and z[f"inv_{i}"].dtype == np.float32
        assert len(z[f"dist_cands_{i}"]) == D
        if f"pr_{i}" in z:
            assert tuple(z[f"pr_{i}"].shape) == (B, D, OH, OW)
    assert [tuple(z[f"inv_{i}"].shape[2:]) for i in (7, 8, 9)] == [(10, 19), (17, 32), (3, 6)]
    assert sum(f"pr_{i}" in z for i in range(len(factors))) >= 9          # all but the [2, 16, 40, 160] one
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "regress_scales.npz")) < 1 << 20


def test_coordinate_rule_reproduces_the_reference(z):
    for i, s in enumerate(z["factors"]):
        inv_idx = (float(z["bf"]) / z[f"dist_cands_{i}"]).astype(f32)
        inv, pr = soft_argmin_numpy(z[f"costs_{i}"][:, 0], inv_idx, float(s))
        e_inv = _rel(inv, z[f"inv_{i}"])
        e_pr = _rel(pr, z[f"pr_{i}"]) if f"pr_{i}" in z else 0.0
        print(f"row {i} x{float(s):g}: inv_dist {e_inv:.2e} norm_costs {e_pr:.2e}")
        assert inv.shape == z[f"inv_{i}"].shape
        assert e_inv <= 1e-5 and e_pr <= 1e-5, (i, float(s), e_inv, e_pr)


def test_path_config_takes_any_factor():
    base = CONFIGS["G16V"]
    assert base.interp_scale_factor == 2
    for s in (4, 1.5):
        cfg = dataclasses.replace(base, interp_scale_factor=s)
        assert cfg.interp_scale_factor == s and cfg.pre_interp and cfg.dist_cands == base.dist_cands
    assert {f.name: f.type for f in dataclasses.fields(base)}["interp_scale_factor"] in (float, "float")


def test_dropin_regressor_constructs_with_factor_4():
    dr = dropin.DistanceRegressorWithFixedCandidates(bf=96, dist_cands=[0.5, 1, 2, 4], interp_scale_factor=4, pre_interp=True)
    assert dr.interp_scale_factor == 4 and dr.pre_interp is True and dr.bf == 96
    assert list(dr.state_dict()) == ["inv_dist_idx"] and tuple(dr.inv_dist_idx.shape) == (1, 4, 1, 1)
    assert dropin.DistanceRegressorWithFixedCandidates(interp_scale_factor=2.5, pre_interp=True).interp_scale_factor == 2.5
