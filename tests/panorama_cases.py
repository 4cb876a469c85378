"""What the cases of the stages over the rig panorama share (temporal_cases.py, tsdf_cases.py): the constants, the affine map, the ray
table, rotations, the seeded bad values, and the numpy restatement of the panorama cell (csrc/panorama_map.hpp's pano_cell,
dropin.reproject.panorama_cell).  TEST INFRASTRUCTURE ONLY.

The cell of a point q of the rig frame (include/mvsgi.h, "temporal fusion", step A4); fp32, one IEEE operation per written operation:
    xz = sqrt(qx qx + qz qz), lon = -1 * atan2(qz, qx), lat = atan2(qy, xz), gx = lon / pi, gy = (2 * lat) / pi;
    u = gx * au + bu, v = gy * av + bv; cx = floor(u), cy = floor(v); wrap: cx += W when cx < 0, cx -= W when cx >= W;
    inside = 0 <= cx < W and 0 <= cy < H
The one operation that is not correctly rounded everywhere is atan2: numpy's and the device's may differ in the last bits, which moves
a cell only when a coordinate sits within that of a cell's edge.
"""
import math

import numpy as np

from oracle import grid_oracle as G

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
PI_F = F32(np.pi)
BAD = (0.0, -1.0, float("nan"), float("inf"))
FULL = ((-math.pi, math.pi), (0.0, math.pi))
PART = ((-math.pi / 2, math.pi / 2), (math.pi / 4, 3 * math.pi / 4))


def affine(ranges, hw):
    """(au, bu, av, bv) as float32, each rounded once from float64, and wrap: include/mvsgi.h's formulas"""
    (lo0, lo1), (la0, la1) = ranges
    Hh, W = hw
    c = (math.pi * W / (lo1 - lo0), -lo0 * W / (lo1 - lo0), (math.pi / 2) * Hh / (la1 - la0), (math.pi / 2 - la0) * Hh / (la1 - la0))
    return tuple(F32(v) for v in c) + (abs(lo1 - lo0 - 2 * math.pi) < 1e-6,)


def rays(ranges, hw):
    """The rig panorama's ray table [3, H, W] float32"""
    return G.rays_panorama(np.ones(1, np.float32), ranges[0], ranges[1], hw)[:, 0].numpy()


def _rot(yaw=0.0, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])               # about the vertical: longitude theta -> theta + yaw
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def _seed_bad(rng, a, frac, keep=None):
    flat = a.reshape(-1)
    if frac:
        pos = rng.permutation(flat.size)[:max(int(round(frac * flat.size)), len(BAD))]
        flat[pos] = np.asarray(BAD, F32)[np.arange(pos.size) % len(BAD)]
    if keep is not None and frac:                                     # the same bad values at chosen places
        for k, at in enumerate(keep):
            flat[at] = F32(BAD[k % len(BAD)])


def cell(qx, qy, qz, aff, hw):
    """-> fx, fy (whole floats: column, row), inside, u, v of float32 arrays qx, qy, qz"""
    Hh, W = hw
    au, bu, av, bv, wrap = aff
    with np.errstate(all="ignore"):
        xz = np.sqrt(qx * qx + qz * qz)
        lon = F32(-1.0) * np.arctan2(qz, qx)
        lat = np.arctan2(qy, xz)
        gx = lon / PI_F
        gy = (F32(2.0) * lat) / PI_F
        u = gx * au + bu
        v = gy * av + bv
        fx, fy = np.floor(u), np.floor(v)
        if wrap:
            fx = np.where(fx < 0, fx + F32(W), np.where(fx >= W, fx - F32(W), fx))
        inside = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < Hh)
    assert all(a.dtype == F32 for a in (xz, lon, lat, gx, gy, u, v, fx, fy))
    return fx, fy, inside, u, v
