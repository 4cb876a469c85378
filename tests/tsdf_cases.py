"""Cases and numpy restatement of the volumetric fusion (mvs_gi_amd/dropin/tsdf.py, csrc/tsdf.hip).  TEST INFRASTRUCTURE ONLY.

Definition (include/mvsgi.h, "volumetric fusion"), sequence b; fp32, one IEEE operation per written operation
(every array below is float32 and numpy does not contract; the fused multiply-adds of a transform's row are grid_exact_cases.fma_f32):
  integrate, slot s of the toroidal store [Nz, Ny, Nx, 2]:
    1. i = origin + ((s - origin) mod N) per axis (floored); fresh = i outside [origin_prev, origin_prev + N) on some axis;
       (f, w) = fresh ? (1, 0) : vol[s]
    2. c = (float(i) + 0.5) * vs; q = T c (per row fma(t2, z, fma(t1, y, t0 * x)) + t3); r2 = (qx qx + qy qy) + qz qz, rejected unless
       0 < r2 <= FLT_MAX; r = sqrt(r2), rejected unless r_min <= r <= r_max
    3. the panorama cell of q (panorama_cases.cell, the temporal splat's step 4: the projection, the affine map, floor, the column
       wrapped once); rejected outside the map
    4. m = inv[cell]; rejected where mask[cell] == 0; d = bf / m; rejected unless 0 < m <= FLT_MAX and d <= FLT_MAX
    5. sdf = d - r; rejected if sdf < -trunc; obs = min(sdf, trunc) / trunc
    6. w_obs = 1, or with std: sig = std[cell] * d / m, w_obs = t2 / (t2 + sig * sig), rejected unless 0 < w_obs <= 1
    7. W = w + w_obs; f' = (f * w + obs * w_obs) / W; w' = min(W, w_max);    8. a rejected voxel keeps the (f, w) of step 1
  raycast, pixel (i, j):
    1. dir = R_P ray (the row without its translation), o = P[:3, 3]
    2. t_k = t0 + float(k) * step; p = o + dir * t_k; g = floor(p * inv_vs); inside = origin <= g < origin + N on every axis;
       (f_k, w_k) = the pair of slot g mod N; valid_k = inside and w_k >= w_min
    3. the first k >= 1 with valid_k, valid_{k-1}, f_{k-1} > 0 and f_k <= 0: t* = t_{k-1} + step * (f_{k-1} / (f_{k-1} - f_k)),
       inv = bf / t*, weight = w_k, steps = k; without: 0, 0, K
The operations that are not correctly rounded everywhere are atan2 (numpy's and the device's may differ in the last bits, which moves
a cell only when a coordinate sits within that of a cell's edge) and, on the device, the root of r (which the tests bound).

THE BAR OF THE SEMANTIC CASE (SPHERE below: a sphere of radius R = 2 m about the world's origin seen from inside, exact distances,
integrated from four rig positions and ray-cast from a fifth, every position within a_max of the centre).  To first order in the
voxel and the cell:
  * A stored value is a mean over the observations n of e_n(c) = D_n(cell of c) - |c - a_n| at the voxel's centre c.  The exact
    projective distance s_n(c) = D_n(direction of c) - |c - a_n| vanishes on the surface, so its gradient there is along the normal:
    moving dt along the ray of a_n changes it by -dt, hence |grad s_n| = 1 / cos i_n, i_n the angle of incidence of that ray.
  * Nearest-voxel sampling: the march's sample p reads the voxel whose centre is within h = (sqrt(3) / 2) voxel of p, which changes
    s_n by at most h / cos i_n.
  * The measurement's nearest-cell look-up: the cell's value is D_n at the cell's centre, at most half a cell's diagonal
    dtheta = (1 / 2) sqrt(dlon^2 + dlat^2) away in angle (a step in longitude is at most that much of an angle), and
    |dD / dtheta| = D tan i <= (R + a_max) tan i_max on a sphere, with sin i_max = a_max / R.  eps_cell = (R + a_max) tan(i_max) dtheta.
  * Along the cast ray (incidence i_u) the mean falls at the rate cos i_u / cos i_n, so the zero crossing moves by at most
    (h / cos i_n + eps_cell) cos i_n / cos i_u <= (h + eps_cell) / cos i_max.
  BAR = (h + eps_cell) / cos i_max.  With voxel = 0.125, a 24 x 48 full sphere (dlon = dlat = pi / 24), a_max = 0.3742:
  h = 0.10825, i_max = 0.1882 rad, dtheta = 0.09256, eps_cell = 0.0419, BAR = 0.1529 m = 1.22 voxel.  The linear interpolation
  between two samples and the clamping at +-trunc are second order here (trunc = 3 voxel, step = voxel / 2) and not in the bar.
  sphere_bar() computes it from the case's numbers; nothing in it was fitted to a result.
"""
import math

import numpy as np

import grid_exact_cases as GE
import panorama_cases as PC
from panorama_cases import BAD, F32, FLT_MAX, FULL, PART, PI_F, _rot, _seed_bad, affine  # noqa: F401  (this module's public names)

VOXEL = 0.25

# name: sequences, voxels (Nx, Ny, Nz), the panorama and its ranges
CASES = {
    "odd": dict(B=1, dims=(10, 6, 5), hw=(6, 10), ranges=FULL, seed=2401),        # x no multiple of 4; row tail, wrap
    "cube": dict(B=1, dims=(8, 8, 8), hw=(8, 16), ranges=PART, seed=2402),        # no wrap; voxels outside the map
    "line": dict(B=1, dims=(1, 1, 7), hw=(6, 10), ranges=FULL, seed=2403),        # an odd slot count: the 8-byte form
    "b2": dict(B=2, dims=(16, 12, 10), hw=(12, 16), ranges=FULL, seed=2404),      # several blocks per sequence
    "b3": dict(B=3, dims=(16, 12, 10), hw=(12, 16), ranges=FULL, seed=2405),
}
POSES = ("identity", "yaw", "shift", "rigid", "far")
SHIFTS = {"same": (0, 0, 0), "one": (1, 0, 0), "three": (-3, 2, 0), "all": None}      # origin - origin_prev; None: more than N
BFS = (96.0, 1.0)
YAW_COLUMNS = 3
# trunc = 2 voxel and a narrow range window: every rejection and the clamp are reached inside these small volumes
PARAMS = dict(trunc=2 * VOXEL, w_max=8.0, r_range=(0.2, 3.0), w_min=1.0)


def params(bf):
    return dict(PARAMS, vs=VOXEL, bf=bf)


def rays(name):
    c = CASES[name]
    return PC.rays(c["ranges"], c["hw"])


def pose(kind, name, b=0):
    """P [4, 4] float32, the rig in the world: identity (the rig at a voxel's corner); a yaw of whole columns of the full sphere; a
    translation ONTO A VOXEL'S CENTRE (that voxel has r2 = 0) whose coverage straddles zero; a general rigid motion; a place far on
    the negative side (every covered index is negative)."""
    W = CASES[name]["hw"][1]
    P = np.eye(4)
    if kind == "yaw":
        P[:3, :3] = _rot(yaw=2 * math.pi * (YAW_COLUMNS + b) / W)
    elif kind == "shift":
        P[:3, 3] = [0.125 + 0.75 * b, -0.375, 0.625 - 0.25 * b]
    elif kind == "rigid":
        P[:3, :3] = _rot(0.11 + 0.05 * b, -0.04, 0.07)
        P[:3, 3] = [1.31 + 0.3 * b, 0.8, 0.7]
    elif kind == "far":
        P[:3, :3] = _rot(-0.3, 0.02 * b, 0.0)
        P[:3, 3] = [-7.3, -5.2 - 0.4 * b, -4.9]
    elif kind != "identity":
        raise KeyError(kind)
    return P.astype(np.float32)


def poses(kind, name):
    return np.stack([pose(kind, name, b) for b in range(CASES[name]["B"])])


def rigid_inverse(P):
    """T = (R^T, -R^T t) in float32, the products summed over the last axis as TsdfVolume.set_pose does"""
    P = np.asarray(P, dtype=F32)
    T = np.zeros_like(P)
    Rt = np.transpose(P[:, :3, :3], (0, 2, 1))
    T[:, :3, :3] = Rt
    T[:, :3, 3] = -(Rt * P[:, None, :3, 3]).sum(-1, dtype=F32)
    T[:, 3, 3] = 1
    return T


def origin_of(P, dims, voxel=VOXEL):
    """floor(t / voxel) - N // 2 in float32, as TsdfVolume.origin_of"""
    t = np.asarray(P, dtype=F32)[:, :3, 3]
    return np.floor(t / F32(voxel)).astype(np.int32) - np.asarray([n // 2 for n in dims], np.int32)


def shifted(origin, kind, dims):
    """origin_prev of a scroll of SHIFTS[kind]"""
    d = SHIFTS[kind]
    d = np.asarray([n + 2 for n in dims] if d is None else d, np.int32)
    return (np.asarray(origin, np.int32) - d).astype(np.int32)


def make_inputs(name, bf=96.0):
    """-> dict(vol [B, Nz, Ny, Nx, 2], inv, std [B, H, W] float32, mask [B, H, W] uint8): a surface that crosses the volume (a smooth
    one with depth steps), its standard deviation a third of it, a mask with holes, the seeded bad values in inv and std, and a
    volume that already holds something: f in [-1, 1], w up to beyond w_max, some exactly at it, some never observed."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    B, (Nx, Ny, Nz), (Hh, W) = c["B"], c["dims"], c["hw"]
    scale = max(0.3 * max(c["dims"]) * VOXEL, 2 * VOXEL)
    i, j = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    d = np.empty((B, Hh, W))
    for b in range(B):
        d[b] = scale * (1.0 + 0.35 * np.sin(2 * math.pi * (j + 2 * b) / W) * np.cos(math.pi * (i + 0.5) / Hh) + 0.15 * np.sin(0.9 * j + 0.7 * i))
        d[b][:, W // 3: W // 2] *= 0.6
    inv = (F32(bf) / d.astype(F32)).astype(F32)
    std = (F32(0.3) * inv * rng.uniform(0.5, 2.0, inv.shape).astype(F32)).astype(F32)
    mask = (rng.uniform(size=inv.shape) > 0.15).astype(np.uint8)
    _seed_bad(rng, inv, 0.06)
    _seed_bad(rng, std, 0.06)
    vol = np.empty((B, Nz, Ny, Nx, 2), F32)
    vol[..., 0] = rng.uniform(-1.0, 1.0, vol.shape[:-1])
    w = rng.uniform(0.0, 10.0, vol.shape[:-1]).astype(F32)
    flat = w.reshape(-1)
    flat[::5] = F32(PARAMS["w_max"])
    flat[1::7] = 0
    vol[..., 1] = w
    return dict(vol=vol, inv=inv, std=std, mask=mask)


# ---------------------------------------------------------------------------------------------- the restatement
def world_index(origin, dims):
    """-> ix [B, 1, 1, Nx], iy [B, 1, Ny, 1], iz [B, Nz, 1, 1] int64: the world voxel of every slot"""
    views = ((1, 1, 1, -1), (1, 1, -1, 1), (1, -1, 1, 1))
    out = []
    for a, N in enumerate(dims):
        s = np.arange(N, dtype=np.int64).reshape(views[a])
        o = np.asarray(origin, np.int64)[:, a].reshape(-1, 1, 1, 1)
        out.append(o + np.mod(s - o, N))                              # numpy's mod is the floored one
    return out


def integrate(vol, inv, std, mask, T, origin, origin_prev, par, aff, r=None):
    """-> dict(vol: the new volume, r, r2 float32 and near bool [B, Nz, Ny, Nx], cx, cy (floats), hit: the voxels updated, fresh,
    u, v: the affine coordinates).  r replaces the restatement's own root (the device's)."""
    vol, inv, T = (np.ascontiguousarray(a, dtype=F32) for a in (vol, inv, T))
    B, Nz, Ny, Nx, _ = vol.shape
    dims = (Nx, Ny, Nz)
    Hh, W = inv.shape[1:]
    vs, trunc, w_max, bf = F32(par["vs"]), F32(par["trunc"]), F32(par["w_max"]), F32(par["bf"])
    t2 = F32(float(par["trunc"]) * float(par["trunc"]))
    r_min, r_max = F32(par["r_range"][0]), F32(min(par["r_range"][1], float(FLT_MAX)))
    full = (B, Nz, Ny, Nx)
    idx = world_index(origin, dims)
    fresh = np.zeros(full, bool)
    for a, N in enumerate(dims):
        op = np.asarray(origin_prev, np.int64)[:, a].reshape(-1, 1, 1, 1)
        fresh = fresh | (idx[a] < op) | (idx[a] >= op + N)
    with np.errstate(all="ignore"):
        f = np.where(fresh, F32(1), vol[..., 0])
        w = np.where(fresh, F32(0), vol[..., 1])
        c = np.stack([np.broadcast_to((i.astype(F32) + F32(0.5)) * vs, full) for i in idx], 1)
        q = GE.transform(T, c.reshape(B, 3, -1)).reshape(B, 3, Nz, Ny, Nx)
        qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
        r2 = (qx * qx + qy * qy) + qz * qz
        near = (r2 > 0) & (r2 <= FLT_MAX)
        rr = np.sqrt(r2) if r is None else np.asarray(r, dtype=F32)
        ok = near & (rr >= r_min) & (rr <= r_max)
        fx, fy, inside, u, v = PC.cell(qx, qy, qz, aff, (Hh, W))
        ok = ok & inside
        cell = (np.where(ok, fy, 0).astype(np.int64) * W + np.where(ok, fx, 0).astype(np.int64)).reshape(B, -1)
        take = lambda a: np.take_along_axis(np.asarray(a).reshape(B, -1), cell, axis=1).reshape(full)
        m = take(inv)
        if mask is not None:
            ok = ok & (take(mask) != 0)
        d = bf / m
        ok = ok & (m > 0) & (m <= FLT_MAX) & (d <= FLT_MAX)
        sdf = d - rr
        ok = ok & ~(sdf < -trunc)
        obs = np.minimum(sdf, trunc) / trunc
        if std is not None:
            sd = take(np.asarray(std, dtype=F32))
            sig = sd * d / m
            w_obs = t2 / (t2 + sig * sig)
            ok = ok & (w_obs > 0) & (w_obs <= 1)
        else:
            w_obs = np.ones(full, F32)
        Wn = w + w_obs
        f_new = (f * w + obs * w_obs) / Wn
        w_new = np.minimum(Wn, w_max)
        assert all(a.dtype == F32 for a in (f, w, c, q, r2, rr, u, v, fx, fy, m, d, sdf, obs, w_obs, Wn, f_new, w_new))
        out = np.stack([np.where(ok, f_new, f), np.where(ok, w_new, w)], -1).astype(F32)
    return dict(vol=out, r=rr, r2=r2, near=near, cx=fx, cy=fy, hit=ok, fresh=fresh, u=u, v=v, sdf=sdf, obs=obs)


def exact_root(r2):
    """RN_fp32(sqrt(float64(r2))): 53 bits against 24, the double rounding is harmless"""
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(r2, dtype=F32).astype(np.float64)).astype(F32)


def raycast(vol, ray_table, P, origin, voxel, t0, step, K, w_min, bf):
    """-> dict(inv, weight float32, steps int32 [B, H, W], t: float64 t* (nan without a crossing))"""
    vol, ray_table, P = (np.ascontiguousarray(a, dtype=F32) for a in (vol, ray_table, P))
    B, Nz, Ny, Nx, _ = vol.shape
    _, Hh, W = ray_table.shape
    t0, step, inv_vs, w_min, bf = F32(t0), F32(step), F32(1.0 / float(voxel)), F32(w_min), F32(bf)
    R = P.copy()
    R[:, :3, 3] = 0
    with np.errstate(all="ignore"):
        dirs = GE.transform(R, np.broadcast_to(ray_table.reshape(1, 3, -1), (B, 3, Hh * W))).reshape(B, 3, Hh, W)
        o = P[:, :3, 3].reshape(B, 3, 1, 1)
        org = np.asarray(origin, np.int64).reshape(B, 3, 1, 1)
        n = np.asarray([Nx, Ny, Nz], np.int64).reshape(1, 3, 1, 1)
        lo, hi = org.astype(F32), (org + n).astype(F32)
        pairs = vol.reshape(B, -1, 2)
        plane = (B, Hh, W)
        inv, weight, steps = np.zeros(plane, F32), np.zeros(plane, F32), np.full(plane, K, np.int32)
        tstar = np.full(plane, np.nan)
        done, pf, pv = np.zeros(plane, bool), np.zeros(plane, F32), np.zeros(plane, bool)
        for k in range(K):
            tk = t0 + F32(k) * step
            p = o + dirs * tk
            g = np.floor(p * inv_vs)
            inside = ((g >= lo) & (g < hi)).all(1)
            s = np.mod(np.where(inside[:, None], g, 0).astype(np.int64), n)
            slot = ((s[:, 2] * Ny + s[:, 1]) * Nx + s[:, 0]).reshape(B, -1)
            f = np.take_along_axis(pairs[..., 0], slot, axis=1).reshape(plane)
            w = np.take_along_axis(pairs[..., 1], slot, axis=1).reshape(plane)
            valid = inside & (w >= w_min)
            cross = valid & pv & (pf > 0) & (f <= 0) & ~done
            tp = t0 + F32(k - 1) * step
            ts = tp + step * (pf / (pf - f))
            assert all(a.dtype == F32 for a in (p, g, f, w, ts)) and isinstance(tk, F32)
            inv = np.where(cross, bf / ts, inv)
            weight = np.where(cross, w, weight)
            steps = np.where(cross, np.int32(k), steps)
            tstar = np.where(cross, ts.astype(np.float64), tstar)
            done = done | cross
            pf, pv = f, valid
    return dict(inv=inv.astype(F32), weight=weight.astype(F32), steps=steps.astype(np.int32), t=tstar)


def plane_volume(dims, B=1):
    """A hand-made volume whose zero crossing is a plane at a dyadic place: f = (3.5 - ix) / 4 in slot ix of the x axis (f = 0.125 in
    voxel 3, -0.125 in voxel 4: the crossing lies between them), w = 2 everywhere.  Every value is a small dyadic number, so
    f_{k-1} / (f_{k-1} - f_k) = 0.5 and t* are exact."""
    Nx, Ny, Nz = dims
    vol = np.empty((B, Nz, Ny, Nx, 2), F32)
    vol[..., 0] = ((F32(3.5) - np.arange(Nx, dtype=F32)) / F32(4)).reshape(1, 1, 1, Nx)
    vol[..., 1] = 2
    return vol


# ---------------------------------------------------------------------------------------------- the semantic case
SPHERE = dict(R=2.0, dims=(40, 40, 40), voxel=0.125, hw=(24, 48), trunc=3 * 0.125, step=0.125 / 2, t0=0.2, t_max=3.0, bf=96.0,
              views=((0.3, 0.0, 0.1), (-0.2, 0.1, -0.3), (0.0, -0.3, 0.2), (-0.1, 0.2, 0.3)), cast=(0.15, -0.1, -0.05))


def sphere_bar():
    """The bar on |t* - t_true| in metres, from the case's numbers alone (the derivation is in this module's docstring)"""
    s = SPHERE
    a_max = max(math.sqrt(sum(v * v for v in a)) for a in s["views"] + (s["cast"],))
    i_max = math.asin(a_max / s["R"])
    h = math.sqrt(3.0) / 2.0 * s["voxel"]
    dlon, dlat = 2 * math.pi / s["hw"][1], math.pi / s["hw"][0]
    dtheta = 0.5 * math.sqrt(dlon * dlon + dlat * dlat)
    eps_cell = (s["R"] + a_max) * math.tan(i_max) * dtheta
    return (h + eps_cell) / math.cos(i_max)


def sphere_rays():
    return PC.rays(FULL, SPHERE["hw"])


def sphere_distance(a, ray_table):
    """The exact distance (float64) from a inside the sphere to it along every ray of the table"""
    u = np.asarray(ray_table, np.float64)
    u = u / np.linalg.norm(u, axis=0, keepdims=True)
    a = np.asarray(a, np.float64)
    au = np.tensordot(a, u, axes=(0, 0))
    return -au + np.sqrt(au * au + SPHERE["R"] ** 2 - a @ a)


def sphere_pose(a):
    P = np.eye(4, dtype=F32)
    P[:3, 3] = a
    return P[None]


def sphere_inv(a):
    return (F32(SPHERE["bf"]) / sphere_distance(a, sphere_rays()).astype(F32)).astype(F32)[None]


def sphere_K():
    s = SPHERE
    return int(math.floor((s["t_max"] - s["t0"]) / s["step"])) + 1


def sphere_on_the_cpu():
    """The semantic case through the restatement -> (the ray-cast's dict, the exact distances from the fifth position)"""
    s = SPHERE
    Nx, Ny, Nz = s["dims"]
    ray_table = sphere_rays()
    aff = affine(FULL, s["hw"])
    par = dict(vs=s["voxel"], trunc=s["trunc"], w_max=64.0, r_range=(0.0, float(FLT_MAX)), bf=s["bf"])
    vol = np.empty((1, Nz, Ny, Nx, 2), F32)
    vol[..., 0], vol[..., 1] = 1, 0
    prev = origin_of(sphere_pose((0, 0, 0)), s["dims"], s["voxel"])
    for a in s["views"]:
        P = sphere_pose(a)
        org = origin_of(P, s["dims"], s["voxel"])
        vol = integrate(vol, sphere_inv(a), None, None, rigid_inverse(P), org, prev, par, aff)["vol"]
        prev = org
    P = sphere_pose(s["cast"])
    got = raycast(vol, ray_table, P, prev, s["voxel"], s["t0"], s["step"], sphere_K(), 1.0, s["bf"])
    return got, sphere_distance(s["cast"], ray_table)[None]
