"""The sampling-grid generator (csrc/grids.hip, csrc/camera_models.hpp) restated on the host, numpy only, for
tests/test_grid_exact_host.py and tests/test_gpu_grids_exact.py.

Two kinds of statement:
  * transform_points and grid_double_sphere use only + - x / sqrt, fma and a compare, all correctly rounded in IEEE arithmetic, so
    `transform` and `double_sphere` emulate them operation by operation in float32 and the kernels must return the same bits;
  * rays_panorama, grid_equirect and rays_equirect_surrogate call sinf / cosf / atan2f.  Their ARGUMENTS are float32 values that
    are emulated exactly (`panorama_args`, `surrogate_args`, `equirect_args`); the float64 closed form evaluated from those
    arguments is the exact value to ~1e-16, and every element carries a bound in units of 2^-23 |exact|:
        an IEEE rounding is 0.5 ulp, a libm call U ulp with U_sin = U_cos = 4, U_atan2 = 6 (the OpenCL full-profile limits the
        ROCm device library's fp32 sin / cos / atan2 are built to meet: a specification, not a measurement), 1 ulp <= 2^-23 |v|;
        rays x, z = (d sin phi) cos|sin theta      4 + 4 + 2 x 0.5 = 9          rays y = -d cos phi         4 + 0.5 = 4.5
        equirect gx = -atan2(z, x) / pi_f          6 + 0.5 = 6.5                gy = 2 atan2(y, xz) / pi_f  6.5 (xz is the emulated
        surrogate cos lat cos|sin lon              4 + 4 + 0.5 = 8.5            fp32 value; 2 x is exact)   surrogate sin lat: 4
    times (1 + 2^-20) for the second-order terms, plus one subnormal (2^-149) as an absolute floor.
"""
import math
import zlib

import numpy as np

F32 = np.float32
PI_F = F32(np.pi)                         # kPiF of camera_models.hpp
U_SIN = U_COS = 4.0
U_ATAN2 = 6.0
EPS = 2.0 ** -23
FLOOR = 2.0 ** -149
UNITS_PANORAMA = np.array([U_SIN + U_COS + 1.0, U_COS + 0.5, U_SIN + U_SIN + 1.0])          # x, y, z
UNITS_EQUIRECT = U_ATAN2 + 0.5
UNITS_SURROGATE = np.array([U_COS + U_COS + 0.5, U_SIN, U_COS + U_SIN + 0.5])               # x, y, z


# ------------------------------------------------------------------------------ exact float32 arithmetic
def fma_f32(a, b, c):
    """RN_f32(a * b + c) for float32 arrays, exactly.  The product of two float32 is exact in float64; the float64 sum s and its
    exact error e (two-sum) are the exact sum.  Rounding s to float32 is then wrong only where s sits exactly half-way between two
    neighbouring float32 and e != 0: there the sign of e decides, not the tie rule."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(np.float32)
        rb = r.astype(np.float64)
        other = np.where(rb > s, np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))).astype(np.float32)
        ob = other.astype(np.float64)
        mid = (rb != s) & ((rb + ob) / 2 == s)
        lo, hi = np.minimum(r, other), np.maximum(r, other)
        return np.where(mid & (e > 0), hi, np.where(mid & (e < 0), lo, r)).astype(np.float32)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def same_bits(got, want):
    """Equal bit for bit, except that any NaN equals any NaN (the payload is not part of the contract): -0 differs from +0,
    a NaN where `want` holds a number -- an unwritten element -- differs."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype != np.float32:
        return bool(np.array_equal(got, want))
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


def first_difference(got, want):
    """A line for the assertion message: where two float32 arrays first differ under `same_bits`."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    if got.dtype == np.float32:
        bad = (np.isnan(got) != np.isnan(want)) | (~np.isnan(got) & ~np.isnan(want) & (got.view(np.uint32) != want.view(np.uint32)))
    else:
        bad = got != want
    if not bad.any():
        return "equal"
    i = tuple(int(v[0]) for v in np.nonzero(bad))
    return f"{int(bad.sum())} of {bad.size} elements differ; first at {i}: got {got[i]!r} want {want[i]!r}"


# ------------------------------------------------------------------------------ the bit-exact kernels
def transform(T, p):
    """transform_points_kernel: T [B, 4, 4], p [B, 3, M] -> [B, 3, M]; per row fma(t2, z, fma(t1, y, t0 * x)) + t3."""
    T, p = _f32(T), _f32(p)
    B, _, M = p.shape
    assert T.shape == (B, 4, 4) and p.shape[1] == 3
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for i in range(3):
            t = [np.broadcast_to(T[:, i, k, None], (B, M)) for k in range(4)]
            out[:, i] = fma_f32(t[2], z, fma_f32(t[1], y, t[0] * x)) + t[3]
    return out


def ds_w2(xi, alpha):
    """The host's part of DoubleSphereSampleGridMaker (Python floats)."""
    w1 = alpha / (1 - alpha) if alpha <= 0.5 else (1 - alpha) / alpha
    return (w1 + xi) / math.sqrt(2 * w1 * xi + xi ** 2 + 1)


def double_sphere(points, xi, alpha, fx, fy, cx, cy, calib_h, calib_w, w2):
    """project_double_sphere + make_ds_params: points [B, 3, M] -> (grid [B, M, 2] float32, mask [B, M] bool)."""
    p = _f32(points)
    xi, alpha, fx, fy, cx, cy, w2 = (F32(v) for v in (xi, alpha, fx, fy, cx, cy, w2))          # the C ABI takes floats
    one_minus_alpha = F32(1.0 - np.float64(alpha))
    wm1, hm1, neg_w2 = F32(calib_w - 1), F32(calib_h - 1), -w2
    two, one = F32(2.0), F32(1.0)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x2, y2, z2 = x * x, y * y, z * z
        d1 = np.sqrt((x2 + y2) + z2)
        s = xi * d1 + z
        d2 = np.sqrt((x2 + y2) + s * s)
        t = alpha * d2 + one_minus_alpha * s
        gx = ((fx / t * x + cx) / wm1) * two - one
        gy = ((fy / t * y + cy) / hm1) * two - one
        mask = z > neg_w2 * d1
    grid = np.stack([gx, gy], -1)
    assert grid.dtype == np.float32
    return grid, mask


def double_sphere_reciprocal_form(points, xi, alpha, fx, fy, cx, cy, calib_h, calib_w, w2):
    """The reference's own rounding sequence: `self.fx / t` is Tensor.__rtruediv__, reciprocal(t) * fx -- two roundings where
    the kernel's fx / t has one.  Only the grid; for counting the golden elements either form reproduces."""
    p = _f32(points)
    xi, alpha, fx, fy, cx, cy = (F32(v) for v in (xi, alpha, fx, fy, cx, cy))
    one_minus_alpha = F32(1.0 - np.float64(alpha))
    wm1, hm1, two, one = F32(calib_w - 1), F32(calib_h - 1), F32(2.0), F32(1.0)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x2, y2, z2 = x * x, y * y, z * z
        d1 = np.sqrt((x2 + y2) + z2)
        s = xi * d1 + z
        d2 = np.sqrt((x2 + y2) + s * s)
        r = one / (alpha * d2 + one_minus_alpha * s)
        gx = ((r * fx * x + cx) / wm1) * two - one
        gy = ((r * fy * y + cy) / hm1) * two - one
    return np.stack([gx, gy], -1)


# ------------------------------------------------------------------------------ arguments of the libm kernels
def panorama_args(N, H, W, lat, lon):
    """rays_panorama_kernel's phi [H] and theta [W] in float32; lat / lon are the (start, end) pairs the launcher receives."""
    def axis(n, rng):
        a0, a1 = F32(rng[0]), F32(rng[1])                                   # c_float arguments
        span = F32(np.float64(a1) - np.float64(a0))
        i = np.arange(n, dtype=np.float32)
        return ((i + F32(0.5)) / F32(n) * span) + a0
    phi, theta = axis(H, lat), axis(W, lon)
    assert phi.dtype == theta.dtype == np.float32
    return phi, theta


def surrogate_args(H, W):
    """rays_equirect_surrogate_kernel's u [W], v [H], lon [W], lat [H] in float32."""
    u = (2 * np.arange(W) + 1).astype(np.float32) / F32(W) - F32(1.0)
    v = (2 * np.arange(H) + 1).astype(np.float32) / F32(H) - F32(1.0)
    lon, lat = u * PI_F, (v * PI_F) / F32(2.0)
    assert lon.dtype == lat.dtype == np.float32
    return u, v, lon, lat


def equirect_args(points):
    """project_equirect's xz = sqrt(x * x + z * z) in float32; points [B, 3, M] -> [B, M]."""
    p = _f32(points)
    with np.errstate(all="ignore"):
        return np.sqrt(p[:, 0] * p[:, 0] + p[:, 2] * p[:, 2])


# ------------------------------------------------------------------------------ float64 closed forms from those arguments, bounds
def panorama_exact(dist, phi, theta):
    """-> rays [3, N, H, W] float64 from the float32 arguments, and the units [3, 1, 1, 1] of the bound."""
    d = _f32(dist).astype(np.float64)[:, None, None]
    ph, th = phi.astype(np.float64)[None, :, None], theta.astype(np.float64)[None, None, :]
    ds = d * np.sin(ph)
    rays = np.stack(np.broadcast_arrays(ds * np.cos(th), -d * np.cos(ph), -ds * np.sin(th)))
    return rays, UNITS_PANORAMA.reshape(3, 1, 1, 1)


def panorama_exact_at(dist, phi, theta, idx):
    """The same closed form at flat indices idx of one [N][H][W] plane only -> [3, len(idx)] float64 (for windows of a volume too
    large to evaluate whole)."""
    H, W = len(phi), len(theta)
    idx = np.asarray(idx, dtype=np.int64)
    d = _f32(dist).astype(np.float64)[idx // (W * H)]
    ph, th = phi.astype(np.float64)[(idx // W) % H], theta.astype(np.float64)[idx % W]
    ds = d * np.sin(ph)
    return np.stack([ds * np.cos(th), -d * np.cos(ph), -ds * np.sin(th)])


def equirect_exact(points):
    """points [B, 3, M] float32 -> grid [B, M, 2] float64 (NaN where an argument is NaN), units of the bound."""
    p = _f32(points)
    xz = equirect_args(p).astype(np.float64)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    pi = np.float64(PI_F)
    with np.errstate(all="ignore"):
        return np.stack([-np.arctan2(z, x) / pi, 2.0 * np.arctan2(y, xz) / pi], -1), UNITS_EQUIRECT


def surrogate_exact(H, W):
    """-> rays [3, H, W] float64 from the float32 lon / lat, units [3, 1, 1]."""
    _, _, lon, lat = surrogate_args(H, W)
    lo, la = lon.astype(np.float64)[None, :], lat.astype(np.float64)[:, None]
    rays = np.stack(np.broadcast_arrays(np.cos(la) * np.cos(lo), np.sin(la) + 0 * lo, -(np.cos(la) * np.sin(lo))))
    return rays, UNITS_SURROGATE.reshape(3, 1, 1)


def bound(exact, units):
    with np.errstate(all="ignore"):
        return units * EPS * np.abs(exact) * (1.0 + 2.0 ** -20) + FLOOR


def check_bound(got, exact, units):
    """-> (ok [same shape] bool, worst error in units of 2^-23 |exact| over the elements whose exact value is a normal float32).
    An element is ok when it is within its bound; a NaN is ok only where the exact value is NaN."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == exact.shape, (got.dtype, got.shape, exact.shape)
    g = got.astype(np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(g - exact)
        ok = np.where(np.isnan(exact), np.isnan(g), err <= bound(exact, units))
        normal = np.isfinite(exact) & (np.abs(exact) >= 2.0 ** -126)
        worst = float((err[normal] / (EPS * np.abs(exact[normal]))).max()) if normal.any() else 0.0
    return ok, worst


def describe_failures(ok, got, exact, units, args=None):
    """The first element outside its bound, for the assertion message."""
    if ok.all():
        return "all within bounds"
    i = tuple(int(v[0]) for v in np.nonzero(~ok))
    b = np.broadcast_to(bound(exact, units), exact.shape)[i]
    extra = "" if args is None else f", arguments {args(i)}"
    return (f"{int((~ok).sum())} of {ok.size} elements outside their bound; first at {i}: got {float(np.asarray(got)[i])!r}, exact "
            f"{float(exact[i])!r}, |d| {abs(float(np.asarray(got)[i]) - float(exact[i])):.3e} > {float(b):.3e}{extra}")


def error_figures(got, exact):
    """(max_rel, mean_l1_rel, max_pixel_rel) as tests/parity_log.py defines them, over the finite elements."""
    g, e = np.asarray(got, np.float64).ravel(), np.asarray(exact, np.float64).ravel()
    f = np.isfinite(g) & np.isfinite(e)
    g, e = g[f], e[f]
    d = np.abs(g - e)
    nz = np.abs(e) >= 2.0 ** -126
    return (float(d.max() / max(np.abs(e).max(), 1e-30)), float(d.mean() / max(np.abs(e).mean(), 1e-30)),
            float((d[nz] / np.abs(e[nz])).max()) if nz.any() else 0.0)


# ------------------------------------------------------------------------------ cases
SHAPES = [(1, 1, 1), (3, 5, 7), (5, 7, 13), (2, 9, 29)]          # (N, H, W): odd widths, no multiple of 256; 522 points: two blocks
GOLDEN_SHAPE = (16, 8, 32)                                       # 4096 points: the exact multiple of the 256-thread block
ALL_SHAPES = SHAPES + [GOLDEN_SHAPE]
BATCHES = (1, 3)
REGIMES = ("random", "zeros", "subnormal", "overflow", "nan", "origin")
TRANSFORM_KINDS = ("identity", "ring", "far", "subnormal")

DS_PARAMS = {                                                     # name -> ((xi, alpha, fx, fy, cx, cy), (calib_h, calib_w))
    "default": ((-0.203, 0.589, 232.0, 232.0, 611.5, 513.5), (1028, 1224)),
    "ds2": ((0.1, 0.45, 300.0, 310.0, 320.0, 240.0), (480, 640)),
    "pinhole": ((0.0, 0.0, 232.0, 232.0, 611.5, 513.5), (1028, 1224)),
    "alpha_half": ((0.3, 0.5, 250.0, 240.0, 320.0, 240.0), (480, 640)),      # alpha = 0.5: the other branch of w1
}

PANORAMA_RANGES = {                                               # name -> (lat, lon)
    "full_sphere": ((0.0, math.pi), (-math.pi, math.pi)),
    "g16_band": ((-math.pi / 2, 0.0), (0.0, 2 * math.pi)),
    "zero_span": ((0.0, 0.0), (1.25, 1.25)),                     # phi = 0: x and z are exact zeros
}
SURROGATE_SHAPES = [(1, 1), (5, 7), (9, 29), (16, 64)]


def ds_args(name):
    """-> the ten arguments of `double_sphere` after the points."""
    (xi, alpha, fx, fy, cx, cy), (h, w) = DS_PARAMS[name]
    return (xi, alpha, fx, fy, cx, cy, h, w, ds_w2(xi, alpha))


def candidate_distances(N):
    """The goldens' 0.5 ... 100 (geometric), and from three candidates on 1e-3 first and 1e4 last."""
    d = np.geomspace(0.5, 100.0, N).astype(np.float32)
    if N >= 3:
        d[0], d[-1] = 1e-3, 1e4
    return d


def _seed(*key):
    return zlib.crc32(repr(key).encode())                         # the same in every process, unlike hash()


def _subnormals(rng, n):
    bits = rng.integers(1, 1 << 23, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))
    return bits.view(np.float32)


def points(shape, B, regime):
    """Seeded points [B, 3, N, H, W] float32 of one value regime (every regime keeps ordinary points beside its special ones)."""
    N, H, W = shape
    M = N * H * W
    rng = np.random.default_rng(_seed("points", shape, B, regime))
    p = (rng.standard_normal((B, 3, M)) * np.geomspace(0.05, 50.0, M)[rng.permutation(M)]).astype(np.float32)
    pick = lambda frac: rng.random((B, M)) < frac
    sign = lambda n: rng.choice(np.array([-1.0, 1.0], np.float32), n)
    if regime == "random":
        pass
    elif regime == "zeros":                                        # single coordinates +-0
        for k in range(3):
            m = pick(0.3)
            p[:, k][m] = sign(int(m.sum())) * F32(0.0)
    elif regime == "subnormal":                                    # whole points subnormal, and single subnormal coordinates
        m = pick(0.4)
        for k in range(3):
            p[:, k][m] = _subnormals(rng, int(m.sum()))
            one = pick(0.2) & ~m
            p[:, k][one] = _subnormals(rng, int(one.sum()))
        p[0, :, 0] = _subnormals(rng, 3)
    elif regime == "overflow":                                     # 1e19: squares of 1e38, their sums up to 3e38 or inf; 1e20: x * x = inf
        for k in range(3):
            m = pick(0.25)
            p[:, k][m] = sign(int(m.sum())) * rng.choice(np.array([1e19, 1e20], np.float32), int(m.sum()))
        p[0, 0, 0], p[0, 1, 0] = F32(1e20), F32(1e19)
    elif regime == "nan":
        for k in range(3):
            m = pick(0.2)
            p[:, k][m] = np.nan
        p[0, M // 2 % 3, 0] = np.nan
    elif regime == "origin":                                       # t = 0: the grid is NaN or inf
        m = pick(0.3)
        for k in range(3):
            p[:, k][m] = sign(int(m.sum())) * F32(0.0)
        p[0, :, 0] = F32(0.0)
    else:
        raise KeyError(regime)
    return np.ascontiguousarray(p.reshape(B, 3, N, H, W))


def ring_pose_inverses(n=4):
    """float32 inverses of the synthetic ring rig's poses (oracle/grid_oracle.py), inverted in float64 as make_sweep_grid does."""
    from oracle.grid_oracle import ring_poses
    return [np.linalg.inv(np.asarray(p, dtype=np.float64)).astype(np.float32) for p in ring_poses(n)]


def one_transform(kind, k=0):
    T = np.eye(4, dtype=np.float32)
    rng = np.random.default_rng(_seed("transform", kind, k))
    if kind == "identity":
        pass
    elif kind == "ring":
        T = ring_pose_inverses(4)[1 + k % 3]
    elif kind == "far":                                            # a translation of 1e6: the sum cancels or swamps the rotation
        T[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0].astype(np.float32)
        T[:3, 3] = np.array([1e6, -1e6, 1e6], np.float32) * rng.uniform(0.5, 1.0, 3).astype(np.float32)
    elif kind == "subnormal":                                      # subnormal entries in the rotation and the translation
        T[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0].astype(np.float32)
        T[0, 1], T[1, 2], T[2, 0] = _subnormals(rng, 3)
        T[:2, 3] = _subnormals(rng, 2)
    else:
        raise KeyError(kind)
    return T


def transforms(B, first):
    """[B, 4, 4]: a different transform per batch element, starting at kind number `first`."""
    return np.stack([one_transform(TRANSFORM_KINDS[(first + b) % len(TRANSFORM_KINDS)], b) for b in range(B)])


# ------------------------------------------------------------------------------ the field-of-view boundary
def _ordered(f):
    """float32 -> int64, monotone in the value (-0 just below +0)."""
    b = f.view(np.uint32).astype(np.int64)
    return np.where(b < (1 << 31), b, -(b - (1 << 31)) - 1)


def _from_ordered(o):
    return np.where(o >= 0, o, (-o - 1) + (1 << 31)).astype(np.uint32).view(np.float32)


def fov_boundary_points(name, n_dirs=64):
    """For one parameter set: [1, 3, n_dirs, 1, 3] points -- per direction (x, y) three neighbouring floats z: the last one
    inside the field of view, the first one outside, one further -- found by bisection on the EMULATED predicate
    z > neg_w2 * d1, so the mask flips between adjacent floats.  Asserts the emulated mask is 1, 0, 0."""
    args = ds_args(name)
    rng = np.random.default_rng(_seed("fov", name))
    keep_x, keep_y, keep_z = [], [], []
    n_kept = 0
    for _ in range(20):
        n = 2 * n_dirs
        xy = (rng.standard_normal((2, n)) * np.geomspace(0.01, 100.0, n)).astype(np.float32)
        r = np.sqrt(xy[0].astype(np.float64) ** 2 + xy[1].astype(np.float64) ** 2)

        def inside(z):
            return double_sphere(np.stack([xy[0], xy[1], z])[None], *args)[1][0]
        hi, lo = _ordered((r * 10).astype(np.float32)), _ordered((-r * 1e8).astype(np.float32))
        usable = inside(_from_ordered(hi)) & ~inside(_from_ordered(lo))
        while ((hi - lo) > 1).any():
            mid = (hi + lo) // 2
            m = inside(_from_ordered(mid))
            hi, lo = np.where(m, mid, hi), np.where(m, lo, mid)
        z3 = np.stack([_from_ordered(hi), _from_ordered(lo), _from_ordered(lo - 1)], -1)          # [n, 3]
        m3 = double_sphere(np.stack([np.repeat(xy[0], 3), np.repeat(xy[1], 3), z3.ravel()])[None], *args)[1][0].reshape(n, 3)
        good = usable & (m3 == np.array([True, False, False])).all(-1)
        keep_x.append(xy[0][good]), keep_y.append(xy[1][good]), keep_z.append(z3[good])
        n_kept += int(good.sum())
        if n_kept >= n_dirs:
            break
    x, y, z = np.concatenate(keep_x)[:n_dirs], np.concatenate(keep_y)[:n_dirs], np.concatenate(keep_z)[:n_dirs]
    assert len(x) == n_dirs, f"{name}: only {len(x)} boundary directions found"
    pts = np.stack([np.repeat(x, 3), np.repeat(y, 3), z.ravel()]).reshape(1, 3, n_dirs, 1, 3).astype(np.float32)
    mask = double_sphere(pts.reshape(1, 3, -1), *args)[1].reshape(n_dirs, 3)
    assert (mask == np.array([True, False, False])).all(), name
    assert (_ordered(z[:, 0]) - _ordered(z[:, 1]) == 1).all() and (_ordered(z[:, 1]) - _ordered(z[:, 2]) == 1).all()
    return np.ascontiguousarray(pts)


# ------------------------------------------------------------------------------ equirect: branch cut, poles, origin
CUT_Z = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 1e-30, -1e-30], dtype=np.float32)


def branch_cut_points(n_x=7):
    """[1, 3, n_x, 1, 6]: x < 0 with z in {+0, -0, +-smallest subnormal, +-1e-30}; y ordinary."""
    rng = np.random.default_rng(_seed("cut"))
    x = -np.geomspace(0.01, 100.0, n_x).astype(np.float32)
    p = np.empty((1, 3, n_x, 1, len(CUT_Z)), np.float32)
    p[0, 0] = x[:, None, None]
    p[0, 1] = rng.standard_normal((n_x, 1, len(CUT_Z))).astype(np.float32)
    p[0, 2] = CUT_Z[None, None, :]
    return p


def pole_points():
    """[1, 3, 1, 1, 12]: x = z = 0 in every combination of signs, with y in {1.5, -1.5} (the poles) and y in {+0, -0} (the origin)
    -- and once more the poles with the other signs of zero."""
    xs = np.array([0.0, -0.0, 0.0, -0.0] * 3, np.float32)
    zs = np.array([0.0, 0.0, -0.0, -0.0] * 3, np.float32)
    ys = np.array([1.5] * 2 + [-1.5] * 2 + [0.0, -0.0, 0.0, -0.0] + [-2.5e-3, 7e4, 1e-30, -1e19], np.float32)
    return np.stack([xs, ys, zs]).reshape(1, 3, 1, 1, 12)
