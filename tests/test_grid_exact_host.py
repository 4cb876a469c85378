"""CPU: the host restatement of the grid generator (tests/grid_exact_cases.py) against exact rational arithmetic, against the
reference's own outputs (tests/golden/sweep_grids.npz) and against float64 -- what makes the bit-exact and per-element GPU
tests of tests/test_gpu_grids_exact.py mean something."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import grid_exact_cases as GC

RIGS = ("g16", "e8_full_sphere")


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "sweep_grids.npz"))


def _golden_ds(z):
    """(points key, grid key, mask key or None, parameter set) of every double-sphere golden."""
    out = [(f"{n}_pts{i}", f"{n}_ds_grid{i}", f"{n}_ds_mask{i}", "default") for n in RIGS for i in range(len(z[n + "_poses"]))]
    return out + [("g16_pts1", "ds2_grid", "ds2_mask", "ds2")]


# ------------------------------------------------------------------------------ fma_f32
def _round_to_f32(q: Fraction) -> np.float32:
    """Round a rational to the nearest float32, ties to even, from the exact distances to the neighbouring candidates."""
    r = np.float32(float(q))
    cands = {float(r), float(np.nextafter(r, np.float32(-np.inf))), float(np.nextafter(r, np.float32(np.inf)))}
    best = min(cands, key=lambda c: (abs(Fraction(c) - q), int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


def _fma_operands():
    rng = np.random.default_rng(1)
    n = 1500

    def rand(lo_exp, hi_exp):
        return (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(lo_exp, hi_exp, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    a, b, c = [rand(-20, 20)], [rand(-20, 20)], [rand(-40, 40)]
    a.append(rand(-70, -60)), b.append(rand(-70, -60)), c.append(rand(-140, -128))           # subnormal results
    # half-way cases: c + a b with a b = h (half an ulp of c: the tie rule decides), h (1 - 2^-46) and h (1 + 2^-33): the float64
    # sum is the exact half-way point and only the error term knows the side
    cc = rand(-10, 10)
    half = np.abs(np.nextafter(cc, np.float32(np.inf)) - cc).astype(np.float64) / 2
    half = np.minimum(half, np.abs(cc - np.nextafter(cc, np.float32(-np.inf))).astype(np.float64) / 2).astype(np.float32)
    pairs = [(1.0, 1.0), (1 + 2.0 ** -23, 1 - 2.0 ** -23), (1 + 2.0 ** -11, 1 - 2.0 ** -11 + 2.0 ** -22)]
    for fa, fb in pairs:
        assert float(np.float32(fa)) == fa and float(np.float32(fb)) == fb
        for sgn in (1.0, -1.0):
            a.append(np.full(n, fa, np.float32)), b.append((np.float32(sgn * fb) * half).astype(np.float32)), c.append(cc)
    return np.concatenate(a), np.concatenate(b), np.concatenate(c)


def test_fma_f32_is_the_rounded_exact_value():
    a, b, c = _fma_operands()
    got = GC.fma_f32(a, b, c)
    want = np.array([_round_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(w))) for x, y, w in zip(a, b, c)], np.float32)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    print(f"fma_f32: {len(a)} operand triples, {int((naive.view(np.uint32) != want.view(np.uint32)).sum())} of them wrong when rounded twice")
    assert len(a) >= 3000 and (naive.view(np.uint32) != want.view(np.uint32)).any()          # the cases exercise the correction
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------ double sphere against the goldens
def test_emulated_mask_is_the_reference_mask_bit_for_bit(z):
    """No band around the field-of-view boundary is excluded."""
    for pk, _, mk, name in _golden_ds(z):
        pts = z[pk]
        _, mask = GC.double_sphere(pts.reshape(1, 3, -1), *GC.ds_args(name))
        assert np.array_equal(mask.reshape(z[mk].shape), z[mk]), mk
    assert float(z["ds2_w2"]) == GC.ds_w2(0.1, 0.45)


def test_emulated_grid_against_the_reference_grid(z):
    """Element for element within 8 x 2^-23 (|golden| + 2): the difference is the reference's two-rounding reciprocal(t) * fx
    and the roundings after it.  Counts the elements that differ in bits under the kernel's form (fx / t) and under the
    reference's (reciprocal(t) * fx)."""
    n_all = n_div = n_rcp = n2_div = n2_rcp = 0
    worst = 0.0
    for pk, gk, _, name in _golden_ds(z):
        pts, ref = z[pk].reshape(1, 3, -1), z[gk]
        assert np.isfinite(ref).all()
        grid, _ = GC.double_sphere(pts, *GC.ds_args(name))
        rcp = GC.double_sphere_reciprocal_form(pts, *GC.ds_args(name))
        grid, rcp = grid.reshape(ref.shape), rcp.reshape(ref.shape)
        d = np.abs(grid.astype(np.float64) - ref.astype(np.float64))
        assert (d <= 8 * GC.EPS * (np.abs(ref.astype(np.float64)) + 2)).all(), gk
        worst = max(worst, float((d / (GC.EPS * (np.abs(ref.astype(np.float64)) + 1))).max()))
        div, rc = int((grid.view(np.uint32) != ref.view(np.uint32)).sum()), int((rcp.view(np.uint32) != ref.view(np.uint32)).sum())
        if name == "ds2":
            n2_div, n2_rcp = div, rc
        else:
            n_all, n_div, n_rcp = n_all + ref.size, n_div + div, n_rcp + rc
    print(f"double-sphere grid goldens: {n_all} values; differing in bits: {n_div} under fx / t (the kernel), {n_rcp} under "
          f"reciprocal(t) * fx (the reference); ds2_grid (8192 values): {n2_div} and {n2_rcp}; worst |d| = {worst:.2f} x 2^-23 (|g| + 1)")
    assert n_all == 39936
    assert n_rcp < n_div < n_all // 4 and n2_rcp < n2_div < 8192 // 4           # the reciprocal form is the reference's; the kernel's differs in last bits only


# ------------------------------------------------------------------------------ closed forms against the goldens
def test_closed_forms_accept_the_reference_rays(z):
    for n in RIGS:
        H, W = (int(v) for v in z[n + "_shape"])
        dist = z[n + "_dist"]
        phi, theta = GC.panorama_args(len(dist), H, W, tuple(z[n + "_lat"]), tuple(z[n + "_lon"]))
        exact, units = GC.panorama_exact(dist, phi, theta)
        ok, worst = GC.check_bound(z[n + "_rays"], exact, units)
        print(f"{n}_rays: worst {worst:.2f} x 2^-23 |exact| (bounds 9 / 4.5 / 9)")
        assert ok.all(), GC.describe_failures(ok, z[n + "_rays"], exact, units)


def test_closed_forms_accept_the_reference_equirect_grids(z):
    for n in RIGS:
        for i in range(len(z[n + "_poses"])):
            pts, ref = z[f"{n}_pts{i}"], z[f"{n}_eq_grid{i}"]
            exact, units = GC.equirect_exact(pts.reshape(1, 3, -1))
            exact = exact.reshape(ref.shape)
            ok, worst = GC.check_bound(ref, exact, units)
            print(f"{n}_eq_grid{i}: worst {worst:.2f} x 2^-23 |exact| (bound 6.5)")
            assert ok.all(), GC.describe_failures(ok, ref, exact, units)


def _transform_bound(T, p):
    """(float64 R p + t, 2 x 2^-23 (|R| |p| + |t|)) for T [B, 4, 4], p [B, 3, M]."""
    T64, p64 = T.astype(np.float64), p.astype(np.float64)
    with np.errstate(all="ignore"):
        exact = np.einsum("bij,bjm->bim", T64[:, :3, :3], p64) + T64[:, :3, 3:4]
        mag = np.einsum("bij,bjm->bim", np.abs(T64[:, :3, :3]), np.abs(p64)) + np.abs(T64[:, :3, 3:4])
    return exact, 2 * GC.EPS * mag + GC.FLOOR


def test_reference_points_within_the_transform_bound(z):
    """The reference's matmul may sum in another order than the kernel: its points sit inside the bound of `transform`."""
    for n in RIGS:
        rays = z[n + "_rays"].reshape(1, 3, -1)
        for i, pose in enumerate(z[n + "_poses"]):
            T = torch.linalg.inv(torch.from_numpy(pose)).to(torch.float32).numpy()[None]
            exact, bnd = _transform_bound(T, rays)
            ref = z[f"{n}_pts{i}"].reshape(1, 3, -1)
            assert (np.abs(ref - exact) <= bnd).all(), f"{n}_pts{i}"
            emu = GC.transform(T, rays)
            print(f"{n}_pts{i}: {int((emu.view(np.uint32) != ref.view(np.uint32)).sum())} of {ref.size} elements differ in bits from the emulated kernel")


@pytest.mark.parametrize("regime", ["random", "zeros", "subnormal"])
def test_emulated_transform_against_float64(regime):
    for shape in GC.ALL_SHAPES:
        for B in GC.BATCHES:
            for first in range(len(GC.TRANSFORM_KINDS)):
                T = GC.transforms(B, first)
                p = GC.points(shape, B, regime).reshape(B, 3, -1)
                exact, bnd = _transform_bound(T, p)
                got = GC.transform(T, p)
                assert (np.abs(got - exact) <= bnd).all(), (shape, B, first)


# ------------------------------------------------------------------------------ generator invariants
def test_shapes_and_batches():
    for shape in GC.SHAPES:
        m = shape[0] * shape[1] * shape[2]
        assert m % 256 != 0 and shape[2] % 2 == 1
        assert (3 * m) % 256 != 0
    assert max(s[0] * s[1] * s[2] for s in GC.SHAPES) > 256                 # more than one block
    assert GC.GOLDEN_SHAPE[0] * GC.GOLDEN_SHAPE[1] * GC.GOLDEN_SHAPE[2] % 256 == 0      # the named exact multiple
    for B in GC.BATCHES:
        T = GC.transforms(B, 0)
        assert T.shape == (B, 4, 4) and len({T[b].tobytes() for b in range(B)}) == B     # a different transform per batch element
    assert np.abs(GC.one_transform("far")[:3, 3]).min() >= 5e5
    sub = GC.one_transform("subnormal")
    assert ((sub != 0) & (np.abs(sub) < 2.0 ** -126)).sum() == 5


@pytest.mark.parametrize("regime", GC.REGIMES)
def test_every_regime_holds_its_values(regime):
    tiny = lambda a: (a != 0) & (np.abs(a) < 2.0 ** -126)
    for shape in GC.ALL_SHAPES:
        for B in GC.BATCHES:
            p = GC.points(shape, B, regime)
            assert p.shape == (B, 3, *shape) and p.dtype == np.float32
            assert np.array_equal(p.view(np.uint32), GC.points(shape, B, regime).view(np.uint32))          # seeded
            q = p.reshape(B, 3, -1)
            with np.errstate(over="ignore"):
                squares_overflow = np.isinf(q[:, 0] * q[:, 0]).any()
            has = {"random": np.isfinite(p).all(), "zeros": (p == 0).any(), "subnormal": tiny(q).all(1).any(),
                   "overflow": (np.abs(p) == np.float32(1e19)).any() and squares_overflow, "nan": np.isnan(p).any(), "origin": (q == 0).all(1).any()}[regime]
            assert has, (regime, shape, B)
    if regime in ("zeros", "origin"):
        p = GC.points(GC.GOLDEN_SHAPE, 3, regime)
        assert (np.signbit(p) & (p == 0)).any() and (~np.signbit(p) & (p == 0)).any()                     # both zeros


@pytest.mark.parametrize("name", list(GC.DS_PARAMS))
def test_boundary_triples_flip_between_neighbouring_floats(name):
    from mvs_gi_amd.dropin import sweep_grids as SG
    params, calib = GC.DS_PARAMS[name]
    assert SG.DoubleSphereSampleGridMaker(params, calib).w2 == GC.ds_w2(params[0], params[1])
    pts = GC.fov_boundary_points(name)                          # asserts 1, 0, 0 itself
    assert pts.shape == (1, 3, 64, 1, 3)
    zz = pts[0, 2, :, 0, :]
    assert (np.nextafter(zz[:, 0], np.float32(-np.inf)).view(np.uint32) == zz[:, 1].view(np.uint32)).all()
    _, mask = GC.double_sphere(pts.reshape(1, 3, -1), *GC.ds_args(name))
    assert np.array_equal(mask.reshape(64, 3), np.tile([True, False, False], (64, 1)))
    # the origin and the non-finite pattern of the emulation: t = 0 gives inf or NaN, never a number
    g, m = GC.double_sphere(np.zeros((1, 3, 1), np.float32), *GC.ds_args(name))
    assert not np.isfinite(g).any() and not m.any()


def test_equirect_special_points():
    cut = GC.branch_cut_points()
    exact, _ = GC.equirect_exact(cut.reshape(1, 3, -1))
    gx = exact[0, :, 0].reshape(-1, len(GC.CUT_Z))
    assert (np.sign(gx) == -np.where(np.signbit(GC.CUT_Z), -1.0, 1.0)).all() and np.allclose(np.abs(gx), np.pi / np.float64(GC.PI_F), rtol=1e-12)
    poles = GC.pole_points().reshape(1, 3, -1)
    assert (poles[0, 0] == 0).all() and (poles[0, 2] == 0).all() and (GC.equirect_args(poles) == 0).all()
