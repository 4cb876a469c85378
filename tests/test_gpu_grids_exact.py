"""GPU (MI355X): the five kernels of csrc/grids.hip element for element.  transform_points and grid_double_sphere use only
correctly rounded operations, so they must return the bits of the host emulation (tests/grid_exact_cases.py; pinned to exact
rational arithmetic and to the reference's outputs by tests/test_grid_exact_host.py) -- no field-of-view band, no conditioning
mask, NaN positions included.  rays_panorama, grid_equirect and rays_equirect_surrogate call the device sin / cos / atan2: every
element must sit within its bound (grid_exact_cases' docstring) of the float64 closed form evaluated from the exactly emulated
float32 arguments -- the branch cut, the poles and zero spans included.  Every test runs with guarded allocations
(tests/guard_arena.py) and carves its inputs from the arena."""
import numpy as np
import pytest
import torch

import grid_exact_cases as GC
import guard_arena
import parity_log
from mvs_gi_amd.dropin import image_sampler, sweep_grids as SG
from oracle import grid_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def arena(request):
    """The guarded allocator of tests/guard_arena.py, as in every GPU module; the tests here also carve their inputs from it."""
    yield from guard_arena.fixture_body(request)


def _in(arena, a):
    return arena.guarded(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))


def _ds_maker(name):
    params, calib = GC.DS_PARAMS[name]
    return SG.DoubleSphereSampleGridMaker(params, calib)


def _record(kernel, tag, got, exact, worst):
    max_rel, mean_l1_rel, max_pixel_rel = GC.error_figures(got, exact)
    print(f"[grid_exact] {kernel}{tag}: worst element {worst:.2f} x 2^-23 |exact|; max_rel {max_rel:.3e}, max_pixel_rel {max_pixel_rel:.3e}")
    parity_log.record(f"grid_exact/{kernel}{tag}", "f32", 1, max_rel, mean_l1_rel, "float64 closed form", max_pixel_rel)


# ------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("regime", GC.REGIMES)
def test_transform_points_bit_for_bit(arena, regime):
    for shape in GC.ALL_SHAPES:
        for B in GC.BATCHES:
            p = GC.points(shape, B, regime)
            for first in range(len(GC.TRANSFORM_KINDS)):
                T = GC.transforms(B, first)
                got = SG.transform_3D_points_torch(_in(arena, T), _in(arena, p)).cpu().numpy()
                want = GC.transform(T, p.reshape(B, 3, -1)).reshape(p.shape)
                assert GC.same_bits(got, want), f"{regime} {shape} B={B} transforms from {first}: {GC.first_difference(got, want)}"


def _assert_double_sphere(arena, name, p, what):
    B = p.shape[0]
    grid, mask = _ds_maker(name).make_grid(_in(arena, p))
    want_grid, want_mask = GC.double_sphere(p.reshape(B, 3, -1), *GC.ds_args(name))
    assert mask.dtype == torch.bool and tuple(mask.shape) == (B, *p.shape[2:]) and tuple(grid.shape) == (B, *p.shape[2:], 2)
    got_grid, got_mask = grid.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(got_mask, want_mask.reshape(got_mask.shape)), \
        f"{what}: mask: {GC.first_difference(got_mask, want_mask.reshape(got_mask.shape))}"
    want_grid = want_grid.reshape(got_grid.shape)
    assert GC.same_bits(got_grid, want_grid), f"{what}: grid: {GC.first_difference(got_grid, want_grid)}"
    return want_grid, want_mask


@pytest.mark.parametrize("regime", GC.REGIMES)
@pytest.mark.parametrize("name", list(GC.DS_PARAMS))
def test_grid_double_sphere_bit_for_bit(arena, name, regime):
    saw_non_finite = saw_inf_square = False
    for shape in GC.ALL_SHAPES:
        for B in GC.BATCHES:
            p = GC.points(shape, B, regime)
            g, _ = _assert_double_sphere(arena, name, p, f"{name} {regime} {shape} B={B}")
            saw_non_finite |= not np.isfinite(g).all()
            with np.errstate(over="ignore"):
                saw_inf_square |= bool(np.isinf(p * p).any())
    # the special values reached the comparison: NaN and the origin (t = 0) give a non-finite grid under every parameter set; an
    # overflowing square need not (xi > 0: t = +inf, fx / t = 0 and the grid is the principal point), so there the input is checked
    assert saw_non_finite or regime not in ("nan", "origin")
    assert saw_inf_square or regime != "overflow"


@pytest.mark.parametrize("name", list(GC.DS_PARAMS))
def test_grid_double_sphere_on_the_field_of_view_boundary(arena, name):
    """The mask flips between neighbouring floats exactly where the emulated predicate does: 1, 0, 0 on every triple."""
    p = GC.fov_boundary_points(name)
    _, mask = _assert_double_sphere(arena, name, p, f"{name} boundary")
    assert np.array_equal(mask.reshape(-1, 3), np.tile([True, False, False], (p.shape[2], 1)))
    p3 = np.ascontiguousarray(np.concatenate([p, p[:, :, ::-1], p[:, :, :, :, ::-1]], 0))      # B = 3, reordered per batch element
    _assert_double_sphere(arena, name, p3, f"{name} boundary B=3")


# ------------------------------------------------------------------------------ per-element bounds
def _panorama(arena, dist, lat, lon, shape):
    rm = SG.RayMaker_UEPanorama(np.zeros(1, np.float32), lon, lat, device=DEV)
    rm.dist = _in(arena, dist)
    return rm.make_rays_for_candidates(shape)


@pytest.mark.parametrize("span", list(GC.PANORAMA_RANGES))
def test_rays_panorama_within_bounds(arena, span):
    lat, lon = GC.PANORAMA_RANGES[span]
    worst, gots, exacts = 0.0, [], []
    for N, H, W in GC.ALL_SHAPES:
        dist = GC.candidate_distances(N)
        got = _panorama(arena, dist, lat, lon, (H, W)).cpu().numpy()
        phi, theta = GC.panorama_args(N, H, W, lat, lon)
        exact, units = GC.panorama_exact(dist, phi, theta)
        assert got.shape == (3, N, H, W)
        ok, w = GC.check_bound(got, exact, units)
        assert ok.all(), f"{span} {(N, H, W)}: " + GC.describe_failures(
            ok, got, exact, units, lambda i: f"d={dist[i[1]]!r} phi={phi[i[2]]!r} theta={theta[i[3]]!r}")
        assert (got[exact == 0] == 0).all(), f"{span} {(N, H, W)}: an exact zero is not +-0"
        worst = max(worst, w)
        gots.append(got.ravel()), exacts.append(exact.ravel())
    if span == "zero_span":
        assert (np.concatenate(exacts) == 0).any()
    assert dist[0] == np.float32(1e-3) and dist[-1] == np.float32(1e4)
    _record("rays_panorama", f"[{span}]", np.concatenate(gots), np.concatenate(exacts), worst)


def _assert_equirect(arena, p, what):
    """Every element within its bound; where x = z = 0 (poles, origin) gy within its bound and gx finite with |gx| <= 1."""
    B = p.shape[0]
    got = SG.EquirectangularSampleGridMaker().make_grid(_in(arena, p)).cpu().numpy()
    assert got.shape == (B, *p.shape[2:], 2)
    got = got.reshape(B, -1, 2)
    q = p.reshape(B, 3, -1)
    exact, units = GC.equirect_exact(q)
    ok, worst = GC.check_bound(got, exact, units)
    pole = (q[:, 0] == 0) & (q[:, 2] == 0)
    gx = got[..., 0]
    ok[..., 0] = np.where(pole, np.isfinite(gx) & (np.abs(gx) <= 1), ok[..., 0])
    assert ok.all(), f"{what}: " + GC.describe_failures(ok, got, exact, units, lambda i: f"x, y, z = {q[i[0], :, i[1]]!r}")
    assert np.array_equal(np.isnan(got), np.isnan(exact)), f"{what}: NaN in must give NaN out, and nothing else may"
    keep = ~np.stack([pole, np.zeros_like(pole)], -1)
    return got[keep], exact[keep], worst


@pytest.mark.parametrize("regime", GC.REGIMES)
def test_grid_equirect_within_bounds(arena, regime):
    worst, gots, exacts = 0.0, [], []
    for shape in GC.ALL_SHAPES:
        for B in GC.BATCHES:
            g, e, w = _assert_equirect(arena, GC.points(shape, B, regime), f"{regime} {shape} B={B}")
            worst = max(worst, w)
            gots.append(g), exacts.append(e)
    _record("grid_equirect", f"[{regime}]", np.concatenate(gots), np.concatenate(exacts), worst)


def test_grid_equirect_branch_cut_and_poles(arena):
    """x < 0 with z in {+0, -0, +-smallest subnormal, +-1e-30}: |gx| = 1 within the bound with the sign of -z; x = z = 0: gy within
    the bound, gx finite and |gx| <= 1 (which of the admissible values the device atan2 returns at signed zeros is not asserted)."""
    cut = GC.branch_cut_points()
    g, e, worst = _assert_equirect(arena, cut, "branch cut")
    got = SG.EquirectangularSampleGridMaker().make_grid(_in(arena, cut)).cpu().numpy()
    gx = got[0, :, 0, :, 0]                                                     # [n_x, len(CUT_Z)]
    want_sign = np.where(np.signbit(GC.CUT_Z), 1.0, -1.0)[None, :]
    assert (np.sign(gx) == want_sign).all(), f"gx on the cut: {gx!r}"
    assert (np.abs(np.abs(gx.astype(np.float64)) - 1.0) <= GC.bound(1.0, GC.UNITS_EQUIRECT) + 2.0 ** -24).all()
    poles = GC.pole_points()
    _assert_equirect(arena, poles, "poles and origin")
    _record("grid_equirect", "[branch cut]", g, e, worst)


def test_rays_equirect_surrogate_within_bounds(arena):
    worst, gots, exacts = 0.0, [], []
    for H, W in GC.SURROGATE_SHAPES:
        got = image_sampler.equirect_surrogate_rays(H, W, device=DEV).cpu().numpy()
        exact, units = GC.surrogate_exact(H, W)
        assert got.shape == (3, H, W)
        ok, w = GC.check_bound(got, exact, units)
        _, _, lon, lat = GC.surrogate_args(H, W)
        assert ok.all(), f"{(H, W)}: " + GC.describe_failures(ok, got, exact, units, lambda i: f"lat={lat[i[1]]!r} lon={lon[i[2]]!r}")
        assert (got[exact == 0] == 0).all()
        worst = max(worst, w)
        gots.append(got.ravel()), exacts.append(exact.ravel())
    _record("rays_equirect_surrogate", "", np.concatenate(gots), np.concatenate(exacts), worst)


# ------------------------------------------------------------------------------ composition
def test_make_sweep_grids_is_the_chain_camera_by_camera(arena):
    """A rig mixing double-sphere and equirect makers: make_sweep_grids == make_grid(transform(inv_pose, rays)) per camera."""
    D, shape = 5, (9, 29)
    lat, lon = GC.PANORAMA_RANGES["g16_band"]
    rm = SG.RayMaker_UEPanorama(GC.candidate_distances(D), lon, lat, device=DEV)
    makers = [_ds_maker("default"), SG.EquirectangularSampleGridMaker(), _ds_maker("ds2")]
    poses = G.ring_poses(3)
    grids, masks = SG.make_sweep_grids(rm, makers, poses, shape)
    assert tuple(grids.shape) == (1, 3, D, *shape, 2) and grids.dtype == torch.float32
    assert tuple(masks.shape) == (1, 3, D, *shape, 1) and masks.dtype == torch.bool
    rays = rm.make_rays_for_candidates(shape)
    for n, (maker, pose) in enumerate(zip(makers, poses)):
        inv = torch.linalg.inv(pose.to(torch.float64)).to(torch.float32)
        pts = SG.transform_3D_points_torch(inv.unsqueeze(0).to(DEV), rays.unsqueeze(0))
        out = maker.make_grid(pts)
        g, m = out if isinstance(out, tuple) else (out, torch.ones(out.shape[:-1], dtype=torch.bool, device=DEV))
        assert torch.equal(grids[0, n], g[0]) and torch.equal(masks[0, n, ..., 0], m[0]), f"camera {n}"
        assert not bool(torch.isnan(grids[0, n]).any()), f"camera {n}: an element was not written"
        # and the chain is the emulation's bits on the kernel's own rays
        want_pts = GC.transform(inv.numpy()[None], rays.cpu().numpy().reshape(1, 3, -1))
        assert GC.same_bits(pts.cpu().numpy().reshape(1, 3, -1), want_pts)
    assert bool(masks[0, 1].all()) and not bool(masks[0, 0].all()) and bool(masks[0, 0].any())
