"""CPU: the definition of the volumetric fusion as tests/tsdf_cases.py restates it -- the toroidal store (scrolling and then
integrating is clearing by hand and then integrating), the conditions the GPU tests' cases are chosen for, the semantic case (a
sphere seen from inside, integrated from four places and ray-cast from a fifth, against the bar derived in tsdf_cases), every
Python-side refusal of dropin.TsdfVolume and hip_ops.tsdf_* before a pointer is taken, and set_pose's origin arithmetic.

The semantic case through the fp32 restatement (printed by the test): 0 of 1152 pixels miss; |t* - t_true| is at worst 0.708 voxel
(median 0.144) against the bar of 1.222 voxel."""
import math
import types

import numpy as np
import pytest
import torch

import tsdf_cases as TC
from mvs_gi_amd import dropin, hip_ops as H

F32 = np.float32
ERRORS = (AssertionError, TypeError, ValueError, RuntimeError)


def _setup(name, kind, bf=96.0):
    c = TC.CASES[name]
    P = TC.poses(kind, name)
    return c, TC.make_inputs(name, bf), TC.rigid_inverse(P), TC.origin_of(P, c["dims"]), TC.affine(c["ranges"], c["hw"])


@pytest.mark.parametrize("shift", list(TC.SHIFTS))
@pytest.mark.parametrize("kind", TC.POSES)
@pytest.mark.parametrize("name", list(TC.CASES))
def test_scrolling_is_clearing_by_hand(name, kind, shift):
    """A slot is fresh exactly when it holds another world voxel than at the previous integrate: cleared by hand from that rule and
    integrated at rest, the volume is the bits of the scroll."""
    c, inp, T, origin, aff = _setup(name, kind)
    prev = TC.shifted(origin, shift, c["dims"])
    par = TC.params(96.0)
    got = TC.integrate(inp["vol"], inp["inv"], inp["std"], inp["mask"], T, origin, prev, par, aff)
    now, then = TC.world_index(origin, c["dims"]), TC.world_index(prev, c["dims"])
    moved = np.zeros(inp["vol"].shape[:-1], bool)
    for a in range(3):
        moved = moved | (now[a] != then[a])
    assert np.array_equal(moved, got["fresh"])
    by_hand = inp["vol"].copy()
    by_hand[moved] = (1, 0)
    want = TC.integrate(by_hand, inp["inv"], inp["std"], inp["mask"], T, origin, origin, par, aff)
    assert not want["fresh"].any()
    assert np.array_equal(got["vol"].view(np.uint32), want["vol"].view(np.uint32))
    n = moved[0].size
    expect = {"same": 0, "all": n}.get(shift)
    if expect is not None:
        assert int(moved[0].sum()) == expect
    elif shift == "one":
        assert int(moved[0].sum()) == n // c["dims"][0]                  # one plane of x
    # a fresh voxel that is rejected is stored as (1, 0)
    idle = moved & ~got["hit"]
    assert (got["vol"][idle] == (1, 0)).all()
    for a, N in enumerate(c["dims"]):                                    # every slot holds the world voxel it is the modulus of
        assert ((now[a] >= origin[:, a].reshape(-1, 1, 1, 1)) & (now[a] < origin[:, a].reshape(-1, 1, 1, 1) + N)).all()
        assert (np.mod(now[a], N) == np.arange(N).reshape(now[a].shape[1:])).all()


def test_the_cases_reach_what_they_are_chosen_for():
    classes = set()
    for name, c in TC.CASES.items():
        seen = dict(hit=0, clamp=0, behind=0, outside=0, zero=0, near_only=0, w_sat=0, in_band=0)
        for kind in TC.POSES:
            _, inp, T, origin, aff = _setup(name, kind)
            for b in range(c["B"]):
                lo, hi = origin[b], origin[b] + np.asarray(c["dims"])
                classes.add("negative" if (hi <= 0).all() else "zero" if (lo == 0).all() else "straddle" if ((lo < 0) & (hi > 0)).any() else "positive")
            r = TC.integrate(inp["vol"], inp["inv"], inp["std"], inp["mask"], T, origin, origin, TC.params(96.0), aff)
            hit = r["hit"]
            seen["hit"] += int(hit.sum())
            seen["clamp"] += int((hit & (r["obs"] == 1)).sum())
            seen["in_band"] += int((hit & (np.abs(r["obs"]) < 1)).sum())
            seen["behind"] += int((r["near"] & (r["sdf"] < -F32(TC.PARAMS["trunc"]))).sum())
            seen["outside"] += int((r["near"] & ~((r["cy"] >= 0) & (r["cy"] < c["hw"][0]) & (r["cx"] >= 0) & (r["cx"] < c["hw"][1]))).sum())
            seen["zero"] += int((r["r2"] == 0).sum())
            seen["near_only"] += int((r["near"] & (r["r"] < F32(TC.PARAMS["r_range"][0]))).sum())
            seen["w_sat"] += int((hit & (inp["vol"][..., 1] >= F32(TC.PARAMS["w_max"])) & (r["vol"][..., 1] == F32(TC.PARAMS["w_max"]))).sum())
            assert r["vol"][..., 1].max() <= F32(TC.PARAMS["w_max"]) or not hit.all()
        print(f"[tsdf] {name}: " + ", ".join(f"{k} {v}" for k, v in seen.items()))
        assert seen["hit"] and seen["zero"] and seen["in_band"], (name, seen)       # "shift" puts the rig on a voxel's centre
        if name != "line":
            assert seen["clamp"] and seen["behind"] and seen["near_only"] and seen["w_sat"], (name, seen)
        if c["ranges"] is TC.PART:
            assert seen["outside"], (name, seen)
    assert {"negative", "zero", "straddle"} <= classes, classes
    inp = TC.make_inputs("odd")
    assert all(np.isnan(inp[k]).any() and np.isinf(inp[k]).any() and (inp[k] == 0).any() and (inp[k] < 0).any() for k in ("inv", "std"))
    assert (inp["mask"] == 0).any() and (inp["vol"][..., 1] > TC.PARAMS["w_max"]).any() and (inp["vol"][..., 1] == F32(TC.PARAMS["w_max"])).any()


def test_without_std_the_weight_counts_observations():
    c, inp, T, origin, aff = _setup("b2", "rigid")
    vol = np.empty_like(inp["vol"])
    vol[..., 0], vol[..., 1] = 1, 0
    inv = np.where(np.isfinite(inp["inv"]) & (inp["inv"] > 0), inp["inv"], F32(40.0)).astype(F32)
    par = dict(TC.params(96.0), w_max=2.0)
    hits = None
    for n in (1, 2, 3):
        r = TC.integrate(vol, inv, None, None, T, origin, origin, par, aff)
        hits = r["hit"] if hits is None else hits
        assert np.array_equal(r["hit"], hits)
        assert (r["vol"][..., 1][hits] == min(n, 2)).all() and (r["vol"][..., 1][~hits] == 0).all()
        assert np.allclose(r["vol"][..., 0][hits], r["obs"][hits], rtol=1e-6, atol=1e-6)       # the mean of equal observations
        vol = r["vol"]


def test_a_planar_crossing_at_a_dyadic_place_is_exact():
    dims, voxel, bf = (8, 4, 4), 0.25, 96.0
    vol = TC.plane_volume(dims)
    ray_table = np.zeros((3, 1, 4), F32)
    ray_table[0] = 1                                                     # four rays along +x
    P = np.eye(4, dtype=F32)[None].copy()
    P[0, :3, 3] = [0.125, 0.5, 0.5]
    got = TC.raycast(vol, ray_table, P, np.zeros((1, 3), np.int32), voxel, 0.25, 0.125, 12, 1.0, bf)
    # x_k = 0.125 + 0.25 + 0.125 k enters voxel 4 (x >= 1.0) at k = 5; f = 0.125 -> -0.125: t* = t_4 + step / 2 = 0.8125
    assert (got["steps"] == 5).all() and (got["t"] == 0.8125).all() and (got["weight"] == 2).all()
    assert np.array_equal(got["inv"], np.full((1, 1, 4), F32(bf) / F32(0.8125)))
    # from the other side f rises through zero: a back face, ignored
    P[0, :3, 3] = [1.875, 0.5, 0.5]
    back = TC.raycast(vol, -ray_table, P, np.zeros((1, 3), np.int32), voxel, 0.25, 0.125, 12, 1.0, bf)
    assert (back["steps"] == 12).all() and (back["inv"] == 0).all() and (back["weight"] == 0).all()
    # a weight below w_min on either side of the crossing: no crossing
    vol[..., 3, 1] = 0.5
    assert (TC.raycast(vol, ray_table, np.eye(4, dtype=F32)[None], np.zeros((1, 3), np.int32), voxel, 0.25, 0.125, 12, 1.0, bf)["steps"] == 12).all()


def test_the_sphere_meets_the_derived_bar():
    got, true = TC.sphere_on_the_cpu()
    t = got["t"]
    miss = np.isnan(t)
    bar = TC.sphere_bar()
    err = np.abs(t - true)[~miss]
    vx = TC.SPHERE["voxel"]
    print(f"[tsdf] sphere, fp32 restatement: {int(miss.sum())} of {t.size} pixels miss; |t* - t_true| worst {err.max() / vx:.3f} voxel, "
          f"median {np.median(err) / vx:.3f} voxel; bar {bar / vx:.3f} voxel ({bar:.4f} m)")
    assert abs(bar - 0.1528) < 1e-3                                       # the docstring's figure is what the function computes
    assert not miss.any()
    assert err.max() <= bar
    assert np.array_equal(got["inv"][~miss], (F32(TC.SPHERE["bf"]) / t[~miss].astype(F32)))
    assert (got["weight"][~miss] >= 1).all() and (got["steps"][~miss] < TC.sphere_K()).all()


# ---------------------------------------------------------------------------------------------- the Python side
def _fake_reprojector(**kw):
    a = dict(rays=torch.zeros((3, 6, 10)), bf=96.0, out_shape=(6, 10), reproject=None, long_range=TC.FULL[0], lat_range=TC.FULL[1],
             _inv=lambda t: t)
    a.update(kw)
    return types.SimpleNamespace(**a)


@pytest.fixture
def no_launch(monkeypatch):
    launched = []
    monkeypatch.setattr(H, "_call", lambda name, *a: launched.append(name))
    yield launched
    assert not launched, launched


def test_the_volume_refuses_what_it_cannot_take(no_launch):
    rp = _fake_reprojector()
    ok = dict(dims=(10, 6, 5), voxel=0.25)
    v = dropin.TsdfVolume(rp, **ok)
    assert v.trunc == 1.0 and v.step == 0.125 and v.r_range == (0.0, H.TSDF_FLT_MAX) and v.w_min == 1.0 and v.w_max == 64.0
    assert v.t0 == 0.25 and v.K == int(math.floor((0.5 * 0.25 * math.sqrt(161) - 0.25) / 0.125)) + 1
    assert dropin.TsdfVolume(rp, march=(0.5, 2.0, 0.25), **ok).K == 7
    for make in (lambda: dropin.TsdfVolume(object(), **ok), lambda: dropin.TsdfVolume(_fake_reprojector(long_range=None, lat_range=None), **ok),
                 lambda: dropin.TsdfVolume(_fake_reprojector(lat_range=(-1.0, 1.0)), **ok),
                 lambda: dropin.TsdfVolume(rp, dims=(10, 6), voxel=0.25), lambda: dropin.TsdfVolume(rp, dims=(10, 0, 5), voxel=0.25),
                 lambda: dropin.TsdfVolume(rp, dims=(10.5, 6, 5), voxel=0.25), lambda: dropin.TsdfVolume(rp, dims=(1 << 11, 1 << 10, 1 << 10), voxel=0.25),
                 lambda: dropin.TsdfVolume(rp, dims=None, voxel=0.25),
                 lambda: dropin.TsdfVolume(rp, dims=(10, 6, 5), voxel=0.0), lambda: dropin.TsdfVolume(rp, dims=(10, 6, 5), voxel=-1.0),
                 lambda: dropin.TsdfVolume(rp, dims=(10, 6, 5), voxel=float("nan")), lambda: dropin.TsdfVolume(rp, dims=(10, 6, 5), voxel=float("inf")),
                 lambda: dropin.TsdfVolume(rp, trunc=0.0, **ok), lambda: dropin.TsdfVolume(rp, trunc=-1.0, **ok),
                 lambda: dropin.TsdfVolume(rp, trunc=1e30, **ok), lambda: dropin.TsdfVolume(rp, trunc=float("nan"), **ok),
                 lambda: dropin.TsdfVolume(rp, w_max=0.0, **ok), lambda: dropin.TsdfVolume(rp, w_max=float("inf"), **ok),
                 lambda: dropin.TsdfVolume(rp, r_range=(1.0, 1.0), **ok), lambda: dropin.TsdfVolume(rp, r_range=(-0.1, 1.0), **ok),
                 lambda: dropin.TsdfVolume(rp, r_range=(float("nan"), 1.0), **ok), lambda: dropin.TsdfVolume(rp, r_range=1.0, **ok),
                 lambda: dropin.TsdfVolume(rp, w_min=float("nan"), **ok), lambda: dropin.TsdfVolume(rp, w_min=float("inf"), **ok),
                 lambda: dropin.TsdfVolume(rp, march=(0.0, 1.0, 0.0), **ok), lambda: dropin.TsdfVolume(rp, march=(1.0, 0.5, 0.1), **ok),
                 lambda: dropin.TsdfVolume(rp, march=(0.0, 1000.0, 0.1), **ok), lambda: dropin.TsdfVolume(rp, march=(-0.1, 1.0, 0.1), **ok),
                 lambda: dropin.TsdfVolume(rp, march=(0.0, float("inf"), 0.1), **ok), lambda: dropin.TsdfVolume(rp, march=(0.0, 1.0), **ok)):
        with pytest.raises(ERRORS):
            make()
    with pytest.raises(ValueError):
        dropin.TsdfVolume(_fake_reprojector(long_range=None, lat_range=None), **ok)
    # the stage on the CPU: refused before any buffer's address is taken
    inv = torch.ones((1, 6, 10))
    for call in (lambda: v.integrate(inv), lambda: v.integrate(inv.double()), lambda: v.integrate(inv.numpy()),
                 lambda: v.raycast(want=("inv", "nothing")), lambda: v.raycast(want=()), lambda: v.raycast(P=torch.eye(3)),
                 lambda: v.set_pose(torch.eye(4).double()), lambda: v.set_pose(torch.eye(4).repeat(2, 1, 1), B=3)):
        with pytest.raises(ERRORS):
            call()


def test_the_wrappers_refuse_host_tensors_and_bad_scalars(no_launch):
    vol, inv, T = torch.zeros((1, 5, 6, 10, 2)), torch.ones((1, 6, 10)), torch.eye(4)[None]
    org = torch.zeros((1, 3), dtype=torch.int32)
    aff = H.temporal_affine(TC.FULL[0], TC.FULL[1], (6, 10))
    with pytest.raises(RuntimeError):
        H.tsdf_integrate(vol, inv, T, org, org, 96.0, aff, 0.25, 1.0)
    with pytest.raises(RuntimeError):
        H.tsdf_raycast(vol, torch.zeros((3, 6, 10)), T, org, 96.0, 0.25, 0.25, 0.125, 8)
    for args in ((0, 10, 6, 5), (1, 0, 6, 5), (1, 1 << 11, 1 << 10, 1 << 10), (1 << 24, 1 << 10, 1 << 10, 1 << 9)):
        with pytest.raises(ValueError):
            H.tsdf_dims(*args)
    H.tsdf_dims(64, 256, 256, 64)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError):
            H._tsdf_scalar(bad, "voxel")
    assert H._tsdf_scalar(0.0, "t0", low_ok=True) == 0.0
    for shape in ((1, 1 << 25, 4), (1, 1 << 16, 1 << 15), (1 << 22, 1 << 12, 1 << 12)):
        with pytest.raises(ValueError):
            H._pano_map("volumetric fusion", 31, *shape)


def test_the_origin_of_a_negative_position_is_floored():
    half = torch.tensor([5, 3, 2], dtype=torch.int32)
    t = torch.tensor([[-0.01, 0.0, 0.26], [-7.3, -5.25, -4.9], [0.125, -0.375, 0.625], [1.31, 0.8, 0.7]])
    got = dropin.TsdfVolume.origin_of(t, 0.25, half)
    assert got.dtype == torch.int32
    want = [[-1 - 5, 0 - 3, 1 - 2], [-30 - 5, -21 - 3, -20 - 2], [0 - 5, -2 - 3, 2 - 2], [5 - 5, 3 - 3, 2 - 2]]
    assert got.tolist() == want
    P = np.tile(np.eye(4, dtype=F32), (4, 1, 1))
    P[:, :3, 3] = t.numpy()
    assert np.array_equal(TC.origin_of(P, (10, 6, 5)), np.asarray(want, np.int32))
    # the rig's voxel is the middle one of the coverage
    rig = np.floor(t.numpy() / F32(0.25)).astype(np.int64)
    assert ((rig >= got.numpy()) & (rig < got.numpy() + np.asarray([10, 6, 5]))).all() and np.array_equal(rig - got.numpy(), np.tile([5, 3, 2], (4, 1)))
    T = TC.rigid_inverse(TC.poses("rigid", "b3"))
    back = np.einsum("bij,bjk->bik", T.astype(np.float64), TC.poses("rigid", "b3").astype(np.float64))
    assert np.abs(back - np.eye(4)).max() < 1e-6
