"""CPU: the camera range images and the visibility test -- the definition's restatement (tests/visibility_cases.py) on analytic scenes
whose answer is known, the conditions its cases exist for, its steps 1-5 against tests/reproject_cases.py's composition, header /
binding agreement for the three new symbols, the entry points' own validation, and every argument error of hip_ops, dropin.Visibility,
PhotoConsistency(visibility=) and InferencePipeline(visibility=) that is raised before anything touches a device.

The scenes: three equirectangular cameras on G.ring_poses(3, r), the rig map 40 x 160 (RC.LON x RC.LAT), bf = 1."""
import ctypes
import os
import re

import pytest
import torch

import reproject_cases as RC
import visibility_cases as VC
from mvs_gi_amd import _lib, dropin, hip_ops as H
from mvs_gi_amd.configs import CONFIGS
from mvs_gi_amd.pipeline import InferencePipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvsgi_camera_range_f32", "mvsgi_visibility_f32", "mvsgi_photo_consistency_seen_f32")
HW = (40, 160)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _occluded(v, r):
    return v["valid"] & v["live"].unsqueeze(1) & ~r["visible"]


# ------------------------------------------------------------------------------ the definition on scenes with a known answer
@pytest.mark.parametrize("radius", [0.1, 0.3])
def test_a_sphere_occludes_nothing(radius):
    """(a) d = 10 everywhere: every point is on one convex surface around the rig, so no camera's view of a point is blocked.  A cell
    still holds the minimum over its points, which lie at slightly different ranges: tol = 0.02 absorbs that at every buffer, tol = 0
    does not (about half the pixels at 40 x 160), which shows that the tolerance is what decides."""
    v = VC.ring_scene(torch.full((1,) + HW, 0.1), radius)
    n_ok = int((v["valid"] & v["live"].unsqueeze(1)).sum())
    assert n_ok == 3 * HW[0] * HW[1]                                      # an equirectangular camera sees every direction
    for zshape in [(80, 160), (40, 160), (40, 80)]:
        r = VC.restate(v, zshape, tol=0.02)
        assert int(_occluded(v, r).sum()) == 0, zshape
        assert int(r["n_visible"].min()) == 3
    strict = int(_occluded(v, VC.restate(v, (40, 160), tol=0.0)).sum())
    print(f"[visibility] sphere, ring {radius}: tol 0 at 40 x 160 flags {strict} of {n_ok} ({strict / n_ok:.1%})")
    assert 0.3 * n_ok < strict < 0.7 * n_ok


def test_b_a_step_occludes_background_beside_it_only():
    """(b) d = 1 on columns W/4 .. W/2 - 1, d = 10 elsewhere; buffer 80 x 160, tol 0.02.  No foreground pixel is occluded in any camera,
    every occluded pixel is background, and the occluded pixels lie in the band of columns next to the foreground that the ring's
    parallax can reach: [0, W/4) on one side, [W/2, W/2 + W/6) on the other."""
    H_, W = HW
    d = torch.full((1, H_, W), 10.0)
    d[:, :, W // 4:W // 2] = 1.0
    v = VC.ring_scene(1.0 / d)
    occ = _occluded(v, VC.restate(v, (80, 160), tol=0.02))[0]               # [N, H, W]
    cols = torch.arange(W)
    foreground = (cols >= W // 4) & (cols < W // 2)
    band = (cols < W // 4) | ((cols >= W // 2) & (cols < W // 2 + W // 6))
    for n in range(3):
        hit = occ[n].any(dim=0)
        where = torch.nonzero(hit).flatten().tolist()
        print(f"[visibility] step: camera {n}: {int(occ[n].sum())} occluded pixels, columns {where[:1]} .. {where[-1:]}")
        assert not bool(hit[foreground].any()), n
        assert not bool(hit[~band].any()), n
    assert bool(occ.any())                                                # the step does hide something


def test_c_a_masked_out_occluder_occludes_nothing():
    H_, W = HW
    d = torch.full((1, H_, W), 10.0)
    d[:, :, W // 4:W // 2] = 1.0
    v = VC.ring_scene(1.0 / d)
    mask = torch.ones((H_, W), dtype=torch.uint8)
    mask[:, W // 4:W // 2] = 0
    r = VC.restate(v, (80, 160), tol=0.02, mask=mask)
    occ = _occluded(v, r)[0]
    cols = torch.arange(W)
    background = (cols < W // 4) | (cols >= W // 2)
    assert not bool(occ[:, :, background].any())                          # the background sees through the unrendered foreground
    assert not bool(r["splat"][0][:, :, ~background].any()) and bool(r["splat"][0][:, :, background].all())
    # the excluded pixels are tested all the same: against the background's buffer they are nearer than anything, so visible
    assert bool(r["visible"][0][:, :, ~background].all())


def test_d_values_that_are_not_live_are_never_visible_and_never_splatted():
    inv = torch.full((1,) + HW, 0.1)
    bad = torch.tensor(VC.BAD_INV)
    inv[0, 5, :8] = bad.repeat(2)
    inv[0, 20, 100:104] = bad
    v = VC.ring_scene(inv)
    not_live = ~v["live"][0]
    assert int(not_live.sum()) == 12
    clean = VC.ring_scene(torch.where(not_live, torch.full_like(inv[0], 0.1), inv[0]).unsqueeze(0))
    for fp in (1, 2):
        r = VC.restate(v, (80, 160), footprint=fp)
        assert not bool(r["visible"][0][:, not_live].any()) and not bool(r["splat"][0][:, not_live].any())
        assert bool((r["n_visible"][0][not_live] == 0).all())
        # the buffer is that of the scene without them, less their own cells' contributions: never smaller anywhere
        assert bool((r["z2"] >= VC.restate(clean, (80, 160), footprint=fp)["z2"]).all())


@pytest.mark.parametrize("name", list(VC.ALL))
def test_e_footprint_two_fills_at_least_as_many_cells(name):
    one, two = VC.build(name, 1)["restated"], VC.build(name, 2)["restated"]
    f1, f2 = torch.isfinite(one["z2"]), torch.isfinite(two["z2"])
    print(f"[visibility] {name}: {int(f1.sum())} cells filled with footprint 1, {int(f2.sum())} with 2, of {f1.numel()}")
    assert int(f2.sum()) >= int(f1.sum())
    # empty cells are +inf, and the root of the buffer is the range image
    assert bool((one["z2"][~f1] == float("inf")).all()) and bool((one["range"][~f1] == float("inf")).all())


# ------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", list(VC.ALL))
def test_cases_meet_their_conditions_and_views_are_the_reprojection(name):
    """VC.build asserts the conditions; steps 1-5 of views() are reproject_cases.compose's bits on the same rig."""
    c = VC.build(name)
    s = c["spec"]
    for mask in ("mask_hw", "mask_frames"):
        m = VC.build(name, mask=mask)
        assert int(m["restated"]["splat"].sum()) < int(c["restated"]["splat"].sum()), (name, mask)
    r = RC.compose(s["base"], c["inp"]["inv"], None, ray_table=VC.rays(s["hw"]))
    assert torch.equal(r["valid"], c["views"]["valid"])
    assert torch.equal(r["grid"].view(torch.int32), c["views"]["grid"].view(torch.int32))
    print(f"[visibility] {name}: {int(c['occluded'].sum())} occluded of {int((c['views']['valid'] & c['views']['live'].unsqueeze(1)).sum())} valid live (pixel, camera) pairs")
    if name == "one_cell":
        z = c["restated"]["z2"]
        ok = c["views"]["valid"] & c["views"]["live"].unsqueeze(1)
        for b in range(s["B"]):
            for n in range(s["N"]):
                assert float(z[b, n, 0, 0]) == float(c["views"]["r2"][b, n][ok[b, n]].min())


def test_k2_is_rounded_once_from_double():
    assert float(VC.k2(0.02)) == float(torch.tensor((1.0 + 0.02) * (1.0 + 0.02), dtype=torch.float32))
    assert H.visibility_k2(0.0) == 1.0 and H.visibility_k2(0.02) == 1.02 * 1.02 and H.VISIBILITY_TOL == VC.TOL
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            H.visibility_k2(bad)


# ------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_binding_lists_the_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsgi.h")).read(), flags=re.S)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/mvsgi.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert name in text
    photo, seen = _lib.SIGNATURES["mvsgi_photo_consistency_f32"][1], _lib.SIGNATURES["mvsgi_photo_consistency_seen_f32"][1]
    assert len(photo) == 26 and len(seen) == 27 and seen[:25] == photo[:25] and seen[25] is ctypes.c_void_p and seen[26] is photo[25]
    assert tuple(H.VISIBILITY_OUTPUTS) == ("visible", "n_visible", "range")


P = ctypes.c_void_p
_T = (ctypes.c_float * 16)(*[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
_EQ = (ctypes.c_float * 10)(1, *[0] * 9)
_BAD_CAM = (ctypes.c_float * 10)(2, *[0] * 9)
_DS_CAM = (ctypes.c_float * 10)(0, -0.2, 0.6, 200, 200, 600, 500, 0.5, 0, 1223)
_SHARED = [(dict(inv=None), b"null pointer"), (dict(rays=None), b"null pointer"), (dict(T=None), b"null pointer"),
           (dict(cams=None), b"null pointer"), (dict(z2=None), b"null pointer (z2)"), (dict(N=0), b"cameras"), (dict(N=9), b"cameras"),
           (dict(B=0), b"non-positive"), (dict(H=0), b"non-positive"), (dict(W=0), b"non-positive"), (dict(Hz=0), b"non-positive"),
           (dict(Wz=0), b"non-positive"), (dict(H=1 << 16, W=1 << 15), b"too large"), (dict(Hz=1 << 16, Wz=1 << 15), b"too large"),
           (dict(Hz=(1 << 24) + 1, Wz=1), b"2^24"), (dict(B=1 << 31), b"too large"),
           (dict(cams=ctypes.cast(_BAD_CAM, P)), b"unknown model id"), (dict(cams=ctypes.cast(_DS_CAM, P)), b"calib shape"),
           (dict(inv=P(68)), b"16-byte aligned when W"), (dict(rays=P(72)), b"16-byte aligned when W"), (dict(z2=P(72)), b"16-byte")]


def test_camera_range_validates_before_launching(lib):
    ok = dict(inv=P(64), rays=P(64), T=ctypes.cast(_T, P), cams=ctypes.cast(_EQ, P), mask=None, mpf=0, footprint=1, z2=P(64), B=1, N=1, H=4,
              W=8, Hz=8, Wz=8, bf=96.0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mvsgi_camera_range_f32(*[a[k] for k in ok], None)
    for kw, text in _SHARED + [(dict(footprint=0), b"footprint"), (dict(footprint=3), b"footprint"), (dict(mpf=2), b"mask_per_frame"),
                               (dict(mask=P(66)), b"4-byte")]:
        assert call(**kw) != 0, kw
        assert text in lib.mvsgi_last_error(), (kw, lib.mvsgi_last_error())


def test_visibility_validates_before_launching(lib):
    ok = dict(inv=P(64), rays=P(64), T=ctypes.cast(_T, P), cams=ctypes.cast(_EQ, P), z2=P(64), k2=1.0404, visible=P(64), n_visible=P(64),
              range=P(64), B=1, N=1, H=4, W=8, Hz=8, Wz=8, bf=96.0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mvsgi_visibility_f32(*[a[k] for k in ok], None)
    for kw, text in _SHARED + [(dict(visible=None, n_visible=None, range=None), b"every output is NULL"), (dict(k2=0.99), b"k2"),
                               (dict(k2=float("nan")), b"k2"), (dict(k2=float("inf")), b"k2"), (dict(visible=P(68)), b"16-byte"),
                               (dict(n_visible=P(72)), b"16-byte"), (dict(range=P(68)), b"16-byte")]:
        assert call(**kw) != 0, kw
        assert text in lib.mvsgi_last_error(), (kw, lib.mvsgi_last_error())


def test_photo_seen_validates_like_the_entry_point_it_extends(lib):
    wsb = lib.mvsgi_photo_ws_bytes(1, 4, 8)
    ok = dict(inv=P(64), rays=P(64), imgs=P(64), kind=0, cam_masks=None, T=ctypes.cast(_T, P), cams=ctypes.cast(_EQ, P), mask=None, mpf=0,
              thresh=0.1, n_views=P(64), var=P(64), std=P(64), mean=P(64), ws=P(64), wsb=wsb, table=P(64), B=1, N=1, C=3, Hr=4, Wr=4, H=4, W=8,
              bf=96.0, cam_seen=P(64))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mvsgi_photo_consistency_seen_f32(*[a[k] for k in ok], None)
    for kw, text in [(dict(inv=None), b"null pointer"), (dict(imgs=None), b"null pointer"), (dict(N=9), b"cameras"), (dict(C=4), b"uint8 images"),
                     (dict(mpf=2), b"mask_per_frame"), (dict(thresh=float("nan")), b"NaN"), (dict(var=P(72)), b"16-byte"),
                     (dict(cam_seen=P(66)), b"4-byte"), (dict(mask=P(66)), b"4-byte"), (dict(ws=None), b"the table needs ws"),
                     (dict(cam_seen=None, ws=None), b"the table needs ws")]:
        assert call(**kw) != 0, kw
        err = lib.mvsgi_last_error()
        assert text in err and err.startswith(b"mvsgi_photo_consistency_seen_f32"), (kw, err)


# ------------------------------------------------------------------------------ Python argument errors: nothing touches a device
def test_wrappers_refuse_cpu_tensors():
    inv, rays, T, cams = torch.zeros(1, 4, 4), torch.zeros(3, 4, 4), torch.eye(4)[None], torch.zeros(1, 10)
    with pytest.raises(RuntimeError, match="GPU only"):
        H.camera_range(inv, rays, T, cams, 96.0, (8, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        H.visibility(inv, rays, T, cams, 96.0, torch.zeros(1, 1, 8, 4))


class _Rp:
    """What Visibility and PhotoConsistency read of a Reprojector, without a device."""
    rays, T, cams, bf, out_shape, num_cams = torch.zeros(3, 16, 64), torch.eye(4)[None].repeat(3, 1, 1), torch.zeros(3, 10), 1.0, (16, 64), 3

    def reproject(self, *a, **k):
        raise AssertionError("not reached")


def test_visibility_argument_errors():
    rp = _Rp()
    with pytest.raises(TypeError, match="Reprojector"):
        dropin.Visibility(object())
    with pytest.raises(ValueError, match="zshape"):
        dropin.Visibility(rp, zshape=(0, 4))
    with pytest.raises(ValueError, match="zshape"):
        dropin.Visibility(rp, zshape=7)
    with pytest.raises(ValueError, match="tol"):
        dropin.Visibility(rp, tol=-1.0)
    with pytest.raises(ValueError, match="footprint"):
        dropin.Visibility(rp, footprint=3)
    with pytest.raises(TypeError, match="mask"):
        dropin.Visibility(rp, mask=torch.zeros(16, 64))
    with pytest.raises(AssertionError, match="mask"):
        dropin.Visibility(rp, mask=torch.zeros(16, 32, dtype=torch.bool))
    vis = dropin.Visibility(rp)
    assert vis.zshape == (32, 64) and vis.tol == 0.02 and vis.footprint == 1 and vis.mask is None       # the default buffer: (2 H, W)
    assert dropin.Visibility(rp, zshape=(5, 7), tol=0.0, footprint=2).zshape == (5, 7)
    with pytest.raises(ValueError, match="want"):
        vis.evaluate(torch.zeros(1, 16, 64), want=("visible", "nonsense"))
    with pytest.raises(ValueError, match="want"):
        vis.evaluate(torch.zeros(1, 16, 64), want=())


def test_photo_and_pipeline_refuse_a_visibility_that_does_not_fit():
    """Raised by the constructors' first lines: no weights, constants or device are needed to get there."""
    rp, other = _Rp(), _Rp()
    vis = dropin.Visibility(rp)
    with pytest.raises(ValueError, match="same reprojector"):
        dropin.PhotoConsistency(other, visibility=vis)
    assert dropin.PhotoConsistency(rp, visibility=vis).visibility is vis and dropin.PhotoConsistency(rp).visibility is None
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32))
    with pytest.raises(ValueError, match="visibility: the stage needs reprojector="):
        InferencePipeline(cfg, None, None, visibility=vis)
    with pytest.raises(ValueError, match="visibility: the stage needs reprojector="):
        InferencePipeline(cfg, None, None, reprojector=other, visibility=vis)
    with pytest.raises(ValueError, match="another Visibility"):
        InferencePipeline(cfg, None, None, reprojector=rp, visibility=vis, photo=dropin.PhotoConsistency(rp, visibility=dropin.Visibility(rp)))
    with pytest.raises(ValueError, match="pass it as visibility="):
        InferencePipeline(cfg, None, None, reprojector=rp, photo=dropin.PhotoConsistency(rp, visibility=vis))
