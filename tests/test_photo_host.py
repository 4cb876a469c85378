"""CPU: the photometric consistency's definition (tests/photo_cases.py) -- the conditions its cases exist for, the restatement against
the reference's own SphericalSweepStdMasked.sweep (tests/golden/photo.npz, tools/make_photo_goldens.py), the table's restatement, the
workspace layout against the library's byte count, the entry point's own validation, header / binding agreement for the two symbols,
and every argument error of CloudPacker("photo_std") and InferencePipeline(photo=...) that is raised before anything touches a device."""
import ctypes
import hashlib
import math
import os
import re

import numpy as np
import pytest
import torch

import photo_cases as PC
from mvs_gi_amd import _lib, dropin, hip_ops as H
from mvs_gi_amd.configs import CONFIGS
from mvs_gi_amd.pipeline import InferencePipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvsgi_photo_ws_bytes", "mvsgi_photo_consistency_f32")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def built():
    return {name: PC.build(name) for name in PC.CASES}          # the builder asserts the conditions of every case


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "photo.npz"))


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------ the cases
def test_cases_meet_their_conditions(built):
    """Conditions, not measurements: the reused cases have the views and scored pixels the issue lists; every multi-camera case built
    here has pixels with 0, with exactly 1 and with at least 2 views; the camera-mask case has pixels where the mask alone removes a
    camera; the pixel-mask cases mask scored and unscored pixels.  (PC.build asserts them; here they are shown.)"""
    for name, c in built.items():
        print(f"[photo] {name}: views histogram {c['hist'].tolist()}, scored {int(c['table'][-1, 0])} of {c['restated']['n_views'].numel()}")
    assert built["tail_u8"]["hist"].tolist()[:4] == [0, 6, 34, 80] and built["tail_u8"]["table"][-1, 0] == 114
    assert built["eight_u8"]["table"][-1, 0] == 14 and built["eq_f32c3"]["table"][-1, 0] == 128
    t = built["vec_f32c1"]["table"]
    assert (t[:, 0] == 0).all() and np.isnan(t[:, 1:4]).all() and (t[:, 4] == 0).all() and t[-1, 5:7].tolist() == [20, 108]


@pytest.mark.parametrize("name", list(PC.LARGE))
def test_device_cases_meet_their_conditions(name):
    """The cases the GPU tests add for the launch's geometry: the same conditions (PC.build asserts them), and the geometry itself."""
    c = PC.build(name)
    s = PC.spec(name)
    print(f"[photo] {name}: views histogram {c['hist'].tolist()}, scored {int(c['table'][-1, 0])} of {c['restated']['n_views'].numel()}")
    quads = s["hw"][0] * -(-s["hw"][1] // 4)
    G = H.photo_ws_layout(s["B"], *s["hw"])["G"]
    if name == "waves_f32":
        assert G == 5 and quads >= 4 * 256 and s["B"] == 3
    elif name == "stride_u8":
        assert G == 256 and quads > 256 * 256
    else:
        assert s["N"] > 4 and s["hw"][1] % 4 == 0


def test_values_nobody_should_pass_do_what_the_chain_does(built):
    """No special case: inv = 0 (d = inf) and NaN give coordinates no camera accepts, so cnt = 0, photo_var = 0 and a zero mean
    colour.  inv = -1 (a point behind the rig camera) and inv = inf (d = 0: the rig camera's own centre) are finite points that
    other cameras of the ring may well see: there the chain's arithmetic stands, whatever it gives, and stays finite."""
    c = built["bad_inv"]
    inv = c["inp"]["inv"]
    assert all(int(m.sum()) >= 4 for m in (inv == 0, inv == -1, torch.isnan(inv), torch.isinf(inv)))
    none = (inv == 0) | torch.isnan(inv)
    r = c["restated"]
    assert not bool(c["chain"]["valid"].movedim(1, -1)[none].any())
    assert bool((r["n_views"][none] == 0).all()) and bool((r["photo_var"][none] == 0).all()) and bool((r["mean_colour"].movedim(1, -1)[none] == 0).all())
    assert bool(c["chain"]["valid"].movedim(1, -1)[(inv == -1) | torch.isinf(inv)].any())
    assert bool(torch.isfinite(r["photo_var"]).all()) and bool(torch.isfinite(r["mean_colour"]).all())


# ------------------------------------------------------------------------------ against the reference's own class
@pytest.mark.parametrize("name", PC.CASES)
def test_restatement_against_the_references_class(built, z, name):
    """var_c of the restatement against SphericalSweepStdMasked.sweep on the same samples.  Bar: the rule of the metrics golden,
    4 * |restate(fp32) - restate(float64)| + 4 fp32 ulp, per element."""
    c = built[name]
    h = hashlib.sha256()
    for k in ("inv", "imgs", "cam_masks", "mask"):
        if c["inp"][k] is not None:
            h.update(c["inp"][k].numpy().tobytes())
    assert h.hexdigest() == str(z[f"{name}/sha256"]), "the golden was made from other inputs"
    gold = z[f"{name}/var_c"].astype(np.float64)
    r32 = c["restated"]["var_c"].numpy().astype(np.float64)
    r64 = PC.restate(c["chain"]["warped"], c["chain"]["seen"], torch.float64)["var_c"].numpy()
    assert gold.shape == r32.shape and np.isfinite(gold).all()
    dist = np.abs(gold - r32)
    bar = 4 * np.abs(r32 - r64) + 4 * _ulp32(gold)
    print(f"[photo] {name}: max |reference - restatement| = {dist.max():.3e} ({int((dist > 0).sum())} of {dist.size} elements differ); "
          f"smallest bar where they do {bar[dist > 0].min() if (dist > 0).any() else float('nan'):.3e}")
    assert (dist <= bar).all()
    if PC.spec(name)["N"] <= 4:
        assert dist.max() == 0.0           # up to four cameras torch.sum adds in index order: the reference's bits


# ------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name", PC.CASES)
def test_table_restatement(built, name):
    c = built[name]
    r, t = c["restated"], c["table"]
    std, var, cnt = r["photo_std"].numpy(), r["photo_var"].numpy(), r["n_views"].numpy()
    B = std.shape[0]
    assert t.shape == (B + 1, len(PC.COLUMNS)) == (B + 1, 14) and tuple(H.PHOTO_COLUMNS) == PC.COLUMNS
    mask = c["inp"]["mask"]
    masked = np.ones(cnt.shape, bool) if mask is None else np.broadcast_to(mask.numpy() != 0, cnt.shape)
    assert np.array_equal(std, PC.exact_std(var))
    for b in range(B):
        s = masked[b] & (cnt[b] > 1)
        n = int(s.sum())
        assert t[b, 0] == n and t[b, 5:].sum() == masked[b].sum()
        assert [int(v) for v in t[b, 5:]] == [int(((cnt[b] == k) & masked[b]).sum()) for k in range(9)]
        if n:
            # a plain float64 sum of at most a few hundred fp32 addends is within n ulp of the exactly rounded one
            assert abs(t[b, 1] - std[b][s].astype(np.float64).sum() / n) <= n * np.spacing(t[b, 1])
            assert abs(t[b, 2] ** 2 - var[b][s].astype(np.float64).sum() / n) <= (n + 2) * np.spacing(t[b, 2] ** 2)
            assert t[b, 3] == float((std[b][s] > np.float32(PC.THRESH)).sum()) / n
            assert t[b, 4] == n / masked[b].sum()
        else:
            assert np.isnan(t[b, 1:4]).all()
    # the pooled row: counts add up; its sums are those of all frames' addends, rounded once
    assert t[B, 0] == t[:B, 0].sum() and np.array_equal(t[B, 5:], t[:B, 5:].sum(axis=0))
    if t[B, 0]:
        s = masked & (cnt > 1)
        assert t[B, 1] == math.fsum(float(x) for x in std[s]) / t[B, 0]


# ------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("B,Hh,W", [(1, 1, 1), (1, 6, 10), (2, 7, 13), (3, 160, 640), (1, 512, 2048), (128, 160, 640)])
def test_workspace_layout_is_the_librarys_byte_count(lib, B, Hh, W):
    lay = H.photo_ws_layout(B, Hh, W)
    assert lay["total"] * 8 == lib.mvsgi_photo_ws_bytes(B, Hh, W)
    assert lay["G"] == H.photo_ws_layout(1, Hh, W)["G"] and 1 <= lay["G"] <= 256            # G is a function of (H, W) alone
    assert lay["records"] == 0 and lay["frame_sums"] == B * lay["G"] * 16 and lay["total"] == lay["frame_sums"] + B * 16


def test_workspace_refuses_bad_shapes(lib):
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (65535, 4, 4), (1, 1 << 16, 1 << 15)]:
        assert lib.mvsgi_photo_ws_bytes(*bad) == 0


def test_header_declares_and_binding_lists_the_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsgi.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/mvsgi.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["mvsgi_photo_consistency_f32"][1]) == 26
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in text for name in SYMBOLS)


def test_entry_point_validates_before_launching(lib):
    P = ctypes.c_void_p
    T = (ctypes.c_float * 16)(*[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
    cams = (ctypes.c_float * 10)(1, *[0] * 9)
    wsb = lib.mvsgi_photo_ws_bytes(1, 4, 8)
    ok = dict(inv=P(64), rays=P(64), imgs=P(64), kind=0, cam_masks=None, T=ctypes.cast(T, P), cams=ctypes.cast(cams, P), mask=None, mpf=0,
              thresh=0.1, n_views=P(64), var=P(64), std=P(64), mean=P(64), ws=P(64), wsb=wsb, table=P(64), B=1, N=1, C=3, Hr=4, Wr=4, H=4, W=8,
              bf=96.0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mvsgi_photo_consistency_f32(*[a[k] for k in ok], None)
    bad_cam = (ctypes.c_float * 10)(2, *[0] * 9)
    ds_cam = (ctypes.c_float * 10)(0, -0.2, 0.6, 200, 200, 600, 500, 0.5, 0, 1223)
    for kw, text in [(dict(inv=None), b"null pointer"), (dict(rays=None), b"null pointer"), (dict(imgs=None), b"null pointer"),
                     (dict(T=None), b"null pointer"), (dict(cams=None), b"null pointer"),
                     (dict(n_views=None, var=None, std=None, mean=None, table=None), b"every output is NULL"),
                     (dict(N=0), b"cameras"), (dict(N=9), b"cameras"), (dict(B=0), b"non-positive"), (dict(H=0), b"non-positive"),
                     (dict(kind=2), b"image kind"), (dict(C=0), b"channels"), (dict(C=4), b"uint8 images have C = 3"),
                     (dict(Hr=0), b"non-positive"), (dict(Wr=1 << 23), b"row bytes"), (dict(kind=1, cam_masks=P(64), Wr=1 << 21), b"row bytes"),
                     (dict(B=65535), b"too large"), (dict(H=1 << 16, W=1 << 15), b"too large"), (dict(mpf=2), b"mask_per_frame"),
                     (dict(thresh=float("nan")), b"NaN"), (dict(cams=ctypes.cast(bad_cam, P)), b"unknown model id"),
                     (dict(cams=ctypes.cast(ds_cam, P)), b"calib shape"), (dict(var=P(72)), b"16-byte"), (dict(n_views=P(68)), b"16-byte"),
                     (dict(inv=P(68)), b"16-byte aligned when W"), (dict(mask=P(66)), b"4-byte"), (dict(kind=1, imgs=P(66)), b"4-byte"),
                     (dict(ws=None), b"the table needs ws"), (dict(wsb=wsb - 1), b"workspace"), (dict(ws=P(68)), b"8-byte"),
                     (dict(table=P(68)), b"8-byte")]:
        assert call(**kw) != 0, kw
        assert text in lib.mvsgi_last_error(), (kw, lib.mvsgi_last_error())


# ------------------------------------------------------------------------------ Python argument errors: nothing touches a device
def test_photo_consistency_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU only"):
        H.photo_consistency(torch.zeros(1, 4, 4), torch.zeros(3, 4, 4), torch.eye(4)[None], torch.zeros(1, 10), 96.0, torch.zeros(1, 3, 4, 4))


class _Rp:
    """What PhotoConsistency reads of a Reprojector, without a device."""
    rays, T, cams, bf, out_shape, num_cams = torch.zeros(3, 16, 64), torch.eye(4)[None].repeat(3, 1, 1), torch.zeros(3, 10), 1.0, (16, 64), 3

    def reproject(self, *a, **k):
        raise AssertionError("not reached")


def test_photo_consistency_argument_errors():
    rp = _Rp()
    with pytest.raises(TypeError, match="Reprojector"):
        dropin.PhotoConsistency(object())
    with pytest.raises(TypeError, match="fp32"):
        dropin.PhotoConsistency(rp, cam_masks=torch.zeros(3, 1, 4, 4, dtype=torch.uint8))
    with pytest.raises(AssertionError, match="cam_masks"):
        dropin.PhotoConsistency(rp, cam_masks=torch.zeros(2, 1, 4, 4))
    with pytest.raises(TypeError, match="mask"):
        dropin.PhotoConsistency(rp, mask=torch.zeros(16, 64))
    with pytest.raises(AssertionError, match="mask"):
        dropin.PhotoConsistency(rp, mask=torch.zeros(16, 32, dtype=torch.bool))
    with pytest.raises(ValueError, match="NaN"):
        dropin.PhotoConsistency(rp, thresh=float("nan"))
    pc = dropin.PhotoConsistency(rp, cam_masks=torch.ones(1, 3, 1, 4, 4), mask=torch.ones(16, 64, dtype=torch.bool), thresh=0.25)
    assert tuple(pc.cam_masks.shape) == (3, 1, 4, 4) and pc.thresh == 0.25 and pc.out_shape == (16, 64)


def test_cloud_packer_takes_photo_std_as_a_gate_and_an_attribute():
    rays = torch.zeros(3, 4, 6)
    p = dropin.CloudPacker(rays, 1.0, gates={"max_prob": (0.5, math.inf), "photo_std": (0.0, 0.2)}, attrs=("photo_std", "spread"), colour=False)
    assert p.maps == ("max_prob", "spread") and p.photo_maps == ("photo_std",)
    assert dropin.CloudPacker(rays, 1.0, attrs=("max_prob",)).photo_maps == ()
    with pytest.raises(ValueError, match="unknown confidence map"):
        dropin.CloudPacker(rays, 1.0, gates={"photo_var": (0.0, 1.0)})
    inv = torch.zeros(1, 4, 6)
    conf = dict(max_prob=torch.zeros(1, 1, 4, 6), spread=torch.zeros(1, 1, 4, 6))
    with pytest.raises(ValueError, match="photo="):
        p.pack(inv, confidence=conf)
    with pytest.raises(ValueError, match="photo="):
        p.pack(inv, confidence=dict(conf, photo_std=torch.zeros(1, 4, 6)))          # not through the confidence maps
    with pytest.raises(AssertionError, match="photo_std"):
        p.pack(inv, confidence=conf, photo=dict(photo_std=torch.zeros(1, 4, 5)))


def test_pipeline_refuses_a_photo_stage_that_does_not_fit():
    """Raised by the constructor's first lines: no weights, constants or device are needed to get there."""
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32))
    rays = torch.zeros(3, 16, 64)
    rp = _Rp()
    gated = dropin.CloudPacker(rays, 1.0, gates={"photo_std": (0.0, 0.2)}, colour=False)
    with pytest.raises(ValueError, match="need a photo= stage"):
        InferencePipeline(cfg, None, None, reprojector=rp, cloud=gated)
    with pytest.raises(ValueError, match="needs reprojector="):
        InferencePipeline(cfg, None, None, photo=dropin.PhotoConsistency(rp))
    with pytest.raises(ValueError, match="needs reprojector="):
        InferencePipeline(cfg, None, None, reprojector=_Rp(), photo=dropin.PhotoConsistency(rp))
