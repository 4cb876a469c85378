"""CPU: the packed point cloud's definition (tests/cloud_cases.py) against a plain loop, the workspace layout against the library's
own byte count, every argument error of hip_ops.pack_cloud, dropin.CloudPacker and InferencePipeline(cloud=...) before anything
touches a device, the entry point's own validation, and header / binding agreement for the two symbols."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import cloud_cases as CC
from mvs_gi_amd import _lib, dropin, hip_ops as H
from mvs_gi_amd.configs import CONFIGS
from mvs_gi_amd.pipeline import InferencePipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mvsgi_cloud_ws_bytes", "mvsgi_cloud_pack_f32")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("name", list(CC.VARIANTS))
def test_numpy_definition_agrees_with_a_plain_loop(name):
    case = CC.make_case(2, 5, 7, seed=3, **CC.VARIANTS[name])
    bad = [0.0, -0.0, -1.0, np.inf, -np.inf, np.nan]
    case["inv"].reshape(-1)[:len(bad)] = bad                                # row 0 of frame 0
    if case["gates"]:
        case["gates"][0][0][1, 2, 3] = np.nan
    for cap in (None, 3):
        if cap is not None:
            case["capacity"] = cap
        p0, i0, c0 = CC.pack_reference(case)
        p1, i1, c1 = CC.pack_loop(case)
        assert np.array_equal(c0, c1)
        for b in range(case["B"]):
            assert CC.same_bits(p0[b], p1[b]) and np.array_equal(i0[b], i1[b]), b
    keep = CC.keep_reference(case)
    assert not keep[0, 0, :len(bad)].any()                                  # 0, -0, negative, +-inf and NaN are dropped


def test_definition_on_a_hand_made_case():
    rays = np.zeros((3, 1, 4), np.float32)
    rays[2] = 1.0
    case = dict(B=1, H=1, W=4, bf=2.0, step=(1, 1), d_range=CC.D_RANGE, require_colour=False, no_colour=9.0, rays=rays,
                inv=np.array([[[1.0, 0.0, 4.0, 0.5]]], np.float32), mask=None, gates=[], attrs=[],
                warped=np.arange(8, dtype=np.float32).reshape(1, 2, 1, 1, 4), valid=np.array([[[[0, 0, 0, 1]], [[1, 0, 0, 1]]]], bool),
                capacity=4)
    pts, idx, counts = CC.pack_reference(case)
    assert counts.tolist() == [[3, 3]] and idx[0].tolist() == [0, 2, 3]
    # z = bf / inv; colour: camera 1 at p = 0, none at p = 2, camera 0 (the lowest) at p = 3
    assert pts[0].tolist() == [[0, 0, 2.0, 4.0], [0, 0, 0.5, 9.0], [0, 0, 4.0, 3.0]]
    case["require_colour"] = True
    assert CC.pack_reference(case)[1][0].tolist() == [0, 3]


def _bernoulli_cases():
    for B, Hh, W in CC.SHAPES:
        for name in CC.BERNOULLI:
            yield (B, Hh, W), name


@pytest.mark.parametrize("shape,name", list(_bernoulli_cases()))
def test_bernoulli_patterns_keep_some_and_drop_some(shape, name):
    """The seeds of the GPU test: 0 < kept < H * W in every frame."""
    k = CC.keep_pattern(name, *shape).reshape(shape[0], -1)
    assert ((k.sum(axis=1) > 0) & (k.sum(axis=1) < k.shape[1])).all()


@pytest.mark.parametrize("shape", CC.SHAPES)
def test_structured_patterns(shape):
    B, Hh, W = shape
    HW = Hh * W
    for name in CC.PATTERNS:
        if not CC.pattern_exists(name, *shape):
            continue
        k = CC.keep_pattern(name, *shape).reshape(B, HW)
        if name.startswith("one@"):
            assert (k.sum(axis=1) == 1).all()
        if name in ("empty_words", "empty_tiles"):
            unit = 64 if name == "empty_words" else CC.TILE
            per = np.add.reduceat(k[0], np.arange(0, HW, unit))
            assert (per == 0).any() and (per > 0).any() and k[0].sum() > 0
    assert CC.keep_pattern("all", *shape).all() and not CC.keep_pattern("none", *shape).any()


@pytest.mark.parametrize("shape", CC.VARIANT_SHAPES)
@pytest.mark.parametrize("name", list(CC.VARIANTS))
def test_variant_cases_keep_some_and_drop_some(name, shape):
    case = CC.make_case(*shape, **CC.VARIANTS[name])
    kept = CC.keep_reference(case).reshape(shape[0], -1).sum(axis=1)
    lattice = case["capacity"]
    assert (kept > 0).all()
    if name != "plain_bf1":
        assert (kept < lattice).all()
    if case["warped"] is not None:
        none_valid = ~case["valid"].any(axis=1)
        assert none_valid.any() and not none_valid.all()


# ------------------------------------------------------------------------------ the workspace
@pytest.mark.parametrize("B,Hh,W", CC.SHAPES + [(128, 160, 640), (16387, 64, 256), (65535, 1, 1)])
def test_workspace_layout_is_the_librarys_byte_count(lib, B, Hh, W):
    lay = H.cloud_ws_layout(B, Hh, W)
    assert lay["total"] == lib.mvsgi_cloud_ws_bytes(B, Hh, W)
    assert lay["tiles"] == -(-Hh * W // CC.TILE) and lay["words_per_frame"] * 64 >= Hh * W > (lay["words_per_frame"] - 16) * 64
    # three parts in order, each a multiple of 16 bytes and large enough for what it holds
    assert 0 == lay["words"] < lay["tile_counts"] < lay["tile_offsets"] < lay["total"]
    assert all(lay[k] % 16 == 0 for k in ("words", "tile_counts", "tile_offsets", "total"))
    assert lay["tile_counts"] - lay["words"] >= B * lay["words_per_frame"] * 8
    assert lay["tile_offsets"] - lay["tile_counts"] >= B * lay["tiles"] * 4 <= lay["total"] - lay["tile_offsets"]


def test_workspace_sizes_are_monotone_and_refuse_bad_shapes(lib):
    shapes = [(1, 1, 1), (1, 32, 32), (1, 32, 33), (2, 32, 33), (2, 64, 64), (3, 160, 640)]
    sizes = [H.cloud_ws_layout(*s)["total"] for s in shapes]
    units = [s[0] * H.cloud_ws_layout(*s)["tiles"] for s in shapes]          # tiles in all: the size grows exactly when they do
    assert units == [1, 1, 2, 4, 8, 300]
    assert all((a < b) == (ua < ub) and a <= b for a, b, ua, ub in zip(sizes, sizes[1:], units, units[1:]))
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (65536, 4, 4), (1, 1 << 16, 1 << 15)]:
        assert lib.mvsgi_cloud_ws_bytes(*bad) == 0
        with pytest.raises(ValueError):
            H.cloud_ws_layout(*bad)
    assert H.cloud_capacity(33, 65) == 33 * 65 and H.cloud_capacity(33, 65, (2, 3)) == 17 * 22
    assert H.CLOUD_D_RANGE == CC.D_RANGE


# ------------------------------------------------------------------------------ symbols
def test_header_declares_and_binding_lists_the_symbols(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsgi.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/mvsgi.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define MVSGI_ABI_VERSION 8" in src and _lib.ABI_VERSION == 8
    res, args = _lib.SIGNATURES["mvsgi_cloud_pack_f32"]
    decl = re.search(r"int mvsgi_cloud_pack_f32\((.*?)\);", src, flags=re.S).group(1)
    assert len(args) == len(decl.split(",")) == 31 and res is ctypes.c_int
    assert _lib.SIGNATURES["mvsgi_cloud_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int])
    assert "cloud.hip" in __import__("__graft_entry__").SOURCES
    assert __import__("__graft_entry__").EXTRA_FLAGS["cloud.hip"] == ["-ffp-contract=off"]


def test_entry_point_validates_before_launching(lib):
    P = ctypes.c_void_p
    tab = (P * 4)(64, 64, 64, 64)
    many = (P * 16)(*[64] * 16)
    f4 = (ctypes.c_float * 4)(0, 0, 0, 0)
    ok = dict(inv=P(64), rays=P(64), mask=None, mpf=0, gates=tab, lo=f4, hi=f4, ng=0, warped=None, valid=None, N=0, C=0, rc=0, nc=0.0,
              attrs=many, A=0, points=P(64), counts=P(64), index=None, cap=16, ws=P(256), wsb=1 << 20, B=1, H=4, W=4, sy=1, sx=1, bf=1.0,
              dmin=0.0, dmax=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mvsgi_cloud_pack_f32(*[a[k] for k in ok], None)
    for kw, text in [(dict(inv=None), b"null pointer"), (dict(points=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                     (dict(B=0), b"non-positive"), (dict(B=65536), b"too large"), (dict(H=1 << 16, W=1 << 15), b"too large"),
                     (dict(sy=0), b"step"), (dict(cap=0), b"capacity"), (dict(cap=1 << 31), b"capacity"),
                     (dict(ng=5), b"gates"), (dict(ng=1, gates=None), b"null pointer"), (dict(ng=1, gates=(P * 1)(None)), b"gate 0"),
                     (dict(warped=P(64)), b"together"), (dict(valid=P(64)), b"together"),
                     (dict(warped=P(64), valid=P(64), N=9, C=3), b"cameras"), (dict(warped=P(64), valid=P(64), N=3, C=5), b"channels"),
                     (dict(warped=P(64), valid=P(64), N=3, C=0), b"channels"), (dict(rc=1), b"require_colour"),
                     (dict(A=14), b"record"), (dict(warped=P(64), valid=P(64), N=3, C=4, A=10), b"record"), (dict(A=2, attrs=None), b"attribute"),
                     (dict(A=1, attrs=(P * 1)(None)), b"attribute 0"),
                     (dict(wsb=lib.mvsgi_cloud_ws_bytes(1, 4, 4) - 1), b"workspace"), (dict(ws=P(8)), b"16-byte"), (dict(inv=P(66)), b"4-byte")]:
        assert call(**kw) != 0, kw
        assert text in lib.mvsgi_last_error(), (kw, lib.mvsgi_last_error())


# ------------------------------------------------------------------------------ Python argument errors: nothing touches a device
def _meta(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def test_pack_cloud_refuses_cpu_tensors():
    inv, rays = _meta((1, 4, 4)), _meta((3, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        H.pack_cloud(inv, rays, 1.0, d_range=H.CLOUD_D_RANGE)
    with pytest.raises(TypeError):
        H.pack_cloud(np.zeros((1, 4, 4), np.float32), rays, 1.0, d_range=H.CLOUD_D_RANGE)


class _Dev(torch.Tensor):
    """A CPU tensor that says it is on the device: pack_cloud's checks run up to the launch without one."""
    @staticmethod
    def make(shape, dtype=torch.float32, contiguous=True):
        t = torch.zeros(shape, dtype=dtype)
        if not contiguous:
            t = torch.zeros(tuple(shape) + (2,), dtype=dtype)[..., 0]
        return t.as_subclass(_Dev)

    @property
    def is_cuda(self):
        return True


def test_pack_cloud_argument_errors(monkeypatch):
    called = []
    monkeypatch.setattr(H, "_call", lambda *a: called.append(a))
    monkeypatch.setattr(H, "sweep_max_cams", lambda: 8)
    B, Hh, W = 2, 4, 6
    inv, rays = _Dev.make((B, Hh, W)), _Dev.make((3, Hh, W))
    g = _Dev.make((B, Hh, W))
    ok = dict(d_range=H.CLOUD_D_RANGE)
    bad = [
        (dict(inv=_Dev.make((B, 2, Hh, W))), AssertionError, "inv must be"),
        (dict(inv=_Dev.make((B, Hh, W), torch.float64)), TypeError, "inv"),
        (dict(inv=_Dev.make((B, Hh, W), contiguous=False)), AssertionError, "contiguous"),
        (dict(rays=_Dev.make((3, Hh, W + 1))), AssertionError, "rays"),
        (dict(rays=torch.zeros(3, Hh, W)), RuntimeError, "GPU only"),
        (dict(step=(0, 1)), ValueError, "step"),
        (dict(gates=[(g, 0, 1)] * 5), ValueError, "gates"),
        (dict(gates=[(_Dev.make((B, Hh, W + 1)), 0, 1)]), AssertionError, r"gates\[0\]"),
        (dict(gates=[(_Dev.make((B, Hh, W), torch.int32), 0, 1)]), TypeError, r"gates\[0\]"),
        (dict(mask=_Dev.make((Hh, W))), TypeError, "mask"),
        (dict(mask=_Dev.make((B, 1, Hh, W), torch.bool)), AssertionError, "mask"),
        (dict(warped=_Dev.make((B, 3, 3, Hh, W))), ValueError, "together"),
        (dict(valid=_Dev.make((B, 3, Hh, W), torch.bool)), ValueError, "together"),
        (dict(warped=_Dev.make((B, 3, 3, Hh, W)), valid=_Dev.make((B, 2, Hh, W), torch.bool)), AssertionError, "valid"),
        (dict(warped=_Dev.make((B, 3, 3, Hh, W)), valid=_Dev.make((B, 3, Hh, W))), TypeError, "valid"),
        (dict(warped=_Dev.make((B, 9, 3, Hh, W)), valid=_Dev.make((B, 9, Hh, W), torch.bool)), ValueError, "cameras"),
        (dict(warped=_Dev.make((B, 3, 5, Hh, W)), valid=_Dev.make((B, 3, Hh, W), torch.bool)), ValueError, "channels"),
        (dict(warped=_Dev.make((B, 3, Hh, W))), ValueError, "together"),
        (dict(require_colour=True), ValueError, "require_colour"),
        (dict(attrs=[g] * 14), ValueError, "record"),
        (dict(attrs=[g] * 10, warped=_Dev.make((B, 3, 4, Hh, W)), valid=_Dev.make((B, 3, Hh, W), torch.bool)), ValueError, "record"),
        (dict(attrs=[_Dev.make((B, Hh))]), AssertionError, r"attrs\[0\]"),
        (dict(capacity=0), ValueError, "capacity"),
        (dict(out=dict(points=_Dev.make((B, Hh * W, 4)))), AssertionError, "points"),
        (dict(out=dict(counts=_Dev.make((B, 2)))), TypeError, "counts"),
        (dict(want_index=True, out=dict(index=_Dev.make((B, Hh * W), torch.int64))), TypeError, "index"),
        (dict(ws=torch.zeros(4)), AssertionError, "ws"),
    ]
    for kw, exc, text in bad:
        a = dict(ok, inv=inv, rays=rays)
        a.update(kw)
        i, r = a.pop("inv"), a.pop("rays")
        with pytest.raises(exc, match=text):
            H.pack_cloud(i, r, 1.0, **a)
    assert not called                                                       # nothing was launched
    with pytest.raises(TypeError):
        H.pack_cloud(inv, rays, 1.0)                                        # d_range is required


def test_cloud_packer_argument_errors():
    rays = torch.zeros(3, 4, 6)
    inf = math.inf
    ok = dropin.CloudPacker(rays, 1.0, gates={"max_prob": (0.5, inf), "spread": (-inf, 2.0)}, attrs=("max_prob",), step=(2, 3))
    assert ok.maps == ("max_prob", "spread") and ok.out_shape == (4, 6) and ok.capacity == 2 * 2 and ok.colour
    assert ok.d_range == H.CLOUD_D_RANGE and ok.record_width(3) == 7
    assert dropin.CloudPacker(rays, 1.0, colour=False, attrs="entropy").record_width() == 4

    class Rp:
        out_shape, bf = (4, 6), 1.0
    Rp.rays = rays
    assert dropin.CloudPacker(Rp()).bf == 1.0
    for args, kw, exc, text in [
            ((rays,), {}, ValueError, "needs bf"),
            ((Rp(), 96.0), {}, ValueError, "bf"),
            (("rays", 1.0), {}, TypeError, "Reprojector or a ray table"),
            ((torch.zeros(4, 6), 1.0), {}, AssertionError, "rays"),
            ((rays.double(), 1.0), {}, AssertionError, "rays"),
            ((rays, 1.0), dict(gates={"argmax": (0, 1)}), ValueError, "argmax"),
            ((rays, 1.0), dict(attrs=("argmax",)), ValueError, "argmax"),
            ((rays, 1.0), dict(attrs=("sharpness",)), ValueError, "unknown confidence map"),
            ((rays, 1.0), dict(attrs=("spread", "spread")), ValueError, "repeats"),
            ((rays, 1.0), dict(gates={"spread": (math.nan, 1)}), ValueError, "NaN"),
            ((rays, 1.0), dict(step=(1, 0)), ValueError, "step"),
            ((rays, 1.0), dict(capacity=0), ValueError, "capacity"),
            ((rays, 1.0), dict(colour=False, require_colour=True), ValueError, "require_colour"),
            ((rays, 1.0), dict(mask=torch.zeros(4, 6)), TypeError, "mask"),
            ((rays, 1.0), dict(mask=torch.zeros(4, 7, dtype=torch.bool)), AssertionError, "mask")]:
        with pytest.raises(exc, match=text):
            dropin.CloudPacker(*args, **kw)
    # pack(): what is missing or misshapen is refused before any buffer is made
    inv = torch.ones(1, 1, 4, 6)
    conf = dict(max_prob=torch.ones(1, 1, 4, 6), spread=torch.ones(1, 1, 4, 6))
    warped, valid = torch.zeros(1, 3, 3, 4, 6), torch.ones(1, 3, 4, 6, dtype=torch.bool)
    for a, kw, exc, text in [
            ((torch.ones(1, 4, 7),), {}, AssertionError, "inv must be"),
            ((inv,), dict(confidence=conf), ValueError, "warped and valid"),
            ((inv,), dict(confidence=dict(max_prob=conf["max_prob"]), warped=warped, valid=valid), ValueError, "'spread'"),
            ((inv,), dict(confidence=dict(conf, spread=torch.ones(1, 1, 4, 7)), warped=warped, valid=valid), AssertionError, "spread"),
            ((inv,), dict(confidence=dict(conf, spread=torch.ones(1, 1, 4, 6, dtype=torch.int32)), warped=warped, valid=valid), TypeError, "spread"),
            ((inv,), dict(confidence=conf, warped=torch.zeros(1, 3, 4, 6), valid=valid), AssertionError, "warped"),
            ((inv,), dict(confidence=conf, warped=warped, valid=valid), RuntimeError, "GPU only")]:
        with pytest.raises(exc, match=text):
            ok.pack(*a, **kw)
    assert ok._bufs == {}
    with pytest.raises(ValueError, match="colour=False"):
        dropin.CloudPacker(rays, 1.0, colour=False).pack(inv, warped=warped, valid=valid)


def test_pipeline_refuses_a_packer_that_does_not_fit():
    """Raised by the constructor's first lines: no weights, constants or device are needed to get there."""
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32))
    rays = torch.zeros(3, 16, 64)
    rp = object()
    with pytest.raises(ValueError, match="no reprojector"):
        InferencePipeline(cfg, None, None, cloud=dropin.CloudPacker(rays, 1.0))
    with pytest.raises(ValueError, match="confidence= selects"):
        InferencePipeline(cfg, None, None, reprojector=rp, cloud=dropin.CloudPacker(rays, 1.0, gates={"max_prob": (0.5, 1.0)}))
    with pytest.raises(ValueError, match=r"\['spread'\]"):
        InferencePipeline(cfg, None, None, reprojector=rp, confidence=("max_prob",),
                          cloud=dropin.CloudPacker(rays, 1.0, gates={"max_prob": (0.5, 1.0)}, attrs=("spread",)))
    with pytest.raises(ValueError, match="out_shape"):
        InferencePipeline(cfg, None, None, confidence=("max_prob",),
                          cloud=dropin.CloudPacker(torch.zeros(3, 16, 32), 1.0, colour=False, attrs=("max_prob",)))
