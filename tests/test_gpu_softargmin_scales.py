"""GPU (MI355X): the fused upsample + soft-argmin at any interp_scale_factor (mvsgi_softargmin_scaled_f32) -- the drop-in
regressor against the reference's own outputs at factors 4, 3, 8, 1.5, 2.5, 0.5 (tests/golden/regress_scales.npz), the row-band
kernel against the thread-per-pixel kernel, the whole path at x4 against the CPU oracle, and the argument checks of the entry."""
import ctypes
import dataclasses
import math
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_cases import SMALL_CASES
import guard_arena
from mvs_gi_amd import _lib, dropin, hip_ops as H, synth
from mvs_gi_amd.pipeline import HotPath, InferencePipeline
from oracle import mvsgi_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor the library allocates during a test of this module sits between NaN-sentinel guards, and unwritten
    fp32 outputs read as NaN (tests/guard_arena.py: what is guarded, guard sizes, exemptions)."""
    yield from guard_arena.fixture_body(request)


@pytest.fixture(autouse=True)
def _exact_mode_unless_parametrized():
    """As in tests/test_gpu_parity.py: exact fp32 convolutions unless a test is parametrized over `conv_mode`, and the sticky
    range report starts and ends cleared."""
    old = H.get_conv_mode()
    H.set_conv_mode("f32")
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    H.set_conv_mode(old)
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)


@pytest.fixture(params=["f32", "bf16x3", "f16x3"])
def conv_mode(request):
    old = H.get_conv_mode()
    H.set_conv_mode(request.param)
    yield request.param
    H.set_conv_mode(old)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ulp_report(tag, a, b):
    """How many elements of two fp32 tensors differ, and by how many ulp at most (printed, not asserted)."""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    n = int((a != b).sum())
    ulp = int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if n else 0
    print(f"{tag}: {n} of {a.size} elements differ, max {ulp} ulp")
    return n, ulp


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "regress_scales.npz"))


def _rows(z):
    return [(i, float(s)) for i, s in enumerate(z["factors"])]


# ------------------------------------------------------------------------------ 1, 2: the drop-in against the reference
def test_regressor_at_every_golden_factor(z):
    for i, s in _rows(z):
        costs = _g(z[f"costs_{i}"])
        dr = dropin.DistanceRegressorWithFixedCandidates(bf=float(z["bf"]), dist_cands=list(z[f"dist_cands_{i}"]),
                                                         interp_scale_factor=s, pre_interp=True).to(DEV)
        inv, pr = dr(costs)
        B, _, D, Hh, W = costs.shape
        assert tuple(inv.shape) == (B, 1, math.floor(Hh * s), math.floor(W * s)) and tuple(pr.shape) == (B, D, *inv.shape[2:])
        e_inv = _rel(inv.cpu().numpy(), z[f"inv_{i}"])
        e_pr = _rel(pr.cpu().numpy(), z[f"pr_{i}"]) if f"pr_{i}" in z else 0.0
        print(f"row {i} x{s:g} {tuple(costs.shape)}: inv_dist {e_inv:.2e} norm_costs {e_pr:.2e}")
        assert e_inv <= 1e-5 and e_pr <= 1e-5, (i, s, e_inv, e_pr)
        dr.return_norm_costs = False
        inv2, pr2 = dr(costs)
        assert pr2 is None and torch.equal(inv, inv2), (i, s)


def test_full_resolution_shape():
    dr = dropin.DistanceRegressorWithFixedCandidates(dist_cands=list(np.geomspace(0.5, 100.0, 16)), interp_scale_factor=4,
                                                     pre_interp=True).to(DEV)
    dr.return_norm_costs = False
    inv, pr = dr(torch.randn(2, 1, 16, 80, 320, device=DEV))
    assert tuple(inv.shape) == (2, 1, 320, 1280) and pr is None and bool(torch.isfinite(inv).all())


# ------------------------------------------------------------------------------ 3, 5: row-band kernel vs thread-per-pixel kernel
ROW_PAIR_SHAPES = [(2, 16, 5, 8), (1, 16, 7, 10), (2, 5, 6, 9), (1, 32, 4, 12), (1, 48, 6, 10), (1, 16, 3, 700), (1, 20, 1, 4),
                   (3, 16, 80, 320)]


def _band_vs_pixel(c, inv_idx, s, tag):
    inv_b, pr_b = H.softargmin(c, inv_idx, s, True, variant=H.SA_BAND)
    inv_p, pr_p = H.softargmin(c, inv_idx, s, True, variant=H.SA_PIXEL)
    inv_a, pr_a = H.softargmin(c, inv_idx, s, True)
    assert torch.equal(inv_a, inv_b) and torch.equal(pr_a, pr_b)          # integer factors >= 3 dispatch to the row-band kernel
    only_b, none_b = H.softargmin(c, inv_idx, s, False, variant=H.SA_BAND)
    only_p, none_p = H.softargmin(c, inv_idx, s, False, variant=H.SA_PIXEL)
    assert none_b is None and none_p is None and torch.equal(only_b, inv_b) and torch.equal(only_p, inv_p)
    _ulp_report(f"{tag} x{s} inv_dist band vs pixel", inv_b, inv_p)
    _ulp_report(f"{tag} x{s} norm_costs band vs pixel", pr_b, pr_p)
    assert _rel(inv_b.cpu().numpy(), inv_p.cpu().numpy()) <= 1e-5
    assert _rel(pr_b.cpu().numpy(), pr_p.cpu().numpy()) <= 1e-5
    for variant in (H.SA_BAND, H.SA_PIXEL):
        div, _ = H.softargmin(c, inv_idx, s, False, post_div=96.0, variant=variant)
        ref = (inv_b if variant == H.SA_BAND else inv_p).cpu().numpy()
        assert _rel(div.cpu().numpy() * 96.0, ref) <= 1e-6
    return inv_b, pr_b


@pytest.mark.parametrize("s", [3, 4, 8])
def test_row_band_kernel_equals_pixel_kernel_on_golden_inputs(z, s):
    for i, _ in _rows(z):
        c = _g(z[f"costs_{i}"][:, 0])
        inv_idx = _g((float(z["bf"]) / z[f"dist_cands_{i}"]).astype(np.float32))
        _band_vs_pixel(c, inv_idx, s, f"golden row {i}")


@pytest.mark.parametrize("s", [3, 4, 8])
@pytest.mark.parametrize("shape", ROW_PAIR_SHAPES)
def test_row_band_kernel_equals_pixel_kernel_and_interpolate(shape, s):
    B, D, Hh, W = shape
    rng = np.random.default_rng(sum(shape))
    costs = (rng.standard_normal((B, D, Hh, W)) * 4).astype(np.float32)
    inv_idx = _g((96.0 / np.geomspace(0.5, 100.0, D)).astype(np.float32))
    inv, pr = _band_vs_pixel(_g(costs), inv_idx, s, str(shape))
    up = F.interpolate(torch.from_numpy(costs), scale_factor=s, mode="bilinear")
    ref_pr = F.softmax(up, 1)
    ref_inv = (ref_pr * inv_idx.cpu().view(1, -1, 1, 1)).sum(1, keepdim=True)
    assert _rel(inv.cpu().numpy(), ref_inv.numpy()) <= 1e-5 and _rel(pr.cpu().numpy(), ref_pr.numpy()) <= 1e-5


# ------------------------------------------------------------------------------ 4: factors 1 and 2 through the new symbol
@pytest.mark.parametrize("s", [1, 2])
def test_factors_1_and_2_forward_to_the_existing_launches(s):
    lib = _lib.load()
    rng = np.random.default_rng(11)
    c = _g((rng.standard_normal((2, 16, 6, 12)) * 4).astype(np.float32))
    inv_idx = _g((96.0 / np.geomspace(0.5, 100.0, 16)).astype(np.float32))
    inv_old, pr_old = H.softargmin(c, inv_idx, s, True, post_div=3.0)
    inv = torch.full_like(inv_old, float("nan"))
    pr = torch.full_like(pr_old, float("nan"))
    rc = lib.mvsgi_softargmin_scaled_f32(c.data_ptr(), inv_idx.data_ptr(), inv.data_ptr(), pr.data_ptr(), 2, 16, 6, 12, float(s),
                                         6 * s, 12 * s, 3.0, H.SA_AUTO, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mvsgi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(inv, inv_old) and torch.equal(pr, pr_old)


# ------------------------------------------------------------------------------ 6: pickle
def test_x4_regressor_survives_pickle(z):
    costs = _g(z["costs_1"])
    dr = dropin.DistanceRegressorWithFixedCandidates(bf=96, dist_cands=list(z["dist_cands_1"]), interp_scale_factor=4,
                                                     pre_interp=True).to(DEV)
    inv, pr = dr(costs)
    dr2 = pickle.loads(pickle.dumps(dr))
    assert dr2.interp_scale_factor == 4 and dr2.pre_interp and not any(k.startswith("_mvsgi_") for k in dr2.__dict__)
    inv2, pr2 = dr2(costs)
    assert torch.equal(inv, inv2) and torch.equal(pr, pr2)


# ------------------------------------------------------------------------------ 7: the whole path at x4
def test_hot_path_x4_vs_oracle(conv_mode):
    case = SMALL_CASES["std_d8"]
    cfg = dataclasses.replace(case["cfg"], interp_scale_factor=4)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    w = synth.make_weights(cfg, seed=case["seed"], gain=case["gains"][0])
    t = O.to_torch(inp)
    ref = O.hot_path(t["feats"], t["grids"], t["grid_masks"], t["masks"], O.to_torch(w), cfg.builder, cfg.dist_cands, cfg.bf,
                     cfg.interp_scale_factor, cfg.pre_interp, return_stages=True)
    hp = HotPath(cfg, w, inp, device=DEV)
    feats = _g(inp["feats"])
    inv, pr = hp(feats)
    assert tuple(inv.shape) == (case["batch"], 1, 4 * cfg.cv_hw[0], 4 * cfg.cv_hw[1]) == tuple(ref["inv_dist"].shape)
    err = _rel(inv.cpu().numpy(), ref["inv_dist"].numpy())
    print(f"std_d8 x4 [{conv_mode}]: inv_dist max-rel {err:.3e}")
    assert err <= 1e-3, err                       # the north-star bar
    if conv_mode == "f32":
        assert err <= 2e-4, err                   # the bound test_small_cases_vs_reference_goldens holds the exact path to
    # the regressor alone on the oracle's costs
    inv_r, pr_r = hp.dist_regressor(_g(ref["costs"].numpy()))
    o_inv, o_pr = O.soft_argmin(ref["costs"], cfg.dist_cands, cfg.bf, 4, True)
    assert _rel(inv_r.cpu().numpy(), o_inv.numpy()) <= 1e-5 and _rel(pr_r.cpu().numpy(), o_pr.numpy()) <= 1e-5


def test_inference_pipeline_x4_eager_and_graph():
    """InferencePipeline on a x4 PathConfig: full-resolution output, and the captured hipGraph replays the eager result."""
    H.set_conv_mode("f16x3")
    case = SMALL_CASES["std_d8"]
    cfg = dataclasses.replace(case["cfg"], interp_scale_factor=4)
    seed = case["seed"]
    w = synth.make_weights(cfg, seed=seed)
    w["feature_extractor"] = synth.make_extractor_weights(seed)
    pipe = InferencePipeline(cfg, w, synth.make_inputs(cfg, seed=seed, batch=1), device=DEV)
    Hi, Wi = cfg.feat_hw
    u8 = (np.random.default_rng(seed).random((cfg.num_cams, 4 * Hi, 4 * Wi, 3)) * 255).astype(np.uint8)
    out = pipe({"imgs": [im for im in u8]})
    assert out.shape == (4 * cfg.cv_hw[0], 4 * cfg.cv_hw[1]) and np.isfinite(out).all()
    # inv_dist / bf is a convex combination of 1 / dist over the candidates
    assert out.min() >= 1.0 / max(cfg.dist_cands) - 1e-6 and out.max() <= 1.0 / min(cfg.dist_cands) + 1e-6
    t = torch.from_numpy(u8).to(DEV)
    pipe.capture(t)
    assert np.array_equal(pipe.replay(t).squeeze().cpu().numpy(), out)
    assert np.array_equal(pipe({"imgs": [im for im in u8]}), out)


# ------------------------------------------------------------------------------ 8: rejections (host-side, nothing is launched)
def test_bad_factors_and_sizes_are_rejected_before_any_launch():
    lib = _lib.load()
    B, D, Hh, W = 1, 8, 4, 6
    c = torch.zeros((B, D, Hh, W), device=DEV)
    inv_idx = torch.ones(D, device=DEV)
    inv = torch.full((B, 1, 4 * Hh, 4 * W), -7.0, device=DEV)
    pr = torch.full((B, D, 4 * Hh, 4 * W), -7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(scale, OH, OW, variant=H.SA_AUTO):
        rc = lib.mvsgi_softargmin_scaled_f32(c.data_ptr(), inv_idx.data_ptr(), inv.data_ptr(), pr.data_ptr(), B, D, Hh, W,
                                             scale, OH, OW, 1.0, variant, st)
        return rc, lib.mvsgi_last_error().decode()

    rc, msg = call(float("nan"), 16, 24)
    assert rc != 0 and "nan" in msg.lower(), msg
    rc, msg = call(float("inf"), 16, 24)
    assert rc != 0 and "inf" in msg.lower(), msg
    rc, msg = call(-1.0, 16, 24)
    assert rc != 0 and "-1" in msg, msg
    rc, msg = call(0.0, 16, 24)
    assert rc != 0 and "scale 0" in msg, msg
    rc, msg = call(4.0, 16, 23)                       # the caller allocated another size than floor(in * scale)
    assert rc != 0 and "16 x 23" in msg and "16 x 24" in msg, msg
    rc, msg = call(0.1, 0, 0)                         # floor(4 * 0.1) = 0 rows
    assert rc != 0 and "empty" in msg, msg
    rc, msg = call(2.5, 10, 15, H.SA_BAND)            # the row-band kernel is for integer factors
    assert rc != 0 and "2.5" in msg, msg
    rc, msg = call(4.0, 16, 24, 7)
    assert rc != 0 and "variant 7" in msg, msg
    torch.cuda.synchronize()
    assert bool((inv == -7.0).all()) and bool((pr == -7.0).all())
    with pytest.raises(ValueError):
        H.softargmin(c, inv_idx, float("nan"), False)
    with pytest.raises(ValueError):
        H.softargmin(c, inv_idx, 0.1, False)
    rc, msg = call(4.0, 16, 24)                       # and the same buffers with the right sizes run
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert bool((inv != -7.0).all()) and bool((pr != -7.0).all())
