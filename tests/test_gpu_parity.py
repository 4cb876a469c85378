"""GPU (MI355X) parity tests: the HIP path, called through the C ABI, against the golden
vectors of the reference (tests/golden) and against the CPU oracle on the same seeded
inputs.  Tolerances are written per assertion:
  * sweep: bit-exact (the kernel follows the reference op by op, contraction off);
  * single conv block / resize: 2e-5 relative to the tensor's max (fp32, different
    summation order than oneDNN);
  * whole path: inv_dist within 1e-3 relative (BASELINE.json north_star), costs 1e-4.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_cases import FULL_CASES, SMALL_CASES
import guard_arena
from mvs_gi_amd import dropin, hip_ops as H, synth
from mvs_gi_amd.pipeline import HotPath, build_modules
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
    """Tests that are not parametrized over `conv_mode` hold the exact-fp32 tolerances; the library default
    (f16x3) is checked by tests/test_dropin_host.py::test_default_conv_mode_is_the_fp16_split and the `conv_mode` cases.  The fp16 split's sticky range report
    (hip_ops.saturation_flags) starts every test cleared: the tests that saturate on purpose must not fail the next HotPath call."""
    old = H.get_conv_mode()
    H.set_conv_mode("f32")
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    H.set_conv_mode(old)
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _pix(a, b):
    """max over pixels of |a - b| / |b|: the per-pixel relative error of an inverse-distance map (inv_dist >= 0.96 by construction --
    a convex combination of bf / dist candidates -- so the division is well defined).  _rel() divides by the MAP's maximum (192):
    1e-3 of that is 0.19 absolute = 20 % of a far pixel; this is the figure a depth consumer sees (distance = bf / inv_dist)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-30)).max())


def _ncdhw(y_ndhwc):
    return y_ndhwc.permute(0, 4, 1, 2, 3).contiguous().cpu().numpy()


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------ K1 sweep
def test_sweep_edges_bit_exact(golden_dir):
    z = _load(golden_dir, "sweep_edges")
    f, g, m = _g(z["feats"]), _g(z["grids"]), _g(z["masks"])
    gm = _g(z["grid_masks_bool"])
    for gmask in (gm, gm.float(), gm.to(torch.uint8)):
        v = _ncdhw(H.sweep_std(f, g, gmask, m))          # C = 5: plane-gather (NCHW) kernel
        assert np.array_equal(v, z["vol_raw_std_bool"])
    assert np.array_equal(_ncdhw(H.sweep_cat(f, g)), z["vol_raw_cat"])
    # channels-last kernels on the same edge cases: pad C 5 -> 8 with zero planes
    f8 = torch.cat([f, torch.zeros_like(f[:, :, :3])], dim=2).contiguous()
    for gmask in (gm, gm.float()):
        v8 = _ncdhw(H.sweep_std(f8, g, gmask, m))
        assert np.array_equal(v8[:, :5], z["vol_raw_std_bool"]) and not v8[:, 5:].any()
        # rig-constant validity byte + the candidate-walking kernel: same bits
        v8c = _ncdhw(H.sweep_std_valid(f8, g, H.sweep_validity(g, gmask, m)))
        assert np.array_equal(v8c, v8)
    c8 = _ncdhw(H.sweep_cat(f8, g)).reshape(2, 3, 8, *z["vol_raw_cat"].shape[2:])
    assert np.array_equal(c8[:, :, :5].reshape(z["vol_raw_cat"].shape), z["vol_raw_cat"])


@pytest.mark.parametrize("name", ["std_d8", "std_d16_rand", "cat_d8", "std_d10_odd"])
def test_sweep_seeded_bit_exact(golden_dir, name):
    case = SMALL_CASES[name]
    cfg = case["cfg"]
    z = _load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"])
    feats = _g(inp["feats"])
    feats_cl = feats.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)   # already channels-last storage
    for layout, ft in (("auto", feats), ("auto", feats_cl), ("nchw", feats)):
        if cfg.builder == "std":
            v = H.sweep_std(ft, _g(inp["grids"]), _g(inp["grid_masks"]), _g(inp["masks"]), layout=layout)
        else:
            v = H.sweep_cat(ft, _g(inp["grids"]), layout=layout)
        assert np.array_equal(_ncdhw(v), z["vol_raw"]), layout
    if cfg.builder == "std":
        vm = H.sweep_validity(_g(inp["grids"]), _g(inp["grid_masks"]), _g(inp["masks"]))
        assert vm.dtype == torch.uint8 and int(vm.max()) < (1 << cfg.num_cams)
        for ft in (feats, feats_cl):
            assert np.array_equal(_ncdhw(H.sweep_std_valid(ft, _g(inp["grids"]), vm)), z["vol_raw"])


@pytest.mark.parametrize("scale", [1e-19, 3e-13, 1.0, 1e16, 2e18])
def test_sweep_masked_variance_divisions_exact_from_subnormal_to_huge(scale):
    """The walking kernel divides by the camera count with a reciprocal + two fmas (correctly rounded for every finite
    input) and takes the hardware division beyond 1e30: bit-equal to the oracle's torch.div with variances down in the
    subnormals (scale 1e-19) and up past the switch (scale 2e18 -> variances ~ 1e36)."""
    cfg = SMALL_CASES["std_d8"]["cfg"]
    inp = synth.make_inputs(cfg, seed=11, batch=2)
    feats = (inp["feats"].astype(np.float64) * scale).astype(np.float32)
    want = O.sweep_std_masked(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (feats, inp["grids"], inp["grid_masks"], inp["masks"]))).numpy()
    assert np.isfinite(want).all()
    if scale < 1e-15:
        assert (np.abs(want[want != 0]) < 1.2e-38).any()            # some variances really are subnormal
    g = _g(inp["grids"])
    vm = H.sweep_validity(g, _g(inp["grid_masks"]), _g(inp["masks"]))
    f = _g(feats)
    for ft in (f, f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)):
        assert np.array_equal(_ncdhw(H.sweep_std_valid(ft, g, vm)), want)


def test_rig_constant_cache_follows_the_tensors():
    """The drop-in caches the validity byte per (grids, grid_masks, masks) identity + version: an
    in-place edit or a different tensor must be picked up, cache off must give the same volume."""
    cfg = SMALL_CASES["std_d8"]["cfg"]
    inp = synth.make_inputs(cfg, seed=5, batch=2)
    w = synth.make_weights(cfg, seed=5)
    cvb, _, _ = build_modules(cfg, w, DEV)
    f, g, gm, m = (_g(inp[k]) for k in ("feats", "grids", "grid_masks", "masks"))
    with torch.no_grad():
        v_cached = cvb.sweep(f, g, gm, m).clone()
        assert np.array_equal(cvb.sweep(f, g, gm, m).cpu().numpy(), v_cached.cpu().numpy())     # cache hit
        cvb.cache_rig_constants = False
        assert np.array_equal(cvb.sweep(f, g, gm, m).cpu().numpy(), v_cached.cpu().numpy())
        cvb.cache_rig_constants = True
        m.zero_()                                             # in-place edit: every camera masked out
        assert not cvb.sweep(f, g, gm, m).any()
        m2 = _g(inp["masks"])                                 # a different tensor
        assert np.array_equal(cvb.sweep(f, g, gm, m2).cpu().numpy(), v_cached.cpu().numpy())
        # free-then-reallocate: a second rig's same-shaped tensors that the caching allocator may place at the
        # first rig's addresses (version 0 again) must not hit the first rig's entry
        inp_b = synth.make_inputs(cfg, seed=6, batch=2, grid_kind="random", grid_mask_dtype="bool")   # another rig
        ref_b = cvb.sweep(f, *(_g(inp_b[k]) for k in ("grids", "grid_masks", "masks"))).clone()
        cvb.cache_rig_constants = False
        ref_a = cvb.sweep(f, _g(inp["grids"]), _g(inp["grid_masks"]), _g(inp["masks"])).clone()
        cvb.cache_rig_constants = True
        assert not torch.equal(ref_a, ref_b)
        for which in (inp, inp_b, inp, inp_b):
            g_, gm_, m_ = (_g(which[k]) for k in ("grids", "grid_masks", "masks"))
            out = cvb.sweep(f, g_, gm_, m_)
            assert torch.equal(out, ref_a if which is inp else ref_b)
            del g_, gm_, m_, out


# ------------------------------------------------------------------------------ K2 conv
CONV_SHAPES = [
    # (B, Cin, Cout, D, H, W, stride, res, slope)
    (1, 16, 16, 8, 16, 24, 1, False, 0.01),     # post_vol-like, N16 kernel, exact tiles
    (2, 16, 16, 5, 9, 11, 1, False, 0.01),      # ragged bricks
    (1, 16, 32, 8, 16, 16, 2, False, 0.01),     # down.first stride 2
    (1, 16, 32, 7, 9, 13, 2, False, 0.01),      # stride 2, odd sizes
    (1, 32, 32, 8, 16, 32, 1, True, 0.01),      # residual block conv, big-brick kernel
    (1, 32, 32, 4, 6, 10, 1, True, 0.01),       # small-brick kernel
    (1, 32, 64, 4, 8, 8, 2, False, 0.01),
    (2, 64, 64, 4, 8, 16, 1, True, 0.01),
    (1, 64, 128, 4, 8, 8, 2, False, 0.01),
    (1, 128, 128, 2, 5, 9, 1, True, 0.01),
    (1, 128, 64, 4, 6, 8, 1, True, 0.01),       # up conv + skip
    (1, 32, 16, 6, 10, 12, 1, False, 0.01),     # out_costs.0
    (2, 16, 16, 9, 7, 37, 1, True, 0.01),       # Cout 16 with residual, ragged in every axis
    (1, 64, 16, 4, 8, 32, 1, False, 0.0),       # 4 slices into 16 couts
    (1, 48, 48, 4, 8, 12, 1, False, 0.01),      # concat builder post_vol (3 cout tiles)
    (1, 48, 96, 4, 8, 12, 2, False, 0.01),
    (1, 96, 96, 3, 6, 10, 1, True, 0.0),        # ReLU
    (1, 96, 192, 3, 6, 10, 2, False, 0.01),
    (1, 64, 32, 5, 7, 9, 1, False, 1.0),        # identity activation
    (32, 128, 128, 2, 10, 40, 1, True, 0.01),   # UNet level 2 at 32 frames: the 2 x 5 x 16 brick variant (H a multiple of 5, not of 4)
    (32, 64, 64, 3, 15, 21, 1, True, 0.01),     # ragged in D and W (two rounds of 2 x 4 x 16 bricks by the unit-cost rule)
    (40, 64, 64, 3, 15, 21, 1, True, 0.01),     # ... 2 x 5 x 16 bricks, ragged in D and W
    (40, 64, 64, 3, 10, 24, 1, True, 0.01),     # 2 x 10 x 8 bricks (W = 8 mod 16, H a multiple of 10), ragged in D
    (48, 32, 96, 2, 15, 40, 1, True, 0.01),     # W = 8 mod 16 but H not a multiple of 10: 2 x 5 x 16 bricks stay
    (6, 64, 64, 4, 20, 80, 1, True, 0.01),      # UNet level 1 at six frames: 2 x 5 x 16 bricks put the launch into one round
    (8, 128, 128, 2, 10, 40, 1, True, 0.01),    # UNet level 2 at eight frames: 2 x 4 x 16 bricks, one round
    (32, 32, 96, 4, 10, 40, 1, True, 0.01),     # 96-cout units on 2 x 5 x 16 bricks (the fint96 regulators' level 2 at D = 16)
    (24, 32, 128, 1, 10, 40, 1, True, 0.01),    # one-plane volume (E8's level 2): 1 x 5 x 16 bricks, 128-cout units
    (64, 16, 192, 1, 10, 40, 1, False, 0.01),   # ... 192-cout units
    (96, 16, 128, 1, 7, 21, 1, True, 0.0),      # one-plane volume, H not a multiple of 5: 1 x 4 x 16 bricks, ragged
    (64, 16, 96, 8, 16, 24, 2, False, 0.01),    # stride 2 in 96-cout units
    (48, 32, 128, 7, 17, 23, 2, False, 0.01),   # stride 2 in 128-cout units, odd sizes
    (64, 16, 192, 8, 16, 24, 2, False, 0.0),    # stride 2 in 192-cout units
    (1, 32, 384, 1, 10, 40, 1, True, 0.01),     # one-plane volume at ONE frame (E8's level 2 on the latency path): the small-launch rule, not 18 128-cout units
    (2, 32, 384, 1, 10, 40, 1, False, 0.01),    # ... at two frames
    (20, 64, 96, 4, 20, 80, 1, True, 0.01),     # 96-cout units on 2 x 4 x 16 bricks; with the rows above and below every brick of the 32-channel-slice kernels
    (40, 64, 96, 3, 15, 21, 1, False, 0.01),    # ... 2 x 5 x 16, ragged
    (40, 32, 96, 4, 10, 24, 1, True, 0.01),     # ... 2 x 10 x 8
    (96, 32, 128, 1, 7, 21, 1, True, 0.0),      # one-plane 1 x 4 x 16 x 128 couts on 32 input channels
    (24, 64, 128, 1, 15, 21, 1, True, 0.01),    # one-plane 1 x 5 x 16 x 128
    (64, 32, 192, 1, 15, 21, 1, False, 0.01),   # one-plane 1 x 5 x 16 x 192
    (64, 32, 192, 1, 10, 40, 1, False, 0.01),   # one-plane 1 x 10 x 8 x 192
    (1, 128, 128, 2, 10, 40, 1, True, 0.01),    # UNet level 2 at one frame: the one-plane 32-cout units with the depth skip per unit (18 of 27 slots)
    (5, 64, 128, 2, 10, 40, 1, True, 0.01),     # ... 64-cout units
    (48, 32, 64, 4, 20, 80, 1, True, 0.01),     # a volume FOUR planes deep in layers of >= 4 rounds of bricks: the border-plane skip (bottom bricks and top
    (44, 32, 96, 4, 18, 70, 1, False, 0.01),    # bricks as launches of their own on kernels without the taps that meet the padding), 64- and 96-cout units, ragged
    (1, 64, 128, 4, 20, 80, 2, False, 0.01),    # the stride-2 conv into UNet level 2 at one frame: 60 units of 32 couts, not 30 of 64
    (8, 64, 128, 4, 20, 80, 2, False, 0.01),    # ... at eight frames: 64-cout units
    (1, 64, 64, 4, 20, 80, 1, True, 0.01),      # UNet level 1 at one frame: 200 units of 32 couts, waves as (voxel half, cout tile)
    (2, 64, 64, 4, 20, 80, 1, True, 0.01),      # ... at two frames: 200 units of 64 couts
]
EXPECTED_VARIANT = {        # (B, Cin, Cout, D, H, W) -> brick / unit shape the dispatcher must pick
    (1, 16, 32, 8, 16, 16): "<1, 2, 2, 2, 2, 4, 8, 2", (1, 16, 32, 7, 9, 13): "<1, 2, 2, 2, 2, 4, 8, 2",       # stride 2, 32 couts
    (1, 128, 128, 2, 5, 9): "<1, 1, 4, 1, 1, 4, 16, 1, 3, false, false, false, true>",      # one frame: 16-cout units, weights through LDS
    (2, 64, 64, 4, 8, 16): "<1, 1, 4, 1, 1, 4, 16, 1, 3, false, false, false, true>",
    (32, 128, 128, 2, 10, 40): "<2, 5, 2, 2, 2, 10, 8", (32, 64, 64, 3, 15, 21): "<2, 4, 2, 2, 2, 4, 16",      # (two full rounds of 2 x 4 x 16 bricks: the unit-cost rule)
    (32, 32, 96, 4, 10, 40): "<3, 5, 2, 2, 2, 10, 8", (24, 32, 128, 1, 10, 40): "<2, 5, 1, 4, 1, 10, 8",
    (64, 16, 192, 1, 10, 40): "<3, 5, 1, 4, 1, 10, 8", (96, 16, 128, 1, 7, 21): "<2, 4, 1, 4, 1, 4, 16",
    (1, 32, 384, 1, 10, 40): "<1, 1, 4, 1, 1, 4, 16, 1, 3, false, false, false, true>", (2, 32, 384, 1, 10, 40): "<1, 2, 2, 2, 1, 4, 16, 1, 3, false, false, false, false>",     # 32-cout units: waves as (voxel half, cout tile)
    (40, 64, 64, 3, 10, 24): "<2, 5, 2, 2, 2, 10, 8", (48, 32, 96, 2, 15, 40): "<3, 5, 2, 2, 2, 5, 16",
    (40, 64, 64, 3, 15, 21): "<2, 5, 2, 2, 2, 5, 16", (6, 64, 64, 4, 20, 80): "<2, 5, 2, 2, 2, 5, 16", (8, 128, 128, 2, 10, 40): "<2, 4, 2, 2, 2, 4, 16",
    (1, 64, 128, 4, 20, 80): "<1, 2, 2, 2, 2, 4, 8, 2", (8, 64, 128, 4, 20, 80): "<2, 2, 2, 2, 2, 4, 8, 2",
    (1, 64, 64, 4, 20, 80): "<1, 2, 2, 2, 1, 4, 16, 1, 3, false, false, false, false>", (2, 64, 64, 4, 20, 80): "<2, 2, 2, 2, 1, 4, 16, 1, 3, false, false, false, false>",
    (64, 16, 96, 8, 16, 24): "<3, 2, 2, 2, 2, 4, 8, 2", (48, 32, 128, 7, 17, 23): "<2, 4, 1, 4, 2, 4, 8, 2", (64, 16, 192, 8, 16, 24): "<3, 4, 1, 4, 2, 4, 8, 2",
}


def _d32_kernel_expected(prefix: str, name: str, D: int) -> str:
    """The name a 32-channel-slice launch must carry (`name`: what the library says; template args ..., TD, TH, TW): the depth-skip
    forms where the volume is as deep as the brick (_dk_) or two planes deep on a one-plane small-launch unit (_dk2_)."""
    args = name.split("<")[1].rstrip(">")
    td = int(args.split(",")[4])
    small = args in ("1, 2, 2, 2, 1, 4, 16", "2, 2, 2, 2, 1, 4, 16")
    if small:
        return prefix + ("_d32_dk2_kernel<" if D == 2 else "_d32_kernel<")
    return prefix + ("_d32_dk_kernel<" if (D == td and D <= 2) else "_d32_kernel<")


def _conv_case(rng, B, Cin, Cout, D, Hh, W, stride, res, slope, bias=False):
    x = rng.standard_normal((B, Cin, D, Hh, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3, 3)) / np.sqrt(27 * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    Do, Ho, Wo = (D - 1) // stride + 1, (Hh - 1) // stride + 1, (W - 1) // stride + 1
    r = rng.standard_normal((B, Cout, Do, Ho, Wo)).astype(np.float32) if res else None
    y = F.conv3d(torch.from_numpy(x), torch.from_numpy(w), None, stride=stride, padding=1)
    y = y * torch.from_numpy(scale).view(1, -1, 1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1, 1)
    if res:
        y = y + torch.from_numpy(r)
    y = torch.where(y > 0, y, y * slope)
    return x, w, scale, shift, r, y.numpy()


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3d_mfma_and_direct_vs_oracle(shape):
    rng = np.random.default_rng(hash(shape) % (2 ** 31))
    B, Cin, Cout, D, Hh, W, stride, res, slope = shape
    x, w, scale, shift, r, yref = _conv_case(rng, *shape)
    xg = _g(x).permute(0, 2, 3, 4, 1).contiguous()
    rg = None if r is None else _g(r).permute(0, 2, 3, 4, 1).contiguous()
    wg = _g(w)
    wp = H.pack_conv_weights(wg)
    assert wp is not None
    outs = {}
    for name, impl in (("mfma", H.CONV_MFMA), ("direct", H.CONV_DIRECT)):
        y = H.conv3d(xg, wg, wp, _g(scale), _g(shift), res=rg, stride=stride, neg_slope=slope, impl=impl)
        outs[name] = _ncdhw(y)
        assert outs[name].shape == yref.shape
        assert _rel(outs[name], yref) <= 2e-5, (name, _rel(outs[name], yref))
    assert _rel(outs["mfma"], outs["direct"]) <= 2e-5


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3d_bf16x3_vs_oracle(shape):
    """Split-bf16 MFMA path: 16-bit operands, fp32 accumulation -> 1e-4 of the tensor max
    (the fp32 paths above hold 2e-5)."""
    rng = np.random.default_rng(hash(shape) % (2 ** 31))
    B, Cin, Cout, D, Hh, W, stride, res, slope = shape
    x, w, scale, shift, r, yref = _conv_case(rng, *shape)
    xg = _g(x).permute(0, 2, 3, 4, 1).contiguous()
    rg = None if r is None else _g(r).permute(0, 2, 3, 4, 1).contiguous()
    wg = _g(w)
    wp = H.pack_conv_weights_bf16x3(wg)
    assert "bf16x3" in H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3)
    if shape[:6] in {(k[0], k[1], k[2], k[3], k[4], k[5]) for k in EXPECTED_VARIANT}:
        assert EXPECTED_VARIANT[shape[:6]] in H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3)
    y = H.conv3d(xg, wg, wp, _g(scale), _g(shift), res=rg, stride=stride, neg_slope=slope, impl=H.CONV_BF16X3)
    err = _rel(_ncdhw(y), yref)
    assert err <= 1e-4, err
    if H.conv3d_d32_applies(B, Cin, D, Hh, W, Cout, stride):      # the same bricks on 32-channel slices (27 k-steps per 32 channels)
        assert Cin % 32 == 0 and stride == 1
        name = H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3_D32)
        # (volumes one or two planes deep: the depth-skip kernels, which multiply only the kd taps that meet a plane of the volume)
        assert name.startswith(_d32_kernel_expected("conv3d_bf16x3", name, D)), name
        base = H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3)
        # the same brick as the tap-pair choice -- except a two-plane volume's one-round launch, which takes the 32-cout units with the
        # depth skip instead of the 16-cout units with their weight slice in LDS
        assert name.split("<")[1].rstrip(">") in base or ("dk2" in name and "<1, 1, 4, 1, 1, 4, 16" in base), (name, base)
        yd = H.conv3d(xg, wg, H.pack_conv_weights_bf16x3_d32(wg), _g(scale), _g(shift), res=rg, stride=stride, neg_slope=slope, impl=H.CONV_BF16X3_D32)
        assert _rel(_ncdhw(yd), yref) <= 1e-4
        assert _rel(_ncdhw(yd), _ncdhw(y)) <= 4e-6      # same products, another summation order
    if Cout == 16 and stride == 1:       # the plane-schedule kernel of the Cout == 16 layers
        assert "true, false, false>" in H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3_C16)
        yp = H.conv3d(xg, wg, H.pack_conv_weights_bf16x3_c16(wg), _g(scale), _g(shift), res=rg, stride=stride,
                      neg_slope=slope, impl=H.CONV_BF16X3_C16)
        assert _rel(_ncdhw(yp), yref) <= 1e-4
        assert _rel(_ncdhw(yp), _ncdhw(y)) <= 2e-6      # same products, different summation order


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3d_f16x3_vs_oracle(shape):
    """The fp16 split (MVSGI_CONV_F16): every dispatcher variant of the streaming kernel in its f16 instantiation -- 11 + 11
    significant bits per operand, per-output-channel power-of-two weight pre-scaling undone in the epilogue's scale -- lands 10x
    closer to the fp32 convolution than the bf16 split's 1e-4 bar; the kernel's name says which arithmetic ran."""
    rng = np.random.default_rng(hash(shape) % (2 ** 31))
    B, Cin, Cout, D, Hh, W, stride, res, slope = shape
    x, w, scale, shift, r, yref = _conv_case(rng, *shape)
    xg = _g(x).permute(0, 2, 3, 4, 1).contiguous()
    rg = None if r is None else _g(r).permute(0, 2, 3, 4, 1).contiguous()
    wg = _g(w) * 0.01                                   # small weights: un-scaled, their lo parts would be fp16 subnormals
    yref = None
    y64 = F.conv3d(torch.from_numpy(x).double(), (torch.from_numpy(w) * 0.01).double(), None, stride=stride, padding=1)
    y64 = y64 * torch.from_numpy(scale).double().view(1, -1, 1, 1, 1) + torch.from_numpy(shift).double().view(1, -1, 1, 1, 1)
    if res:
        y64 = y64 + torch.from_numpy(r).double()
    yref = torch.where(y64 > 0, y64, y64 * slope).float().numpy()
    wp, unscale = H.pack_conv_weights_f16x3(wg)
    assert float(unscale.max()) <= 2.0 ** -4 and float((wg.abs().amax(dim=(1, 2, 3, 4)) / unscale).min()) > 512.0
    name = H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3 | H.CONV_F16)
    assert name.startswith("conv3d_f16x3_kernel<")
    assert name.replace("f16x3", "bf16x3") == H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3)      # the same variant
    y = H.conv3d(xg, wg, wp, _g(scale) * unscale, _g(shift), res=rg, stride=stride, neg_slope=slope, impl=H.CONV_BF16X3 | H.CONV_F16)
    err = _rel(_ncdhw(y), yref)
    assert err <= 5e-6, err
    yb = H.conv3d(xg, wg, H.pack_conv_weights_bf16x3(wg), _g(scale), _g(shift), res=rg, stride=stride, neg_slope=slope, impl=H.CONV_BF16X3)
    eb = _rel(_ncdhw(yb), yref)                          # ... and closer than the bf16 split on the same problem (a residual of
    assert (eb > 1.5 * err) if not res else (eb >= err or err <= 2.5e-7), (eb, err)   # O(1) beside the x 0.01 convolution hides both splits behind the final add's rounding: an ulp either way)
    if H.conv3d_d32_applies(B, Cin, D, Hh, W, Cout, stride):
        wpd, und = H.pack_conv_weights_f16x3(wg, H.CONV_BF16X3_D32)
        n16 = H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3_D32 | H.CONV_F16)
        assert n16.startswith(_d32_kernel_expected("conv3d_f16x3", n16, D)), n16
        yd = H.conv3d(xg, wg, wpd, _g(scale) * und, _g(shift), res=rg, stride=stride, neg_slope=slope, impl=H.CONV_BF16X3_D32 | H.CONV_F16)
        assert _rel(_ncdhw(yd), yref) <= 5e-6 and _rel(_ncdhw(yd), _ncdhw(y)) <= 2e-6
    if Cout == 16 and stride == 1:
        wpc, un = H.pack_conv_weights_f16x3(wg, H.CONV_BF16X3_C16)
        yp = H.conv3d(xg, wg, wpc, _g(scale) * un, _g(shift), res=rg, stride=stride, neg_slope=slope, impl=H.CONV_BF16X3_C16 | H.CONV_F16)
        assert _rel(_ncdhw(yp), yref) <= 5e-6


def test_conv3d_f16x3_saturates_and_rejects_misuse():
    """fp16's range: operands beyond +-65504 are CLAMPED (never inf / nan); zero weights pack; the flag is refused on the exact paths."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 4, 6, 16, 16)).astype(np.float32)
    x[0, 1, 2, 3, :4] = [1e5, -3e6, 65504.0, 7e4]
    w = (rng.standard_normal((16, 16, 3, 3, 3)) / np.sqrt(27 * 16)).astype(np.float32)
    w[3] = 0.0
    xg, wg = _g(x), _g(w)
    wp, un = H.pack_conv_weights_f16x3(wg)
    assert float(un[3]) == 1.0
    one, zero = torch.ones(16, device=DEV), torch.zeros(16, device=DEV)
    y = H.conv3d(xg, wg, wp, one * un, zero, neg_slope=1.0, impl=H.CONV_BF16X3 | H.CONV_F16)
    assert torch.isfinite(y).all() and not y[..., 3].any()
    ref = F.conv3d(torch.from_numpy(np.clip(x, -65504.0, 65504.0)).permute(0, 4, 1, 2, 3).double(), torch.from_numpy(w).double(), padding=1)
    assert _rel(_ncdhw(y), ref.float().numpy()) <= 5e-6
    with pytest.raises(RuntimeError, match="MVSGI_CONV_F16"):
        H.conv3d(xg, wg, H.pack_conv_weights(wg), one, zero, impl=H.CONV_MFMA | H.CONV_F16)


def test_conv3d_dispatcher_fuzz_vs_exact_kernel():
    """Forty random layer shapes around the dispatcher's thresholds (one-plane volumes, 5-row planes, 16- to 384-cout layers, stride
    1 and 2, one frame to 33, with and without residual, three activations): the split-bf16 kernel the dispatcher picks against the
    exact-fp32 MFMA kernel on the same device tensors (tools/conv_fuzz.py; 150 shapes of another seed ran clean at 5.9e-6)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("conv_fuzz", os.path.join(root, "tools", "conv_fuzz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    worst, seen = mod.run(40, seed=0, verbose=False)
    assert worst <= 1e-4, worst
    assert len(seen) >= 5          # several kernel variants were exercised


@pytest.mark.parametrize("shape", [
    # (B, Cin, Cout, D, H, W, res, slope, up2)
    (24, 32, 32, 8, 16, 64, True, 0.01, False),      # 32 couts: 4x4x16 bricks, residual
    (3, 32, 32, 9, 37, 70, False, 0.01, False),      # ragged in every axis
    (22, 64, 64, 4, 10, 48, True, 0.0, False),       # 64 couts: 2x4x16 bricks, two 32-cout waves
    (22, 128, 128, 2, 10, 40, True, 0.01, False),    # two cout blocks per brick
    (26, 64, 32, 2, 8, 32, True, 0.01, True),        # up1-like: fused upsample
    (26, 128, 64, 2, 5, 24, True, 0.01, True),       # up0-like: fused upsample, 64 couts
    (17, 16, 96, 4, 12, 32, False, 1.0, False),      # 3 tiles of 32: the last workgroup's second wave is clamped
])
def test_conv3d_v32_schedule_vs_oracle(shape):
    """The 32x32x16-MFMA schedule (MVSGI_CONV_BF16X3_V32): same arithmetic as the 16x16x32 kernels, 1e-4 of the
    tensor max against ATen, and the same products as the 16x16x32 kernel (different summation order)."""
    B, Cin, Cout, D, Hh, W, res, slope, up2 = shape
    rng = np.random.default_rng(sum(shape[:6]))
    x = rng.standard_normal((B, Cin, D, Hh, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3, 3)) / np.sqrt(27 * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    xin = torch.from_numpy(x)
    if up2:
        xin = F.interpolate(xin, scale_factor=2, mode="trilinear", align_corners=False)
    r = rng.standard_normal((B, Cout, *xin.shape[2:])).astype(np.float32) if res else None
    y = F.conv3d(xin, torch.from_numpy(w), None, padding=1)
    y = y * torch.from_numpy(scale).view(1, -1, 1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1, 1)
    if res:
        y = y + torch.from_numpy(r)
    yref = torch.where(y > 0, y, y * slope).numpy()
    xg = _g(x).permute(0, 2, 3, 4, 1).contiguous()
    rg = _g(r).permute(0, 2, 3, 4, 1).contiguous() if res else None
    wg = _g(w)
    assert H.conv3d_v32_applies(B, Cin, *xin.shape[2:], Cout, 1)
    wv = H.pack_conv_weights_bf16x3_v32(wg)
    if up2:
        assert "true, false, true, false>" in H.conv3d_up2_variant(B, Cin, D, Hh, W, Cout, H.CONV_BF16X3_V32)
        got = H.conv3d_up2(xg, wv, _g(scale), _g(shift), res=rg, neg_slope=slope, w_layout=H.CONV_BF16X3_V32)
        old = H.conv3d_up2(xg, H.pack_conv_weights_bf16x3(wg), _g(scale), _g(shift), res=rg, neg_slope=slope)
    else:
        assert "false, false, true, false>" in H.conv3d_variant(B, Cin, D, Hh, W, Cout, 1, H.CONV_BF16X3_V32)
        got = H.conv3d(xg, wg, wv, _g(scale), _g(shift), res=rg, neg_slope=slope, impl=H.CONV_BF16X3_V32)
        old = H.conv3d(xg, wg, H.pack_conv_weights_bf16x3(wg), _g(scale), _g(shift), res=rg, neg_slope=slope,
                       impl=H.CONV_BF16X3)
    assert _rel(_ncdhw(got), yref) <= 1e-4
    assert _rel(_ncdhw(got), _ncdhw(old)) <= 3e-6
    # too small a problem: the dispatcher says so instead of launching a mostly idle grid
    assert not H.conv3d_v32_applies(1, Cin, 2, 4, 16, Cout, 1)


@pytest.mark.parametrize("shape", [
    # (B, Cin, Cout, Dl, Hl, Wl, res)
    (1, 32, 16, 4, 8, 16, False),      # out_costs.0-like: exact 4x4x16 bricks
    (2, 32, 16, 3, 5, 9, False),       # ragged bricks, odd low-res sizes
    (1, 64, 32, 2, 6, 8, True),        # up block + skip, small-brick (TD = 2) variant
    (3, 64, 32, 4, 20, 24, True),      # big-brick variant (>= 384 bricks)
    (1, 128, 64, 1, 3, 5, True),       # Dl = 1: every corner clamps along D
    (1, 96, 48, 2, 4, 8, False),       # 3 cout tiles
    (1, 192, 96, 2, 4, 8, True),       # 6 cout tiles
    (1, 128, 64, 2, 10, 40, True),     # an up block at one frame: 2 x 2 x 16 bricks x 32 couts (200 units, one round of the chip)
    (2, 128, 64, 2, 10, 40, True),     # ... at two frames: 2 x 4 x 16 bricks x 64 couts
    (1, 64, 64, 3, 5, 9, False),       # the one-round units on ragged bricks
    (8, 128, 64, 2, 10, 40, True),     # 2 x 4 x 16 bricks x 64 couts at eight frames: also on 32-channel slices
    (12, 64, 96, 3, 5, 9, False),      # ... 96 couts in 64-cout units, ragged
    (16, 64, 96, 4, 10, 10, False),    # ... x 96 couts
    (48, 32, 64, 2, 10, 40, True),     # onto a volume FOUR planes deep, layers of >= 4 rounds of bricks: the border-plane skip of the fused form
    (48, 64, 96, 1, 10, 40, True),     # out of a ONE-plane level (the upsampled volume is two planes deep): the depth-skip form of those kernels
    (64, 32, 64, 1, 10, 40, True),     # ... 64 couts
    (1, 64, 32, 4, 20, 80, True),      # the last up block at one frame: 200 units of 4 x 4 x 16 in one round, not 400 of 2 x 4 x 16 in two
])
def test_conv3d_fused_upsample_vs_interpolate_then_conv(shape):
    """mvsgi_conv3d_up2_f32 == conv3d(F.interpolate(x, scale 2, trilinear, align_corners=False)):
    ResizeConv3d.forward (common_modules.py:332-355) with the upsample inside the conv's producers."""
    B, Cin, Cout, Dl, Hl, Wl, res = shape
    rng = np.random.default_rng(sum(shape[:6]))
    xl = rng.standard_normal((B, Cin, Dl, Hl, Wl)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3, 3)) / np.sqrt(27 * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    r = rng.standard_normal((B, Cout, 2 * Dl, 2 * Hl, 2 * Wl)).astype(np.float32) if res else None
    up = F.interpolate(torch.from_numpy(xl), scale_factor=2, mode="trilinear", align_corners=False)
    y = F.conv3d(up, torch.from_numpy(w), None, padding=1)
    y = y * torch.from_numpy(scale).view(1, -1, 1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1, 1)
    if res:
        y = y + torch.from_numpy(r)
    yref = torch.where(y > 0, y, y * 0.01).numpy()
    xg = _g(xl).permute(0, 2, 3, 4, 1).contiguous()
    rg = _g(r).permute(0, 2, 3, 4, 1).contiguous() if res else None
    got = H.conv3d_up2(xg, H.pack_conv_weights_bf16x3(_g(w)), _g(scale), _g(shift), res=rg, neg_slope=0.01)
    assert "true" in H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout)
    if shape[:6] == (1, 64, 32, 4, 20, 80):
        assert "<2, 4, 4, 1, 4, 4, 16," in H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout)
    if shape[:6] in ((1, 128, 64, 2, 10, 40), (2, 128, 64, 2, 10, 40)):
        assert ("<1, 2, 2, 2, 2, 2, 16," if B == 1 else "<2, 4, 2, 2, 2, 4, 16,") in H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout)
    assert _rel(_ncdhw(got), yref) <= 1e-4
    if Cout == 16:
        assert "true, true, false, false>" in H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout, H.CONV_BF16X3_C16)
        gp = H.conv3d_up2(xg, H.pack_conv_weights_bf16x3_c16(_g(w)), _g(scale), _g(shift), res=rg, neg_slope=0.01,
                          w_layout=H.CONV_BF16X3_C16)
        assert _rel(_ncdhw(gp), yref) <= 1e-4
    if H.conv3d_up2_d32_applies(B, Cin, Dl, Hl, Wl, Cout):      # the same launch on 32-channel slices, both splits
        assert H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout, H.CONV_BF16X3_D32).startswith("conv3d_bf16x3_d32u_dk_kernel<" if Dl == 1 else "conv3d_bf16x3_d32u_kernel<")
        gd = H.conv3d_up2(xg, H.pack_conv_weights_bf16x3_d32(_g(w)), _g(scale), _g(shift), res=rg, neg_slope=0.01, w_layout=H.CONV_BF16X3_D32)
        assert _rel(_ncdhw(gd), yref) <= 1e-4 and _rel(_ncdhw(gd), _ncdhw(got)) <= 4e-6
        wpd, und = H.pack_conv_weights_f16x3(_g(w), H.CONV_BF16X3_D32)
        assert H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout, H.CONV_BF16X3_D32 | H.CONV_F16).startswith("conv3d_f16x3_d32u_dk_kernel<" if Dl == 1 else "conv3d_f16x3_d32u_kernel<")
        gd16 = H.conv3d_up2(xg, wpd, _g(scale) * und, _g(shift), res=rg, neg_slope=0.01, w_layout=H.CONV_BF16X3_D32 | H.CONV_F16)
        assert _rel(_ncdhw(gd16), yref) <= 1e-5
    wp16, un16 = H.pack_conv_weights_f16x3(_g(w))      # the fp16 split of the same launch
    g16 = H.conv3d_up2(xg, wp16, _g(scale) * un16, _g(shift), res=rg, neg_slope=0.01, w_layout=H.CONV_BF16X3 | H.CONV_F16)
    assert H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout, H.CONV_BF16X3 | H.CONV_F16).startswith("conv3d_f16x3_kernel<")
    assert _rel(_ncdhw(g16), yref) <= 1e-5
    # and the two-launch path it replaces
    two = H.conv3d(H.resize_trilinear(xg, (2 * Dl, 2 * Hl, 2 * Wl)), _g(w), H.pack_conv_weights_bf16x3(_g(w)),
                   _g(scale), _g(shift), res=rg, neg_slope=0.01, impl=H.CONV_BF16X3)
    assert _rel(_ncdhw(got), _ncdhw(two)) <= 1e-5


def test_cost_head_whole_depth_march_and_epilogue():
    """>= 1024 (frame, window) pairs: every workgroup marches the whole depth (no D split);
    also the residual / LeakyReLU epilogue and ragged H, W."""
    rng = np.random.default_rng(8)
    for (B, dims, res, slope) in ((4, (3, 128, 512), False, 1.0), (3, (5, 125, 470), True, 0.01)):
        x, w, scale, shift, r, yref = _conv_case(rng, B, 16, 1, *dims, 1, res, slope)
        xg = _g(x).permute(0, 2, 3, 4, 1).contiguous()
        rg = _g(r).permute(0, 2, 3, 4, 1).contiguous() if res else None
        y = H.conv3d(xg, _g(w), H.pack_conv_weights(_g(w)), _g(scale), _g(shift), res=rg, neg_slope=slope)
        assert "head" in H.conv3d_variant(B, 16, *dims, 1)
        assert _rel(_ncdhw(y), yref) <= 2e-5


def test_conv3d_direct_odd_channels_and_cost_head():
    rng = np.random.default_rng(3)
    for (Cin, Cout) in ((4, 8), (16, 1), (5, 3), (48, 1), (64, 1)):
        for dims in ((5, 7, 9), (8, 16, 24)):
            x, w, scale, shift, r, yref = _conv_case(rng, 2, Cin, Cout, *dims, 1, False, 1.0)
            xg = _g(x).permute(0, 2, 3, 4, 1).contiguous()
            wp = H.pack_conv_weights(_g(w))
            y = H.conv3d(xg, _g(w), wp, _g(scale), _g(shift), neg_slope=1.0)
            assert _rel(_ncdhw(y), yref) <= 2e-5
            name = H.conv3d_variant(2, Cin, *dims, Cout)
            if Cout == 1 and Cin % 16 == 0:
                assert "head" in name     # LDS-tiled cost head
                yd = H.conv3d(xg, _g(w), wp, _g(scale), _g(shift), neg_slope=1.0, impl=H.CONV_DIRECT)
                assert _rel(_ncdhw(y), _ncdhw(yd)) <= 2e-5
            else:
                assert "direct" in name


# ------------------------------------------------------------------------------ K3 resize
@pytest.mark.parametrize("shape,size", [((1, 32, 4, 6, 10), (8, 12, 20)), ((2, 16, 3, 5, 7), (6, 10, 14)),
                                        ((1, 64, 4, 4, 10), (3, 3, 10)), ((1, 5, 2, 3, 5), (5, 6, 20)),
                                        ((1, 128, 2, 2, 5), (4, 4, 10))])
def test_resize_trilinear_vs_aten(shape, size):
    rng = np.random.default_rng(9)
    x = rng.standard_normal(shape).astype(np.float32)
    ref = F.interpolate(torch.from_numpy(x), size=size, mode="trilinear", align_corners=False).numpy()
    y = H.resize_trilinear(_g(x).permute(0, 2, 3, 4, 1).contiguous(), size)
    assert _rel(_ncdhw(y), ref) <= 2e-6


# ------------------------------------------------------------------------------ K4 soft-argmin
def test_softargmin_variants(golden_dir):
    z = _load(golden_dir, "regress_variants")
    costs = _g(z["costs"])
    cands = list(z["dist_cands"])
    for tag, kw in dict(s2_pre=dict(interp_scale_factor=2, pre_interp=True),
                        s0_pre=dict(interp_scale_factor=0, pre_interp=True),
                        s2_post=dict(interp_scale_factor=2, pre_interp=False)).items():
        dr = dropin.DistanceRegressorWithFixedCandidates(bf=96, dist_cands=cands, **kw).to(DEV)
        inv, pr = dr(costs)
        assert _rel(inv.cpu().numpy(), z[f"inv_{tag}"]) <= 1e-5
        assert _rel(pr.cpu().numpy(), z[f"pr_{tag}"]) <= 1e-5
        dr.return_norm_costs = False
        inv2, pr2 = dr(costs)
        assert pr2 is None and torch.equal(inv, inv2)
    dr = dropin.DistanceRegressorWithFixedCandidates(bf=96, dist_cands=cands, interp_scale_factor=2,
                                                     pre_interp=True).to(DEV)
    dr.update_dist_cands(list(z["updated_cands"]))
    assert _rel(dr(costs)[0].cpu().numpy(), z["inv_updated"]) <= 1e-5


# ------------------------------------------------------------------------------ layout
def test_layout_roundtrip_and_regulator_accepts_both_formats():
    rng = np.random.default_rng(4)
    x = _g(rng.standard_normal((2, 24, 3, 5, 70)).astype(np.float32))
    y = H.ncdhw_to_ndhwc(x)
    assert torch.equal(y, x.permute(0, 2, 3, 4, 1).contiguous())
    assert torch.equal(H.ndhwc_to_ncdhw(y), x)
    reg = dropin.UNetCostVolumeRegulatorBase(16, 32).eval().to(DEV)
    v = _g(rng.standard_normal((1, 16, 8, 8, 16)).astype(np.float32))
    a = reg(v)                                                   # contiguous NCDHW in
    b = reg(v.contiguous(memory_format=torch.channels_last_3d))  # channels-last in
    assert tuple(a.shape) == (1, 1, 8, 8, 16) and torch.equal(a, b)


# ------------------------------------------------------------------------------ whole path
@pytest.fixture(params=["f32", "bf16x3", "f16x3"])
def conv_mode(request):
    old = H.get_conv_mode()
    H.set_conv_mode(request.param)
    yield request.param
    H.set_conv_mode(old)


@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_small_cases_vs_reference_goldens(golden_dir, name, conv_mode):
    case = SMALL_CASES[name]
    cfg = case["cfg"]
    z = _load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"])
    feats = _g(inp["feats"])
    for gain in case["gains"]:
        w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
        hp = HotPath(cfg, w, inp, device=DEV)
        vol = hp.cv_builder(feats, hp.grids, hp.grid_masks, hp.masks)
        costs = hp.cv_regulator(vol)
        inv, pr = hp.dist_regressor(costs)
        assert tuple(vol.shape) == (case["batch"], cfg.vol_chs, cfg.num_cands, *cfg.cv_hw)
        err = _rel(inv.cpu().numpy(), z[f"inv_dist_g{gain:g}"])
        import parity_log
        parity_log.record(name, conv_mode, gain, err,
                          float(np.abs(inv.cpu().numpy() - z[f"inv_dist_g{gain:g}"]).mean() / np.abs(z[f"inv_dist_g{gain:g}"]).mean()),
                          "golden", _pix(inv.cpu().numpy(), z[f"inv_dist_g{gain:g}"]))
        print(f"{name} [{conv_mode}] gain {gain}: inv_dist max-rel {err:.3e}")
        assert err <= 1e-3, (gain, err)          # the north-star bar
        if conv_mode == "f32":
            assert err <= 2e-4, (gain, err)      # what the exact-fp32 path actually delivers
        if "vol" in z and gain == case["gains"][0]:
            tol = 1.0 if conv_mode == "f32" else 10.0
            assert _rel(vol.contiguous().cpu().numpy(), z["vol"]) <= 2e-5 * tol
            assert _rel(costs.contiguous().cpu().numpy(), z["costs"]) <= 1e-4 * tol
            assert _rel(pr.cpu().numpy(), z["norm_costs"]) <= 1e-3 * tol


@pytest.mark.parametrize("switch", ["MVSGI_POLY", "MVSGI_S2RS", "MVSGI_HEAD_SPLIT", "MVSGI_RIG_CACHE", "MVSGI_FRONT_CHUNK", "MVSGI_CONV_MODE"])
def test_product_switches_off(golden_dir, switch):
    """The product's configuration surface (hip_ops lists it): the std_d16_rand golden (random grids, float grid masks,
    two frames, a peaky gain) through the whole path with each switch turned away from its default -- every alternative path
    stays within the north-star bar.  (The switches are read at import; the test sets what they set.)"""
    from mvs_gi_amd.dropin import cost_volume_builder as cb, cost_volume_regulator as cr
    case = SMALL_CASES["std_d16_rand"]
    cfg = case["cfg"]
    z = _load(golden_dir, "std_d16_rand")
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"])
    saved = (H.get_conv_mode(), cr._USE_POLY, cr._POLY_MIN_UNITS, cr._USE_S2RS, cr._HEAD_SPLIT, cb._FRONT_CHUNK)
    try:
        H.set_conv_mode("bf16x3")
        cr._POLY_MIN_UNITS = 0                 # the polyphase tail runs at this size (its default threshold is four full-size frames)
        rig_cache = True
        if switch == "MVSGI_POLY":
            cr._USE_POLY = False
        elif switch == "MVSGI_S2RS":
            cr._USE_S2RS = False
        elif switch == "MVSGI_HEAD_SPLIT":
            cr._HEAD_SPLIT = False
        elif switch == "MVSGI_RIG_CACHE":
            rig_cache = False
        elif switch == "MVSGI_FRONT_CHUNK":
            cb._FRONT_CHUNK = 1                # the sweep -> post_vol front end one frame at a time
        else:
            H.set_conv_mode("f32")
        gain = 16.0
        hp = HotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=gain), inp, device=DEV)
        hp.cv_builder.cache_rig_constants = rig_cache
        inv, _ = hp(_g(inp["feats"]))
        err = _rel(inv.cpu().numpy(), z[f"inv_dist_g{gain:g}"])
        print(f"{switch} off: inv_dist max-rel {err:.3e}")
        assert err <= 1e-3, (switch, err)
    finally:
        H.set_conv_mode(saved[0])
        cr._USE_POLY, cr._POLY_MIN_UNITS, cr._USE_S2RS, cr._HEAD_SPLIT, cb._FRONT_CHUNK = saved[1:]


_ORACLE_FULL = {}       # (case, gain) -> oracle inv_dist, shared by the two conv modes


def _l1(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).mean() / np.abs(np.asarray(b, np.float64)).mean())


@pytest.mark.parametrize("name", list(FULL_CASES))
def test_full_size_vs_reference_goldens(golden_dir, name, conv_mode):
    """BASELINE.json configs at full size (G16V, G16VV, E8, 4cam-32): inv_dist of the REFERENCE forward,
    committed as fixtures, against the HIP path on regenerated inputs.  The inputs must be bit-identical to
    the golden run's (sha256): if this host's libm regenerates different smooth grids the test FAILS -- it
    never changes its reference silently (the comparison against the oracle on that host's arrays is
    test_full_size_vs_oracle's job)."""
    import parity_log
    case = FULL_CASES[name]
    cfg = case["cfg"]
    z = _load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    # never a silent change of reference: a host whose libm regenerates other smooth grids FAILS here (test_full_size_vs_oracle
    # still pins the path against the oracle on that host's arrays)
    assert synth.digest(inp) == str(z["inputs_sha256"]), f"{name}: regenerated inputs differ from the golden run's (host libm)"
    feats = _g(inp["feats"])
    for gain in case["gains"]:
        w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
        hp = HotPath(cfg, w, inp, device=DEV)
        inv, _ = hp(feats)
        ref = z[f"inv_dist_g{gain:g}"]
        got = inv.cpu().numpy()
        err, l1 = _rel(got, ref), _l1(got, ref)
        px = _pix(got, ref)
        parity_log.record(name, conv_mode, gain, err, l1, "golden", px)
        print(f"{name} [{conv_mode}] gain {gain}: max-rel {err:.3e} per-pixel max-rel {px:.3e} mean-L1-rel {l1:.3e} (ref=golden)")
        assert err <= 1e-3, (gain, err)
        del hp
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", list(FULL_CASES))
def test_full_size_vs_oracle(name, conv_mode):
    """The same full-size cases against the CPU oracle on the same arrays (always runs; the oracle is pinned to
    the reference goldens by tests/test_oracle_golden.py)."""
    import parity_log
    case = FULL_CASES[name]
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    feats = _g(inp["feats"])
    gain = case["gains"][-1]
    w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
    if (name, gain) not in _ORACLE_FULL:
        t = O.to_torch(inp)
        _ORACLE_FULL[(name, gain)] = O.hot_path(t["feats"], t["grids"], t["grid_masks"], t["masks"], O.to_torch(w),
                                                cfg.builder, cfg.dist_cands, cfg.bf, cfg.interp_scale_factor,
                                                cfg.pre_interp).numpy()
    ref = _ORACLE_FULL[(name, gain)]
    hp = HotPath(cfg, w, inp, device=DEV)
    got = hp(feats)[0].cpu().numpy()
    err, l1 = _rel(got, ref), _l1(got, ref)
    parity_log.record(name, conv_mode, gain, err, l1, "oracle", _pix(got, ref))
    assert err <= 1e-3, (gain, err)
    del hp
    torch.cuda.empty_cache()


# (case, frames per part): bench.py's EXTRA_CONFIGS -- the batch at which each configuration is measured
BENCH_PARTS = [("full_G16VV", 32), ("full_E8", 64), ("full_4cam-32", 16), ("full_E16-48-96", 32)]


@pytest.mark.parametrize("split", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("name,part", BENCH_PARTS)
def test_full_size_at_bench_batch_streamed_vs_reference_golden(golden_dir, name, part, split):
    """The other three BASELINE.json configurations at bench.py's operating point -- two parts of `part` frames on two HIP
    streams inside one hipGraph (StreamedHotPath), where the dispatcher picks other units than at one frame (96 / 128 / 192-cout
    units, the >= 384 / 512-unit rules): the first and the last frame of the step reproduce the single-frame REFERENCE golden,
    at the sharpest gain the fixture holds; a scaled frame differs; equal frames give equal bits in either part."""
    import parity_log
    from mvs_gi_amd.pipeline import StreamedHotPath
    case = FULL_CASES[name]
    cfg, z = case["cfg"], _load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=1, grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"]), "regenerated inputs differ from the golden run's (host libm)"
    old = H.get_conv_mode()
    try:
        H.set_conv_mode(split)
        gain = max(case["gains"])
        ref = z[f"inv_dist_g{gain:g}"]
        shp = StreamedHotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=gain), inp, device=DEV, n_streams=2)
        f = _g(inp["feats"]).expand(2 * part, -1, -1, -1, -1).contiguous()
        f[3::8] *= 0.5
        shp.capture(f)
        parts = shp.replay()
        torch.cuda.synchronize()
        got = np.concatenate([p[0].cpu().numpy() for p in parts], 0)
        n = 2 * part
        for fr in (0, n - 1):
            assert (fr - 3) % 8 != 0
            err = _rel(got[fr:fr + 1], ref)
            parity_log.record(f"{name}(2x{part} streamed)[{fr}]", split, gain, err, _l1(got[fr:fr + 1], ref), "golden", _pix(got[fr:fr + 1], ref))
            print(f"{name} 2x{part} streamed [{split}] frame {fr} gain {gain}: max-rel {err:.3e} (ref=golden)")
            assert err <= (1e-3 if split == "bf16x3" else 2e-4), (fr, err)      # the fp16 split: 5x inside the bar on these rows
        assert np.array_equal(got[0], got[n - 1]) and np.array_equal(got[3], got[n - 5]) and not np.array_equal(got[3], got[0])
        del shp, parts, f
    finally:
        H.set_conv_mode(old)
        torch.cuda.empty_cache()


# Gain ladders (tools/make_goldens.py ladder): the REFERENCE's inv_dist with out_costs.1 scaled x2 per rung until its softmax over
# the candidates is an arg-max in all but name (mean max-probability >= 0.995).  LADDER_BAR[arithmetic] = the mean max-probability
# up to which that arithmetic must stay inside the north star's 1e-3 on EVERY configuration (DESIGN.md "Precision modes": the
# deployer's rule); rungs beyond it are measured and recorded, not asserted.
# (the bf16 split -- not the default -- sits ON the bar at G16V's 0.944 rung: 9.3e-4 with the one-frame units of round 5's dispatcher,
# 1.05e-3 with round 6's (same products, another summation order): its asserted range ends below that rung)
LADDER_BAR = {"bf16x3": 0.94, "f32": 0.9945, "f16x3": 0.9945}


@pytest.mark.parametrize("name", list(FULL_CASES))
def test_full_size_gain_ladder_vs_reference_goldens(golden_dir, name, conv_mode):
    import parity_log
    case = FULL_CASES[name]
    cfg = case["cfg"]
    z = np.load(os.path.join(golden_dir, name + "_ladder.npz"))
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"]), f"{name}: regenerated inputs differ from the golden run's (host libm)"
    feats = _g(inp["feats"])
    for gain, mp in zip(z["gains"], z["mean_maxprob"]):
        hp = HotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=float(gain)), inp, device=DEV)
        got = hp(feats)[0].cpu().numpy()
        ref = z[f"inv_dist_g{gain:g}"]
        err, l1 = _rel(got, ref), _l1(got, ref)
        parity_log.record(f"{name}(ladder, max-prob {mp:.3f})", conv_mode, float(gain), err, l1, "golden", _pix(got, ref))
        print(f"{name} [{conv_mode}] ladder gain {gain:g} (mean max-prob {mp:.4f}): max-rel {err:.3e}")
        if mp <= LADDER_BAR[conv_mode]:
            assert err <= 1e-3, (float(gain), float(mp), err)
        del hp
    torch.cuda.empty_cache()


def test_precision_check_estimates_the_bf16_split_error(golden_dir):
    """HotPath.precision_check -- the deployer's per-checkpoint measurement: its bf16x3-vs-f16x3 discrepancy tracks the bf16
    split's TRUE error against the reference golden (within 25 %) up the gain ladder; it recommends the fp16 split (the library's
    default) both where the splits agree and where the exact mode has to arbitrate (a sharp softmax)."""
    case = FULL_CASES["full_G16V"]
    cfg = case["cfg"]
    z = np.load(os.path.join(golden_dir, "full_G16V_ladder.npz"))
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=1, grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"])
    feats = _g(inp["feats"])
    old = H.get_conv_mode()
    try:
        seen = set()
        z1 = np.load(os.path.join(golden_dir, "full_G16V.npz"))       # gain 1: the operating point (same inputs as the ladder's)
        assert str(z1["inputs_sha256"]) == str(z["inputs_sha256"])
        for gain in (1.0, 4.0):     # the bf16 split at 2.6e-4 and ~1e-3 of the reference (the 2.0 rung sits on the 5e-4 threshold)
            hp = HotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=gain), inp, device=DEV)
            chk = hp.precision_check(feats)
            H.set_conv_mode("bf16x3")
            true = _rel(hp(feats)[0].cpu().numpy(), (z1 if gain == 1.0 else z)[f"inv_dist_g{gain:g}"])
            assert abs(chk["bf16x3_vs_f16x3"] - true) <= 0.25 * true, (gain, chk, true)
            assert chk["recommended"] == "f16x3" and ("f16x3_vs_f32" in chk) == (true > 5e-4), (gain, chk, true)
            seen.add("f16x3_vs_f32" in chk)
            assert H.get_conv_mode() == "bf16x3"
            del hp
        assert seen == {False, True}           # one rung where the splits agree, one where the exact mode arbitrated
    finally:
        H.set_conv_mode(old)
        torch.cuda.empty_cache()


def test_precision_check_prefers_the_bf16_split_outside_fp16_range():
    """Features 300x too large: the cost volume (a variance) leaves fp16's range, the fp16 split clamps it, the bf16 split does not
    care -- precision_check sees the two splits disagree, lets the exact mode arbitrate and recommends bf16x3."""
    case = SMALL_CASES["std_d16_rand"]
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind="smooth", grid_mask_dtype="bool")
    feats = _g(inp["feats"] * np.float32(300.0))
    hp = HotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=1e-5), inp, device=DEV)
    old = H.get_conv_mode()
    try:
        chk = hp.precision_check(feats)
        print(chk)
        assert chk["bf16x3_vs_f16x3"] > chk["bar"] and chk["f16x3_vs_f32"] > 4 * chk["bf16x3_vs_f32"]
        assert chk["recommended"] == "bf16x3" and H.get_conv_mode() == old
    finally:
        H.set_conv_mode(old)


def test_unpickled_reference_modules_run_on_hip(golden_dir, request):
    import mvs_gi_amd
    assert mvs_gi_amd.install() in ("alias", "patch")
    request.addfinalizer(mvs_gi_amd.dropin.uninstall)       # the host tests of install() start from a process without the aliases
    hp = torch.load(os.path.join(golden_dir, "pickled_modules_tiny.pt"), weights_only=False)["hyper_parameters"]
    z = _load(golden_dir, "pickled_modules_tiny_io")
    cvb, reg, dr = (hp[k].eval().to(DEV) for k in ("cv_builder", "cv_regulator", "dist_regressor"))
    vol = cvb(_g(z["feats"]), _g(z["grids"]), _g(z["grid_masks"]), _g(z["masks"]))
    costs = reg(vol)
    inv, _ = dr(costs)
    assert _rel(vol.contiguous().cpu().numpy(), z["vol"]) <= 2e-5
    assert _rel(costs.contiguous().cpu().numpy(), z["costs"]) <= 1e-4
    assert _rel(inv.cpu().numpy(), z["inv_dist"]) <= 1e-3
    assert _rel(reg(_g(z["x_reg"])).contiguous().cpu().numpy(), z["y_reg"]) <= 1e-4


# ------------------------------------------------------------------------------ properties
def test_full_size_properties_batch_and_determinism():
    """Size-independent properties at BASELINE.json's G16V size, in the EXACT-fp32 mode (this file's autouse fixture): a batch
    of 2 equals two single-frame runs bit for bit (frames are independent), and the path is deterministic run to run.  In the
    default fp16 split the level-0 convs' form follows the batch (Winograd / direct) and a frame's bits with it: there the
    statement is a tolerance, tests/test_gpu_range.py::test_default_mode_frame_depends_on_its_launch_only_within_the_arithmetic;
    what frame sharding relies on -- the same launch geometry gives the same bits on every rank -- is tests/test_bench_sharding.py's."""
    from mvs_gi_amd.configs import CONFIGS
    cfg = CONFIGS["G16V"]
    inp = synth.make_inputs(cfg, seed=3, batch=1)
    w = synth.make_weights(cfg, seed=3)
    hp = HotPath(cfg, w, inp, device=DEV)
    rng = np.random.default_rng(0)
    f2 = _g(rng.standard_normal((2, *inp["feats"].shape[1:]), dtype=np.float32))
    a0, _ = hp(f2[:1].contiguous())
    a1, _ = hp(f2[1:].contiguous())
    both, _ = hp(f2)
    assert torch.equal(both[0], a0[0]) and torch.equal(both[1], a1[0])
    again, _ = hp(f2)
    assert torch.equal(both, again)
    assert torch.isfinite(both).all()
    lo, hi = hp.dist_regressor.inv_dist_idx_min, hp.dist_regressor.inv_dist_idx_max
    assert float(both.min()) >= lo - 1e-3 and float(both.max()) <= hi + 1e-3   # convex combination


def test_hipgraph_replay_equals_eager():
    """The captured hipGraph of the whole path replays to bit-identical results, also for new
    input contents written into the static buffer."""
    from mvs_gi_amd.configs import CONFIGS, DIST_8L
    cfg = CONFIGS["G16V"].scaled(feat_hw=(32, 128), mask_hw=(64, 256), cv_hw=(16, 64), dist_cands=DIST_8L)
    inp = synth.make_inputs(cfg, seed=7, batch=1)
    hp = HotPath(cfg, synth.make_weights(cfg, seed=7), inp, device=DEV)
    rng = np.random.default_rng(1)
    f1 = _g(rng.standard_normal((2, *inp["feats"].shape[1:]), dtype=np.float32))
    f2 = _g(rng.standard_normal((2, *inp["feats"].shape[1:]), dtype=np.float32))
    e1 = hp(f1)[0].clone()
    e2 = hp(f2)[0].clone()
    hp.capture(f1)
    g1 = hp.replay(f1)[0].clone()
    g2 = hp.replay(f2)[0].clone()
    g1b = hp.replay(f1)[0].clone()
    assert torch.equal(e1, g1) and torch.equal(e2, g2) and torch.equal(g1, g1b)
    assert not torch.equal(g1, g2)


@pytest.mark.parametrize("conv_mode", ["bf16x3"])
def test_streamed_hot_path_equals_one_stream(conv_mode):
    """StreamedHotPath (the batch in two parts on two HIP streams, fork / join; one hipGraph) returns, part by part, exactly what
    one HotPath returns for the whole batch -- eagerly and as a graph replay, also for new contents of the static input -- at a
    size where the register-stationary kernels and the split-padded hand-over run (module-owned buffers per replica)."""
    from mvs_gi_amd.configs import CONFIGS, DIST_8L
    from mvs_gi_amd.pipeline import StreamedHotPath
    old = H.get_conv_mode()
    H.set_conv_mode(conv_mode)
    try:
        cfg = CONFIGS["G16V"].scaled(feat_hw=(32, 128), mask_hw=(64, 256), cv_hw=(16, 64), dist_cands=DIST_8L)
        inp = synth.make_inputs(cfg, seed=7, batch=1)
        w = synth.make_weights(cfg, seed=7)
        hp = HotPath(cfg, w, inp, device=DEV)
        shp = StreamedHotPath(cfg, w, inp, device=DEV, n_streams=2)
        rng = np.random.default_rng(3)
        f1 = _g(rng.standard_normal((6, *inp["feats"].shape[1:]), dtype=np.float32))
        f2 = _g(rng.standard_normal((6, *inp["feats"].shape[1:]), dtype=np.float32))
        ref1, ref2 = [t.clone() for t in hp(f1)], [t.clone() for t in hp(f2)]
        for attempt in range(3):                               # repeated: a race between the parts' buffers would show as a flaky mismatch
            parts = shp(f1)
            torch.cuda.synchronize()
            assert len(parts) == 2
            assert torch.equal(torch.cat([p[0] for p in parts]), ref1[0]) and torch.equal(torch.cat([p[1] for p in parts]), ref1[1])
        shp.capture(f1)
        for f, ref in ((f1, ref1), (f2, ref2), (f1, ref1)):
            parts = shp.replay(f)
            torch.cuda.synchronize()
            assert torch.equal(torch.cat([p[0] for p in parts]), ref[0])
        with pytest.raises(ValueError):
            shp(f1[:5])                                        # five frames do not split into two equal parts
    finally:
        H.set_conv_mode(old)


def test_cold_compile_and_load_on_this_box(tmp_path):
    """The library normally travels with the tree (its source hash matches, so build() re-uses it); this compiles two of its
    translation units from scratch with this box's hipcc, links them and runs a kernel of the result on this GPU: the build
    recipe of __graft_entry__ works where the tests run, not only where the library was made."""
    import ctypes
    import subprocess
    import __graft_entry__ as g
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    for src in ("api.cpp", "layout.hip"):
        o = str(tmp_path / (src + ".o"))
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(g.CSRC, src), "-o", o],
                       check=True, timeout=600)
        objs.append(o)
    so = str(tmp_path / "libcold.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", so] + objs, check=True, timeout=600)
    lib = ctypes.CDLL(so)
    lib.mvsgi_abi_version.restype = ctypes.c_int
    from mvs_gi_amd import _lib
    assert lib.mvsgi_abi_version() == _lib.ABI_VERSION
    x = torch.arange(2 * 3 * 5, dtype=torch.float32, device=DEV).reshape(2, 3, 5)          # [B, C, V]
    y = torch.empty((2, 5, 3), dtype=torch.float32, device=DEV)
    lib.mvsgi_ncv_to_nvc_f32.restype = ctypes.c_int
    lib.mvsgi_ncv_to_nvc_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p]
    assert lib.mvsgi_ncv_to_nvc_f32(x.data_ptr(), y.data_ptr(), 2, 3, 5, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, x.permute(0, 2, 1))
    assert not g._needs_rebuild()          # and the travelling library is the one this tree's sources hash to


def test_bench_default_submission_line():
    """`python bench.py --full` at N = 1 (here with a small batch): the step is two parts on two HIP streams inside one
    hipGraph behind a settle phase; one JSON line with metric / value / roofline (+ traffic from profiles/pmc_traffic.json) / every
    launch attributed / parity against the oracle frame / cpu_baseline."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--batch", "8", "--steps", "3", "--warmup", "2", "--full", "--no-extras",
                        "--settle-seconds", "0.2", "--cpu-seconds", "1"], capture_output=True, text=True, env=env, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["unit"] == "frames/s" and d["value"] > 0 and d["vs_baseline"] is None and d["higher_is_better"]
    assert d["config"]["frames_per_gpu_per_step"] == 8 and d["config"]["streams"].startswith("2 independent parts of 4 frames")
    assert "hipGraph" in d["config"]["submission"] and "settle" in d["config"]
    assert d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] < 1 / 3 and d["roofline"]["peak"] == 2500.0
    assert d["parity"]["max_rel"] <= 1e-3 and d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1
    assert any(k.startswith("sweep_std") for k in d["kernels"]) and any(k.startswith("softargmin") for k in d["kernels"])


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """`python bench.py` without --full: the headline only (exactly --steps timed steps, ms_per_step), and --dump-outputs writes what
    the last timed step returned -- the same numbers this process computes from the same seeded frames through the same path."""
    import json
    import subprocess
    import sys
    import bench
    from mvs_gi_amd.configs import CONFIGS
    from mvs_gi_amd.pipeline import StreamedHotPath
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out_dir = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--batch", "8", "--steps", "4", "--warmup", "2",
                        "--settle-seconds", "0.2", "--dump-outputs", out_dir], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["value"] > 0 and d["higher_is_better"] and d["unit"] == "frames/s" and d["dtype"].startswith("f16x3")
    assert abs(d["value"] - 8 * 4 / (d["ms_per_step"] * 4e-3)) / d["value"] < 0.01
    assert not {"roofline", "kernels", "parity", "cpu_baseline", "extras", "configs"} & set(d)
    assert d["outputs_dumped"]["frames"] == list(range(8))          # 8 G16V frames fit in bench.DUMP_BYTES
    files = sorted(os.listdir(out_dir))
    assert files == ["inv_dist.npy", "norm_costs.npy"]
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64e6
    got = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert got["inv_dist"].dtype == np.float32 and got["inv_dist"].shape == (8, 1, 160, 640)
    assert got["norm_costs"].dtype == np.float32 and got["norm_costs"].shape == (8, 16, 160, 640)
    H.set_conv_mode("f16x3")      # bench.py's default --mode (this file's autouse fixture restores its own)
    cfg = CONFIGS["G16V"]
    x = bench.draw_feats(8,(1, cfg.num_cams, cfg.feat_chs, *cfg.feat_hw), np.random.default_rng(1000), np)
    shp = StreamedHotPath(cfg, synth.make_weights(cfg, seed=0), synth.make_inputs(cfg, seed=0, batch=1), device=DEV, n_streams=2)
    parts = shp(bench.upload_feats(x, torch.device(DEV), torch))
    torch.cuda.synchronize()
    for i, name in enumerate(bench.OUTPUT_NAMES):
        ref = torch.cat([p[i] for p in parts]).cpu().numpy()
        assert np.abs(got[name] - ref).max() <= 1e-6 * np.abs(ref).max(), name


def test_bench_two_ranks_frame_sharded_on_one_gpu():
    """bench.py's N>1 path end to end (rendezvous, per-rank frames, barrier, max-over-ranks, one JSON
    line from rank 0): two ranks share this box's single GPU, control plane over gloo."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MVSGI_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29655")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29655", os.path.join(root, "bench.py"),
                        "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "2", "--backend", "gloo", "--settle-seconds", "0", "--full"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0)"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 3
    assert d["value"] > 0 and abs(d["value"] - 2 * 2 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 0.02
    assert "cpu_baseline" not in d and d["roofline"]["bound"] == "mfma"
    assert d["parity"]["max_rel"] <= 1e-3 and d["parity"]["frames"] == 1        # a multi-rank line carries an error figure too


def test_bench_self_launches_its_ranks():
    """`python bench.py --gpus 4` with no WORLD_SIZE in the environment (how a driver that does not use torchrun would call
    it) starts its own ranks as a child torch.distributed.run and relays rank 0's single line; the line says how many ranks
    and which device ordinals really ran, and attributes the HBM-bound launches (sweep, soft-argmin) beside the convs.
    Four ranks: a GPU box admits at most six processes on its card, this test process included (the eight-rank control plane runs over gloo on the CPU,
    tests/test_bench_sharding.py::test_control_plane_world8_gloo)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["MVSGI_BENCH_SHARE_GPU"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--steps", "3", "--warmup", "1",
                        "--batch", "1", "--backend", "gloo", "--settle-seconds", "0", "--full"], capture_output=True, text=True, env=env, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0)"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["n_ranks_seen"] == 4 and d["devices"] == [0] * 4
    assert d["value"] > 0 and d["scaling"] == "weak" and d["parity"]["max_rel"] <= 1e-3
    hbm = {k: v for k, v in d["kernels"].items() if v.get("bound") == "hbm"}
    assert any(k.startswith("sweep_std") for k in hbm) and any(k.startswith("softargmin") for k in hbm) and any(k.startswith("conv3d_head") for k in hbm)
    assert all(v["GBps"] > 0 for v in hbm.values())
    assert d["roofline"]["attributed_time_frac_of_step"] > 0.2      # (four ranks share the card here: each rank's wall time holds the others' kernels)


# ------------------------------------------------------------------------------ feature extractor (§8(f) rank 1)
@pytest.mark.parametrize("shape", [(2, 16, 16, 20, 36, 1, True), (1, 16, 16, 33, 47, 1, False), (2, 16, 16, 24, 40, 2, False),
                                   (1, 32, 32, 17, 30, 1, True), (1, 16, 64, 16, 32, 2, False), (1, 64, 64, 12, 20, 1, True),
                                   # the channel / stride rows of exact_cases.CONV2D_WIDE_SHAPES: Cout / 16 of 3 and 5 against the two-tile templates
                                   (1, 32, 32, 9, 21, 2, False), (1, 48, 48, 9, 21, 1, True), (1, 48, 48, 10, 22, 2, False),
                                   (1, 80, 80, 5, 19, 1, False), (1, 16, 32, 9, 21, 1, False)])
def test_conv2d_bf16x3_and_direct_vs_aten(shape):
    B, Cin, Cout, Hh, W, stride, res = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((B, Cin, Hh, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    y = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, stride=stride, padding=1)
    y = y * torch.from_numpy(scale).view(1, -1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1)
    r = rng.standard_normal(tuple(y.shape)).astype(np.float32) if res else None
    if res:
        y = y + torch.from_numpy(r)
    yref = torch.where(y > 0, y, y * 0.01).numpy()
    xg = _g(x).permute(0, 2, 3, 1).contiguous()
    rg = None if r is None else _g(r).permute(0, 2, 3, 1).contiguous()
    wg = _g(w)
    yd = H.conv2d(xg, wg, None, _g(scale), _g(shift), res=rg, stride=stride, impl=H.CONV_DIRECT)
    assert _rel(yd.permute(0, 3, 1, 2).cpu().numpy(), yref) <= 2e-5
    assert "bf16x3" in H.conv2d_variant(Cin, Cout, 3, stride, H.CONV_BF16X3)
    yb = H.conv2d(xg, wg, H.pack_conv2d_weights_bf16x3(wg), _g(scale), _g(shift), res=rg, stride=stride, impl=H.CONV_BF16X3)
    assert _rel(yb.permute(0, 3, 1, 2).cpu().numpy(), yref) <= 1e-4
    wpf = H.pack_conv2d_weights_f32(wg)
    if wpf is not None:
        assert "conv3d_mfma_kernel" in H.conv2d_variant(Cin, Cout, 3, stride, H.CONV_MFMA)
        ym = H.conv2d(xg, wg, wpf, _g(scale), _g(shift), res=rg, stride=stride, impl=H.CONV_MFMA)
        assert _rel(ym.permute(0, 3, 1, 2).cpu().numpy(), yref) <= 2e-5


def test_conv2d_batch_beyond_32bit_offsets_matches_its_halves():
    """A 192-image extractor batch (B=64 frames x 3 cameras) exceeds the one-volume 32-bit byte offsets; the entry then
    walks the images as frames with 64-bit bases.  Same numbers as the two halves run through the one-volume path."""
    g = torch.Generator(device="cuda").manual_seed(5)
    N, Hh, Ww = 132, 256, 1024                                   # 132*256*1024*16 > 2^29 elements
    x = torch.randn(N, Hh, Ww, 16, device="cuda", generator=g)
    w = torch.randn(16, 16, 3, 3, device="cuda", generator=g) * 0.1
    scale = torch.rand(16, device="cuda", generator=g) + 0.5
    shift = torch.randn(16, device="cuda", generator=g) * 0.1
    wp = H.pack_conv2d_weights_bf16x3(w)
    for stride in (1, 2):
        y = H.conv2d(x, w, wp, scale, shift, stride=stride, impl=H.CONV_BF16X3)
        h = N // 2
        for lo in (0, h):
            yh = H.conv2d(x[lo:lo + h], w, wp, scale, shift, stride=stride, impl=H.CONV_BF16X3)
            assert torch.equal(y[lo:lo + h], yh)
        del y, yh


def test_conv2d_stem_5x5_nchw_input():
    rng = np.random.default_rng(12)
    x = rng.random((2, 3, 30, 52)).astype(np.float32)
    w = (rng.standard_normal((16, 3, 5, 5)) / np.sqrt(75)).astype(np.float32)
    yref = F.leaky_relu(F.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, stride=2, padding=2), 0.01).numpy()
    y = H.conv2d(_g(x), _g(w), None, torch.ones(16, device=DEV), torch.zeros(16, device=DEV), stride=2, in_nchw=True)
    assert _rel(y.permute(0, 3, 1, 2).cpu().numpy(), yref) <= 2e-5


@pytest.mark.parametrize("hw", [(30, 52), (37, 132), (64, 256), (5, 4), (21, 30)])      # W = 30: not a multiple of 4 -> the fp32 stem
def test_conv2d_stem_uint8_on_the_matrix_cores(hw):
    """uint8 HWC camera images through the 5x5 stride-2 stem: the MFMA kernel (exact pixels, w / 255 in three bf16 pieces)
    against float64 of the reference's arithmetic (x.float() / 255 -> conv -> BN -> LeakyReLU) and against the LDS-tiled
    fp32 kernel; ragged tile edges, a one-tile image and a batch."""
    rng = np.random.default_rng(21)
    Hh, Ww = hw
    u8 = rng.integers(0, 256, (3, Hh, Ww, 3), dtype=np.uint8)
    w = (rng.standard_normal((16, 3, 5, 5)) / np.sqrt(75)).astype(np.float32)
    scale = (rng.random(16) + 0.5).astype(np.float32)
    shift = (rng.standard_normal(16) * 0.1).astype(np.float32)
    x64 = torch.from_numpy(u8).permute(0, 3, 1, 2).double() / 255.0
    ref = F.conv2d(x64, torch.from_numpy(w).double(), None, stride=2, padding=2)
    ref = F.leaky_relu(ref * torch.from_numpy(scale).double().view(1, -1, 1, 1) + torch.from_numpy(shift).double().view(1, -1, 1, 1), 0.01).numpy()
    wg = _g(w)
    wp = H.pack_conv2d_stem_weights(wg)
    assert wp is not None
    y_mfma = H.conv2d(_g(u8), wg, wp, _g(scale), _g(shift), stride=2).permute(0, 3, 1, 2).cpu().numpy()
    y_valu = H.conv2d(_g(u8), wg, None, _g(scale), _g(shift), stride=2).permute(0, 3, 1, 2).cpu().numpy()
    assert y_mfma.shape == ref.shape
    assert _rel(y_mfma, ref) <= 5e-7            # a few fp32 ulps: exact products, fp32 accumulation
    assert _rel(y_valu, ref) <= 5e-6
    assert _rel(y_mfma, y_valu) <= 5e-6


def test_feature_extractor_and_end_to_end_vs_reference(golden_dir, conv_mode):
    """SimpleFeatExtraction drop-in and the imgs -> inv_dist composition against the reference's outputs."""
    from mvs_gi_amd.configs import CONFIGS, DIST_8L
    z = _load(golden_dir, "extractor_small")
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32), dist_cands=DIST_8L)
    seed = 8
    imgs = synth.make_images(cfg, seed=seed, batch=2)
    inp = synth.make_inputs(cfg, seed=seed, batch=2)
    assert synth.digest({"imgs": imgs}) == str(z["imgs_sha256"])
    fe = dropin.SimpleFeatExtraction(in_size=(64, 256), in_chs=3, chs=16, k_sz=3, layers=[5, 10])
    fe.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_extractor_weights(seed).items()}, strict=True)
    hp = HotPath(cfg, synth.make_weights(cfg, seed=seed), inp, device=DEV)
    model = dropin.SphericalSweepStereoBase(fe.eval().to(DEV), hp.cv_builder, hp.cv_regulator, hp.dist_regressor)
    with torch.no_grad():
        feats = model.extract_features(_g(imgs))
        inv, _ = model(_g(imgs), hp.grids, hp.grid_masks, hp.masks)
    assert tuple(feats.shape) == tuple(z["feats"].shape)
    ferr = _rel(feats.contiguous().cpu().numpy(), z["feats"])
    ierr = _rel(inv.cpu().numpy(), z["inv_dist"])
    print(f"extractor [{conv_mode}]: feats max-rel {ferr:.3e}, end-to-end inv_dist max-rel {ierr:.3e}")
    assert ferr <= (2e-5 if conv_mode == "f32" else 2e-4)
    assert ierr <= 1e-3


def test_feature_extractor_full_size_sample(golden_dir, conv_mode):
    from mvs_gi_amd.configs import CONFIGS
    z = _load(golden_dir, "extractor_full_sample")
    imgs = synth.make_images(CONFIGS["G16V"], seed=8, batch=1)
    assert synth.digest({"imgs": imgs}) == str(z["imgs_sha256"])
    fe = dropin.SimpleFeatExtraction(in_size=(512, 2048), in_chs=3, chs=16, k_sz=3, layers=[5, 10])
    fe.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_extractor_weights(8).items()}, strict=True)
    with torch.no_grad():
        f = fe.eval().to(DEV)(_g(imgs[0]))
    assert tuple(f.shape) == (3, 16, 128, 512)
    err = _rel(f[:, :, ::8, ::8].contiguous().cpu().numpy(), z["feats_8x8"])
    print(f"extractor full size [{conv_mode}]: max-rel {err:.3e}")
    assert err <= (2e-5 if conv_mode == "f32" else 2e-4)
    assert abs(float(f.abs().mean()) - float(z["feats_abs_mean"])) / float(z["feats_abs_mean"]) < 1e-4


def test_inference_pipeline_uint8_in_metric_out(golden_dir, conv_mode):
    """uint8 HWC camera images -> inv_dist / bf on the host, against the reference's
    preprocess_imgs / model / postprocess_imgs chain (api/inference_class.py:97-127)."""
    from mvs_gi_amd.configs import CONFIGS, DIST_8L
    from mvs_gi_amd.pipeline import InferencePipeline
    z = _load(golden_dir, "pipeline_u8")
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32), dist_cands=DIST_8L)
    seed = 8
    w = synth.make_weights(cfg, seed=seed)
    w["feature_extractor"] = synth.make_extractor_weights(seed)
    inp = synth.make_inputs(cfg, seed=seed, batch=1)
    pipe = InferencePipeline(cfg, w, inp, device=DEV)
    out = pipe({"imgs": [im for im in z["imgs_u8"]]})
    assert out.shape == z["inv_dist_over_bf"].shape == (16, 64)
    err = _rel(out, z["inv_dist_over_bf"])
    print(f"pipeline u8 [{conv_mode}]: max-rel {err:.3e}")
    assert err <= 1e-3
    # the whole chain as one hipGraph: the same numbers, also for other images of that shape, and through __call__
    imgs = torch.from_numpy(np.stack(list(z["imgs_u8"]), 0)).to(DEV)
    pipe.capture(imgs)
    assert np.array_equal(pipe.replay(imgs).squeeze().cpu().numpy(), out)
    other = imgs.flip(0).contiguous()
    eager = pipe.forward_device(other).squeeze().cpu().numpy()
    assert np.array_equal(pipe.replay(other).squeeze().cpu().numpy(), eager)
    assert np.array_equal(pipe({"imgs": [im for im in z["imgs_u8"]]}), out)


def test_inference_pipeline_with_sphere_extractor(conv_mode):
    """The G16VV front end (sphere-conv final layer) through the same facade: uint8 images in, inv_dist / bf out,
    against the oracle chain (sphere extractor -> hot path); deform_conv2d itself is restated, see oracle header."""
    from mvs_gi_amd.configs import CONFIGS, DIST_8L
    from mvs_gi_amd.pipeline import InferencePipeline
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32), dist_cands=DIST_8L)
    seed = 9
    w = synth.make_weights(cfg, seed=seed)
    w["feature_extractor"] = _sphere_weights(seed)
    inp = synth.make_inputs(cfg, seed=seed, batch=1)
    pipe = InferencePipeline(cfg, w, inp, device=DEV, extractor="sphere")
    rng = np.random.default_rng(seed)
    imgs_u8 = rng.integers(0, 256, (cfg.num_cams, 64, 256, 3), dtype=np.uint8)
    out = pipe({"imgs": [im for im in imgs_u8]})
    t = O.to_torch(inp)
    p = {k_: torch.from_numpy(v) for k_, v in w["feature_extractor"].items()}
    p["final_layer.blk.0.offset"] = pipe.feature_extractor.final_layer.blk[0].offset.cpu()
    with torch.no_grad():
        x = torch.from_numpy(imgs_u8).permute(0, 3, 1, 2).float() / 255.0              # inference_class.py:104-107
        f = O.sphere_feature_extractor(x, p)
        ref = O.hot_path(f.unsqueeze(0), t["grids"], t["grid_masks"], t["masks"], O.to_torch(w), cfg.builder,
                         cfg.dist_cands, cfg.bf, cfg.interp_scale_factor, cfg.pre_interp)
    ref = (ref / cfg.bf).squeeze().numpy()
    assert out.shape == ref.shape == (16, 64)
    assert _rel(out, ref) <= 1e-3


# ------------------------------------------------------------------ sampling-grid generator
def test_sweep_grid_generator_vs_reference_goldens(golden_dir):
    """HIP closed forms (dropin/sweep_grids.py, reference class names) vs the reference's own outputs.
    Tolerances: device sin/cos/atan2/sqrt are within ~2 ulp of the host libm; projections are compared
    where they are well conditioned (inside the field of view, away from the atan2 branch cut).  The per-element check -- bit for
    bit for the transform and the double sphere, ulp bounds for the trigonometric kernels, nothing masked out -- is
    tests/test_gpu_grids_exact.py."""
    from mvs_gi_amd.dropin import sweep_grids as SG
    z = _load(golden_dir, "sweep_grids")
    for name in ("g16", "e8_full_sphere"):
        shape = tuple(int(v) for v in z[name + "_shape"])
        rm = SG.RayMaker_UEPanorama(z[name + "_dist"], tuple(z[name + "_lon"]), tuple(z[name + "_lat"]), device=DEV)
        rays = rm.make_rays_for_candidates(shape)
        ref_rays = z[name + "_rays"]
        assert rays.shape == ref_rays.shape and _rel(rays.cpu().numpy(), ref_rays) <= 2e-6
        ds, eq = SG.DoubleSphereSampleGridMaker(), SG.EquirectangularSampleGridMaker()
        for i, pose in enumerate(z[name + "_poses"]):
            inv = torch.linalg.inv(torch.from_numpy(pose)).to(torch.float32)
            ref_pts = z[f"{name}_pts{i}"]
            pts = SG.transform_3D_points_torch(inv.unsqueeze(0).to(DEV), _g(ref_rays).unsqueeze(0))
            assert _rel(pts.cpu().numpy(), ref_pts) <= 2e-6
            gp = _g(ref_pts)                                   # projections on the reference's exact points
            g, m = ds.make_grid(gp)
            rg, rm_ = z[f"{name}_ds_grid{i}"], z[f"{name}_ds_mask{i}"]
            x, y, zz = ref_pts[:, 0], ref_pts[:, 1], ref_pts[:, 2]
            d1 = np.sqrt(x * x + y * y + zz * zz)
            edge = np.abs(zz + ds.w2 * d1) < 1e-5 * d1        # on the field-of-view boundary either answer is right
            assert np.array_equal(m.cpu().numpy()[~edge], rm_[~edge])
            well = rm_ & (np.abs(rg).max(-1) < 4)
            assert well.sum() > 100 and np.abs(g.cpu().numpy() - rg)[well].max() <= 2e-5
            e = eq.make_grid(gp).cpu().numpy()
            cut = (x < 0) & (np.abs(zz) < 1e-4 * np.abs(x))    # atan2 branch cut: u flips between -1 and +1
            assert np.abs(e - z[f"{name}_eq_grid{i}"])[~cut].max() <= 2e-6
        # the composed rig call: layout the cv_builder takes
        grids, gms = SG.make_sweep_grids(rm, [ds] * len(z[name + "_poses"]), list(z[name + "_poses"]), shape)
        D = len(z[name + "_dist"])
        assert tuple(grids.shape) == (1, len(z[name + "_poses"]), D, *shape, 2)
        assert tuple(gms.shape) == (1, len(z[name + "_poses"]), D, *shape, 1) and gms.dtype == torch.bool
        ok = z[f"{name}_ds_mask0"][0] & (np.abs(z[f"{name}_ds_grid0"][0]).max(-1) < 4)
        assert np.abs(grids[0, 0].cpu().numpy() - z[f"{name}_ds_grid0"][0])[ok].max() <= 5e-5
    g2, m2 = SG.DoubleSphereSampleGridMaker(params=[0.1, 0.45, 300.0, 310.0, 320.0, 240.0],
                                            calib_shape=[480, 640]).make_grid(_g(z["g16_pts1"]))
    well = z["ds2_mask"] & (np.abs(z["ds2_grid"]).max(-1) < 4)
    assert np.abs(g2.cpu().numpy() - z["ds2_grid"])[well].max() <= 2e-5


# ------------------------------------------------------------------ sphere convolution
@pytest.mark.parametrize("case", [
    # (N, Cin, Cout, H, W, k, stride, pad, dil, res, slope)
    (2, 16, 16, 12, 40, 3, 1, 1, 1, True, 0.01),       # quad-lane kernel, SphereConvBlk-like
    (1, 16, 16, 9, 21, 5, 2, 2, 1, False, 1.0),        # 5x5 stride 2, ragged pixel count
    (1, 16, 16, 10, 16, 3, 1, 2, 2, False, 0.0),       # dilation 2, ReLU
    (2, 8, 12, 7, 11, 3, 1, 1, 1, True, 0.01),         # generic kernel (other channel counts)
])
def test_deform_conv2d_vs_oracle(case):
    N, Cin, Cout, Hh, W, k, st, pad, dil, res, slope = case
    rng = np.random.default_rng(sum(case[:9]))
    x = rng.standard_normal((N, Cin, Hh, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(k * k * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.normal(0, 0.2, Cout).astype(np.float32)
    Ho = (Hh + 2 * pad - (dil * (k - 1) + 1)) // st + 1
    Wo = (W + 2 * pad - (dil * (k - 1) + 1)) // st + 1
    # offsets: sub-pixel, a few pixels, far outside, exactly on the -1 / H borders
    off = rng.normal(0, 1.5, (N, 2 * k * k, Ho, Wo)).astype(np.float32)
    off[:, :, 0, :] = np.round(off[:, :, 0, :])
    off[:, 0, 1, :] = -50.0
    off[:, 3, 2 % Ho, :] = 1e4
    r = rng.standard_normal((N, Cout, Ho, Wo)).astype(np.float32) if res else None
    y = O.deform_conv2d(torch.from_numpy(x), torch.from_numpy(off), torch.from_numpy(w), None, (st, st), (pad, pad), (dil, dil))
    y = y * torch.from_numpy(scale).view(1, -1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1)
    if res:
        y = y + torch.from_numpy(r)
    yref = torch.where(y > 0, y, y * slope).numpy()
    xg = _g(x).permute(0, 2, 3, 1).contiguous()
    rg = _g(r).permute(0, 2, 3, 1).contiguous() if res else None
    got = H.deform_conv2d(xg, _g(off), H.pack_deform_conv2d_weights(_g(w)), _g(scale), _g(shift), (k, k), (st, st),
                          (pad, pad), (dil, dil), res=rg, neg_slope=slope)
    assert _rel(got.permute(0, 3, 1, 2).cpu().numpy(), yref) <= 2e-5
    # a single shared offset field (what SphereConvEquirect2d registers) == the same field per image
    shared = H.deform_conv2d(xg, _g(off[:1]), H.pack_deform_conv2d_weights(_g(w)), _g(scale), _g(shift), (k, k),
                             (st, st), (pad, pad), (dil, dil), neg_slope=slope)
    per = H.deform_conv2d(xg, _g(np.repeat(off[:1], N, 0)), H.pack_deform_conv2d_weights(_g(w)), _g(scale), _g(shift),
                          (k, k), (st, st), (pad, pad), (dil, dil), neg_slope=slope)
    assert torch.equal(shared, per)


def _sphere_weights(seed, chs=16):
    sd = synth.make_extractor_weights(seed, chs=chs)
    out = {}
    for k_, v in sd.items():
        k_ = k_.replace("final_layer.conv_layer.", "final_layer.blk.0.").replace("final_layer.norm_layer.", "final_layer.blk.1.")
        out[k_] = v
    return out


def test_sphere_feature_extractor_vs_oracle(conv_mode):
    """SphereEquirectFeatExtraction (G16VV's extractor, sphere_feature_extractor.py:8-83) as HIP: 2-D MFMA convs +
    the deformable final layer with the reference's offset field, vs the oracle (deform_conv2d restated from
    torchvision's definition: parity unpinned for that operator, offsets pinned)."""
    Hh, W = 64, 256
    fe = dropin.SphereEquirectFeatExtraction(in_size=(Hh, W), in_chs=3, chs=16, k_sz=3, layers=[5, 10])
    sd = {k_: torch.from_numpy(v) for k_, v in _sphere_weights(3).items()}
    missing = fe.load_state_dict(sd, strict=False)
    assert missing.missing_keys == ["final_layer.blk.0.offset"] and not missing.unexpected_keys
    assert tuple(fe.final_layer.blk[0].offset.shape) == (1, 18, Hh // 4, W // 4)
    fe = fe.eval().to(DEV)
    rng = np.random.default_rng(12)
    imgs = rng.random((3, 3, Hh, W), dtype=np.float32)
    with torch.no_grad():
        f = fe(_g(imgs))
    p = dict(sd)
    p["final_layer.blk.0.offset"] = fe.final_layer.blk[0].offset.cpu()
    with torch.no_grad():
        ref = O.sphere_feature_extractor(torch.from_numpy(imgs), p).numpy()
    assert f.shape == ref.shape
    assert _rel(f.cpu().numpy(), ref) <= (2e-5 if conv_mode == "f32" else 2e-4)      # the extractor is bf16-split in both split modes
    # module-level pieces keep the reference's call signatures
    blk = fe.final_layer
    x = torch.from_numpy(rng.standard_normal((2, 16, Hh // 4, W // 4)).astype(np.float32))
    with torch.no_grad():
        y = blk(_g(x), res=_g(x))
    p2 = {"fl." + k_[len("final_layer."):]: v for k_, v in p.items() if k_.startswith("final_layer.")}
    yref = O.sphere_block2d(x, p2, "fl", res=x).numpy()
    assert _rel(y.cpu().numpy(), yref) <= 2e-5


# ------------------------------------------------------------------ fused residual block of the extractor
@pytest.mark.parametrize("shape", [(2, 30, 45), (1, 14, 14), (3, 64, 256), (1, 9, 100), (5, 29, 15)])
def test_fused_resblock2d_vs_two_convs(shape):
    """mvsgi_resblock2d_f32 (both 3x3 convs of ResConvBlk2d in one launch, intermediate in LDS) vs the oracle's two
    conv blocks and vs the two-launch HIP path; images smaller / larger than a 14x14 brick, ragged edges."""
    N, Hh, W = shape
    rng = np.random.default_rng(sum(shape))
    p = {}
    for name in ("blk1", "blk2"):
        p[f"{name}.conv_layer.weight"] = (rng.standard_normal((16, 16, 3, 3)) / 12).astype(np.float32)
        p[f"{name}.norm_layer.weight"] = rng.uniform(0.5, 1.5, 16).astype(np.float32)
        p[f"{name}.norm_layer.bias"] = rng.normal(0, 0.3, 16).astype(np.float32)      # non-zero: conv1 of zero padding is not zero
        p[f"{name}.norm_layer.running_mean"] = rng.normal(0, 0.1, 16).astype(np.float32)
        p[f"{name}.norm_layer.running_var"] = rng.uniform(0.5, 1.5, 16).astype(np.float32)
    x = rng.standard_normal((N, 16, Hh, W)).astype(np.float32)
    pt = {k_: torch.from_numpy(v) for k_, v in p.items()}
    xt = torch.from_numpy(x)
    ref = O.conv_block2d(O.conv_block2d(xt, pt, "blk1"), pt, "blk2", res=xt).numpy()
    blk = dropin.ResConvBlk2d(16, 16, 3, activation=torch.nn.LeakyReLU(), norm_layer=torch.nn.BatchNorm2d(16))
    blk.load_state_dict(pt, strict=False)
    blk = blk.eval().to(DEV)
    old_mode = H.get_conv_mode()
    try:
        H.set_conv_mode("bf16x3")
        with torch.no_grad():
            y = blk(_g(x))
            from mvs_gi_amd.dropin import feature_extractor as FE
            xn = _g(x).permute(0, 2, 3, 1).contiguous()
            two = FE.lower_conv2d_block(blk.blk2).run(FE.lower_conv2d_block(blk.blk1).run(xn), res=xn)
    finally:
        H.set_conv_mode(old_mode)
    assert _rel(y.cpu().numpy(), ref) <= 1e-4
    assert _rel(y.permute(0, 2, 3, 1).cpu().numpy(), two.cpu().numpy()) <= 2e-5


# ------------------------------------------------- the residual block on pre-split activations (csrc/resblock2d_rs.hip)
def _resblk_params(rng):
    p = {}
    for name in ("blk1", "blk2"):
        p[f"{name}.conv_layer.weight"] = (rng.standard_normal((16, 16, 3, 3)) / 12).astype(np.float32)
        p[f"{name}.norm_layer.weight"] = rng.uniform(0.5, 1.5, 16).astype(np.float32)
        p[f"{name}.norm_layer.bias"] = rng.normal(0, 0.3, 16).astype(np.float32)
        p[f"{name}.norm_layer.running_mean"] = rng.normal(0, 0.1, 16).astype(np.float32)
        p[f"{name}.norm_layer.running_var"] = rng.uniform(0.5, 1.5, 16).astype(np.float32)
    return p


def test_split2d_format_round_trip_and_border():
    rng = np.random.default_rng(5)
    x = _g(rng.standard_normal((3, 5, 7, 16), dtype=np.float32) * 10)
    s = H.f32_to_split2d(x)
    assert tuple(s.shape) == (3, 9, 11, 64) and s.dtype == torch.uint8
    back = H.split2d_to_f32(s)
    assert float(((back - x).abs() / x.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16      # hi + lo keeps 16-17 significant bits
    border = s.clone()
    border[:, 2:-2, 2:-2] = 0
    assert int(border.count_nonzero()) == 0


@pytest.mark.parametrize("shape", [(2, 30, 45), (1, 14, 30), (3, 64, 256), (1, 9, 100), (5, 29, 15), (1, 1, 1), (2, 15, 31), (9, 44, 91), (3, 200, 500)])
def test_resblock2d_split_vs_oracle(shape):
    """mvsgi_resblock2d_split (ResConvBlk2d in one launch on 2-D split-padded activations, LDS-DMA staging, skip from LDS) vs
    the oracle's two conv blocks: images smaller / larger than a 14x30 brick, ragged edges, more bricks than resident
    workgroups (3 x 200 x 500: a persistent walk of several bricks per workgroup); both output formats; the output buffer's zero border stays zero."""
    N, Hh, W = shape
    rng = np.random.default_rng(sum(shape) + 1)
    p = _resblk_params(rng)
    x = rng.standard_normal((N, 16, Hh, W)).astype(np.float32)
    pt = {k_: torch.from_numpy(v) for k_, v in p.items()}
    xt = torch.from_numpy(x)
    ref = O.conv_block2d(O.conv_block2d(xt, pt, "blk1"), pt, "blk2", res=xt).permute(0, 2, 3, 1).numpy()
    from mvs_gi_amd.dropin import feature_extractor as FE
    blk = dropin.ResConvBlk2d(16, 16, 3, activation=torch.nn.LeakyReLU(), norm_layer=torch.nn.BatchNorm2d(16))
    blk.load_state_dict(pt, strict=False)
    blk = blk.eval().to(DEV)
    L1, L2 = FE.lower_conv2d_block(blk.blk1), FE.lower_conv2d_block(blk.blk2)
    w1, w2 = L1.rs_weights(), L2.rs_weights()
    xs = H.f32_to_split2d(_g(x).permute(0, 2, 3, 1).contiguous())
    y32 = H.resblock2d_split(xs, w1, L1.shift, w2, L2.shift, L1.neg_slope)
    out = H.split2d_buffer(N, Hh, W, xs.device)
    ys = H.resblock2d_split(xs, w1, L1.shift, w2, L2.shift, L1.neg_slope, out_split=out)
    assert _rel(y32.cpu().numpy(), ref) <= 1e-4
    assert _rel(H.split2d_to_f32(ys).cpu().numpy(), ref) <= 1e-4
    border = ys.clone()
    border[:, 2:-2, 2:-2] = 0
    assert int(border.count_nonzero()) == 0
    # a chain of two blocks through the split format = the same two blocks through fp32
    y2 = H.resblock2d_split(ys, w1, L1.shift, w2, L2.shift, L1.neg_slope)
    reft = torch.from_numpy(ref).permute(0, 3, 1, 2)
    ref2 = O.conv_block2d(O.conv_block2d(reft, pt, "blk1"), pt, "blk2", res=reft).permute(0, 2, 3, 1).numpy()
    assert _rel(y2.cpu().numpy(), ref2) <= 2e-4


def test_conv2d_out_split2d_matches_fp32_output():
    """The stem (fp32 NCHW and uint8 HWC images) and the stride-2 / stride-1 3x3 layers writing the 2-D split-padded format:
    the same values as their fp32 outputs, split (hi + lo: 16-17 bits)."""
    rng = np.random.default_rng(11)
    from mvs_gi_amd.dropin import feature_extractor as FE
    stem = dropin.BaseConvBlk2d(3, 16, 5, stride=2, activation=torch.nn.LeakyReLU(), norm_layer=torch.nn.BatchNorm2d(16)).eval().to(DEV)
    mid = dropin.BaseConvBlk2d(16, 16, 3, stride=2, activation=torch.nn.LeakyReLU(), norm_layer=torch.nn.BatchNorm2d(16)).eval().to(DEV)
    one = dropin.BaseConvBlk2d(16, 16, 3, stride=1, activation=torch.nn.LeakyReLU(), norm_layer=torch.nn.BatchNorm2d(16)).eval().to(DEV)
    with torch.no_grad():
        for m in (stem, mid, one):
            m.norm_layer.running_mean.normal_(0, 0.1)
            m.norm_layer.running_var.uniform_(0.5, 1.5)
            m.norm_layer.bias.normal_(0, 0.3)
    old_mode = H.get_conv_mode()
    try:
        H.set_conv_mode("bf16x3")
        for imgs, nchw in ((_g(rng.random((2, 3, 36, 52), dtype=np.float32)), True),
                           (torch.from_numpy(rng.integers(0, 256, (2, 36, 52, 3), dtype=np.uint8)).to(DEV), True)):
            L = FE.lower_conv2d_block(stem)
            y = L.run(imgs, in_nchw=nchw)
            ys = L.run(imgs, in_nchw=nchw, out_split=H.split2d_buffer(2, 18, 26, imgs.device))
            back = H.split2d_to_f32(ys)
            assert float(((back - y).abs() / y.abs().clamp_min(1e-20)).max()) <= 2.0 ** -15
        x = _g(rng.standard_normal((3, 37, 53, 16), dtype=np.float32))
        for m, (ho, wo) in ((mid, (19, 27)), (one, (37, 53))):
            L = FE.lower_conv2d_block(m)
            y = L.run(x)
            ys = L.run(x, out_split=H.split2d_buffer(3, ho, wo, x.device))
            back = H.split2d_to_f32(ys)
            assert float(((back - y).abs() / y.abs().clamp_min(1e-20)).max()) <= 2.0 ** -15
            border = ys.clone()
            border[:, 2:-2, 2:-2] = 0
            assert int(border.count_nonzero()) == 0
    finally:
        H.set_conv_mode(old_mode)


@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 16, 32), (3, 17, 33), (1, 9, 100), (5, 64, 256), (2, 35, 47), (4, 256, 1024)])
def test_conv2d_s2_split_vs_reference_conv(shape):
    """The extractor's stride-2 layer on 2-D split-padded activations (LDS-DMA staging, even / odd column de-interleave) against
    conv2d(stride 2, padding 1) + scale / shift + LeakyReLU in float64 on the same (16-bit-split) input: even and odd sizes,
    ragged bricks, several bricks per workgroup; the output's zero border untouched."""
    N, Hh, W = shape
    rng = np.random.default_rng(sum(shape) + 17)
    x = _g(rng.standard_normal((N, Hh, W, 16), dtype=np.float32))
    wt = (rng.standard_normal((16, 16, 3, 3)) / 12).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, 16).astype(np.float32), (rng.standard_normal(16) * 0.2).astype(np.float32)
    xs = H.f32_to_split2d(x)
    ho, wo = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
    ys = H.conv2d_s2_split(xs, H.pack_resblock2d_split_weights(_g(wt), _g(sc)), _g(sh), H.split2d_buffer(N, ho, wo, x.device), 0.01)
    y = H.split2d_to_f32(ys).cpu().numpy()
    xq = H.split2d_to_f32(xs).cpu().double().permute(0, 3, 1, 2)
    ref = F.conv2d(xq, torch.from_numpy(wt).double(), padding=1, stride=2) * torch.from_numpy(sc).double().view(1, -1, 1, 1) \
        + torch.from_numpy(sh).double().view(1, -1, 1, 1)
    ref = torch.where(ref > 0, ref, ref * 0.01).permute(0, 2, 3, 1).numpy()
    assert _rel(y, ref) <= 1e-4
    border = ys.clone()
    border[:, 2:-2, 2:-2] = 0
    assert int(border.count_nonzero()) == 0


def test_resblock2d_split_at_bench_size_matches_round2_block():
    """K5 at the end-to-end bench's size (192 images of 256 x 1024: 3.3 GB tensors, byte offsets beyond 2^31, 127 680 bricks on a
    persistent grid) against the round-2 fused block on fp32 activations, both output formats."""
    N, Hh, W = 192, 256, 1024
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn((N, Hh, W, 16), device=DEV, generator=g)
    w1 = torch.randn((16, 16, 3, 3), device=DEV, generator=g) / 12
    w2 = torch.randn((16, 16, 3, 3), device=DEV, generator=g) / 12
    sc1, sh1 = torch.rand(16, device=DEV, generator=g) + 0.5, torch.randn(16, device=DEV, generator=g) * 0.3
    sc2, sh2 = torch.rand(16, device=DEV, generator=g) + 0.5, torch.randn(16, device=DEV, generator=g) * 0.3
    ref = H.resblock2d(x, H.pack_conv2d_weights_bf16x3(w1), sc1, sh1, H.pack_conv2d_weights_bf16x3(w2), sc2, sh2, 0.01)
    q1, q2 = H.pack_resblock2d_split_weights(w1, sc1), H.pack_resblock2d_split_weights(w2, sc2)
    xs = H.f32_to_split2d(x)
    del x
    scale = float(ref.abs().max())
    y = H.resblock2d_split(xs, q1, sh1, q2, sh2, 0.01)
    assert float((y - ref).abs().max()) / scale <= 1e-4
    del y
    ys = H.resblock2d_split(xs, q1, sh1, q2, sh2, 0.01, out_split=H.split2d_buffer(N, Hh, W, DEV))
    back = H.split2d_to_f32(ys)
    assert float((back - ref).abs().max()) / scale <= 1e-4
    assert int(ys[:, :2].count_nonzero()) == 0 and int(ys[:, -2:].count_nonzero()) == 0
    assert int(ys[:, :, :2].count_nonzero()) == 0 and int(ys[:, :, -2:].count_nonzero()) == 0


def test_conv2d_out_split2d_per_image_frames_at_bench_size():
    """The stride-2 extractor layer at the end-to-end bench's size (192 images of 256 x 1024 x 16: beyond the one-volume 32-bit
    offsets, so the launcher runs the images as frames): split-padded output == the split of the fp32 output, border zero."""
    from mvs_gi_amd.dropin import feature_extractor as FE
    mid = dropin.BaseConvBlk2d(16, 16, 3, stride=2, activation=torch.nn.LeakyReLU(), norm_layer=torch.nn.BatchNorm2d(16)).eval().to(DEV)
    N, Hh, W = 192, 256, 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((N, Hh, W, 16), device=DEV, generator=g)
    old_mode = H.get_conv_mode()
    try:
        H.set_conv_mode("bf16x3")
        L = FE.lower_conv2d_block(mid)
        y = L.run(x)
        ys = L.run(x, out_split=H.split2d_buffer(N, Hh // 2, W // 2, x.device))
    finally:
        H.set_conv_mode(old_mode)
    back = H.split2d_to_f32(ys)
    assert float(((back - y).abs() / y.abs().clamp_min(1e-20)).max()) <= 2.0 ** -15
    assert int(ys[:, :2].count_nonzero()) == 0 and int(ys[:, -2:].count_nonzero()) == 0
    assert int(ys[:, :, :2].count_nonzero()) == 0 and int(ys[:, :, -2:].count_nonzero()) == 0


# ------------------------------------------------------------------------------ register-stationary conv (csrc/conv3d_rs.hip)
def test_split_padded_format_round_trip_and_border():
    rng = np.random.default_rng(3)
    x = _g(rng.standard_normal((2, 3, 5, 7, 32), dtype=np.float32) * 10)
    s = H.act_to_split(x)
    assert tuple(s.buf.shape) == (2, 5, 7, 9, 32) and s.buf.dtype == torch.int32
    back = H.act_from_split(s)
    # hi + lo keeps 16-17 significant bits
    assert float(((back - x).abs() / x.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
    again = H.act_from_split(H.act_to_split(back))
    assert torch.equal(again, back)                                   # the representable set is closed under the conversion
    for sl in (s.buf[:, 0], s.buf[:, -1], s.buf[:, :, 0], s.buf[:, :, -1], s.buf[:, :, :, 0], s.buf[:, :, :, -1]):
        assert int(sl.abs().max()) == 0                               # the border is never written


@pytest.mark.parametrize("shape", [(1, 2, 4, 16), (1, 4, 8, 32), (2, 5, 7, 37), (3, 3, 9, 16), (1, 8, 12, 48),
                                   (4, 9, 30, 70),       # 800 ragged bricks on <= 256 workgroups: the steady-state walk (n > 1 per workgroup)
                                   (2, 1, 1, 4), (2, 2, 1, 8)])      # the deepest levels of a stage_factor=1 / keep_last_chs regulator: axes of length 1
@pytest.mark.parametrize("res,slope,out_f32", [(True, 0.01, False), (False, 0.01, True), (True, 0.0, True), (False, 1.0, False)])
def test_conv3d_rs_vs_oracle(shape, res, slope, out_f32):
    """Register-stationary 32 -> 32 conv on split-padded activations against the CPU oracle's conv block on the SAME
    (16-bit-split) inputs; bricks ragged in every axis, one-brick and many-brick launches, residual, fp32 hand-over."""
    B, d, h, w = shape
    rng = np.random.default_rng(hash(shape) % 1000)
    x = _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32))
    r = _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32)) if res else None
    wt = (rng.standard_normal((32, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    sh = (rng.standard_normal(32) * 0.1).astype(np.float32)
    xs, rs = H.act_to_split(x), (H.act_to_split(r) if res else None)
    y = H.conv3d_rs(xs, H.pack_conv_weights_rs(_g(wt)), _g(sc), _g(sh), res=rs, neg_slope=slope, out_f32=out_f32)
    got = (y if out_f32 else H.act_from_split(y)).cpu().numpy()
    xq = H.act_from_split(xs).cpu().permute(0, 4, 1, 2, 3)            # what the kernel actually multiplied
    rq = H.act_from_split(rs).cpu().permute(0, 4, 1, 2, 3) if res else None
    ref = F.conv3d(xq, torch.from_numpy(wt), padding=1) * torch.from_numpy(sc).view(1, -1, 1, 1, 1) + torch.from_numpy(sh).view(1, -1, 1, 1, 1)
    if res:
        ref = ref + rq
    ref = torch.where(ref > 0, ref, ref * slope).permute(0, 2, 3, 4, 1).numpy()
    assert _rel(got, ref) <= 1e-4                                     # split-bf16 products: ~2^-16 each
    if not out_f32:
        for sl in (y.buf[:, 0], y.buf[:, -1], y.buf[:, :, 0], y.buf[:, :, -1], y.buf[:, :, :, 0], y.buf[:, :, :, -1]):
            assert int(sl.abs().max()) == 0


@pytest.mark.parametrize("shape", [(1, 16, 32, 8, 16, 16, 2), (2, 16, 32, 7, 9, 13, 2), (1, 32, 32, 4, 6, 10, 1), (1, 16, 16, 5, 9, 11, 1),
                                   # stride 2 at Cin 32 / 48: the first conv of a deeper 32 -> 32 level, of a (48, 32) regulator
                                   (2, 32, 32, 7, 9, 13, 2), (2, 32, 32, 2, 2, 8, 2), (2, 48, 32, 5, 7, 19, 2)])
def test_streaming_conv_split_padded_output_is_the_split_of_its_fp32_output(shape):
    B, cin, cout, d, h, w, s = shape
    rng = np.random.default_rng(11)
    x = _g(rng.standard_normal((B, d, h, w, cin), dtype=np.float32))
    wt = _g((rng.standard_normal((cout, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32))
    wp = H.pack_conv_weights_bf16x3(wt)
    sc, sh = _g(rng.uniform(0.5, 1.5, cout).astype(np.float32)), _g((rng.standard_normal(cout) * 0.1).astype(np.float32))
    y = H.conv3d(x, wt, wp, sc, sh, stride=s, impl=H.CONV_BF16X3)
    ys = H.SplitAct(*y.shape[:4], cout, x.device)
    H.conv3d_out_split(x, wp, sc, sh, out=ys, stride=s)
    assert torch.equal(ys.buf, H.act_to_split(y).buf)                 # bit for bit, border included


def test_regulator_register_stationary_chain_matches_streaming_and_goldens(golden_dir):
    """UNet level 0 of the (16, 32) regulator on the register-stationary kernels (forced on for a small case) against the
    streaming kernels and the reference goldens."""
    from mvs_gi_amd.dropin import cost_volume_regulator as cr
    import parity_log
    name = "std_d16_rand"
    case = SMALL_CASES[name]
    cfg, z = case["cfg"], _load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    feats = _g(inp["feats"])
    old_mode, old_use = H.get_conv_mode(), cr._USE_RS
    try:
        H.set_conv_mode("bf16x3")
        for gain in case["gains"]:
            w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
            outs = {}
            for use in (False, True):
                cr._USE_RS = use
                hp = HotPath(cfg, w, inp, device=DEV)
                outs[use] = hp(feats)[0].cpu().numpy()
                if use:
                    assert "_mvsgi_rs_bufs" in hp.cv_regulator.down_blks[0].__dict__      # the chain really ran
            ref = z[f"inv_dist_g{gain:g}"]
            err = _rel(outs[True], ref)
            parity_log.record(name + "(rs)", "bf16x3", gain, err, _l1(outs[True], ref), "golden")
            assert err <= 1e-3 and _rel(outs[True], outs[False]) <= 5e-4      # two 16-bit approximations of the same path
    finally:
        H.set_conv_mode(old_mode)
        cr._USE_RS = old_use


def test_split_padded_hand_over_between_builder_and_regulator(golden_dir):
    """The cost volume crossing the builder -> regulator boundary as a module-owned split-padded buffer (post_vol writes it, the
    regulator's stride-2 first layer stages it by LDS-DMA) against the fp32-tensor boundary and the reference goldens; the
    modules' own forward() keep the tensor interface; a batch of 3 with the hand-over equals the frames one by one."""
    from mvs_gi_amd.dropin import cost_volume_regulator as cr
    from mvs_gi_amd.dropin.torch_only import build_and_regulate
    import parity_log
    name = "std_d16_rand"
    case = SMALL_CASES[name]
    cfg, z = case["cfg"], _load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    feats = _g(inp["feats"])
    old_mode, old_use = H.get_conv_mode(), cr._USE_S2RS
    try:
        H.set_conv_mode("bf16x3")
        for gain in case["gains"]:
            w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
            outs = {}
            for use in (False, True):
                cr._USE_S2RS = use
                hp = HotPath(cfg, w, inp, device=DEV)
                outs[use] = hp(feats)[0].cpu().numpy()
                assert ("_mvsgi_rs_x0" in hp.cv_builder.__dict__) == use             # the hand-over really ran / did not
            ref = z[f"inv_dist_g{gain:g}"]
            err = _rel(outs[True], ref)
            parity_log.record(name + "(split hand-over)", "bf16x3", gain, err, _l1(outs[True], ref), "golden")
            assert err <= 1e-3 and _rel(outs[True], outs[False]) <= 5e-4
        cr._USE_S2RS = True
        hp = HotPath(cfg, w, inp, device=DEV)
        g, gm, m = hp.grids, hp.grid_masks, hp.masks
        vol = hp.cv_builder(feats, g, gm, m)                      # the modules' tensor interface is unchanged
        assert isinstance(vol, torch.Tensor) and vol.dtype == torch.float32 and vol.shape[1] == 16
        costs_t = hp.cv_regulator(vol)
        costs_s = build_and_regulate(hp.cv_builder, hp.cv_regulator, feats, g, gm, m)
        assert _rel(costs_s.cpu().numpy(), costs_t.cpu().numpy()) <= 5e-4
        f3 = torch.cat([feats, feats.flip(1), feats * 0.5], 0)
        b3 = hp(f3)[0]
        for i in range(3):
            assert _rel(b3[i:i + 1].cpu().numpy(), hp(f3[i:i + 1].contiguous())[0].cpu().numpy()) <= 1e-5
    finally:
        H.set_conv_mode(old_mode)
        cr._USE_S2RS = old_use


def test_full_size_winograd_level0_vs_direct_kernel_and_reference_golden(golden_dir):
    """G16V at full size in the fp16 split: UNet level 0's six 32 -> 32 convs ([8, 40, 160]) on the Winograd-form kernel (the dispatcher's
    choice) and on the direct register-stationary kernel (MVSGI_WINO=0) -- both reproduce the reference golden 3x inside the fp16
    split's 1e-4, and differ from each other by less than either does from the golden."""
    from mvs_gi_amd.dropin import cost_volume_regulator as cr
    import parity_log
    case = FULL_CASES["full_G16V"]
    cfg, z = case["cfg"], _load(golden_dir, "full_G16V")
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=1, grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"]), "regenerated inputs differ from the golden run's (host libm)"
    old, old_use, old_a32, real = H.get_conv_mode(), cr._USE_WINO, cr._WINO_A32, H.conv3d_wino
    calls = []

    def spy(*a, **k):
        calls.append(k.get("out_f32", False))
        return real(*a, **k)
    try:
        H.set_conv_mode("f16x3")
        H.conv3d_wino = spy
        gain = case["gains"][-1]
        w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
        feats = _g(inp["feats"]).expand(2, -1, -1, -1, -1).contiguous()
        outs = {}
        for use in (True, "pairs", False):          # fp32-padded activations between the layers (the default) | fp16 pairs | the direct kernel
            cr._USE_WINO, cr._WINO_A32 = bool(use), use is True
            calls.clear()
            hp = HotPath(cfg, w, inp, device=DEV)
            outs[use] = hp(feats)[0].cpu().numpy()
            assert calls == ([False] * 5 + [True] if use else [])          # six launches, the last one hands fp32 to the next level
            fmts = {b.fmt for bufs in hp.cv_regulator.down_blks[0].__dict__["_mvsgi_rs_bufs"].values() for b in bufs}
            assert fmts == ({"f32p"} if use is True else {"f16"})
        ref = z[f"inv_dist_g{gain:g}"]
        for i in range(2):
            err = _rel(outs[True][i:i + 1], ref)
            parity_log.record("full_G16V(winograd level 0)", "f16x3", gain, err, _l1(outs[True][i:i + 1], ref), "golden")
            assert err <= 1e-4 and _rel(outs[False][i:i + 1], ref) <= 1e-4 and _rel(outs["pairs"][i:i + 1], ref) <= 1e-4
        assert _rel(outs[True], outs[False]) <= 3e-5 and _rel(outs["pairs"], outs[False]) <= 3e-5
    finally:
        H.conv3d_wino = real
        H.set_conv_mode(old)
        cr._USE_WINO, cr._WINO_A32 = old_use, old_a32


@pytest.mark.parametrize("split", ["bf16x3", "f16x3"])
def test_full_size_batch8_register_stationary_path_vs_reference_golden(golden_dir, split):
    """G16V at full size with 8 frames per launch: the batch at which bench.py's path (register-stationary level-0 convs)
    is active; every frame must reproduce the single-frame reference golden -- in both 16-bit splits (the fp16 split runs the
    same kernels: split-padded buffers tagged 'f16' all the way from the sweep to the cost head)."""
    import parity_log
    case = FULL_CASES["full_G16V"]
    cfg, z = case["cfg"], _load(golden_dir, "full_G16V")
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=1, grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"]), "regenerated inputs differ from the golden run's (host libm)"
    old = H.get_conv_mode()
    try:
        H.set_conv_mode(split)
        gain = case["gains"][-1]
        hp = HotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=gain), inp, device=DEV)
        inv = hp(_g(inp["feats"]).expand(8, -1, -1, -1, -1).contiguous())[0]
        assert "_mvsgi_rs_bufs" in hp.cv_regulator.down_blks[0].__dict__
        fmt = "f16" if split == "f16x3" else "bf16"      # every split-padded buffer of the path carries the mode's split
        lvl0 = "f32p" if split == "f16x3" else fmt        # (the Winograd-form level 0 of the fp16 split passes fp32-padded records between its layers)
        assert all(b.fmt == lvl0 for bufs in hp.cv_regulator.down_blks[0].__dict__["_mvsgi_rs_bufs"].values() for b in bufs)
        assert all(b.fmt == fmt for b in hp.cv_regulator.__dict__["_mvsgi_poly_bufs"].values())
        # the sweep -> post_vol front end in chunks of frames (bench.py's B=64 runs chunks of 16): same bits
        from mvs_gi_amd.dropin import cost_volume_builder as cvb_mod
        old_chunk, cvb_mod._FRONT_CHUNK = cvb_mod._FRONT_CHUNK, 3
        try:
            inv_c = hp(_g(inp["feats"]).expand(8, -1, -1, -1, -1).contiguous())[0]
        finally:
            cvb_mod._FRONT_CHUNK = old_chunk
        assert torch.equal(inv_c, inv)
        ref = z[f"inv_dist_g{gain:g}"]
        got = inv.cpu().numpy()
        for f in (0, 7):
            err = _rel(got[f:f + 1], ref)
            parity_log.record(f"full_G16V(B=8,rs)[{f}]", split, gain, err, _l1(got[f:f + 1], ref), "golden")
            assert err <= (1e-3 if split == "bf16x3" else 1e-4)
        assert np.array_equal(got[0], got[7])
        # bench.py's batch: 64 frames per launch (front end in chunks of 16, split-padded hand-over, hipGraph replay), every
        # 8th frame scaled so that the frames differ: frames 0 and 63 reproduce the golden, a scaled frame its own single run
        f64 = _g(inp["feats"]).expand(64, -1, -1, -1, -1).contiguous()
        f64[5::8] *= 0.5
        inv64 = hp(f64)[0]
        g64 = inv64.cpu().numpy()
        for f in (0, 63):
            err = _rel(g64[f:f + 1], ref)
            parity_log.record(f"full_G16V(B=64)[{f}]", split, gain, err, _l1(g64[f:f + 1], ref), "golden")
            assert err <= (1e-3 if split == "bf16x3" else 1e-4)
        # equal inputs -> equal bits wherever the frame sits in the batch (chunks of 16, persistent walks); the scaled frames differ.
        # (A batch of 4 or 1 takes other kernel variants -- other fp32 summation orders -- and lands 1.4e-4 away: not compared.)
        assert np.array_equal(g64[0], g64[8]) and np.array_equal(g64[0], g64[63]) and np.array_equal(g64[5], g64[61])
        assert not np.array_equal(g64[5], g64[0])
        hp.capture(f64)
        assert torch.equal(hp.replay()[0], inv64)
        # bench.py's step: the batch in two parts on two HIP streams inside one hipGraph (StreamedHotPath) -- each part the bits
        # of the one-stream launch of the same frames
        from mvs_gi_amd.pipeline import StreamedHotPath
        shp = StreamedHotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=gain), inp, device=DEV, n_streams=2)
        f128 = torch.cat([f64, f64])
        shp.capture(f128)
        parts = shp.replay()
        torch.cuda.synchronize()
        assert len(parts) == 2 and torch.equal(parts[0][0], inv64) and torch.equal(parts[1][0], inv64)
        err = _rel(parts[1][0][63:64].cpu().numpy(), ref)
        parity_log.record("full_G16V(2x64 streamed)[127]", split, gain, err, _l1(parts[1][0][63:64].cpu().numpy(), ref), "golden")
        assert err <= (1e-3 if split == "bf16x3" else 1e-4)
        del parts
        # bench.py's default since round 6: two parts of 128 frames (one more round of units per persistent grid: +1.1 %) -- first and
        # last frame of the step against the golden; equal frames of a part equal bits
        f256 = torch.cat([f128, f128])
        shp.capture(f256)
        parts = shp.replay()
        torch.cuda.synchronize()
        p0, p1 = parts[0][0].cpu().numpy(), parts[1][0].cpu().numpy()
        for tag, fr in (("[0]", p0[0:1]), ("[255]", p1[127:128])):
            err = _rel(fr, ref)
            parity_log.record(f"full_G16V(2x128 streamed){tag}", split, gain, err, _l1(fr, ref), "golden", _pix(fr, ref))
            assert err <= (1e-3 if split == "bf16x3" else 1e-4)
        assert np.array_equal(p0[0], p0[64]) and np.array_equal(p0[0], p1[127]) and np.array_equal(p0[5], p1[69]) and not np.array_equal(p0[5], p0[0])
        del shp, parts, f128, f256
    finally:
        H.set_conv_mode(old)
        torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(1, 4, 4, 16), (2, 5, 7, 37), (1, 9, 6, 20), (3, 8, 16, 48),
                                   (3, 10, 30, 150)])    # 720 ragged bricks: main phases with masked stores mid-walk
@pytest.mark.parametrize("slope", [0.01, 1.0])
def test_conv3d_rs16_vs_oracle(shape, slope):
    """Register-stationary 16 -> 16 conv (post_vol) on a split-padded volume against the oracle's conv block on the same
    (16-bit-split) input: one-brick and ragged launches (the last brick of every workgroup runs the drain phase)."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x = _g(rng.standard_normal((B, d, h, w, 16), dtype=np.float32))
    wt = (rng.standard_normal((16, 16, 3, 3, 3)) / np.sqrt(27 * 16)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, 16).astype(np.float32), (rng.standard_normal(16) * 0.1).astype(np.float32)
    xs = H.act_to_split(x)
    y = H.conv3d_rs16(xs, H.pack_conv_weights_rs(_g(wt)), _g(sc), _g(sh), neg_slope=slope).cpu().numpy()
    xq = H.act_from_split(xs).cpu().permute(0, 4, 1, 2, 3)
    ref = F.conv3d(xq, torch.from_numpy(wt), padding=1) * torch.from_numpy(sc).view(1, -1, 1, 1, 1) + torch.from_numpy(sh).view(1, -1, 1, 1, 1)
    ref = torch.where(ref > 0, ref, ref * slope).permute(0, 2, 3, 4, 1).numpy()
    assert _rel(y, ref) <= 1e-4


@pytest.mark.parametrize("shape", [(1, 4, 4, 16), (2, 5, 7, 37), (3, 8, 16, 48), (3, 10, 30, 150)])
def test_conv3d_rs16_split_output_is_the_split_of_the_fp32_output(shape):
    """post_vol writing the split-padded format (the hand-over to the stride-2 kernel): bit for bit the split of what the fp32
    variant writes, zero border untouched."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 3)
    x = _g(rng.standard_normal((B, d, h, w, 16), dtype=np.float32))
    wt = (rng.standard_normal((16, 16, 3, 3, 3)) / np.sqrt(27 * 16)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, 16).astype(np.float32), (rng.standard_normal(16) * 0.1).astype(np.float32)
    xs, wp = H.act_to_split(x), H.pack_conv_weights_rs(_g(wt))
    y = H.conv3d_rs16(xs, wp, _g(sc), _g(sh), neg_slope=0.01)
    ys = H.conv3d_rs16(xs, wp, _g(sc), _g(sh), neg_slope=0.01, out_split=H.SplitAct(B, d, h, w, 16, x.device))
    assert torch.equal(ys.buf, H.act_to_split(y).buf)


@pytest.mark.parametrize("shape", [(1, 2, 2, 16), (2, 4, 8, 32), (1, 5, 7, 19), (3, 2, 9, 33), (2, 16, 20, 40), (4, 16, 80, 320)])
def test_conv3d_s2rs_vs_reference_conv(shape, th=4):
    """The stride-2 16 -> 32 layer on split-padded activations (LDS-DMA staging, even / odd column de-interleave) against
    conv3d(stride 2, padding 1) + scale / shift + LeakyReLU in float64 on the same (16-bit-split) input: even and odd sizes,
    ragged tiles, a launch with several bricks per workgroup (4 x 16 x 80 x 320: 3200 bricks); the output's zero border untouched."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + th)
    x = _g(rng.standard_normal((B, d, h, w, 16), dtype=np.float32))
    wt = (rng.standard_normal((32, 16, 3, 3, 3)) / np.sqrt(27 * 16)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, 32).astype(np.float32), (rng.standard_normal(32) * 0.1).astype(np.float32)
    xs = H.act_to_split(x)
    do, ho, wo = (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = H.SplitAct(B, do, ho, wo, 32, x.device)
    ys = H.conv3d_s2rs(xs, H.pack_conv_weights_s2rs(_g(wt), _g(sc)), _g(sh), out, neg_slope=0.01)
    y = H.act_from_split(ys).cpu().numpy()
    xq = H.act_from_split(xs).cpu().double().permute(0, 4, 1, 2, 3)
    ref = F.conv3d(xq, torch.from_numpy(wt).double(), padding=1, stride=2) * torch.from_numpy(sc).double().view(1, -1, 1, 1, 1) \
        + torch.from_numpy(sh).double().view(1, -1, 1, 1, 1)
    ref = torch.where(ref > 0, ref, ref * 0.01).permute(0, 2, 3, 4, 1).numpy()
    assert _rel(y, ref) <= 1e-4
    border = ys.buf.clone()
    border[:, 1:-1, 1:-1, 1:-1] = 0
    assert int(border.count_nonzero()) == 0


def test_sweep_split_padded_output_is_the_split_of_vol_raw(golden_dir):
    """The sweep writing its volume split-padded (the register-stationary post_vol's input) against the bit-exact fp32 sweep,
    per-frame rig and one rig for the whole batch."""
    case = SMALL_CASES["std_d16_rand"]
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=2, grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    f, g, gm, m = (_g(inp[k]) for k in ("feats", "grids", "grid_masks", "masks"))
    vm = H.sweep_validity(g, gm, m)
    vol = H.sweep_std_valid(f, g, vm)
    B, D, Ho, Wo, C = vol.shape
    vs = H.sweep_std_valid_split(f, g, vm, out=H.SplitAct(B, D, Ho, Wo, C, f.device))
    assert torch.equal(vs.buf, H.act_to_split(vol).buf)
    vol1 = H.sweep_std_valid(f, g[:1].contiguous(), vm[:1].contiguous())           # one rig for both frames
    vs1 = H.sweep_std_valid_split(f, g[:1].contiguous(), vm[:1].contiguous(), out=H.SplitAct(B, D, Ho, Wo, C, f.device))
    assert torch.equal(vs1.buf, H.act_to_split(vol1).buf)


def test_builder_register_stationary_post_vol_matches_streaming_and_goldens(golden_dir):
    from mvs_gi_amd.dropin import cost_volume_builder as cb
    name = "std_d16_rand"
    case = SMALL_CASES[name]
    cfg, z = case["cfg"], _load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    w = synth.make_weights(cfg, seed=case["seed"], gain=1.0)
    f, g, gm, m = (_g(inp[k]) for k in ("feats", "grids", "grid_masks", "masks"))
    old_mode, old_use = H.get_conv_mode(), cb._USE_RS
    try:
        H.set_conv_mode("bf16x3")
        outs = {}
        for use in (False, True):
            cb._USE_RS = use
            cvb, _, _ = build_modules(cfg, w, DEV)
            outs[use] = cvb(f, g, gm, m).contiguous().cpu().numpy()
            assert ("_mvsgi_rs_vol" in cvb.__dict__) == use
        assert _rel(outs[True], z["vol"]) <= 2e-4 and _rel(outs[True], outs[False]) <= 5e-5
    finally:
        H.set_conv_mode(old_mode)
        cb._USE_RS = old_use


# ------------------------------------------------------------------------------ round-3 review items
def test_softargmin_many_candidates_multi_pass_branch():
    """D = 48 > 32: the soft-argmin kernel's multi-pass branch (the register path serves D <= 32), x2 / x1, with and without
    norm_costs, against the oracle."""
    rng = np.random.default_rng(48)
    D = 48
    costs = (rng.standard_normal((2, 1, D, 6, 10)) * 3).astype(np.float32)
    cands = list(np.geomspace(0.5, 100.0, D))
    for scale, pre in ((2, True), (0, True)):
        dr = dropin.DistanceRegressorWithFixedCandidates(bf=96, dist_cands=cands, interp_scale_factor=scale, pre_interp=pre).to(DEV)
        inv, pr = dr(_g(costs))
        ref_inv, ref_pr = O.soft_argmin(torch.from_numpy(costs), cands, 96, scale, pre)
        assert _rel(inv.cpu().numpy(), ref_inv.numpy()) <= 1e-5
        assert _rel(pr.cpu().numpy(), ref_pr.numpy()) <= 1e-5
        assert abs(float(pr.sum(1).mean()) - 1.0) < 1e-5
        dr.return_norm_costs = False
        assert torch.equal(dr(_g(costs))[0], inv)


@pytest.mark.parametrize("N", [5, 6])
def test_sweep_std_nchw_five_and_six_cameras(N):
    """The plane-gather (NCHW) std sweep with more cameras than the channels-last kernels take (N <= 4).  The kernel adds the
    cameras in order; ATen's sum over the camera axis does too for N <= 4 (hence the bit-exact tests above), but from five
    addends on it changes association for some element positions (its vectorised row reduction), so here the bar is 2 ulp-ish:
    1e-6 of the tensor's maximum, and the samples / validity (which involve no sum) are exact: zeros agree exactly."""
    rng = np.random.default_rng(N)
    B, C, Hi, Wi, D, Ho, Wo, Hm, Wm = 2, 6, 12, 20, 3, 5, 9, 24, 40
    feats = rng.standard_normal((B, N, C, Hi, Wi)).astype(np.float32)
    grids = rng.uniform(-1.15, 1.15, (B, N, D, Ho, Wo, 2)).astype(np.float32)
    gm = rng.random((B, N, D, Ho, Wo, 1)) < 0.8
    masks = (rng.random((B, N, 1, Hm, Wm)) < 0.7).astype(np.float32)
    want = O.sweep_std_masked(*(torch.from_numpy(a) for a in (feats, grids, gm, masks))).numpy()
    for gmask in (_g(gm), _g(gm).float()):
        got = _ncdhw(H.sweep_std(_g(feats), _g(grids), gmask, _g(masks)))
        assert _rel(got, want) <= 1e-6 and np.array_equal(got == 0, want == 0)
        assert (got != want).mean() < 0.05          # the association differs for a few positions only


def test_front_end_without_rig_cache_and_with_a_tail_chunk():
    """Review items: (1) cache_rig_constants = False with a batch above the front-end chunk and stride-0 rig views must take the
    streaming path (it used to hand None to the post_vol kernel); (2) a batch that is not a multiple of the chunk re-uses ONE
    chunk-sized buffer (a leading slice for the tail): same bits as the unchunked run, buffer identity stable over steps."""
    from mvs_gi_amd.dropin import cost_volume_builder as cb
    cfg = SMALL_CASES["std_d16_rand"]["cfg"]
    inp = synth.make_inputs(cfg, seed=3, batch=1)
    w = synth.make_weights(cfg, seed=3)
    old_mode, old_chunk = H.get_conv_mode(), cb._FRONT_CHUNK
    try:
        H.set_conv_mode("bf16x3")
        rng = np.random.default_rng(0)
        feats = _g(rng.standard_normal((7, *inp["feats"].shape[1:]), dtype=np.float32))
        cb._FRONT_CHUNK = 0
        hp0 = HotPath(cfg, w, inp, device=DEV)
        whole = hp0(feats)[0].clone()
        cb._FRONT_CHUNK = 3                       # chunks of 3, 3 and a tail of 1
        hp = HotPath(cfg, w, inp, device=DEV)
        a = hp(feats)[0].clone()
        bufs = dict(hp.cv_builder.__dict__["_mvsgi_rs_vol"])
        b = hp(feats)[0].clone()
        assert torch.equal(a, whole) and torch.equal(b, whole)
        after = hp.cv_builder.__dict__["_mvsgi_rs_vol"]
        assert len(after) == 1 and all(after[k] is bufs[k] for k in bufs)      # one chunk-sized buffer, never replaced
        hp.cv_builder.cache_rig_constants = False
        c = hp(feats)[0].clone()                  # masks re-sampled every call: streaming post_vol, fp32 volume
        assert _rel(c.cpu().numpy(), whole.cpu().numpy()) <= 5e-4
    finally:
        H.set_conv_mode(old_mode)
        cb._FRONT_CHUNK = old_chunk


def test_hipgraph_survives_eager_calls_at_other_batch_sizes():
    """A captured graph holds the addresses of the module-owned split-padded buffers: an eager call with another batch size in
    between must neither free nor re-zero them; replay() with a mismatching shape raises instead of replaying stale geometry."""
    from mvs_gi_amd.configs import CONFIGS, DIST_8L
    cfg = CONFIGS["G16V"].scaled(feat_hw=(32, 128), mask_hw=(64, 256), cv_hw=(16, 64), dist_cands=DIST_8L)
    inp = synth.make_inputs(cfg, seed=7, batch=1)
    old_mode = H.get_conv_mode()
    try:
        H.set_conv_mode("bf16x3")
        hp = HotPath(cfg, synth.make_weights(cfg, seed=7), inp, device=DEV)
        rng = np.random.default_rng(2)
        f2 = _g(rng.standard_normal((2, *inp["feats"].shape[1:]), dtype=np.float32))
        f3 = _g(rng.standard_normal((3, *inp["feats"].shape[1:]), dtype=np.float32))
        e2 = hp(f2)[0].clone()
        hp.capture(f2)
        g_a = hp.replay(f2)[0].clone()
        e3 = hp(f3)[0].clone()                      # another batch size, eagerly
        junk = [torch.full((1 << 22,), 7, device=DEV, dtype=torch.int32) for _ in range(8)]     # would land in freed buffers
        g_b = hp.replay(f2)[0].clone()
        assert torch.equal(g_a, e2) and torch.equal(g_b, e2)
        assert torch.equal(hp(f3)[0], e3)
        del junk
        with pytest.raises(ValueError):
            hp.replay(f3)
    finally:
        H.set_conv_mode(old_mode)


@pytest.mark.parametrize("shape", [(2, 16, 5, 8), (1, 16, 7, 10), (2, 5, 6, 9), (1, 32, 4, 12), (1, 48, 6, 10), (1, 16, 3, 700), (1, 20, 1, 4),
                                   (3, 16, 80, 320)])
def test_softargmin_row_pair_kernel_equals_pixel_kernel_and_oracle(shape):
    """The x2 soft-argmin as one workgroup per low-resolution row pair (LDS-staged rows, four pixels per thread, 16-byte stores)
    against the thread-per-pixel kernel (run at scale 1 on the upsampled costs) and the oracle: W % 4 != 0, odd W, two column tiles, H = 1,
    D in registers (<= 16, <= 32) and the multi-pass form (D = 48), with and without norm_costs, with the / bf post-division."""
    B, D, Hh, W = shape
    rng = np.random.default_rng(sum(shape))
    costs = (rng.standard_normal((B, D, Hh, W)) * 4).astype(np.float32)
    inv_idx = _g((96.0 / np.geomspace(0.5, 100.0, D)).astype(np.float32))
    c = _g(costs)
    inv, pr = H.softargmin(c, inv_idx, 2, True)
    inv_only, none = H.softargmin(c, inv_idx, 2, False, post_div=96.0)
    # the thread-per-pixel kernel serves scale 1: upsampling first and running it at scale 1 is the same arithmetic as its x2 path
    up_dev = F.interpolate(c, scale_factor=2, mode="bilinear").contiguous()
    inv_p, pr_p = H.softargmin(up_dev, inv_idx, 1, True)
    assert none is None and _rel(inv_only.cpu().numpy() * 96.0, inv.cpu().numpy()) <= 1e-6
    assert _rel(inv.cpu().numpy(), inv_p.cpu().numpy()) <= 1e-5 and _rel(pr.cpu().numpy(), pr_p.cpu().numpy()) <= 1e-5
    up = F.interpolate(torch.from_numpy(costs), scale_factor=2, mode="bilinear")
    ref_pr = F.softmax(up, 1)
    ref_inv = (ref_pr * inv_idx.cpu().view(1, -1, 1, 1)).sum(1, keepdim=True)
    assert _rel(inv.cpu().numpy(), ref_inv.numpy()) <= 1e-5 and _rel(pr.cpu().numpy(), ref_pr.numpy()) <= 1e-5


# ------------------------------------------------------------------------------ polyphase ResizeConv3d (out_costs.0)
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 1, 3, 5), (1, 2, 4, 16), (1, 3, 5, 7), (2, 4, 6, 18), (3, 5, 9, 33), (1, 2, 2, 2),
                                   (2, 8, 40, 160), (9, 3, 12, 40)])
@pytest.mark.parametrize("slope", [0.01, 1.0])
def test_conv3d_up2_polyphase_vs_interpolate_then_conv(shape, slope):
    """ResizeConv3d 32 -> 16 in polyphase form (8 phase convolutions over the low-resolution tensor on the register-stationary
    kernel + face / edge corrections) against F.interpolate(trilinear x2) -> conv3d -> scale / shift -> LeakyReLU on the same
    16-bit-split input: single-cell axes (every cell first AND last), two-cell axes (no interior), odd and ragged sizes, the
    full out_costs.0 size, and more bricks than workgroups."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x = _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32))
    wt = (rng.standard_normal((16, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, 16).astype(np.float32)
    sh = (rng.standard_normal(16) * 0.1).astype(np.float32)
    xs = H.act_to_split(x)
    plan = H.conv3d_up2_poly_plan(_g(wt), d, h, w)
    y = torch.full((B, 2 * d, 2 * h, 2 * w, 16), float("nan"), device=DEV)          # every voxel must be written
    H.conv3d_up2_poly(xs, plan, _g(sc), _g(sh), neg_slope=slope, out=y)
    xq = H.act_from_split(xs).cpu().permute(0, 4, 1, 2, 3).double()
    up = F.interpolate(xq, scale_factor=2, mode="trilinear", align_corners=False)
    ref = F.conv3d(up, torch.from_numpy(wt).double(), padding=1) * torch.from_numpy(sc).double().view(1, -1, 1, 1, 1) \
        + torch.from_numpy(sh).double().view(1, -1, 1, 1, 1)
    ref = torch.where(ref > 0, ref, ref * slope).permute(0, 2, 3, 4, 1).numpy()
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    assert _rel(got, ref) <= 1e-4                                     # split-bf16 products: ~2^-16 each
    # the faces on their own (a wrong correction is a small fraction of the tensor's maximum only there)
    for sl in (np.s_[:, :2], np.s_[:, -2:], np.s_[:, :, :2], np.s_[:, :, -2:], np.s_[:, :, :, :2], np.s_[:, :, :, -2:]):
        assert _rel(got[sl], ref[sl]) <= 1e-4


def test_regulator_polyphase_tail_matches_streaming_and_goldens(golden_dir):
    """The (16, 32) regulator with out_costs.0 in polyphase form (and the last up block writing split-padded) against the
    streaming kernels and the reference goldens."""
    from mvs_gi_amd.dropin import cost_volume_regulator as cr
    import parity_log
    name = "std_d16_rand"
    case = SMALL_CASES[name]
    cfg, z = case["cfg"], _load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    feats = _g(inp["feats"])
    old_mode, old_use, old_min = H.get_conv_mode(), cr._USE_POLY, cr._POLY_MIN_UNITS
    try:
        H.set_conv_mode("bf16x3")
        cr._POLY_MIN_UNITS = 0
        for gain in case["gains"]:
            w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
            outs = {}
            for use in (False, True):
                cr._USE_POLY = use
                hp = HotPath(cfg, w, inp, device=DEV)
                outs[use] = hp(feats)[0].cpu().numpy()
                assert ("_mvsgi_poly_bufs" in hp.cv_regulator.__dict__) == use        # the polyphase tail really ran
            ref = z[f"inv_dist_g{gain:g}"]
            err = _rel(outs[True], ref)
            parity_log.record(name + "(poly)", "bf16x3", gain, err, _l1(outs[True], ref), "golden")
            assert err <= 1e-3 and _rel(outs[True], outs[False]) <= 5e-4
    finally:
        H.set_conv_mode(old_mode)
        cr._USE_POLY, cr._POLY_MIN_UNITS = old_use, old_min


@pytest.mark.parametrize("shape", [(1, 16, 1, 1, 1), (1, 16, 3, 5, 7), (2, 16, 5, 9, 33), (1, 32, 4, 9, 33), (2, 48, 5, 8, 32), (3, 16, 16, 80, 320),
                                   (70, 16, 2, 8, 32)])
def test_cost_head_on_split_padded_input_vs_conv3d(shape):
    """out_costs.1 (Conv3d(Cin -> 1, bias)) on a split-padded input, split-bf16 MFMA with the 27 taps as the M dimension, against
    F.conv3d on the same 16-bit-split input: one to three channel slices, windows ragged in H and W, whole-depth and chunked marches."""
    B, cin, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x = _g(rng.standard_normal((B, d, h, w, cin), dtype=np.float32))
    wt = (rng.standard_normal((1, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32)
    bias = 0.37
    xs = H.act_to_split(x)
    y = H.conv3d_head_split(xs, H.pack_head_split_weights(_g(wt)), 1.0, bias)
    xq = H.act_from_split(xs).cpu().permute(0, 4, 1, 2, 3).double()
    ref = (F.conv3d(xq, torch.from_numpy(wt).double(), padding=1) + bias).permute(0, 2, 3, 4, 1).numpy()
    assert tuple(y.shape) == (B, d, h, w, 1)
    assert _rel(y.cpu().numpy(), ref) <= 1e-4


# ------------------------------------------------------------------------------ the split-padded kernels in the fp16 split
def _bn(rng, c):
    return rng.uniform(0.5, 1.5, c).astype(np.float32), (rng.standard_normal(c) * 0.1).astype(np.float32)


def _conv_ref64(xq, wt, sc, sh, slope, stride=1, res=None):
    """conv3d + scale / shift (+ res) + LeakyReLU in float64 on NDHWC device tensors -> NDHWC numpy."""
    y = F.conv3d(xq.cpu().double().permute(0, 4, 1, 2, 3), torch.from_numpy(wt).double(), padding=1, stride=stride)
    y = y * torch.from_numpy(sc).double().view(1, -1, 1, 1, 1) + torch.from_numpy(sh).double().view(1, -1, 1, 1, 1)
    if res is not None:
        y = y + res.cpu().double().permute(0, 4, 1, 2, 3)
    return torch.where(y > 0, y, y * slope).permute(0, 2, 3, 4, 1).float().numpy()


def test_split_padded_format_in_the_fp16_split_round_trip_range_and_border():
    """fp32 -> split-padded fp16 pairs -> fp32: 22 significant bits (the bf16 split keeps 16-17), values beyond +-65504 clamped, never
    inf / nan, the zero border untouched; a buffer's split is a tag its readers check."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 5, 7, 32), dtype=np.float32) * np.float32(10.0)
    x[0, 0, 0, 0, :4] = [1e5, -3e9, 65504.0, 6.1e-5]
    xs16, xsb = H.act_to_split(_g(x), fmt="f16"), H.act_to_split(_g(x))
    assert xs16.fmt == "f16" and xsb.fmt == "bf16"
    back16, backb = H.act_from_split(xs16).cpu().numpy(), H.act_from_split(xsb).cpu().numpy()
    ref = np.clip(x, -65504.0, 65504.0)
    assert np.isfinite(back16).all()
    assert np.abs(back16 - ref).max() <= 2.0 ** -21 * np.abs(ref).max() and np.abs(backb - x)[0, 1:].max() > 50 * np.abs(back16 - ref)[0, 1:].max()
    assert float(back16[0, 0, 0, 0, 0]) == 65504.0 and float(back16[0, 0, 0, 0, 1]) == -65504.0
    for sl in (xs16.buf[:, 0], xs16.buf[:, -1], xs16.buf[:, :, 0], xs16.buf[:, :, -1], xs16.buf[:, :, :, 0], xs16.buf[:, :, :, -1]):
        assert int(sl.abs().max()) == 0
    wp = H.pack_conv_weights_rs(_g((rng.standard_normal((32, 32, 3, 3, 3)) * 0.05).astype(np.float32)))
    with pytest.raises(AssertionError, match="does not match"):       # a residual of the other split
        H.conv3d_rs(xs16, wp, torch.ones(32, device=DEV), torch.zeros(32, device=DEV), res=xsb)


@pytest.mark.parametrize("shape", [(1, 2, 4, 16), (2, 5, 7, 37), (1, 8, 12, 48), (3, 10, 30, 150)])
@pytest.mark.parametrize("res,slope,out_f32", [(True, 0.01, False), (False, 0.01, True), (True, 1.0, False)])
def test_conv3d_rs_in_the_fp16_split_vs_oracle(shape, res, slope, out_f32):
    """The register-stationary 32 -> 32 kernel in the fp16 split (conv3d_rs32_kernel<MODE, true>: the same generated schedule, the
    fp16 matrix instruction, fp16 residual and epilogue split): 20x inside the bf16 split's 1e-4 against float64 on what it multiplied."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 16)
    x, r = _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32)), _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32))
    wt = (rng.standard_normal((32, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32) * np.float32(0.02)
    sc, sh = _bn(rng, 32)
    xs, rs = H.act_to_split(x, fmt="f16"), (H.act_to_split(r, fmt="f16") if res else None)
    wp, un = H.pack_conv_weights_rs(_g(wt), "f16")
    y = H.conv3d_rs(xs, wp, _g(sc) * un, _g(sh), res=rs, neg_slope=slope, out_f32=out_f32)
    assert out_f32 or y.fmt == "f16"
    got = (y if out_f32 else H.act_from_split(y)).cpu().numpy()
    ref = _conv_ref64(H.act_from_split(xs), wt, sc, sh, slope, res=H.act_from_split(rs) if res else None)
    assert _rel(got, ref) <= 5e-6
    if not out_f32:
        for sl in (y.buf[:, 0], y.buf[:, -1], y.buf[:, :, 0], y.buf[:, :, -1], y.buf[:, :, :, 0], y.buf[:, :, :, -1]):
            assert int(sl.abs().max()) == 0


@pytest.mark.parametrize("shape", [(1, 8, 2, 32), (2, 8, 6, 64), (5, 8, 12, 32), (3, 8, 40, 160), (2, 16, 4, 32), (1, 16, 40, 160)])
@pytest.mark.parametrize("res,slope,out_f32", [(True, 0.01, False), (False, 0.01, True), (True, 1.0, True), (False, 0.0, False)])
@pytest.mark.parametrize("act32", [False, True])
def test_conv3d_winograd_in_the_fp16_split_vs_oracle(shape, res, slope, out_f32, act32):
    """The Winograd F(2x2, 3x3) x direct-D form of the 32 -> 32 layers (csrc/conv3d_wino.hip; BaseConvBlk3d.forward,
    common_modules.py:107-115): transformed weights and activations in the fp16 split, 2.25 x fewer matrix instructions.  The same
    5e-6 bar as the direct kernel in this split, against float64 on what it multiplied; volumes of 8 and of 16 planes (the unit is
    unrolled over either), units of several workgroups and of one (the stream's tail), every epilogue variant, activations as
    split-padded fp16 pairs or fp32-padded (`act32`: the hand-over between Winograd layers); the border of a padded output stays zero."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 18)
    x, r = _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32)), _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32))
    wt = (rng.standard_normal((32, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32) * np.float32(0.02)
    sc, sh = _bn(rng, 32)
    assert H.conv3d_wino_applies(32, 32, d, h, w, 1, slope)
    to_act, from_act, fmt = (H.act_to_f32p, H.act_from_f32p, "f32p") if act32 else (lambda t: H.act_to_split(t, fmt="f16"), H.act_from_split, "f16")
    xs, rs = to_act(x), (to_act(r) if res else None)
    wp, un = H.pack_conv_weights_wino(_g(wt))
    y = H.conv3d_wino(xs, wp, _g(sc) * un, _g(sh), res=rs, neg_slope=slope, out_f32=out_f32)
    assert out_f32 or y.fmt == fmt
    got = (y if out_f32 else from_act(y)).cpu().numpy()
    ref = _conv_ref64(from_act(xs), wt, sc, sh, slope, res=from_act(rs) if res else None)
    assert _rel(got, ref) <= 5e-6
    if not out_f32:
        for sl in (y.buf[:, 0], y.buf[:, -1], y.buf[:, :, 0], y.buf[:, :, -1], y.buf[:, :, :, 0], y.buf[:, :, :, -1]):
            assert int(sl.abs().max()) == 0
    if act32:
        with pytest.raises(AssertionError, match="does not match the input"):      # a residual in the other activation format
            H.conv3d_wino(xs, wp, _g(sc) * un, _g(sh), res=H.act_to_split(r, fmt="f16"))
        return
        # the direct kernel in the same split on the same operands: the two forms agree far inside either one's error against the reference
        wpd, und = H.pack_conv_weights_rs(_g(wt), "f16")
        yd = H.act_from_split(H.conv3d_rs(xs, wpd, _g(sc) * und, _g(sh), res=rs, neg_slope=slope)).cpu().numpy()
        assert _rel(got, yd) <= 5e-6


def test_conv3d_winograd_weights_range_and_misuse():
    """The packed weights are U = G g G^T, pre-scaled per cout by a power of two into (512, 1024] and split; saturating inputs stay
    finite; geometries and formats the kernel does not serve are refused, not mis-served."""
    rng = np.random.default_rng(181)
    wt = (rng.standard_normal((32, 32, 3, 3, 3)) * np.exp(rng.uniform(-6, 6, (32, 1, 1, 1, 1)))).astype(np.float32)
    wt[5] = 0.0                                                         # a dead channel keeps k = 0
    wp, un = H.pack_conv_weights_wino(_g(wt))
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
    U = np.einsum("ah,bw,oidhw->abdoi", G, G, wt.astype(np.float64))                 # [a, b, kd, co, ci]
    amax = np.abs(U).max(axis=(0, 1, 2, 4))
    unh = un.cpu().numpy().astype(np.float64)
    live = amax > 0
    assert (np.log2(unh) == np.round(np.log2(unh))).all() and unh[5] == 1.0
    assert ((amax[live] / unh[live] > 512 * (1 - 1e-6)) & (amax[live] / unh[live] <= 1024 * (1 + 1e-6))).all()
    f = wp.cpu().numpy().view(np.float16).reshape(4, 4, 3, 2, 2, 4, 16, 8).astype(np.float64)      # [a, b, kd, ct, hl, kg, co16, j]
    back = (f[:, :, :, :, 0] + f[:, :, :, :, 1]).transpose(0, 1, 2, 3, 5, 4, 6).reshape(4, 4, 3, 32, 32)  # [a, b, kd, co, ci]
    assert np.abs(back * unh[None, None, None, :, None] - U).max() <= 2.0 ** -20 * np.abs(U).max()
    # inputs at the end of fp16's range: the transform's sums are clamped, nothing turns into inf / nan
    x = torch.full((1, 8, 2, 32, 32), 65504.0, device=DEV)
    xs = H.act_to_split(x, fmt="f16")
    w1 = np.zeros((32, 32, 3, 3, 3), np.float32)
    w1[:, :, 1, 1, 1] = 1.0 / 32
    wp1, un1 = H.pack_conv_weights_wino(_g(w1))
    y = H.act_from_split(H.conv3d_wino(xs, wp1, torch.ones(32, device=DEV) * un1, torch.zeros(32, device=DEV), neg_slope=0.01))
    assert bool(torch.isfinite(y).all()) and float(y.max()) <= 65504.0
    assert not H.conv3d_wino_applies(32, 32, 7, 4, 32, 1, 0.01) and not H.conv3d_wino_applies(32, 32, 8, 3, 32, 1, 0.01)
    assert H.conv3d_wino_applies(32, 32, 16, 4, 32, 1, 0.01) and not H.conv3d_wino_applies(32, 32, 12, 4, 32, 1, 0.01)
    assert not H.conv3d_wino_applies(32, 32, 8, 4, 48, 1, 0.01) and not H.conv3d_wino_applies(16, 32, 8, 4, 32, 1, 0.01)
    with pytest.raises(RuntimeError, match="needs D == 8"):
        H.conv3d_wino(H.act_to_split(torch.zeros((1, 4, 4, 32, 32), device=DEV), fmt="f16"), wp1, un1, un1)
    with pytest.raises(AssertionError, match="fp16 split"):
        H.conv3d_wino(H.act_to_split(torch.zeros((1, 8, 4, 32, 32), device=DEV)), wp1, un1, un1)
    with pytest.raises(AssertionError, match="wrong size"):
        H.conv3d_wino(xs, wp1[:-16], un1, un1)
    # fp32-padded activations are written clamped to +-16376 (the transform then needs no clamp of its own): by the converter, by the
    # stride-2 kernel, by the Winograd kernel's padded output
    big = torch.full((1, 8, 2, 32, 32), 3.0e4, device=DEV)
    xp = H.act_to_f32p(big)
    assert float(H.act_from_f32p(xp).max()) == H.F32P_MAX
    yp = H.conv3d_wino(xp, wp1, torch.ones(32, device=DEV) * un1 * 8.0, torch.zeros(32, device=DEV), neg_slope=0.01)
    back = H.act_from_f32p(yp)
    assert yp.fmt == "f32p" and bool(torch.isfinite(back).all()) and float(back.max()) == H.F32P_MAX
    # the stride-2 kernel's fp32-padded output exists in the fp16 split only
    x16 = torch.zeros((1, 4, 4, 32, 16), device=DEV)
    w16 = _g(np.zeros((32, 16, 3, 3, 3), np.float32))
    wpb = H.pack_conv_weights_s2rs(w16, torch.ones(32, device=DEV))
    with pytest.raises(RuntimeError, match="fp16 split only"):
        H.conv3d_s2rs(H.act_to_split(x16), wpb, torch.zeros(32, device=DEV), H.SplitAct(1, 2, 2, 16, 32, DEV), out_f32p=True)


@pytest.mark.parametrize("shape", [(1, 4, 4, 16), (2, 5, 7, 37), (3, 10, 30, 150)])
def test_front_end_kernels_in_the_fp16_split_vs_oracle(shape):
    """post_vol (16 -> 16, both outputs) and the stride-2 first layer (16 -> 32, LDS-DMA staging, one power of two for the layer) in
    the fp16 split; post_vol's split-padded output is bit for bit the fp16 split of its fp32 output."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 17)
    x = _g(rng.standard_normal((B, d, h, w, 16), dtype=np.float32))
    w16 = (rng.standard_normal((16, 16, 3, 3, 3)) / np.sqrt(27 * 16)).astype(np.float32)
    sc, sh = _bn(rng, 16)
    xs = H.act_to_split(x, fmt="f16")
    wp, un = H.pack_conv_weights_rs(_g(w16), "f16")
    y = H.conv3d_rs16(xs, wp, _g(sc) * un, _g(sh), neg_slope=0.01)
    assert _rel(y.cpu().numpy(), _conv_ref64(H.act_from_split(xs), w16, sc, sh, 0.01)) <= 5e-6
    ys = H.conv3d_rs16(xs, wp, _g(sc) * un, _g(sh), neg_slope=0.01, out_split=H.SplitAct(B, d, h, w, 16, x.device))
    assert ys.fmt == "f16" and torch.equal(ys.buf, H.act_to_split(y, fmt="f16").buf)
    w32 = (rng.standard_normal((32, 16, 3, 3, 3)) / np.sqrt(27 * 16)).astype(np.float32)
    sc2, sh2 = _bn(rng, 32)
    wp2, up, un2 = H.pack_conv_weights_s2rs(_g(w32), _g(sc2), "f16")
    assert 512.0 < float((np.abs(w32).reshape(32, -1).max(1) * np.abs(sc2)).max()) * up <= 1024.0 and up * un2 == 1.0
    do, ho, wo = (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    z = H.conv3d_s2rs(ys, wp2, _g(sh2) * up, H.SplitAct(B, do, ho, wo, 32, x.device), neg_slope=0.01, unscale=un2)
    assert z.fmt == "f16"
    assert _rel(H.act_from_split(z).cpu().numpy(), _conv_ref64(H.act_from_split(ys), w32, sc2, sh2, 0.01, stride=2)) <= 5e-6
    # the fp32-padded output (for a Winograd-form level 0 behind it): the same values before the split, the border untouched
    z32 = H.conv3d_s2rs(ys, wp2, _g(sh2) * up, H.SplitAct(B, do, ho, wo, 32, x.device), neg_slope=0.01, unscale=un2, out_f32p=True)
    assert z32.fmt == "f32p" and torch.equal(H.act_to_split(H.act_from_f32p(z32), fmt="f16").buf, z.buf)
    for sl in (z32.buf[:, 0], z32.buf[:, -1], z32.buf[:, :, 0], z32.buf[:, :, -1], z32.buf[:, :, :, 0], z32.buf[:, :, :, -1]):
        assert int(sl.abs().max()) == 0


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 2, 4, 16), (3, 5, 9, 33), (2, 8, 40, 160)])
def test_conv3d_up2_polyphase_in_the_fp16_split_vs_interpolate_then_conv(shape):
    """The polyphase ResizeConv3d (main kernel, face and edge corrections, plan) in the fp16 split against interpolate -> conv in
    float64 on the low-resolution input it staged; its split-padded output is the fp16 split of its fp32 output."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 18)
    x = _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32))
    wt = (rng.standard_normal((16, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32)
    sc, sh = _bn(rng, 16)
    xs = H.act_to_split(x, fmt="f16")
    plan, un = H.conv3d_up2_poly_plan(_g(wt), d, h, w, fmt="f16")
    y = H.conv3d_up2_poly(xs, plan, _g(sc) * un, _g(sh), neg_slope=0.01)
    up = F.interpolate(H.act_from_split(xs).cpu().double().permute(0, 4, 1, 2, 3), scale_factor=2, mode="trilinear", align_corners=False)
    ref = F.conv3d(up, torch.from_numpy(wt).double(), padding=1) * torch.from_numpy(sc).double().view(1, -1, 1, 1, 1) \
        + torch.from_numpy(sh).double().view(1, -1, 1, 1, 1)
    ref = torch.where(ref > 0, ref, ref * 0.01).permute(0, 2, 3, 4, 1).float().numpy()
    assert _rel(y.cpu().numpy(), ref) <= 5e-6
    ys = H.conv3d_up2_poly_split(xs, plan, _g(sc) * un, _g(sh), out=H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, x.device), neg_slope=0.01, direct=True)
    assert ys.fmt == "f16" and torch.equal(ys.buf, H.act_to_split(y, fmt="f16").buf)          # (the direct main kernel: the same sums)


@pytest.mark.parametrize("shape", [(1, 8, 2, 32), (1, 8, 4, 64), (3, 8, 6, 32), (2, 8, 40, 160), (7, 8, 40, 160)])
def test_conv3d_up2_polyphase_winograd_form_vs_interpolate_then_conv(shape):
    """K3w (csrc/conv3d_wino_up2.hip): the polyphase ResizeConv3d's main kernel as polyphase over (H, W) x Winograd F(2x2, 3x3) x an
    explicit depth upsample on the transformed planes, against interpolate -> conv in float64 (common_modules.py:332-355) on the
    low-resolution input it staged and against the direct main kernel -- one unit, one unit per role and XCD, ragged walks (600 and
    2100 units on 256 workgroups); face and edge corrections through the residual path; every output plane incl. the first and the last
    (the upsample's clamp and the zero padding of the UPSAMPLED grid along D need no boundary weights in this form)."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 19)
    x = _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32))
    wt = (rng.standard_normal((16, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32)
    sc, sh = _bn(rng, 16)
    xs = H.act_to_split(x, fmt="f16")
    plan, un = H.conv3d_up2_poly_plan(_g(wt), d, h, w, fmt="f16")
    up = F.interpolate(H.act_from_split(xs).cpu().double().permute(0, 4, 1, 2, 3), scale_factor=2, mode="trilinear", align_corners=False)
    ref = F.conv3d(up, torch.from_numpy(wt).double(), padding=1) * torch.from_numpy(sc).double().view(1, -1, 1, 1, 1) \
        + torch.from_numpy(sh).double().view(1, -1, 1, 1, 1)
    ref = torch.where(ref > 0, ref, ref * 0.01).permute(0, 2, 3, 4, 1).numpy()
    out = H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, x.device)
    yw = H.act_from_split(H.conv3d_up2_poly_split(xs, plan, _g(sc) * un, _g(sh), out=out, neg_slope=0.01, wino=True)).cpu().numpy()
    border = out.buf.clone()
    border[:, 1:-1, 1:-1, 1:-1] = 0
    assert out.fmt == "f16" and int(border.abs().max()) == 0                       # the zero border is never written
    err = np.abs(yw - ref).reshape(B, 2 * d, -1).max(axis=(0, 2)) / np.abs(ref).max()
    print(f"winograd-form polyphase {shape}: max-rel per output plane {np.array2string(err, precision=2)}")
    assert err.max() <= 5e-6, err
    yd = H.act_from_split(H.conv3d_up2_poly_split(xs, plan, _g(sc) * un, _g(sh), out=H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, x.device),
                                                  neg_slope=0.01, direct=True)).cpu().numpy()
    assert _rel(yw, yd) <= 5e-6
    # a second call over its own output (the corrections overwrite the face records first), and the dispatcher's own choice
    again = H.act_from_split(H.conv3d_up2_poly_split(xs, plan, _g(sc) * un, _g(sh), out=out, neg_slope=0.01, wino=True)).cpu().numpy()
    assert np.array_equal(again, yw)
    auto = H.act_from_split(H.conv3d_up2_poly_split(xs, plan, _g(sc) * un, _g(sh), out=out, neg_slope=0.01)).cpu().numpy()
    assert np.array_equal(auto, yw if H.conv3d_up2_poly_wino_pays(B, d, h, w) else yd)
    with pytest.raises(RuntimeError, match="Winograd form needs"):
        H.conv3d_up2_poly_split(H.act_to_split(x), H.conv3d_up2_poly_plan(_g(wt), d, h, w), _g(sc), _g(sh), out=out, wino=True)


def test_sweep_split_padded_output_in_the_fp16_split(golden_dir):
    """The sweep writing vol_raw as fp16 pairs: the fp16 split of the bit-exact fp32 volume."""
    case = SMALL_CASES["std_d16_rand"]
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    feats, grids = _g(inp["feats"]), _g(inp["grids"])
    vm = H.sweep_validity(grids, _g(inp["grid_masks"]), _g(inp["masks"]))
    vol = H.sweep_std_valid(feats, grids, vm)
    B, D, Ho, Wo, C = vol.shape
    vs = H.sweep_std_valid_split(feats, grids, vm, out=H.SplitAct(B, D, Ho, Wo, C, feats.device), fmt="f16")
    assert vs.fmt == "f16" and torch.equal(vs.buf, H.act_to_split(vol, fmt="f16").buf)


@pytest.mark.parametrize("shape", [(1, 32, 16, 1, 1, 1), (2, 32, 16, 3, 5, 9), (1, 96, 16, 2, 4, 20), (1, 64, 48, 2, 5, 17)])
def test_cost_head_in_the_fp16_split_behind_a_streaming_layer(shape):
    """The tail of a regulator in f16x3 mode: ResizeConv3d on the streaming kernel writing fp16 pairs split-padded, the split cost
    head reading them (mvsgi_conv3d_head_split_f16) -- against the exact-fp32 head on the same layer's fp32 output; a buffer of the
    other split is refused."""
    B, cin, cmid, dl, hl, wl = shape
    rng = np.random.default_rng(sum(shape))
    xl = _g(rng.standard_normal((B, dl, hl, wl, cin), dtype=np.float32))
    w0 = _g((rng.standard_normal((cmid, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32))
    sc, sh = _g(rng.uniform(0.5, 1.5, cmid).astype(np.float32)), _g((rng.standard_normal(cmid) * 0.1).astype(np.float32))
    w1 = _g((rng.standard_normal((1, cmid, 3, 3, 3)) / np.sqrt(27 * cmid)).astype(np.float32))
    layout = H.CONV_BF16X3_C16 if cmid == 16 else H.CONV_BF16X3
    wp, un = H.pack_conv_weights_f16x3(w0, layout)
    mid = H.conv3d_up2(xl, wp, sc * un, sh, neg_slope=0.01, w_layout=layout | H.CONV_F16)
    buf = H.SplitAct(B, 2 * dl, 2 * hl, 2 * wl, cmid, xl.device)
    H.conv3d_up2_out_split(xl, wp, sc * un, sh, out=buf, neg_slope=0.01, w_layout=layout | H.CONV_F16)
    assert buf.fmt == "f16"
    wph, unh = H.pack_head_split_weights_f16(w1)
    got = H.conv3d_head_split(buf, wph, 1.0 * unh, 0.25, neg_slope=1.0, f16=True).cpu().numpy()
    one, q = torch.ones(1, device=DEV), torch.full((1,), 0.25, device=DEV)
    ref = H.conv3d(mid, w1, H.pack_conv_weights(w1), one, q, neg_slope=1.0, impl=H.CONV_MFMA).cpu().numpy()
    assert _rel(got, ref) <= 5e-6
    with pytest.raises(AssertionError, match="holding f16"):
        H.conv3d_head_split(buf, H.pack_head_split_weights(w1), 1.0, 0.25)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 2, 4, 16), (3, 5, 9, 33), (2, 8, 40, 160)])
def test_polyphase_split_padded_output_is_the_split_of_its_fp32_output(shape):
    """The polyphase layer writing split-padded (the cost head's input): bit for bit the split of its fp32 result, border zero."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 1)
    x = _g(rng.standard_normal((B, d, h, w, 32), dtype=np.float32))
    wt = _g((rng.standard_normal((16, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32))
    sc, sh = _g(rng.uniform(0.5, 1.5, 16).astype(np.float32)), _g((rng.standard_normal(16) * 0.1).astype(np.float32))
    xs = H.act_to_split(x)
    plan = H.conv3d_up2_poly_plan(wt, d, h, w)
    y = H.conv3d_up2_poly(xs, plan, sc, sh)
    ys = H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, x.device)
    ys.buf.fill_(0x7fc07fc0 - (1 << 32) if False else 0)           # (zero border: allocated zero-filled)
    H.conv3d_up2_poly_split(xs, plan, sc, sh, out=ys)
    assert torch.equal(ys.buf, H.act_to_split(y).buf)
    H.conv3d_up2_poly_split(xs, plan, sc, sh, out=ys)              # a second call over its own output (corrections overwrite records first)
    assert torch.equal(ys.buf, H.act_to_split(y).buf)
