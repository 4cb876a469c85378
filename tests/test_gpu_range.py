"""GPU (MI355X) tests of the fp16 split's RANGE REPORT (include/mvsgi.h: mvsgi_saturation_flags): the reference computes in fp32 with no
clamp (dsta_mvs/model/common/common_modules.py:105-115, distance_regressor/distance_regressor.py:51-79), the default arithmetic
saturates at +-65504 (+-16376 on the Winograd level) -- every kernel that clamps must raise its sticky flag exactly when its clamp
engaged, the bf16 split and the fp32 outputs never, and the Python layer must turn the flag into an exception by default.
Also here: how far one frame's result depends on how many frames share its launch in the default mode (the Winograd / direct dispatch
follows the batch), stated as a tolerance instead of the exact-fp32 mode's bit equality."""
import warnings

import numpy as np
import pytest
import torch

from golden_cases import SMALL_CASES
import guard_arena
from mvs_gi_amd import hip_ops as H, synth
from mvs_gi_amd.pipeline import HotPath

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor the library allocates during a test of this module sits between NaN-sentinel guards, and unwritten
    fp32 outputs read as NaN (tests/guard_arena.py: what is guarded, guard sizes, exemptions)."""
    yield from guard_arena.fixture_body(request)


@pytest.fixture(autouse=True)
def _clean_report():
    mode, policy = H.get_conv_mode(), H.get_range_check()
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    H.set_conv_mode(mode)
    H.set_range_check(policy)
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)


def _flags() -> int:
    """flags raised by everything submitted so far (then cleared)"""
    torch.cuda.synchronize()
    return H.saturation_flags(clear=True)


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _centre(cout, cin, value=1.0):
    """[cout, cin, 3, 3, 3] weights whose centre tap copies channel co % cin: y[co] = value * x[co % cin]"""
    w = np.zeros((cout, cin, 3, 3, 3), np.float32)
    for co in range(cout):
        w[co, co % cin, 1, 1, 1] = value
    return w


def _ones(n, v=1.0):
    return torch.full((n,), float(v), device=DEV)


def _zeros(n):
    return torch.zeros(n, device=DEV)


# ------------------------------------------------------------------------------------------------ the C entry point itself
def test_flags_are_sticky_cleared_on_request_and_silent_inside_the_range():
    x = torch.full((1, 2, 4, 16, 32), 6.0e4, device=DEV)
    H.act_to_split(x, fmt="f16")
    assert _flags() == 0                                           # inside fp16's range: nothing
    x[0, 1, 2, 3, 5] = 6.6e4
    xs = H.act_to_split(x, fmt="f16")
    torch.cuda.synchronize()
    assert H.saturation_flags() == H.SAT_SPLIT and H.saturation_flags() == H.SAT_SPLIT      # sticky until cleared
    assert H.saturation_flags(clear=True) == H.SAT_SPLIT and H.saturation_flags() == 0
    assert float(H.act_from_split(xs).max()) == 65504.0            # ... and the value was clamped, not inf
    x[0, 1, 2, 3, 5] = -7.0e4
    H.act_to_split(x, fmt="f16")
    assert _flags() == H.SAT_SPLIT
    H.act_to_split(x, fmt="bf16")                                  # the bf16 split has fp32's range: never
    assert _flags() == 0
    # ragged launch (the last workgroup is partly dead): still reported, from a live lane only
    y = torch.zeros((1, 1, 1, 3, 16), device=DEV)
    y[0, 0, 0, 2, 15] = 1.0e9
    H.act_to_split(y, fmt="f16")
    assert _flags() == H.SAT_SPLIT


# ------------------------------------------------------------------------------------------------ every kernel that clamps
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_register_stationary_convs_report_a_clamped_output(fmt):
    """K2e (32 -> 32), K2f (16 -> 16, post_vol) and K3 (polyphase out_costs.0): the split-padded output raises SAT_SPLIT when a value
    reaches +-65504 in the fp16 split; the fp32 outputs and the bf16 split never do."""
    f16 = fmt == "f16"
    x32 = H.act_to_split(torch.full((2, 4, 8, 32, 32), 100.0, device=DEV), fmt=fmt)
    p = H.pack_conv_weights_rs(_g(_centre(32, 32)), fmt)
    wp, un = p if f16 else (p, _ones(32))
    for s, want in ((100.0, 0), (700.0, H.SAT_SPLIT if f16 else 0), (-7.0e4, H.SAT_SPLIT if f16 else 0)):
        y = H.conv3d_rs(x32, wp, un * s, _zeros(32), neg_slope=1.0)
        assert _flags() == want, (s, want)
        if f16 and want:
            assert float(H.act_from_split(y).abs().max()) == 65504.0
        H.conv3d_rs(x32, wp, un * s, _zeros(32), neg_slope=1.0, out_f32=True)            # fp32 out: no clamp, no report
        assert _flags() == 0
    x16 = H.act_to_split(torch.full((2, 5, 7, 37, 16), 100.0, device=DEV), fmt=fmt)
    p = H.pack_conv_weights_rs(_g(_centre(16, 16)), fmt)
    wp, un = p if f16 else (p, _ones(16))
    for s, want in ((100.0, 0), (700.0, H.SAT_SPLIT if f16 else 0)):
        H.conv3d_rs16(x16, wp, un * s, _zeros(16), out_split=H.SplitAct(2, 5, 7, 37, 16, DEV))
        assert _flags() == want, (s, want)
        H.conv3d_rs16(x16, wp, un * s, _zeros(16))
        assert _flags() == 0
    # polyphase: every phase's folded weights sum to the centre tap's on a constant interior
    xl = H.act_to_split(torch.full((1, 4, 8, 32, 32), 100.0, device=DEV), fmt=fmt)
    p = H.conv3d_up2_poly_plan(_g(_centre(16, 32)), 4, 8, 32, fmt)
    plan, un = p if f16 else (p, _ones(16))
    for s, want in ((100.0, 0), (700.0, H.SAT_SPLIT if f16 else 0)):
        H.conv3d_up2_poly_split(xl, plan, un * s, _zeros(16), H.SplitAct(1, 8, 16, 64, 16, DEV), neg_slope=0.01)
        assert _flags() == want, (s, want)
        H.conv3d_up2_poly(xl, plan, un * s, _zeros(16), neg_slope=0.01)
        assert _flags() == 0


def test_stride2_first_layer_reports_both_of_its_ranges():
    """K2g: the split-padded output clamps at +-65504 (SAT_SPLIT), the fp32-padded one at +-16376 (SAT_WINO: the range a Winograd
    layer behind it needs); the bf16 split has neither."""
    x = H.act_to_split(torch.full((2, 6, 10, 34, 16), 100.0, device=DEV), fmt="f16")
    out = lambda: H.SplitAct(2, 3, 5, 17, 32, DEV)
    for s, f32p, want in ((100.0, False, 0), (700.0, False, H.SAT_SPLIT), (160.0, True, 0), (170.0, True, H.SAT_WINO), (-170.0, True, H.SAT_WINO)):
        wp, up, un = H.pack_conv_weights_s2rs(_g(_centre(32, 16)), _ones(32, s), "f16")
        y = H.conv3d_s2rs(x, wp, _zeros(32), out(), neg_slope=1.0, unscale=un, out_f32p=f32p)
        assert _flags() == want, (s, f32p, want)
        if f32p and want:
            assert float(H.act_from_f32p(y).abs().max()) == H.F32P_MAX
    xb = H.act_to_split(torch.full((2, 6, 10, 34, 16), 100.0, device=DEV), fmt="bf16")
    H.conv3d_s2rs(xb, H.pack_conv_weights_s2rs(_g(_centre(32, 16)), _ones(32, 1.0e6)), _zeros(32), out(), neg_slope=1.0)
    assert _flags() == 0


def test_streaming_kernel_reports_staged_inputs_and_split_outputs():
    """The streaming split kernel (every layer with channel counts beyond 32): its PRODUCER waves clamp the fp32 activations they
    stage (plain and fused-upsample paths), its epilogue clamps a split-padded output."""
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((64, 64, 3, 3, 3)) / np.sqrt(27 * 64)).astype(np.float32)
    wp, un = H.pack_conv_weights_f16x3(_g(w))
    wb = H.pack_conv_weights_bf16x3(_g(w))
    x = _g(rng.standard_normal((2, 4, 8, 16, 64), dtype=np.float32))
    H.conv3d(x, None, wp, un.clone(), _zeros(64), impl=H.CONV_BF16X3 | H.CONV_F16)
    assert _flags() == 0
    big = x.clone()
    big[1, 2, 3, 4, 5] = 1.0e5                                     # ONE staged value beyond the range
    y = H.conv3d(big, None, wp, un.clone(), _zeros(64), impl=H.CONV_BF16X3 | H.CONV_F16)
    assert _flags() == H.SAT_SPLIT and bool(torch.isfinite(y).all())
    H.conv3d(big, None, wb, _ones(64), _zeros(64), impl=H.CONV_BF16X3)          # bf16 split: no range to leave
    assert _flags() == 0
    # stride 2 (the 12-voxel staging of a stride-2 brick) and the fused trilinear upsample in the producers
    H.conv3d(big, None, wp, un.clone(), _zeros(64), stride=2, impl=H.CONV_BF16X3 | H.CONV_F16)
    assert _flags() == H.SAT_SPLIT
    H.conv3d_up2(x[:, :2, :4, :8].contiguous(), wp, un.clone(), _zeros(64), w_layout=H.CONV_BF16X3 | H.CONV_F16)
    assert _flags() == 0
    H.conv3d_up2(big[:, :4, :4, :8].contiguous(), wp, un.clone(), _zeros(64), w_layout=H.CONV_BF16X3 | H.CONV_F16)
    assert _flags() == 0                                           # (the blend spreads ONE 1e5 voxel: 0.75^3 of it at most = 4.2e4)
    H.conv3d_up2(big[:, :4, :4, :8].contiguous() * 10.0, wp, un.clone(), _zeros(64), w_layout=H.CONV_BF16X3 | H.CONV_F16)
    assert _flags() == H.SAT_SPLIT
    # the epilogue's split-padded output
    wc, unc = H.pack_conv_weights_f16x3(_g(_centre(64, 64)))
    c = torch.full((1, 4, 8, 16, 64), 100.0, device=DEV)
    for s, want in ((100.0, 0), (700.0, H.SAT_SPLIT)):
        H.conv3d_out_split(c, wc, unc * s, _zeros(64), H.SplitAct(1, 4, 8, 16, 64, DEV), neg_slope=1.0, fmt="f16")
        assert _flags() == want, s


def test_sweep_reports_a_cost_volume_beyond_fp16():
    """The sweep's split-padded output -- the one un-normalised tensor of the path (a variance of the caller's features)."""
    case = SMALL_CASES["std_d8"]
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=1, grid_kind="smooth", grid_mask_dtype="bool")
    g, gm, m = _g(inp["grids"]), _g(inp["grid_masks"]), _g(inp["masks"])
    vm = H.sweep_validity(g, gm, m)
    B, D, (Ho, Wo) = 1, cfg.num_cands, cfg.cv_hw
    for scale, fmt, want in ((1.0, "f16", 0), (300.0, "f16", H.SAT_SWEEP), (300.0, "bf16", 0)):
        H.sweep_std_valid_split(_g(inp["feats"] * np.float32(scale)), g, vm, H.SplitAct(B, D, Ho, Wo, 16, DEV), fmt=fmt)
        assert _flags() == want, (scale, fmt)


def test_winograd_level_clamps_behind_the_activation_and_reports():
    """K2w.  The fp32-padded epilogue clamps AFTER LeakyReLU (round 5's form let t * neg_slope > 16376 through: any t > 16376 at slope
    1, t > 1.6e6 at slope 0.01 -- unclamped records whose sums of four overflow fp16 in the next layer's transform: inf, then nan);
    a clamp that engages raises SAT_WINO; the plain fp32 output has no range."""
    w1 = np.zeros((32, 32, 3, 3, 3), np.float32)
    w1[:, :, 1, 1, 1] = 1.0 / 32                                   # y[co] = mean over the input channels
    wp, un = H.pack_conv_weights_wino(_g(w1))
    xp = H.act_to_f32p(torch.full((1, 8, 4, 64, 32), 100.0, device=DEV))
    for s, slope, want, lim in ((100.0, 0.01, 0, 1.0e4), (170.0, 0.01, H.SAT_WINO, H.F32P_MAX), (170.0, 1.0, H.SAT_WINO, H.F32P_MAX),
                                (-170.0, 1.0, H.SAT_WINO, H.F32P_MAX), (3.0e4, 0.01, H.SAT_WINO, H.F32P_MAX), (-3.0e8, 0.01, H.SAT_WINO, H.F32P_MAX)):
        y = H.conv3d_wino(xp, wp, un * s, _zeros(32), neg_slope=slope)
        assert _flags() == want, (s, slope)
        back = H.act_from_f32p(y)
        top = float(back.abs().max())
        assert y.fmt == "f32p" and bool(torch.isfinite(back).all()) and (top == lim if want else abs(top - lim) <= 1.0), (s, slope, top)
        # ... and chained through two more layers on fp32-padded records (whose transforms carry no clamp of their own): finite
        z = H.conv3d_wino(H.conv3d_wino(y, wp, un * 4.0, _zeros(32), neg_slope=slope), wp, un * 4.0, _zeros(32), neg_slope=slope)
        assert bool(torch.isfinite(H.act_from_f32p(z)).all()), (s, slope)
        _flags()
        H.conv3d_wino(xp, wp, un * s, _zeros(32), neg_slope=slope, out_f32=True)          # plain fp32 out: no clamp, no report
        assert _flags() == 0
    # fp16 pairs: the transform's sums of four (x1 + x2 of a constant 6e4 volume = 1.2e5) and the split output are clamped at +-65504
    xs = H.act_to_split(torch.full((1, 8, 4, 64, 32), 6.0e4, device=DEV), fmt="f16")
    assert _flags() == 0
    y = H.conv3d_wino(xs, wp, un.clone(), _zeros(32), neg_slope=0.01)
    assert _flags() == H.SAT_WINO and bool(torch.isfinite(H.act_from_split(y)).all())
    xs = H.act_to_split(torch.full((1, 8, 4, 64, 32), 100.0, device=DEV), fmt="f16")
    H.conv3d_wino(xs, wp, un.clone(), _zeros(32), neg_slope=0.01)
    assert _flags() == 0
    H.conv3d_wino(xs, wp, un * 700.0, _zeros(32), neg_slope=0.01)
    assert _flags() == H.SAT_WINO


def test_polyphase_winograd_form_saturates_in_the_conversion_and_reports():
    """K3w (csrc/conv3d_wino_up2.hip) carries no clamp instruction: it runs under MODE.FP16_OVFL, where the fp32 -> fp16 conversions of
    its transformed planes and of its output saturate at +-65504 by themselves (tools/ubench/fp16_ovfl_trapsts.hip); the range report
    sees the values in front of the conversion."""
    plan, un = H.conv3d_up2_poly_plan(_g(_centre(16, 32)), 8, 4, 32, "f16")
    xs = H.act_to_split(torch.full((2, 8, 4, 32, 32), 100.0, device=DEV), fmt="f16")
    for s, want in ((100.0, 0), (700.0, H.SAT_SPLIT), (-7.0e6, H.SAT_SPLIT)):
        y = H.act_from_split(H.conv3d_up2_poly_split(xs, plan, un * s, _zeros(16), H.SplitAct(2, 16, 8, 64, 16, DEV), neg_slope=1.0, wino=True))
        assert _flags() == want, s
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) <= 2 * 65504.0
        if not want:
            assert abs(float(y.abs().max()) - 100.0 * s) <= 1.0
    # the transformed planes: x1 + x2 of a constant 6e4 volume = 1.2e5 saturates in the conversion of V
    xs = H.act_to_split(torch.full((2, 8, 4, 32, 32), 6.0e4, device=DEV), fmt="f16")
    assert _flags() == 0
    y = H.act_from_split(H.conv3d_up2_poly_split(xs, plan, un * 1.0e-3, _zeros(16), H.SplitAct(2, 16, 8, 64, 16, DEV), neg_slope=1.0, wino=True))
    assert _flags() == H.SAT_SPLIT and bool(torch.isfinite(y).all())


# ------------------------------------------------------------------------------------------------ the Python layer's policy
def _small_hot_path(gain=1e-5):
    case = SMALL_CASES["std_d16_rand"]
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind="smooth", grid_mask_dtype="bool")
    return HotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=gain), inp, device=DEV), _g(inp["feats"])


def test_default_mode_raises_when_a_frame_leaves_the_range_and_bf16x3_is_silent():
    """Features 300x too large: in the default arithmetic the cost volume is clamped -- a caller of HotPath gets an exception (from
    check_range() for the frame itself, from the next call for an earlier frame), never a silently saturated map; the same frames in
    the bf16 split (fp32's range) raise nothing."""
    H.set_conv_mode("f16x3")
    H.set_range_check("raise")
    hp, feats = _small_hot_path()
    big = feats * 300.0
    ok, _ = hp(feats)
    assert hp.check_range() == 0                                    # in-range frames: silent
    hp(big)
    with pytest.raises(H.MvsgiRangeError, match="bf16x3") as e:
        hp.check_range()                                            # synchronises, reports THIS frame
    assert "left its range" in str(e.value) and H.saturation_flags() == 0        # reported once, cleared
    hp(big)
    torch.cuda.synchronize()
    with pytest.raises(H.MvsgiRangeError, match="an earlier frame"):
        hp(feats)                                                   # the entry check of the next call
    again, _ = hp(feats)                                            # ... after which the path carries on
    assert hp.check_range() == 0 and torch.equal(again, ok)
    # policy "warn": one warning per kind, results still delivered; "off": nothing
    H.set_range_check("warn")
    H._RANGE_WARNED.clear()
    hp(big)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert hp.check_range() != 0
        hp(big)
        assert hp.check_range() != 0
    assert len([r for r in rec if "left its range" in str(r.message)]) == 1
    H.set_range_check("off")
    hp(big)
    assert hp.check_range() == 0 and _flags() != 0                  # ("off" neither reads nor clears)
    # the answer the message gives: the bf16 split
    H.set_range_check("raise")
    H.set_conv_mode("bf16x3")
    hpb, _ = _small_hot_path()
    hpb(big)
    assert hpb.check_range() == 0
    H.set_conv_mode("f32")
    hpf, _ = _small_hot_path()
    hpf(big)
    assert hpf.check_range() == 0


def test_precision_check_reads_the_report_and_survives_non_finite_outputs():
    """precision_check: a frame that saturates the fp16 split is sent to the exact mode whatever the splits' distance, and the fp16
    split is excluded; a non-finite output (an fp32 overflow reaches the bf16 split too) never wins by a nan comparison."""
    H.set_conv_mode("f16x3")
    hp, feats = _small_hot_path()
    chk = hp.precision_check(feats * 300.0)
    assert chk["f16x3_saturated"] != 0 and chk["recommended"] == "bf16x3" and "saturated" in chk["note"]
    assert H.get_range_check() == "raise" and H.get_conv_mode() == "f16x3" and _flags() == 0
    chk = hp.precision_check(feats)
    assert chk["f16x3_saturated"] == 0 and chk["recommended"] == "f16x3" and chk["finite"] == {"bf16x3": True, "f16x3": True}
    chk = hp.precision_check(feats * 1.0e19)          # the variance overflows fp32: inf in every arithmetic
    assert chk["recommended"] == "f32" and not chk["finite"]["bf16x3"]
    _flags()


# ------------------------------------------------------------------------------------------------ batch dependence in the default mode
def test_default_mode_frame_depends_on_its_launch_only_within_the_arithmetic():
    """In the exact-fp32 mode a frame's bits do not depend on how many frames share its launch
    (test_gpu_parity.py::test_full_size_properties_batch_and_determinism).  In the DEFAULT mode they do: the level-0 convs run in
    Winograd form or on the direct kernel depending on the batch (cost_volume_regulator._wino_pays: 1 frame direct, 2 Winograd,
    3 direct, 4 Winograd at G16V's size), and the streaming kernel picks other units at other batch sizes (other summation trees).
    The results are NOT bit-equal; they agree to the arithmetic's own error: asserted <= 1e-4 of the map's maximum (a tenth of the
    north star's bar; measured ~2e-5) and <= 2e-3 per pixel, and both forms stay inside the bar against each other.  Frame sharding
    (bench.py --gpus N) is exact in this sense: the SAME launch geometry on every rank gives the same bits
    (test_bench_sharding.py), other batch sizes give the same answer to 1e-4."""
    from mvs_gi_amd.configs import CONFIGS
    H.set_conv_mode("f16x3")
    cfg = CONFIGS["G16V"]
    inp = synth.make_inputs(cfg, seed=3, batch=1)
    hp = HotPath(cfg, synth.make_weights(cfg, seed=3), inp, device=DEV)
    rng = np.random.default_rng(0)
    frame = _g(rng.standard_normal((1, *inp["feats"].shape[1:]), dtype=np.float32))
    outs = {}
    for B in (1, 2, 3, 4):
        inv, _ = hp(frame.expand(B, -1, -1, -1, -1).contiguous())
        outs[B] = inv.cpu().numpy()
        assert all(np.array_equal(outs[B][0], outs[B][k]) for k in range(1, B))        # equal frames of one launch: equal bits
    assert hp.check_range() == 0
    ref = outs[1][0].astype(np.float64)
    worst, worst_px, equal = 0.0, 0.0, []
    for B in (2, 3, 4):
        d = np.abs(outs[B][0].astype(np.float64) - ref)
        worst, worst_px = max(worst, float(d.max() / np.abs(ref).max())), max(worst_px, float((d / np.abs(ref)).max()))
        equal.append(bool(np.array_equal(outs[B][0], outs[1][0])))
    print(f"default mode, one G16V frame at B = 1 vs 2, 3, 4: max |d| / max |ref| {worst:.3e}, per pixel {worst_px:.3e}, bit-equal {equal}")
    assert worst <= 1e-4 and worst_px <= 2e-3, (worst, worst_px)
    assert not all(equal)           # if this ever holds the dispatch no longer depends on the batch: update DESIGN.md §5


def test_overlapping_copy_stream_overlaps_uploads_with_compute():
    """pipeline.overlapping_copy_stream: the returned stream's pinned H2D copy finishes INSIDE a spin kernel of the compute stream
    (a stream on the compute stream's hardware queue would be served behind it: tools/host_feed_probe.py --queues)."""
    from mvs_gi_amd.pipeline import overlapping_copy_stream
    for _ in range(5):              # whatever position of the round-robin the process is at
        torch.cuda.Stream(device=DEV)
        cs = overlapping_copy_stream(DEV)
        comp = torch.cuda.current_stream(DEV)
        host = torch.empty(8 << 20, dtype=torch.uint8).pin_memory()
        dst = torch.empty(8 << 20, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        c0, c1, k1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        c0.record(comp)
        torch.cuda._sleep(6_000_000)
        c1.record(comp)
        with torch.cuda.stream(cs):
            cs.wait_event(c0)
            dst.copy_(host, non_blocking=True)
            k1.record(cs)
        torch.cuda.synchronize()
        assert c0.elapsed_time(k1) < 0.7 * c0.elapsed_time(c1), (c0.elapsed_time(k1), c0.elapsed_time(c1))
