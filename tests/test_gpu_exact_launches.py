"""GPU (MI355X): the bit-for-bit check of tests/test_gpu_exact.py at LAUNCH SIZE.  The same exact-arithmetic operands, the same
float64 reference, the same comparison (exact_cases.assert_exact: np.array_equal, no tolerance anywhere), at the sizes where

  - the dispatcher names each row of csrc/conv3d_variants.inc (E.VARIANT_ROWS: every MVSGI_B3 row in both splits, every MVSGI_MFMA
    row; the coverage test at the bottom fails when a row x split is named by no case of this module or of test_gpu_exact.py);
  - launch_bf16x3 runs the border-plane-skip kernels (E.BORDER_ROWS: the launch condition restated and asserted, and a control
    one frame below it);
  - a persistent workgroup walks a second and later unit and the last round is ragged (E.WALKS, and the three streaming rows of
    E.WALK_VARIANT_IDS): units >= 2 R + r;
  - the split cost head marches the whole depth in one block (E.HEAD_MARCH_SHAPES: nd = 1).

The weight packers these launches depend on (csrc/presplit_common.hpp, csrc/conv3d_headsplit.hip) are compared byte for byte with
their lane rules, written once here.

A float64 reference of such batches is affordable because frames of a batch are independent: every case is built, and its
conditions (a)-(c) asserted, on E.FRAMES distinct frames which the kernel sees B times in an irregular order (E.frame_index:
neighbouring frames always differ, no period), and the reference is expanded by the same index; the residual is drawn for all B
frames.  The tables are recorded for 256 CUs, like tests/golden/conv3d_dispatch_pin.json: on another CU count the tests skip.
"""
import functools
import os

import numpy as np
import pytest
import torch

import exact_cases as E
import guard_arena
import test_gpu_exact as X
from mvs_gi_amd import hip_ops as H

pytestmark = pytest.mark.gpu
DEV = X.DEV
F16 = H.CONV_F16
_g, _cl, _want, _np, _lsb = X._g, X._cl, X._want, X._np, X._lsb
VARIANTS = E.parse_variants_inc(os.path.join(os.path.dirname(os.path.abspath(H.__file__)), "csrc", "conv3d_variants.inc"))
LAYOUTS = {"generic": H.CONV_BF16X3, "c16": H.CONV_BF16X3_C16, "v32": H.CONV_BF16X3_V32, "d32": H.CONV_BF16X3_D32}
FMTS = ("bf16", "f16")


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor the library allocates during a test of this module sits between NaN-sentinel guards, and unwritten
    fp32 outputs read as NaN (tests/guard_arena.py: what is guarded, guard sizes, exemptions)."""
    yield from guard_arena.fixture_body(request)


@pytest.fixture(autouse=True)
def _range_report_stays_clear():
    """Condition (c): no clamp of the fp16 split or of the fp32-padded records may engage on these operands."""
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    torch.cuda.synchronize()
    flags = H.saturation_flags(clear=True)
    assert flags == 0, f"range report {flags:#x}"


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def _recorded_cu_count():
    if _cus() != E.LAUNCH_CUS:
        pytest.skip(f"the launch-size tables were recorded for {E.LAUNCH_CUS} CUs, this device has {_cus()}")


def _check_frames(c, B):
    assert c.x.shape[0] == B == len(c.idx) and c.n_frames == min(E.FRAMES, B)
    E.check_frame_index(c.idx, B, c.n_frames)


# ------------------------------------------------------------------------------------------------ every row of conv3d_variants.inc
def _run_variant_row(row, fmt, c):
    """Asserts the variant's name (exactly, as csrc/conv3d.hip:variant_name reports it) BEFORE the call, then the bits."""
    name, fn, B, ci, co, D, Hh, W, s, lay = row
    want_name = E.variant_kernel_name(VARIANTS, name, fmt)
    xg, rg, wg, sc, sh = _cl(c.x), _cl(c.r), _g(c.w), _g(c.scale), _g(c.shift)
    if lay == "mfma":
        assert H.conv3d_variant(B, ci, D, Hh, W, co, s, H.CONV_MFMA) == want_name
        y = H.conv3d(xg, wg, H.pack_conv_weights(wg), sc, sh, res=rg, stride=s, neg_slope=c.slope, impl=H.CONV_MFMA)
    else:
        wp, scg, impl = X._pack3d(wg, sc, fmt, LAYOUTS[lay])
        if fn == "conv":
            assert H.conv3d_variant(B, ci, D, Hh, W, co, s, impl) == want_name
            y = H.conv3d(xg, wg, wp, scg, sh, res=rg, stride=s, neg_slope=c.slope, impl=impl)
        else:
            assert H.conv3d_up2_variant(B, ci, D, Hh, W, co, impl) == want_name
            y = H.conv3d_up2(xg, wp, scg, sh, res=rg, neg_slope=c.slope, w_layout=impl)
    E.assert_exact(_np(y), _want(c), _lsb(c), want_name)


_B3_ROWS = [r for r in E.VARIANT_ROWS if r[9] != "mfma"]
_MFMA_ROWS = [r for r in E.VARIANT_ROWS if r[9] == "mfma"]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("row", _B3_ROWS, ids=E.variant_row_id)
def test_streaming_kernel_every_variant_row(row, regime, fmt):
    """One shape per MVSGI_B3 row at which the dispatcher names it: generic, _C16, _V32 (in the fp16 split too: the library takes
    the combination, fused upsample included) and _D32 layouts, plain and fused-upsample."""
    c = E.variant_case(row, fmt, regime)
    _check_frames(c, row[2])
    if E.variant_row_id(row) in E.WALK_VARIANT_IDS:      # units >= 2 R + r: R = 2 workgroups per CU (launch_bf16x3: persistent_geometry(.., 2, ..))
        name, fn, B, ci, co, D, Hh, W, s, lay = row
        up = 2 if fn == "up2" else 1
        units, R = E.streaming_units(VARIANTS, name, B, up * D, up * Hh, up * W, co), 2 * _cus()
        assert units >= 2 * R and units % R and units % _cus(), (units, R)
    _run_variant_row(row, fmt, c)


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("row", _MFMA_ROWS, ids=E.variant_row_id)
def test_fp32_mfma_kernel_every_variant_row(row, regime):
    c = E.variant_case(row, "f32", regime)
    _check_frames(c, row[2])
    _run_variant_row(row, "f32", c)


# ------------------------------------------------------------------------------------------------ the border-plane skip
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("row", E.BORDER_ROWS, ids=lambda r: f"{r[0]}-{r[2]}")
def test_border_plane_skip_kernels(row, regime, fmt):
    """conv3d_{bf16x3,f16x3}_d32[u]_brd_kernel<.., 1 | 2>: launched instead of the named variant when the output is four planes deep
    and a layer of bricks is at least four rounds of the chip.  The condition is restated here with the device's CU count; the
    control row, one frame below it, runs the named kernel itself on the same frames."""
    name, fn, B, ci, co, D, Hh, W, skip = row
    up = 2 if fn == "up2" else 1
    Do, Ho, Wo = up * D, up * Hh, up * W
    layer = E.border_layer(VARIANTS, name, B, Ho, Wo, co)
    assert Do == 4 and (layer >= 4 * _cus()) == skip and (skip or E.border_layer(VARIANTS, name, B + 1, Ho, Wo, co) >= 4 * _cus())
    c = E.border_case(row, fmt, regime)
    _check_frames(c, B)
    _run_variant_row((name, fn, B, ci, co, D, Hh, W, 1, "d32"), fmt, c)


# ------------------------------------------------------------------------------------------------ unit walks
def _walk(family):
    units, R = E.walk_units(family)
    assert E.LAUNCH_CUS == _cus()
    return E.WALKS[family][0]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("regime", E.REGIMES)
def test_unit_walk_conv3d_rs(regime, fmt):
    B = _walk("conv3d_rs")[0]
    c = E.walk_case("conv3d_rs", fmt, regime)
    _check_frames(c, B)
    xs, rs = X._to_split(_cl(c.x), fmt), X._to_split(_cl(c.r), fmt)
    wp, scg = X._rs_pack(_g(c.w), _g(c.scale), fmt)
    y32 = H.conv3d_rs(xs, wp, scg, _g(c.shift), res=rs, neg_slope=c.slope, out_f32=True)
    E.assert_exact(_np(y32), _want(c), _lsb(c), "fp32 output")
    ys = H.conv3d_rs(xs, wp, scg, _g(c.shift), res=rs, neg_slope=c.slope)
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), "split output")
    X._border_is_zero(ys.buf)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("regime", E.REGIMES)
def test_unit_walk_conv3d_rs16(regime, fmt):
    B, d, h, w = _walk("conv3d_rs16")
    c = E.walk_case("conv3d_rs16", fmt, regime)
    _check_frames(c, B)
    xs = X._to_split(_cl(c.x), fmt)
    wp, scg = X._rs_pack(_g(c.w), _g(c.scale), fmt)
    y = H.conv3d_rs16(xs, wp, scg, _g(c.shift), neg_slope=c.slope)
    E.assert_exact(_np(y), _want(c), _lsb(c), "fp32 output")
    ys = H.conv3d_rs16(xs, wp, scg, _g(c.shift), neg_slope=c.slope, out_split=H.SplitAct(B, d, h, w, 16, DEV))
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), "split output")
    X._border_is_zero(ys.buf)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("regime", E.REGIMES)
def test_unit_walk_conv3d_s2rs(regime, fmt):
    B = _walk("conv3d_s2rs")[0]
    c = E.walk_case("conv3d_s2rs", fmt, regime)
    _check_frames(c, B)
    xs = X._to_split(_cl(c.x), fmt)
    out = H.SplitAct(B, *c.ref.shape[2:], 32, DEV)
    if fmt == "bf16":
        ys = H.conv3d_s2rs(xs, H.pack_conv_weights_s2rs(_g(c.w), _g(c.scale)), _g(c.shift), out, neg_slope=c.slope)
    else:
        wp, up, un = H.pack_conv_weights_s2rs(_g(c.w), _g(c.scale), "f16")
        ys = H.conv3d_s2rs(xs, wp, _g(c.shift) * up, out, neg_slope=c.slope, unscale=un)
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), "split output")
    X._border_is_zero(ys.buf)
    if fmt == "f16":
        z = H.conv3d_s2rs(xs, wp, _g(c.shift) * up, H.SplitAct(B, *c.ref.shape[2:], 32, DEV), neg_slope=c.slope, unscale=un, out_f32p=True)
        E.assert_exact(_np(H.act_from_f32p(z)), _want(c), _lsb(c), "fp32-padded output")
        X._border_is_zero(z.buf)


@pytest.mark.parametrize("act32", [False, True])
@pytest.mark.parametrize("regime", E.REGIMES)
def test_unit_walk_conv3d_wino(regime, act32):
    B, d, h, w = _walk("conv3d_wino")
    c = E.walk_case("conv3d_wino", "f16", regime)
    _check_frames(c, B)
    assert H.conv3d_wino_applies(32, 32, d, h, w, 1, c.slope)
    if act32:
        to_act, from_act = H.act_to_f32p, H.act_from_f32p
    else:
        to_act, from_act = (lambda t: X._to_split(t, "f16")), H.act_from_split
    xs, rs = to_act(_cl(c.x)), to_act(_cl(c.r))
    wp, un = H.pack_conv_weights_wino(_g(c.w))
    scg, sh = _g(c.scale) * un, _g(c.shift)
    y32 = H.conv3d_wino(xs, wp, scg, sh, res=rs, neg_slope=c.slope, out_f32=True)
    E.assert_exact(_np(y32), _want(c), _lsb(c), "fp32 output")
    ys = H.conv3d_wino(xs, wp, scg, sh, res=rs, neg_slope=c.slope)
    E.assert_exact(_np(from_act(ys)), _want(c) if act32 else _want(c, "f16"), _lsb(c), "activation-format output")
    X._border_is_zero(ys.buf)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("regime", E.REGIMES)
def test_unit_walk_conv3d_up2_poly_direct(regime, fmt):
    B, d, h, w = _walk("conv3d_up2_poly")
    c = E.walk_case("conv3d_up2_poly", fmt, regime)
    _check_frames(c, B)
    xs = X._to_split(_cl(c.x), fmt)
    plan, scg = X._poly_plan(c, fmt, d, h, w)
    y = torch.full((B, 2 * d, 2 * h, 2 * w, 16), float("nan"), device=DEV)
    H.conv3d_up2_poly(xs, plan, scg, _g(c.shift), neg_slope=c.slope, out=y)
    E.assert_exact(_np(y), _want(c), _lsb(c), "fp32 output")
    ys = H.conv3d_up2_poly_split(xs, plan, scg, _g(c.shift), out=H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, DEV), neg_slope=c.slope, direct=True)
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), "split output, direct")
    X._border_is_zero(ys.buf)


@pytest.mark.parametrize("regime", E.REGIMES)
def test_unit_walk_conv3d_up2_poly_winograd_form_and_head(regime):
    """The Winograd form with fp16 pairs and with fp32 records, then the cost head reading either (tests/test_gpu_tail_f32.py): the
    records are the exact reference, the pairs its split, and the head's costs from both are the same bits."""
    B, d, h, w = _walk("conv3d_up2_poly_wino")
    c = E.walk_case("conv3d_up2_poly_wino", "f16", regime)
    _check_frames(c, B)
    xs = X._to_split(_cl(c.x), "f16")
    plan, scg = X._poly_plan(c, "f16", d, h, w)
    pairs = H.conv3d_up2_poly_split(xs, plan, scg, _g(c.shift), out=H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, DEV), neg_slope=c.slope, wino=True)
    E.assert_exact(_np(H.act_from_split(pairs)), _want(c, "f16"), _lsb(c), "Winograd form, pairs")
    X._border_is_zero(pairs.buf)
    out = H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, DEV)
    out.rec = "f32"
    recs = H.conv3d_up2_poly_split(xs, plan, scg, _g(c.shift), out=out, neg_slope=c.slope, wino=True)
    assert recs.rec == "f32"
    E.assert_exact(_np(recs.buf.view(torch.float32)[:, 1:-1, 1:-1, 1:-1]), _want(c), _lsb(c), "Winograd form, fp32 records")
    X._border_is_zero(recs.buf)
    hw, hun = H.pack_head_split_weights_f16(_g(E.narrow(np.random.default_rng(7), (1, 16, 3, 3, 3), 3).float()))
    a = H.conv3d_head_split(pairs, hw, hun, 0.0, f16=True)
    b = H.conv3d_head_split(recs, hw, hun, 0.0, f16=True)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("regime", E.RESBLOCK_REGIMES)
def test_unit_walk_resblock2d_fused_and_split(regime):
    B, h, w = _walk("resblock2d")
    c = E.resblock_walk_case(regime)
    _check_frames(c, B)
    xg = _cl(c.x)
    w1, w2, s1, s2, b1, b2 = (_g(t) for t in (c.w1, c.w2, c.s1, c.s2, c.b1, c.b2))
    want = c.ref.permute(0, 2, 3, 1).contiguous()
    y = H.resblock2d(xg, H.pack_conv2d_weights_bf16x3(w1), s1, b1, H.pack_conv2d_weights_bf16x3(w2), s2, b2, c.slope)
    E.assert_exact(_np(y), want.float().numpy(), 1.0 / 64, "fused block on fp32 activations")
    xs = H.f32_to_split2d(xg)
    p1, p2 = H.pack_resblock2d_split_weights(w1, s1), H.pack_resblock2d_split_weights(w2, s2)
    y32 = H.resblock2d_split(xs, p1, b1, p2, b2, c.slope)
    E.assert_exact(_np(y32), want.float().numpy(), 1.0 / 64, "block on split activations, fp32 output")
    ys = H.resblock2d_split(xs, p1, b1, p2, b2, c.slope, out_split=H.split2d_buffer(B, h, w, xg.device))
    E.assert_exact(_np(H.split2d_to_f32(ys)), E.expected_split(want, "bf16"), 1.0 / 64, "block on split activations, split output")
    X._border_is_zero(ys, pad=2)


@pytest.mark.parametrize("regime", E.REGIMES)
def test_unit_walk_conv2d_s2_split(regime):
    B = _walk("conv2d_s2_split")[0]
    c = E.walk_case("conv2d_s2_split", "bf16", regime)
    _check_frames(c, B)
    xg = _cl(c.x)
    xs = H.f32_to_split2d(xg)
    assert torch.equal(H.split2d_to_f32(xs), xg)
    ys = H.conv2d_s2_split(xs, H.pack_resblock2d_split_weights(_g(c.w), _g(c.scale)), _g(c.shift),
                           H.split2d_buffer(B, *c.ref.shape[2:], xg.device), c.slope)
    E.assert_exact(_np(H.split2d_to_f32(ys)), _want(c, "bf16"), _lsb(c), "split output")
    X._border_is_zero(ys, pad=2)


# ------------------------------------------------------------------------------------------------ cost head, whole-depth march
@pytest.mark.parametrize("kind", ["bf16", "f16", "rec32"])
@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("shape", E.HEAD_MARCH_SHAPES, ids=str)
def test_head_split_whole_depth_march(shape, regime, kind):
    """nd = 1 (conv3d_headsplit.hip:286-290): at least 1024 windows, every block marches all D planes.  bf16 pairs, fp16 pairs and
    fp32 records of the same exact operands."""
    B, ci, d, h, w = shape
    assert B * E.cdiv(h, 8) * E.cdiv(w, 32) >= 1024
    fmt = "bf16" if kind == "bf16" else "f16"
    c = E.head_march_case(shape, fmt, regime)
    _check_frames(c, B)
    scale, shift = float(c.scale[0]), float(c.shift[0])
    if kind == "bf16":
        y = H.conv3d_head_split(X._to_split(_cl(c.x), fmt), H.pack_head_split_weights(_g(c.w)), scale, shift, neg_slope=c.slope)
    else:
        wp, un = H.pack_head_split_weights_f16(_g(c.w))
        if kind == "f16":
            xs = X._to_split(_cl(c.x), fmt)
        else:
            xs = H.SplitAct(B, d, h, w, ci, DEV)
            xs.buf.view(torch.float32)[:, 1:-1, 1:-1, 1:-1] = _cl(c.x)
            xs.fmt, xs.rec = "f16", "f32"
        y = H.conv3d_head_split(xs, wp, scale * un, shift, neg_slope=c.slope, f16=True)
    E.assert_exact(_np(y), _want(c), _lsb(c), f"cost head, {kind}")


# ------------------------------------------------------------------------------------------------ weight packers, byte for byte
def _split_bits(v, fmt):
    """(hi, lo) bit patterns of csrc/split_fmt.hpp:sf_split_weight with torch's round-to-nearest casts on the CPU: hi = cast(v),
    lo = cast(v - hi)."""
    dt = E.SPLIT_DT[fmt]
    hi = v.to(dt)
    return hi.view(torch.int16), (v - hi.float()).to(dt).view(torch.int16)


def _pair_lane_rule(w, scale, fmt):
    """The lane rule of csrc/presplit_common.hpp:ps_pack_weights_kernel, written once: [cout tile][pair p][hi | lo][64 lanes][8], lane =
    (kg << 4) | i holds scale[co] * W[co = 16 ct + i][cin = 8 (kg & 1) + j][tap = 2 p + (kg >> 1)], zeros past the last tap."""
    co, taps = w.shape[0], w[0, 0].numel()
    pairs = (taps + 1) // 2
    v = w.float().reshape(co, 16, taps) * scale.float().reshape(co, 1, 1)                 # the fp32 product
    v = torch.nn.functional.pad(v, (0, 2 * pairs - taps))
    x = torch.stack(_split_bits(v, fmt)).reshape(2, co // 16, 16, 2, 8, pairs, 2)         # [hi | lo][ct][i][kg & 1][j][p][kg >> 1]
    return x.permute(1, 5, 0, 6, 3, 2, 4).contiguous().view(torch.uint8).flatten()        # [ct][p][hi | lo][kg >> 1][kg & 1][i][j]


def _head_lane_rule(w, fmt):
    """csrc/conv3d_headsplit.hip:head_split_pack_kernel: [Cin / 16][tap tile tt][A1 | A2][64 lanes][8], lane = (kg << 4) | i, tap =
    16 tt + i (zeros from tap 27); A1 = hi(W[16 cs + 8 (kg & 1) + j][tap]) for every kg, A2 = lo of the same for kg < 2, else zeros."""
    cin = w.shape[1]
    v = torch.nn.functional.pad(w.float().reshape(cin, 27), (0, 5))
    h, l = (t.reshape(cin // 16, 2, 8, 2, 16).permute(0, 3, 1, 4, 2) for t in _split_bits(v, fmt))   # [cs][tt][kg & 1][i][j]
    a1, a2 = torch.cat((h, h), dim=2), torch.cat((l, torch.zeros_like(l)), dim=2)                    # [cs][tt][kg][i][j]
    return torch.stack((a1, a2), dim=2).contiguous().view(torch.uint8).flatten()


def _same_bytes(got, want, what):
    got = got.cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {want.numel()} bytes differ, first at {int(bad[0])}"


def test_weight_packers_byte_for_byte():
    """pack_resblock2d_split_weights (9 taps, one cout tile, bf16), pack_conv_weights_s2rs (27 taps, two cout tiles, both splits, with
    the prescale it returns) and pack_head_split_weights[_f16] (its own A1 | A2 rule) against the lane rules above: every byte, no
    tolerance.  Wide integers (lo != 0) times a per-channel scale that is an odd multiple of 1/8: the products are exact in fp32 and
    need both roundings of the split."""
    rng = np.random.default_rng(2207)
    w2, s2 = E.wide(rng, (16, 16, 3, 3), "bf16", 1.0), (E.narrow(rng, (16,), 7) + 0.5) / 4
    _same_bytes(H.pack_resblock2d_split_weights(_g(w2), _g(s2)), _pair_lane_rule(w2, s2, "bf16"), "resblock2d split packer")
    for fmt in FMTS:
        w3, s3 = E.wide(rng, (32, 16, 3, 3, 3), fmt, 1.0), (E.narrow(rng, (32,), 7) + 0.5) / 4
        if fmt == "bf16":
            wp, up = H.pack_conv_weights_s2rs(_g(w3), _g(s3)), 1.0
        else:
            wp, up, un = H.pack_conv_weights_s2rs(_g(w3), _g(s3), "f16")
            assert up * un == 1.0
        _same_bytes(wp, _pair_lane_rule(w3, s3.float() * up, fmt), f"s2rs packer, {fmt}")
        wh = E.wide(rng, (1, 32, 3, 3, 3), fmt, 1.0)
        if fmt == "bf16":
            hp, un = H.pack_head_split_weights(_g(wh)), 1.0
        else:
            hp, un = H.pack_head_split_weights_f16(_g(wh))
        _same_bytes(hp, _head_lane_rule(wh.float() * (1.0 / un), fmt), f"head packer, {fmt}")


# ------------------------------------------------------------------------------------------------ coverage of conv3d_variants.inc
# (row, split) pairs no exact case names, each with its reason.  Empty: every row has a shape in E.VARIANT_ROWS.
EXEMPT = {}


def named_by_the_small_shape_module():
    """The names test_gpu_exact.py asserts: its cases through its own layout rules (X.split_layouts, X.up2_layouts), and CONV_MFMA."""
    names = set()
    for fmt in FMTS:
        for n in E.ids(f"conv3d_{fmt}"):
            kw = dict(E.TABLE[f"conv3d_{fmt}"])[n]
            dims = (kw["B"], kw["Cin"], kw["Cout"], *kw["dims"])
            for layout in X.split_layouts(dims, kw["stride"]):
                B, ci, co, D, Hh, W = dims
                names.add(H.conv3d_variant(B, ci, D, Hh, W, co, kw["stride"], layout | (F16 if fmt == "f16" else 0)))
        for n in E.ids(f"conv3d_up2_{fmt}"):
            kw = dict(E.TABLE[f"conv3d_up2_{fmt}"])[n]
            dims = (kw["B"], kw["Cin"], kw["Cout"], *kw["dims"])
            for layout in X.up2_layouts(dims, fmt):
                B, ci, co, D, Hh, W = dims
                names.add(H.conv3d_up2_variant(B, ci, D, Hh, W, co, layout | (F16 if fmt == "f16" else 0)))
    for n in E.ids("conv3d_f32"):
        kw = dict(E.TABLE["conv3d_f32"])[n]
        if kw["Cin"] % 16 == 0 and kw["Cout"] % 16 == 0:
            names.add(H.conv3d_variant(kw["B"], kw["Cin"], *kw["dims"], kw["Cout"], kw["stride"], H.CONV_MFMA))
    return names


def test_every_variant_row_is_named_by_an_exact_case():
    """Every MVSGI_B3 row x split and every MVSGI_MFMA row of csrc/conv3d_variants.inc is the asserted variant of a case of this
    module or of test_gpu_exact.py (the names are queried again here, through the same tables), or is a literal exemption."""
    every = {(row, fmt): E.variant_kernel_name(VARIANTS, row, fmt)
             for row, (kind, _, _) in VARIANTS.items() for fmt in (FMTS if kind == "B3" else ("f32",))}
    assert len([r for r, v in VARIANTS.items() if v[0] == "B3"]) == 60 and len(every) == 127
    before = named_by_the_small_shape_module()
    here = set()
    for row in E.VARIANT_ROWS:
        name, fn, B, ci, co, D, Hh, W, s, lay = row
        for fmt in (("f32",) if lay == "mfma" else FMTS):
            impl = H.CONV_MFMA if lay == "mfma" else LAYOUTS[lay] | (F16 if fmt == "f16" else 0)
            got = H.conv3d_variant(B, ci, D, Hh, W, co, s, impl) if fn == "conv" else H.conv3d_up2_variant(B, ci, D, Hh, W, co, impl)
            assert got == every[name, fmt], (row, fmt, got)
            here.add(got)
    n_before = sum(1 for v in every.values() if v in before)
    print(f"rows x splits named by test_gpu_exact.py: {n_before} of {len(every)}; with this module: "
          f"{sum(1 for v in every.values() if v in before | here)}")
    missing = sorted(k for k, v in every.items() if v not in before | here and k not in EXEMPT)
    assert not missing, f"named by no exact case: {missing}"
    assert all(every[k] not in before | here for k in EXEMPT), "an exemption that a case reaches"
