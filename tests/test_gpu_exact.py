"""GPU (MI355X): every convolution kernel against a float64 reference, bit for bit, on the exact-arithmetic operands of
tests/exact_cases.py.  No tolerance anywhere: every comparison is np.array_equal (exact_cases.assert_exact, which reports the count,
the first index and the largest difference in lsb units on a mismatch).  Conditions (a)-(c) are asserted while a case is built,
i.e. before the kernel is called (and on the CPU by tests/test_exact_cases_host.py); the range report must stay clear.

family                       entry point                                             cases (each in both regimes, x_wide and w_wide)
---------------------------  ------------------------------------------------------  -----------------------------------------------
conv3d, fp32                 H.conv3d impl CONV_MFMA, CONV_DIRECT                    CONV3D_SHAPES; CONV3D_DIRECT_ODD (direct only)
conv3d, fp32 cost head       H.conv3d at Cout = 1 (LDS-tiled head), CONV_DIRECT        HEAD_F32_SHAPES
conv3d, bf16 / fp16 split    H.conv3d impl CONV_BF16X3 [| CONV_F16], _D32 and _C16   CONV3D_SHAPES (_D32 / _C16 where the layout takes the shape)
                             where they apply, _V32 on CONV3D_V32_SHAPES             CONV3D_V32_SHAPES (base kernel and 32x32x16 schedule)
conv3d, split output         H.conv3d_out_split, both splits                         CONV3D_OUT_SPLIT_SHAPES
fused upsample + conv        H.conv3d_up2 (base, _C16, _D32 incl. the depth-skip     UP2_SHAPES, both splits (_V32: bf16 split, the only one
                             form, _V32), H.conv3d_up2_out_split                     its schedule test runs)
register-stationary 32->32   H.conv3d_rs, both splits, res on/off, out_f32 on/off    RS_SHAPES
register-stationary 16->16   H.conv3d_rs16 and its split output, both splits         RS16_SHAPES
stride-2 16->32              H.conv3d_s2rs (scale folded into the weights), split    S2RS_SHAPES, both splits
                             and (fp16 split) fp32-padded output
Winograd 32->32              H.conv3d_wino, act32 on/off, out_f32 on/off, res        WINO_SHAPES
polyphase ResizeConv3d       H.conv3d_up2_poly, H.conv3d_up2_poly_split direct       POLY_SHAPES, both splits
                             on/off; Winograd form (wino=True)                       POLY_WINO_SHAPES (fp16 split)
cost head                    H.conv3d_head_split, bf16 and f16=True                  HEAD_SHAPES
2-D conv                     H.conv2d direct, fp32 MFMA, bf16x3, out_split,          CONV2D_SHAPES (stride 1 and 2); 5x5 stem on float NCHW;
                             5x5 stem (in_nchw)                                      CONV2D_WIDE_SHAPES (32, 48, 80 channels, 16 -> 32: fp32 MFMA
                                                                                     at Cout 16 | 32, out_split at Cout 16)
2-D conv, direct kernel      H.conv2d impl CONV_AUTO where only the direct kernel    CONV2D_DIRECT_ROWS (Cout 6 and 8, k of 1 | 5 | 7, NCHW input
                             serves                                                  of 1 and 4 channels)
2-D residual block           H.resblock2d, H.resblock2d_split (both outputs)         RESBLOCK2D_SHAPES x three regimes (w2_wide: conv2's lo weights)
2-D stride-2 on split input  H.conv2d_s2_split                                       S2_2D_SHAPES
deformable conv              H.deform_conv2d, quad-lane and generic kernel           DEFORM_ROWS, shared and per-image offset field
trilinear resize             H.resize_trilinear x2, x4                               RESIZE_CASES
uint8 stem                   LEFT OUT: csrc/conv2d.hip:112 divides every pixel by 255.0f and :177 every weight (w / 255 in three
                             bf16 pieces): 1/255 is not dyadic, no operand makes the products exact.  It keeps its tolerance test
                             (test_gpu_parity.py::test_conv2d_stem_uint8_on_the_matrix_cores).
launch-size variants         tests/test_gpu_exact_launches.py: the same operands and comparison on batches built from four distinct
                             frames -- every row of csrc/conv3d_variants.inc in both splits (the many-frame bricks, the one-plane
                             and depth-skip units, conv3d_up2 with _V32 in the fp16 split), the border-plane-skip kernels under
                             their restated launch condition, a second and later unit of every persistent kernel, the cost
                             head's whole-depth march.  This module keeps the smallest shape of each layout.
"""
import numpy as np
import pytest
import torch

import exact_cases as E
import guard_arena
from mvs_gi_amd import hip_ops as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = H.CONV_F16


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


def _g(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).float().contiguous().to(DEV)


def _cl(t):
    """NC(D)HW on the host -> channels-last on the device."""
    return None if t is None else _g(t.permute(0, *range(2, t.dim()), 1))


def _want(c, split=None):
    """The float64 reference, channels-last, as fp32 (exact: condition (b)); `split`: as a reader of a split output sees it."""
    ref = c.ref.permute(0, *range(2, c.ref.dim()), 1).contiguous()
    assert E.representable(ref)
    return E.expected_split(ref, split) if split else ref.float().numpy()


def _np(y):
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _lsb(c):
    return float(c.scale.min()) * (c.slope if 0 < c.slope < 1 else 1.0)


def _border_is_zero(buf, pad=1):
    b = buf.clone()
    if b.dim() == 5:
        b[:, pad:-pad, pad:-pad, pad:-pad] = 0
    else:
        b[:, pad:-pad, pad:-pad] = 0
    assert int(b.count_nonzero()) == 0, "the zero border of a padded output was written"


def _to_split(x_cl, fmt):
    """Library converter for the INPUT; the join must give the operand back bit for bit (hi + lo == x on the device too)."""
    xs = H.act_to_split(x_cl, fmt=fmt)
    assert torch.equal(H.act_from_split(xs), x_cl)
    return xs


def _dims(c):
    return (c.x.shape[0], c.x.shape[1], c.w.shape[0]) + tuple(c.x.shape[2:])


# ------------------------------------------------------------------------------------------------ H.conv3d, fp32 kernels
@pytest.mark.parametrize("name", E.ids("conv3d_f32"))
def test_conv3d_fp32_mfma_and_direct(name):
    c = E.case("conv3d_f32", name)
    B, Cin, Cout, D, Hh, W = _dims(c)
    xg, rg, wg, sc, sh = _cl(c.x), _cl(c.r), _g(c.w), _g(c.scale), _g(c.shift)
    want = _want(c)
    wp = H.pack_conv_weights(wg)
    assert (wp is None) == bool(Cin % 16 or Cout % 16)
    if wp is not None:
        assert H.conv3d_variant(B, Cin, D, Hh, W, Cout, c.stride, H.CONV_MFMA).startswith("conv3d_mfma_kernel<")
        y = H.conv3d(xg, wg, wp, sc, sh, res=rg, stride=c.stride, neg_slope=c.slope, impl=H.CONV_MFMA)
        E.assert_exact(_np(y), want, _lsb(c), "fp32 MFMA")
    assert H.conv3d_variant(B, Cin, D, Hh, W, Cout, c.stride, H.CONV_DIRECT).startswith("conv3d_direct_kernel<")
    y = H.conv3d(xg, wg, wp, sc, sh, res=rg, stride=c.stride, neg_slope=c.slope, impl=H.CONV_DIRECT)
    E.assert_exact(_np(y), want, _lsb(c), "direct")


@pytest.mark.parametrize("name", E.ids("conv3d_head_f32"))
def test_conv3d_fp32_cost_head(name):
    """Cout = 1 behind H.conv3d: the LDS-tiled fp32 cost head (the dispatcher's choice) and the direct kernel."""
    c = E.case("conv3d_head_f32", name)
    B, Cin, Cout, D, Hh, W = _dims(c)
    xg, rg, wg, sc, sh = _cl(c.x), _cl(c.r), _g(c.w), _g(c.scale), _g(c.shift)
    wp = H.pack_conv_weights(wg)
    assert wp is not None and "head" in H.conv3d_variant(B, Cin, D, Hh, W, 1)
    y = H.conv3d(xg, wg, wp, sc, sh, res=rg, neg_slope=c.slope)
    E.assert_exact(_np(y), _want(c), _lsb(c), "cost head")
    y = H.conv3d(xg, wg, wp, sc, sh, res=rg, neg_slope=c.slope, impl=H.CONV_DIRECT)
    E.assert_exact(_np(y), _want(c), _lsb(c), "direct")


# ------------------------------------------------------------------------------------------------ H.conv3d, split kernels
_BF16_PACK = {H.CONV_BF16X3: H.pack_conv_weights_bf16x3, H.CONV_BF16X3_D32: H.pack_conv_weights_bf16x3_d32,
              H.CONV_BF16X3_C16: H.pack_conv_weights_bf16x3_c16, H.CONV_BF16X3_V32: H.pack_conv_weights_bf16x3_v32}


def _pack3d(wg, sc, fmt, layout=H.CONV_BF16X3):
    """-> (packed weights, scale with the fp16 split's power-of-two unscale folded in, impl / w_layout flags)."""
    if fmt == "bf16":
        wp = _BF16_PACK[layout](wg)
        assert wp is not None
        return wp, sc, layout
    wp, un = H.pack_conv_weights_f16x3(wg, layout)
    return wp, sc * un, layout | F16


def split_layouts(dims, stride):
    """The weight layouts test_conv3d_split_kernels_every_layout runs a case in (also read by the coverage test of
    tests/test_gpu_exact_launches.py)."""
    B, Cin, Cout, D, Hh, W = dims
    layouts = [H.CONV_BF16X3]
    if H.conv3d_d32_applies(B, Cin, D, Hh, W, Cout, stride):
        layouts.append(H.CONV_BF16X3_D32)
    if Cout == 16 and stride == 1:
        layouts.append(H.CONV_BF16X3_C16)
    if H.conv3d_v32_applies(B, Cin, D, Hh, W, Cout, stride):
        layouts.append(H.CONV_BF16X3_V32)
    return layouts


def up2_layouts(dims, fmt):
    """... and test_conv3d_up2 (low-resolution sizes)."""
    B, Cin, Cout, Dl, Hl, Wl = dims
    layouts = [H.CONV_BF16X3]
    if Cout == 16:
        layouts.append(H.CONV_BF16X3_C16)
    if H.conv3d_up2_d32_applies(B, Cin, Dl, Hl, Wl, Cout):      # 32-channel slices; the depth-skip form out of a one-plane level
        layouts.append(H.CONV_BF16X3_D32)
    if fmt == "bf16" and Cout % 32 == 0 and H.conv3d_v32_applies(B, Cin, 2 * Dl, 2 * Hl, 2 * Wl, Cout, 1):
        layouts.append(H.CONV_BF16X3_V32)
    return layouts


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", E.ids("conv3d_bf16"))
def test_conv3d_split_kernels_every_layout(name, fmt):
    c = E.case(f"conv3d_{fmt}", name)
    B, Cin, Cout, D, Hh, W = _dims(c)
    xg, rg, wg, sc, sh = _cl(c.x), _cl(c.r), _g(c.w), _g(c.scale), _g(c.shift)
    want = _want(c)
    kname = f"conv3d_{'f16x3' if fmt == 'f16' else 'bf16x3'}"
    # the template's last four arguments: fused upsample, plane schedule (_C16), 32x32x16 schedule (_V32), weight slice through LDS
    name_oks = {H.CONV_BF16X3: lambda n: n.startswith(kname + "_kernel<") and n.endswith(("false, false, false, false>", "false, false, false, true>")),
                H.CONV_BF16X3_D32: lambda n: n.startswith(kname + "_d32"),
                H.CONV_BF16X3_C16: lambda n: n.startswith(kname + "_kernel<") and n.endswith("false, true, false, false>"),
                H.CONV_BF16X3_V32: lambda n: n.startswith(kname + "_kernel<") and n.endswith("false, false, true, false>")}
    layouts = [(layout, name_oks[layout]) for layout in split_layouts((B, Cin, Cout, D, Hh, W), c.stride)]
    if (B, Cin, Cout, D, Hh, W, c.stride, c.r is not None) in E.CONV3D_V32_SHAPES:
        assert len(layouts) == 2, "the 32x32x16 schedule must take this shape"
    if (B, Cin, Cout) == (1, 128, 128):
        assert len(layouts) == 2, "the 32-channel-slice kernel must take this shape"
    for layout, name_ok in layouts:
        wp, scg, impl = _pack3d(wg, sc, fmt, layout)
        kn = H.conv3d_variant(B, Cin, D, Hh, W, Cout, c.stride, impl)
        assert name_ok(kn), (layout, kn)
        y = H.conv3d(xg, wg, wp, scg, sh, res=rg, stride=c.stride, neg_slope=c.slope, impl=impl)
        E.assert_exact(_np(y), want, _lsb(c), kn)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", E.ids("conv3d_out_split_bf16"))
def test_conv3d_out_split(name, fmt):
    c = E.case(f"conv3d_out_split_{fmt}", name)
    B, Cin, Cout, D, Hh, W = _dims(c)
    xg, rg, wg, sc, sh = _cl(c.x), _cl(c.r), _g(c.w), _g(c.scale), _g(c.shift)
    wp, scg, _ = _pack3d(wg, sc, fmt)
    ys = H.SplitAct(*c.ref.shape[0:1], *c.ref.shape[2:], Cout, DEV)
    H.conv3d_out_split(xg, wp, scg, sh, out=ys, res=rg, stride=c.stride, neg_slope=c.slope, fmt=fmt)
    assert ys.fmt == fmt
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), "split output")
    _border_is_zero(ys.buf)


# ------------------------------------------------------------------------------------------------ fused upsample + conv
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", E.ids("conv3d_up2_bf16"))
def test_conv3d_up2(name, fmt):
    c = E.case(f"conv3d_up2_{fmt}", name)
    B, Cin, Cout, Dl, Hl, Wl = _dims(c)
    xg, rg, wg, sc, sh = _cl(c.x), _cl(c.r), _g(c.w), _g(c.scale), _g(c.shift)
    want = _want(c)
    kname = f"conv3d_{'f16x3' if fmt == 'f16' else 'bf16x3'}"
    heads = {H.CONV_BF16X3: (kname + "_kernel<", "true, false, false, false>"),
             H.CONV_BF16X3_C16: (kname + "_kernel<", "true, true, false, false>"),
             H.CONV_BF16X3_D32: (kname + ("_d32u_dk_kernel<" if Dl == 1 else "_d32u_kernel<"), ">"),
             H.CONV_BF16X3_V32: (kname + "_kernel<", "true, false, true, false>")}
    layouts = [(layout, *heads[layout]) for layout in up2_layouts((B, Cin, Cout, Dl, Hl, Wl), fmt)]
    if (B, Cin, Cout, Dl, Hl, Wl) in ((1, 32, 96, 3, 10, 24), (3, 32, 96, 1, 10, 24)) or (fmt == "bf16" and (B, Cin, Cout) == (6, 16, 64)):
        assert len(layouts) == 2, "this shape is in the table for its second layout"
    for layout, head, tail in layouts:
        wp, scg, wl = _pack3d(wg, sc, fmt, layout)
        kn = H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout, wl)
        assert kn.startswith(head) and kn.endswith(tail), kn
        y = H.conv3d_up2(xg, wp, scg, sh, res=rg, neg_slope=c.slope, w_layout=wl)
        E.assert_exact(_np(y), want, _lsb(c), kn)
    wp, scg, wl = _pack3d(wg, sc, fmt)
    buf = H.SplitAct(B, 2 * Dl, 2 * Hl, 2 * Wl, Cout, DEV)
    H.conv3d_up2_out_split(xg, wp, scg, sh, out=buf, res=rg, neg_slope=c.slope, w_layout=wl)
    assert buf.fmt == fmt
    E.assert_exact(_np(H.act_from_split(buf)), _want(c, fmt), _lsb(c), "split output")
    _border_is_zero(buf.buf)


# ------------------------------------------------------------------------------------------------ register-stationary kernels
def _rs_pack(wg, sc, fmt):
    if fmt == "bf16":
        return H.pack_conv_weights_rs(wg), sc
    wp, un = H.pack_conv_weights_rs(wg, "f16")
    return wp, sc * un


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", E.ids("conv3d_rs_bf16"))
def test_conv3d_rs(name, fmt):
    c = E.case(f"conv3d_rs_{fmt}", name)
    xs = _to_split(_cl(c.x), fmt)
    rs = None if c.r is None else _to_split(_cl(c.r), fmt)
    wp, scg = _rs_pack(_g(c.w), _g(c.scale), fmt)
    sh = _g(c.shift)
    y32 = H.conv3d_rs(xs, wp, scg, sh, res=rs, neg_slope=c.slope, out_f32=True)
    E.assert_exact(_np(y32), _want(c), _lsb(c), "fp32 output")
    ys = H.conv3d_rs(xs, wp, scg, sh, res=rs, neg_slope=c.slope)
    assert ys.fmt == fmt
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), "split output")
    _border_is_zero(ys.buf)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", E.ids("conv3d_rs16_bf16"))
def test_conv3d_rs16(name, fmt):
    c = E.case(f"conv3d_rs16_{fmt}", name)
    B, _, _, d, h, w = _dims(c)
    xs = _to_split(_cl(c.x), fmt)
    wp, scg = _rs_pack(_g(c.w), _g(c.scale), fmt)
    sh = _g(c.shift)
    y = H.conv3d_rs16(xs, wp, scg, sh, neg_slope=c.slope)
    E.assert_exact(_np(y), _want(c), _lsb(c), "fp32 output")
    ys = H.conv3d_rs16(xs, wp, scg, sh, neg_slope=c.slope, out_split=H.SplitAct(B, d, h, w, 16, DEV))
    assert ys.fmt == fmt
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), "split output")
    _border_is_zero(ys.buf)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", E.ids("conv3d_s2rs_bf16"))
def test_conv3d_s2rs(name, fmt):
    c = E.case(f"conv3d_s2rs_{fmt}", name)
    B = c.x.shape[0]
    xs = _to_split(_cl(c.x), fmt)
    out = H.SplitAct(B, *c.ref.shape[2:], 32, DEV)
    if fmt == "bf16":
        ys = H.conv3d_s2rs(xs, H.pack_conv_weights_s2rs(_g(c.w), _g(c.scale)), _g(c.shift), out, neg_slope=c.slope)
    else:
        wp, up, un = H.pack_conv_weights_s2rs(_g(c.w), _g(c.scale), "f16")
        ys = H.conv3d_s2rs(xs, wp, _g(c.shift) * up, out, neg_slope=c.slope, unscale=un)
    assert ys.fmt == fmt
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), "split output")
    _border_is_zero(ys.buf)
    if fmt == "f16":      # the fp32-padded output for a Winograd-form level 0 behind it: the values before the split
        z = H.conv3d_s2rs(xs, wp, _g(c.shift) * up, H.SplitAct(B, *c.ref.shape[2:], 32, DEV), neg_slope=c.slope, unscale=un, out_f32p=True)
        assert z.fmt == "f32p"
        E.assert_exact(_np(H.act_from_f32p(z)), _want(c), _lsb(c), "fp32-padded output")
        _border_is_zero(z.buf)


# ------------------------------------------------------------------------------------------------ Winograd 32 -> 32
@pytest.mark.parametrize("act32", [False, True])
@pytest.mark.parametrize("name", E.ids("conv3d_wino"))
def test_conv3d_wino(name, act32):
    c = E.case("conv3d_wino", name)
    B, _, _, d, h, w = _dims(c)
    assert H.conv3d_wino_applies(32, 32, d, h, w, 1, c.slope)
    if act32:
        to_act, from_act, fmt = H.act_to_f32p, H.act_from_f32p, "f32p"
    else:
        to_act, from_act, fmt = (lambda t: _to_split(t, "f16")), H.act_from_split, "f16"
    xs = to_act(_cl(c.x))
    rs = None if c.r is None else to_act(_cl(c.r))
    if act32:
        assert torch.equal(H.act_from_f32p(xs), _cl(c.x))
    wp, un = H.pack_conv_weights_wino(_g(c.w))
    scg, sh = _g(c.scale) * un, _g(c.shift)
    y32 = H.conv3d_wino(xs, wp, scg, sh, res=rs, neg_slope=c.slope, out_f32=True)
    E.assert_exact(_np(y32), _want(c), _lsb(c), "fp32 output")
    ys = H.conv3d_wino(xs, wp, scg, sh, res=rs, neg_slope=c.slope)
    assert ys.fmt == fmt
    E.assert_exact(_np(from_act(ys)), _want(c) if act32 else _want(c, "f16"), _lsb(c), f"{fmt} output")
    _border_is_zero(ys.buf)


# ------------------------------------------------------------------------------------------------ polyphase ResizeConv3d
def _poly_plan(c, fmt, d, h, w):
    if fmt == "bf16":
        return H.conv3d_up2_poly_plan(_g(c.w), d, h, w), _g(c.scale)
    plan, un = H.conv3d_up2_poly_plan(_g(c.w), d, h, w, fmt="f16")
    return plan, _g(c.scale) * un


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", E.ids("conv3d_up2_poly_bf16"))
def test_conv3d_up2_poly(name, fmt):
    c = E.case(f"conv3d_up2_poly_{fmt}", name)
    B, _, _, d, h, w = _dims(c)
    xs = _to_split(_cl(c.x), fmt)
    plan, scg = _poly_plan(c, fmt, d, h, w)
    sh = _g(c.shift)
    y = torch.full((B, 2 * d, 2 * h, 2 * w, 16), float("nan"), device=DEV)          # every voxel must be written
    H.conv3d_up2_poly(xs, plan, scg, sh, neg_slope=c.slope, out=y)
    E.assert_exact(_np(y), _want(c), _lsb(c), "fp32 output")
    for direct in (True, False):
        ys = H.conv3d_up2_poly_split(xs, plan, scg, sh, out=H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, DEV), neg_slope=c.slope, direct=direct)
        assert ys.fmt == fmt
        E.assert_exact(_np(H.act_from_split(ys)), _want(c, fmt), _lsb(c), f"split output, direct={direct}")
        _border_is_zero(ys.buf)


@pytest.mark.parametrize("name", E.ids("conv3d_up2_poly_wino"))
def test_conv3d_up2_poly_winograd_form(name):
    c = E.case("conv3d_up2_poly_wino", name)
    B, _, _, d, h, w = _dims(c)
    xs = _to_split(_cl(c.x), "f16")
    plan, scg = _poly_plan(c, "f16", d, h, w)
    out = H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, DEV)
    ys = H.conv3d_up2_poly_split(xs, plan, scg, _g(c.shift), out=out, neg_slope=c.slope, wino=True)
    assert ys.fmt == "f16"
    E.assert_exact(_np(H.act_from_split(ys)), _want(c, "f16"), _lsb(c), "Winograd form")
    _border_is_zero(ys.buf)


# ------------------------------------------------------------------------------------------------ cost head
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", E.ids("conv3d_head_split_bf16"))
def test_conv3d_head_split(name, fmt):
    c = E.case(f"conv3d_head_split_{fmt}", name)
    xs = _to_split(_cl(c.x), fmt)
    scale, shift = float(c.scale[0]), float(c.shift[0])
    if fmt == "bf16":
        y = H.conv3d_head_split(xs, H.pack_head_split_weights(_g(c.w)), scale, shift, neg_slope=c.slope)
    else:
        wp, un = H.pack_head_split_weights_f16(_g(c.w))
        y = H.conv3d_head_split(xs, wp, scale * un, shift, neg_slope=c.slope, f16=True)
    E.assert_exact(_np(y), _want(c), _lsb(c), "cost head")


# ------------------------------------------------------------------------------------------------ 2-D
@pytest.mark.parametrize("name", E.ids("conv2d_f32"))
def test_conv2d_fp32_direct_and_mfma(name):
    c = E.case("conv2d_f32", name)
    B, Cin, Cout, Hh, W = _dims(c)
    xg, rg, wg, sc, sh = _cl(c.x), _cl(c.r), _g(c.w), _g(c.scale), _g(c.shift)
    assert H.conv2d_variant(Cin, Cout, 3, c.stride, H.CONV_DIRECT).startswith("conv2d_direct_kernel<")
    y = H.conv2d(xg, wg, None, sc, sh, res=rg, stride=c.stride, neg_slope=c.slope, impl=H.CONV_DIRECT)
    E.assert_exact(_np(y), _want(c), _lsb(c), "direct")
    wpf = H.pack_conv2d_weights_f32(wg)
    assert (wpf is not None) == (Cout in (16, 32))       # the fp32 MFMA kernel's channel counts (every 16 -> 16 row runs it)
    if wpf is None:
        return
    assert H.conv2d_variant(Cin, Cout, 3, c.stride, H.CONV_MFMA).startswith("conv3d_mfma_kernel<")
    y = H.conv2d(xg, wg, wpf, sc, sh, res=rg, stride=c.stride, neg_slope=c.slope, impl=H.CONV_MFMA)
    E.assert_exact(_np(y), _want(c), _lsb(c), "fp32 MFMA")


@pytest.mark.parametrize("name", E.ids("conv2d_bf16"))
def test_conv2d_bf16x3_and_split_output(name):
    c = E.case("conv2d_bf16", name)
    B, Cin, Cout, Hh, W = _dims(c)
    xg, rg, wg, sc, sh = _cl(c.x), _cl(c.r), _g(c.w), _g(c.scale), _g(c.shift)
    assert H.conv2d_variant(Cin, Cout, 3, c.stride, H.CONV_BF16X3).startswith("conv3d_bf16x3_kernel<")
    wp = H.pack_conv2d_weights_bf16x3(wg)
    y = H.conv2d(xg, wg, wp, sc, sh, res=rg, stride=c.stride, neg_slope=c.slope, impl=H.CONV_BF16X3)
    E.assert_exact(_np(y), _want(c), _lsb(c), "bf16x3")
    if Cout != 16:                                       # the 2-D split-padded format holds 16 channels
        return
    ys = H.conv2d(xg, wg, wp, sc, sh, res=rg, stride=c.stride, neg_slope=c.slope, impl=H.CONV_BF16X3,
                  out_split=H.split2d_buffer(B, *c.ref.shape[2:], xg.device))
    E.assert_exact(_np(H.split2d_to_f32(ys)), _want(c, "bf16"), _lsb(c), "split output")
    _border_is_zero(ys, pad=2)


@pytest.mark.parametrize("name", E.ids("conv2d_stem_f32"))
def test_conv2d_stem_5x5_float_nchw(name):
    c = E.case("conv2d_stem_f32", name)
    assert H.conv2d_variant(3, 16, 5, 2, H.CONV_AUTO, True).startswith("conv2d_direct_kernel<")
    y = H.conv2d(_g(c.x), _g(c.w), None, _g(c.scale), _g(c.shift), stride=2, neg_slope=c.slope, in_nchw=True)
    E.assert_exact(_np(y), _want(c), _lsb(c), "5x5 stem")


@pytest.mark.parametrize("name", E.ids("conv2d_direct"))
def test_conv2d_direct_odd_channels_kernel_sizes_and_nchw(name):
    """conv2d_direct_kernel<4> where nothing else serves: Cout of 6 (a tail group of two channels) and 8, k of 1, 5 and 7 on 16
    channels, and the generic NCHW stem on 1 and 4 input channels."""
    c = E.case("conv2d_direct", name)
    B, Cin, Cout, Hh, W = _dims(c)
    k, nchw = int(c.w.shape[-1]), "-nchw-" in name
    assert H.conv2d_variant(Cin, Cout, k, c.stride, H.CONV_AUTO, nchw).startswith("conv2d_direct_kernel<")
    xg = _g(c.x) if nchw else _cl(c.x)
    y = H.conv2d(xg, _g(c.w), None, _g(c.scale), _g(c.shift), res=_cl(c.r), stride=c.stride, neg_slope=c.slope, in_nchw=nchw)
    E.assert_exact(_np(y), _want(c), _lsb(c), f"direct k = {k}")


@pytest.mark.parametrize("name", E.ids("conv2d_s2_split"))
def test_conv2d_s2_split(name):
    c = E.case("conv2d_s2_split", name)
    B = c.x.shape[0]
    xg = _cl(c.x)
    xs = H.f32_to_split2d(xg)
    assert torch.equal(H.split2d_to_f32(xs), xg)
    ys = H.conv2d_s2_split(xs, H.pack_resblock2d_split_weights(_g(c.w), _g(c.scale)), _g(c.shift),
                           H.split2d_buffer(B, *c.ref.shape[2:], xg.device), c.slope)
    E.assert_exact(_np(H.split2d_to_f32(ys)), _want(c, "bf16"), _lsb(c), "split output")
    _border_is_zero(ys, pad=2)


@pytest.mark.parametrize("name", E.RESBLOCK_IDS)
def test_resblock2d_and_resblock2d_split(name):
    c = E.resblock_case(name)
    N, _, Hh, W = c.x.shape
    xg = _cl(c.x)
    w1, w2, s1, s2, b1, b2 = (_g(t) for t in (c.w1, c.w2, c.s1, c.s2, c.b1, c.b2))
    want = c.ref.permute(0, 2, 3, 1).contiguous()
    y = H.resblock2d(xg, H.pack_conv2d_weights_bf16x3(w1), s1, b1, H.pack_conv2d_weights_bf16x3(w2), s2, b2, c.slope)
    E.assert_exact(_np(y), want.float().numpy(), 1.0 / 64, "fused block on fp32 activations")
    xs = H.f32_to_split2d(xg)
    assert torch.equal(H.split2d_to_f32(xs), xg)
    p1, p2 = H.pack_resblock2d_split_weights(w1, s1), H.pack_resblock2d_split_weights(w2, s2)
    y32 = H.resblock2d_split(xs, p1, b1, p2, b2, c.slope)
    E.assert_exact(_np(y32), want.float().numpy(), 1.0 / 64, "block on split activations, fp32 output")
    ys = H.resblock2d_split(xs, p1, b1, p2, b2, c.slope, out_split=H.split2d_buffer(N, Hh, W, xg.device))
    E.assert_exact(_np(H.split2d_to_f32(ys)), E.expected_split(want, "bf16"), 1.0 / 64, "block on split activations, split output")
    _border_is_zero(ys, pad=2)


# ------------------------------------------------------------------------------------------------ deformable conv, resize
@pytest.mark.parametrize("i", range(len(E.DEFORM_ROWS)))
def test_deform_conv2d(i):
    c = E.deform_case(i)
    N, Cin, Cout, Hh, W, k, st, pad, dil, res, slope = c.row
    xg, rg, sc, sh = _cl(c.x), _cl(c.r), _g(c.scale), _g(c.shift)
    wp = H.pack_deform_conv2d_weights(_g(c.w))
    for kind in ("per_image", "shared"):
        y = H.deform_conv2d(xg, _g(c.off[kind]), wp, sc, sh, (k, k), (st, st), (pad, pad), (dil, dil), res=rg, neg_slope=slope)
        want = c.ref[kind].permute(0, 2, 3, 1).contiguous().float().numpy()
        E.assert_exact(_np(y), want, 1.0 / 128, f"{kind} offset field")


@pytest.mark.parametrize("i", range(len(E.RESIZE_CASES)))
def test_resize_trilinear(i):
    c = E.resize_case(i)
    y = H.resize_trilinear(_cl(c.x), c.size)
    E.assert_exact(_np(y), c.ref.permute(0, 2, 3, 4, 1).contiguous().float().numpy(), c.lsb, "trilinear resize")
