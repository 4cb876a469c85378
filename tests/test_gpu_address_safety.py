"""Address safety of every kernel-launching entry-point family of include/mvsgi.h: what the autouse fixture of the other GPU
modules cannot see.  The fixture guards what the library allocates; here the INPUTS sit in arenas with NaN-sentinel guards too
(tests/guard_arena.py), outputs the caller supplies are arenas pre-filled with the sentinel, and every family runs at a ragged
shape (odd in every axis it accepts) plus, where the kernel walks persistently, a shape with several bricks per workgroup.

For each call (`_check`):
  1. the result on guarded tensors is bit-equal to the same call on plain tensors from torch's allocator (an over-read that
     reaches a result shows as a NaN or a changed bit) and within the kernel's existing tolerance of its float64 / ATen reference
     (the tolerances are those of tests/test_gpu_parity.py, test_gpu_instnorm.py and test_gpu_softargmin_scales.py);
  2. every input arena -- guards and body -- is byte-identical after the call;
  3. no sentinel word is left in an fp32 output; a split-padded output keeps its zero border and has no sentinel word left in
     its (sentinel pre-filled) interior;
  4. all guards of everything allocated meanwhile are clean (the autouse fixture's teardown).
hip_ops allocates its outputs (and the instance norm's workspace, the packers' buffers) through the replaced factory functions at
exactly the size mvsgi.h documents, so under the fixture every such output is an arena of its own; where hip_ops takes the
output from the caller (`out=`, split-padded buffers) the test supplies it from the arena.  Nothing here touches memory that is not
allocated.

family (include/mvsgi.h)                                   test
---------------------------------------------------------  ------------------------------------------------------------
sweep_std / cat / std_nhwc / cat_nhwc / validity_u8 /      test_sweeps
  std_nhwc_valid / _valid_rig / _valid_split_fmt (both)
conv3d_f32 DIRECT, MFMA, BF16X3, |F16, _C16, _V32, _D32    test_conv3d_streaming (ragged, dk / dk2, border-plane skip,
  (+ Cout == 1 head)                                         one-plane, persistent walks), test_conv3d_head_and_direct
conv3d_up2_f32, _out_split                                 test_conv3d_up2
conv3d_f32_out_split_fmt                                   test_conv3d_out_split
act_f32_to_split_fmt / act_split_to_f32_fmt                test_split_format_conversions
conv3d_rs_split_fmt                                        test_conv3d_rs
conv3d_rs16_split_fmt (both outputs)                       test_conv3d_rs16
conv3d_s2rs_out_fmt (split and fp32-padded)                test_conv3d_s2rs
conv3d_wino32_f16 (both activation formats)                test_conv3d_wino
conv3d_up2_poly_fmt (y_is_split 0, 3, 5)                   test_conv3d_up2_poly
conv3d_head_split / _f16                                   test_conv3d_head_split
weight packers (3-D, 2-D, stem, rs, s2rs, wino, head,      test_weight_packers
  resblock2d_split, poly plan)
conv2d_f32 (direct, fp32 MFMA, bf16 split, uint8 stem),    test_conv2d
  conv2d_f32_out_split2d
resblock2d_f32, resblock2d_split (both outputs),           test_resblock2d_and_split2d
  conv2d_s2_split, f32_to_split2d / split2d_to_f32
resize_trilinear_f32                                       test_resize_trilinear
softargmin_div_f32 (x1, x2), softargmin_scaled_f32         test_softargmin
ncv_to_nvc / nvc_to_ncv                                    test_layout
instance_norm_f32 (incl. in place)                         test_instance_norm
rays_panorama, transform_points, grid_double_sphere,       test_grid_generators
  grid_equirect
deform_conv2d_f32 (shared and per-image offsets)           test_deform_conv2d
rejections leave the output alone                          test_rejections_leave_memory_alone
whole path, guarded inputs, twice                          test_whole_path_guarded
graph-held rig constants (found by the guards)             test_graph_held_rig_constants_survive_another_batch_size
frame bases beyond 2^31 elements (part C)                  test_large_offsets_* (the grid generators included)
the harness itself                                         test_guard_hits_on_the_device_are_reported

No family is left open.
"""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard_arena
from golden_cases import SMALL_CASES
from guard_arena import SENTINEL
from mvs_gi_amd import _lib, hip_ops as H, synth
from mvs_gi_amd.configs import DIST_10, PathConfig
from mvs_gi_amd.pipeline import HotPath
from oracle import mvsgi_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def arena(request):
    """The guarded allocator of tests/guard_arena.py, as in every GPU module; the tests here also carve their inputs from it."""
    yield from guard_arena.fixture_body(request)


@pytest.fixture(autouse=True)
def _exact_mode_and_clean_flags():
    old = H.get_conv_mode()
    H.set_conv_mode("f32")
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    H.set_conv_mode(old)
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)


# ------------------------------------------------------------------------------ the harness
def _rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Split2d:
    """A 2-D split-padded buffer [N, H + 4, W + 4, 64] uint8 as a result (marks the two-pixel border for the harness)."""

    def __init__(self, buf):
        self.buf = buf


def split_out(B, D, Hh, W, C):
    """A zero-bordered split-padded output whose interior is pre-filled with the sentinel."""
    s = H.SplitAct(B, D, Hh, W, C, DEV)
    s.buf[:, 1:-1, 1:-1, 1:-1] = SENTINEL
    return s


def split2d_out(N, Hh, W):
    b = H.split2d_buffer(N, Hh, W, DEV)
    b.view(torch.int32)[:, 2:-2, 2:-2] = SENTINEL
    return b


def _flat(res):
    """result of a call -> [(kind, tensor)]: kind 'plain' | 'split' (border 1, 3-D) | 'split2d' (border 2)."""
    if res is None:
        return []
    if isinstance(res, (tuple, list)):
        return [p for r in res for p in _flat(r)]
    if isinstance(res, H.SplitAct):
        return [("split", res.buf)]
    if isinstance(res, Split2d):
        return [("split2d", res.buf)]
    assert isinstance(res, torch.Tensor), type(res)
    return [("plain", res)]


def _guard(ga, v):
    if isinstance(v, H.SplitAct):
        s = H.SplitAct(v.B, v.D, v.H, v.W, v.C, v.buf.device, buf=ga.guarded(v.buf))
        s.fmt = v.fmt
        return s
    if isinstance(v, torch.Tensor) and v.is_cuda:
        return ga.guarded(v)
    return v


def _check(ga, fn, ins, ref=None):
    """Run fn(**ins) on plain tensors (torch's allocator) and on guarded copies of the same tensors; assert 1.-3. of the module
    docstring; `ref(result)` asserts the tolerance against the reference.  -> the guarded call's result."""
    with ga.paused():
        want = _flat(fn(**ins))
    gin = {k: _guard(ga, v) for k, v in ins.items()}
    held = [(k, (v.buf if isinstance(v, H.SplitAct) else v)) for k, v in gin.items()
            if isinstance(v, H.SplitAct) or (isinstance(v, torch.Tensor) and v.is_cuda)]
    snaps = [(k, t, ga.snapshot(t)) for k, t in held]
    res = fn(**gin)
    got = _flat(res)
    assert len(got) == len(want) and got
    for i, ((kind, a), (_, b)) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"output {i}: guarded != plain"
        if kind == "plain":
            if a.dtype == torch.float32:
                w = a.contiguous().view(torch.int32)
                assert not bool((w == SENTINEL).any()), f"output {i}: an element was never stored"
                assert bool(torch.isfinite(a).all()), f"output {i}: non-finite"
        else:
            p = 1 if kind == "split" else 2
            w = a.view(torch.int32)
            inner = w[(slice(None),) + (slice(p, -p),) * (w.dim() - 2)]
            assert not bool((inner == SENTINEL).any()), f"output {i}: an interior record was never stored"
            border = w.clone()
            border[(slice(None),) + (slice(p, -p),) * (w.dim() - 2)] = 0
            assert int(border.count_nonzero()) == 0, f"output {i}: the zero border was written"
    for k, t, s in snaps:
        assert ga.unchanged(t, s), f"input {k} (or a guard around it) was written"
    if ref is not None:
        ref(res)
    return res


def _conv_ref64(x_ndhwc, wt, sc, sh, slope, stride=1, res=None, up2=False, dims=3):
    """conv + scale / shift (+ res) + LeakyReLU in float64 on channels-last tensors -> channels-last float64 numpy."""
    to_cf = (0, 4, 1, 2, 3) if dims == 3 else (0, 3, 1, 2)
    to_cl = (0, 2, 3, 4, 1) if dims == 3 else (0, 2, 3, 1)
    d = lambda t: t.detach().cpu().double()
    x = d(x_ndhwc).permute(*to_cf)
    if up2:
        x = F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=False)
    k = wt.shape[-1]
    conv = F.conv3d if dims == 3 else F.conv2d
    y = conv(x, d(wt), padding=k // 2, stride=stride)
    v = (1, -1) + (1,) * dims
    y = y * d(sc).view(*v) + d(sh).view(*v)
    if res is not None:
        y = y + d(res).permute(*to_cf)
    return torch.where(y > 0, y, y * slope).permute(*to_cl).numpy()


def _rand(rng, *shape, s=1.0):
    return _g((rng.standard_normal(shape) * s).astype(np.float32))


def _bn(rng, c):
    return _g(rng.uniform(0.5, 1.5, c).astype(np.float32)), _g((rng.standard_normal(c) * 0.1).astype(np.float32))


def _w3(rng, cout, cin, k=(3, 3, 3), s=1.0):
    return _g((rng.standard_normal((cout, cin) + tuple(k)) / np.sqrt(cin * np.prod(k)) * s).astype(np.float32))


# ------------------------------------------------------------------------------ the harness sees what it claims to see
def test_guard_hits_on_the_device_are_reported():
    """One element written into each guard of a device arena, by indexing the arena tensor itself (allocated memory only):
    the teardown check reports both with side and offset; a clean neighbour is not reported."""
    with guard_arena.GuardArena(patch=False) as ga:
        t = ga.alloc((3, 5, 7), torch.float32, DEV)
        u = ga.alloc((11,), torch.uint8, DEV)
        clean = ga.alloc((3, 5, 7), torch.float32, DEV)
        assert t.is_cuda and t.data_ptr() % 16 == 0 and t.is_contiguous() and bool(t.isnan().all())
        t.fill_(1.0)
        clean.fill_(1.0)
        u.fill_(9)
        e, eu = ga.entry_of(t), ga.entry_of(u)
        assert (t.data_ptr() - e.arena.data_ptr()) % 256 == guard_arena.SKEW
        e.arena[e.body_off // 4 - 1] = 0                                      # the word before the body
        e.arena[(e.body_off + e.nbytes) // 4 + 2] = 0                         # the third word behind it
        eu.arena.view(torch.uint8)[eu.body_off + eu.nbytes] = 0               # the byte behind a body that ends inside a word
    rep = ga.report()
    assert len(rep) == 3, rep
    assert any("before the body of (3, 5, 7)" in r and "offset -4 " in r for r in rep), rep
    assert any("after the body of (3, 5, 7)" in r and "offset +8 " in r for r in rep), rep
    assert any("after the body of (11,) torch.uint8" in r and "offset +0 " in r for r in rep), rep


def test_the_patched_allocator_guards_library_outputs(arena):
    """Under the fixture a library output is an arena view that passes hip_ops._dev unchanged (no silent clone), starts 16-byte
    aligned and not more, and is NaN until a kernel stores it."""
    y = torch.empty((2, 3, 5, 7, 16), device=DEV, dtype=torch.float32)
    e = arena.entry_of(y)
    assert (y.data_ptr() - e.arena.data_ptr()) % 256 == 16 and H._dev(y, "y") is y and bool(y.isnan().all())
    z = torch.zeros((2, 5, 7, 9, 16), device=DEV, dtype=torch.int32)
    assert int(z.count_nonzero()) == 0 and hasattr(z, "_guard_entry")
    with arena.paused():
        assert not hasattr(torch.empty(4, device=DEV), "_guard_entry")
    assert not hasattr(torch.empty(4), "_guard_entry")


# ------------------------------------------------------------------------------ sweeps
def test_sweeps(arena):
    """The five sweeps at a shape odd in every axis (D 7, Ho 7, Wo 29, Hi 13, Wi 45, masks 50 x 178), two frames, random grids
    (samples outside the image in every direction): bit-exact against the CPU oracle as in test_sweep_seeded_bit_exact."""
    cfgs = {"std": PathConfig("odd-std", 3, "std", 16, 32, DIST_10[:7], feat_hw=(13, 45), mask_hw=(50, 178), cv_hw=(7, 29)),
            "cat": PathConfig("odd-cat", 2, "cat", 32, 32, DIST_10[:7], feat_hw=(13, 45), mask_hw=(50, 178), cv_hw=(7, 29))}
    inp = synth.make_inputs(cfgs["std"], seed=3, batch=2, grid_kind="random", grid_mask_dtype="bool")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inp.items()}
    want = O.sweep_std_masked(t["feats"], t["grids"], t["grid_masks"], t["masks"]).permute(0, 2, 3, 4, 1).contiguous()
    f, g, gm, m = (_g(inp[k]) for k in ("feats", "grids", "grid_masks", "masks"))
    f_cl = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)            # channels-last storage
    exact = lambda y: (lambda r: _assert_equal(r, y))
    for gmask in (gm, gm.float(), gm.to(torch.uint8)):
        _check(arena, lambda feats, grids, grid_masks, masks: H.sweep_std(feats, grids, grid_masks, masks, layout="nchw"),
               dict(feats=f, grids=g, grid_masks=gmask, masks=m), exact(want))                       # sweep_std_f32
        _check(arena, lambda feats, grids, grid_masks, masks: H.sweep_std(feats, grids, grid_masks, masks),
               dict(feats=f, grids=g, grid_masks=gmask, masks=m), exact(want))                       # ncv_to_nvc + sweep_std_nhwc_f32
    vm = _check(arena, H.sweep_validity, dict(grids=g, grid_masks=gm, masks=m))                       # sweep_validity_u8
    assert vm.dtype == torch.uint8 and int(vm.max()) < 8
    _check(arena, H.sweep_std_valid, dict(feats=f, grids=g, vmask=vm.clone()), exact(want))           # sweep_std_nhwc_valid_f32
    # one rig for the whole batch: frame b of the result is the sweep of frame b's features through rig 0
    g1, vm1 = g[:1].contiguous(), vm[:1].clone()
    rig = O.sweep_std_masked(t["feats"], t["grids"][:1].expand(2, -1, -1, -1, -1, -1), t["grid_masks"][:1].expand(2, -1, -1, -1, -1, -1),
                             t["masks"][:1].expand(2, -1, -1, -1, -1)).permute(0, 2, 3, 4, 1).contiguous()
    _check(arena, H.sweep_std_valid, dict(feats=f, grids=g1, vmask=vm1), exact(rig))                  # sweep_std_nhwc_valid_rig_f32
    for fmt in ("bf16", "f16"):
        for gg, vv, vol in ((g, vm.clone(), want), (g1, vm1, rig)):
            with arena.paused():
                split_of_vol = H.act_to_split(vol.to(DEV), fmt=fmt).buf
            _check(arena, lambda feats, grids, vmask: H.sweep_std_valid_split(feats, grids, vmask, out=split_out(2, 7, 7, 29, 16), fmt=fmt),
                   dict(feats=f_cl, grids=gg, vmask=vv), lambda r: _assert_equal(r.buf, split_of_vol))   # sweep_std_nhwc_valid_split_fmt
    inc = synth.make_inputs(cfgs["cat"], seed=4, batch=2, grid_kind="random")
    wantc = O.sweep_concat(torch.from_numpy(inc["feats"]), torch.from_numpy(inc["grids"])).permute(0, 2, 3, 4, 1).contiguous()
    for layout in ("nchw", "auto"):                                                                    # sweep_cat_f32, sweep_cat_nhwc_f32
        _check(arena, lambda feats, grids: H.sweep_cat(feats, grids, layout=layout), dict(feats=_g(inc["feats"]), grids=_g(inc["grids"])),
               exact(wantc))


def _assert_equal(got, want):
    assert torch.equal(got.cpu(), want.cpu())


# ------------------------------------------------------------------------------ streaming conv3d
def _conv_call(impl, stride, slope, fmt16=False):
    def fn(x, w, wp, scale, shift, res=None):
        return H.conv3d(x, w, wp, scale, shift, res=res, stride=stride, neg_slope=slope, impl=impl)
    return fn


STREAM_SHAPES = [
    # (B, Cin, Cout, D, H, W, stride, res, slope): from CONV_SHAPES of tests/test_gpu_parity.py
    (2, 16, 16, 9, 7, 37, 1, True, 0.01),        # Cout 16 with residual, ragged in every axis (also the plane-schedule kernel)
    (1, 16, 32, 7, 9, 13, 2, False, 0.01),       # stride 2, odd sizes
    (1, 128, 128, 2, 5, 9, 1, True, 0.01),       # 16-cout units, weights through LDS
    (40, 64, 64, 3, 15, 21, 1, True, 0.01),      # 2 x 5 x 16 bricks ragged in D and W, several bricks per workgroup; 32-channel slices
    (96, 32, 128, 1, 7, 21, 1, True, 0.0),       # one-plane volume, ragged: the depth skip (dk) of the 32-channel-slice kernels
    (1, 128, 128, 2, 10, 40, 1, True, 0.01),     # two planes on one-plane units: dk2
    (44, 32, 96, 4, 18, 70, 1, False, 0.01),     # four planes deep, >= 4 rounds: the border-plane skip, ragged
    (48, 32, 128, 7, 17, 23, 2, False, 0.01),    # stride 2 in 128-cout units, odd sizes
]


@pytest.mark.parametrize("shape", STREAM_SHAPES)
def test_conv3d_streaming(arena, shape):
    B, Cin, Cout, D, Hh, W, stride, res, slope = shape
    rng = np.random.default_rng(sum(shape[:7]))
    x = _rand(rng, B, D, Hh, W, Cin)
    w = _w3(rng, Cout, Cin)
    sc, sh = _bn(rng, Cout)
    Do, Ho, Wo = (D - 1) // stride + 1, (Hh - 1) // stride + 1, (W - 1) // stride + 1
    r = _rand(rng, B, Do, Ho, Wo, Cout) if res else None
    yref = _conv_ref64(x, w, sc, sh, slope, stride, r)
    w16 = w * 0.01                                                   # as test_conv3d_f16x3_vs_oracle: small weights
    yref16 = _conv_ref64(x, w16, sc, sh, slope, stride, r)

    def run(impl, wp, tol, ref, scale=sc, wt=w):
        ins = dict(x=x, w=wt, wp=wp, scale=scale, shift=sh)
        if res:
            ins["res"] = r
        return _check(arena, _conv_call(impl, stride, slope), ins, lambda y: _assert_rel(y, ref, tol))

    run(H.CONV_MFMA, H.pack_conv_weights(w), 2e-5, yref)
    if B * Cout * Do * Ho * Wo <= 1 << 21:                            # the direct kernel on the small shapes only (it is slow)
        run(H.CONV_DIRECT, H.pack_conv_weights(w), 2e-5, yref)
    assert "bf16x3" in H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3)
    run(H.CONV_BF16X3, H.pack_conv_weights_bf16x3(w), 1e-4, yref)
    wp16, un = H.pack_conv_weights_f16x3(w16)
    assert H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3 | H.CONV_F16).startswith("conv3d_f16x3_kernel<")
    run(H.CONV_BF16X3 | H.CONV_F16, wp16, 5e-6, yref16, scale=sc * un, wt=w16)
    if H.conv3d_d32_applies(B, Cin, D, Hh, W, Cout, stride):
        name = H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3_D32)
        assert "_d32_" in name, name
        if shape[:6] == (96, 32, 128, 1, 7, 21):
            assert "_d32_dk_kernel<" in name, name
        if shape[:6] == (1, 128, 128, 2, 10, 40):
            assert "_d32_dk2_kernel<" in name, name
        run(H.CONV_BF16X3_D32, H.pack_conv_weights_bf16x3_d32(w), 1e-4, yref)
        wpd, und = H.pack_conv_weights_f16x3(w16, H.CONV_BF16X3_D32)
        run(H.CONV_BF16X3_D32 | H.CONV_F16, wpd, 5e-6, yref16, scale=sc * und, wt=w16)
    else:
        assert shape[:6] not in ((96, 32, 128, 1, 7, 21), (1, 128, 128, 2, 10, 40), (40, 64, 64, 3, 15, 21))
    if Cout == 16 and stride == 1:
        assert "true, false, false>" in H.conv3d_variant(B, Cin, D, Hh, W, Cout, stride, H.CONV_BF16X3_C16)
        run(H.CONV_BF16X3_C16, H.pack_conv_weights_bf16x3_c16(w), 1e-4, yref)
        wpc, unc = H.pack_conv_weights_f16x3(w16, H.CONV_BF16X3_C16)
        run(H.CONV_BF16X3_C16 | H.CONV_F16, wpc, 5e-6, yref16, scale=sc * unc, wt=w16)


def _assert_rel(got, ref, tol):
    got = H.act_from_split(got) if isinstance(got, H.SplitAct) and got.fmt in ("bf16", "f16") else got
    err = _rel(got, ref)
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("shape", [(3, 32, 32, 9, 37, 70, False, 0.01), (17, 16, 96, 4, 12, 32, False, 1.0), (22, 64, 64, 4, 10, 48, True, 0.0)])
def test_conv3d_v32_schedule(arena, shape):
    """The 32x32x16-MFMA schedule: ragged in every axis; three tiles of 32 couts (the last workgroup's second wave is clamped)."""
    B, Cin, Cout, D, Hh, W, res, slope = shape
    rng = np.random.default_rng(sum(shape[:6]))
    x, w = _rand(rng, B, D, Hh, W, Cin), _w3(rng, Cout, Cin)
    sc, sh = _bn(rng, Cout)
    r = _rand(rng, B, D, Hh, W, Cout) if res else None
    assert H.conv3d_v32_applies(B, Cin, D, Hh, W, Cout, 1)
    assert "false, false, true, false>" in H.conv3d_variant(B, Cin, D, Hh, W, Cout, 1, H.CONV_BF16X3_V32)
    yref = _conv_ref64(x, w, sc, sh, slope, 1, r)
    ins = dict(x=x, w=w, wp=H.pack_conv_weights_bf16x3_v32(w), scale=sc, shift=sh)
    if res:
        ins["res"] = r
    _check(arena, _conv_call(H.CONV_BF16X3_V32, 1, slope), ins, lambda y: _assert_rel(y, yref, 1e-4))
    w16 = w * 0.01
    wp16, un = H.pack_conv_weights_f16x3(w16, H.CONV_BF16X3_V32)
    ins.update(w=w16, wp=wp16, scale=sc * un)
    yref16 = _conv_ref64(x, w16, sc, sh, slope, 1, r)
    _check(arena, _conv_call(H.CONV_BF16X3_V32 | H.CONV_F16, 1, slope), ins, lambda y: _assert_rel(y, yref16, 5e-6))


def test_conv3d_head_and_direct(arena):
    """The Cout == 1 head of mvsgi_conv3d_f32 (whole-depth march, ragged H and W) and the direct kernel on odd channel counts."""
    rng = np.random.default_rng(8)
    for (B, Cin, Cout, dims, res, slope) in ((3, 16, 1, (5, 125, 47), True, 0.01), (2, 48, 1, (5, 7, 9), False, 1.0),
                                             (2, 5, 3, (5, 7, 9), False, 1.0), (2, 4, 8, (3, 5, 11), False, 0.01)):
        x, w = _rand(rng, B, *dims, Cin), _w3(rng, Cout, Cin)
        sc, sh = _bn(rng, Cout)
        r = _rand(rng, B, *dims, Cout) if res else None
        name = H.conv3d_variant(B, Cin, *dims, Cout)
        assert ("head" in name) if (Cout == 1 and Cin % 16 == 0) else ("direct" in name)
        yref = _conv_ref64(x, w, sc, sh, slope, 1, r)
        ins = dict(x=x, w=w, wp=H.pack_conv_weights(w), scale=sc, shift=sh)
        if ins["wp"] is None:
            del ins["wp"]
        if res:
            ins["res"] = r
        fn = (lambda x, w, scale, shift, wp=None, res=None: H.conv3d(x, w, wp, scale, shift, res=res, neg_slope=slope))
        _check(arena, fn, ins, lambda y: _assert_rel(y, yref, 2e-5))


@pytest.mark.parametrize("shape", [(2, 32, 16, 3, 5, 9, False), (1, 128, 64, 1, 3, 5, True), (12, 64, 96, 3, 5, 9, False), (48, 64, 96, 1, 10, 40, True)])
def test_conv3d_up2(arena, shape):
    """mvsgi_conv3d_up2_f32 and _out_split: ragged bricks and odd low-resolution sizes, Dl = 1 (every corner clamps along D), the
    32-channel-slice form on several bricks per workgroup, the depth-skip form out of a one-plane level."""
    B, Cin, Cout, Dl, Hl, Wl, res = shape
    rng = np.random.default_rng(sum(shape[:6]))
    x, w = _rand(rng, B, Dl, Hl, Wl, Cin), _w3(rng, Cout, Cin)
    sc, sh = _bn(rng, Cout)
    r = _rand(rng, B, 2 * Dl, 2 * Hl, 2 * Wl, Cout) if res else None
    yref = _conv_ref64(x, w, sc, sh, 0.01, 1, r, up2=True)
    assert "true" in H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout)

    def run(layout, wp, scale, tol, split=True):
        ins = dict(x=x, wp=wp, scale=scale, shift=sh)
        if res:
            ins["res"] = r
        y = _check(arena, lambda x, wp, scale, shift, res=None: H.conv3d_up2(x, wp, scale, shift, res=res, neg_slope=0.01, w_layout=layout),
                   ins, lambda y: _assert_rel(y, yref, tol))
        if not split:
            return
        fmt = "f16" if layout & H.CONV_F16 else "bf16"
        with arena.paused():
            want = H.act_to_split(y, fmt=fmt).buf
        _check(arena, lambda x, wp, scale, shift, res=None: H.conv3d_up2_out_split(
            x, wp, scale, shift, out=split_out(B, 2 * Dl, 2 * Hl, 2 * Wl, Cout), res=res, neg_slope=0.01, w_layout=layout),
            ins, lambda s: _assert_equal(s.buf, want))

    run(H.CONV_BF16X3, H.pack_conv_weights_bf16x3(w), sc, 1e-4)
    wp16, un = H.pack_conv_weights_f16x3(w)
    run(H.CONV_BF16X3 | H.CONV_F16, wp16, sc * un, 1e-5)
    if Cout == 16:
        run(H.CONV_BF16X3_C16, H.pack_conv_weights_bf16x3_c16(w), sc, 1e-4)
    if H.conv3d_up2_d32_applies(B, Cin, Dl, Hl, Wl, Cout):
        assert ("d32u_dk_kernel<" if Dl == 1 else "d32u_kernel<") in H.conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout, H.CONV_BF16X3_D32)
        run(H.CONV_BF16X3_D32, H.pack_conv_weights_bf16x3_d32(w), sc, 1e-4, split=False)      # (no split-padded output in this layout)
    else:
        assert B < 12


@pytest.mark.parametrize("shape", [(2, 16, 32, 7, 9, 13, 2), (1, 16, 16, 5, 9, 11, 1), (40, 32, 32, 3, 15, 21, 1)])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_conv3d_out_split(arena, shape, fmt):
    """mvsgi_conv3d_f32_out_split_fmt: bit for bit the split of the fp32 output of the same launch, border included."""
    B, cin, cout, d, h, w, s = shape
    rng = np.random.default_rng(11)
    x, wt = _rand(rng, B, d, h, w, cin), _w3(rng, cout, cin)
    sc, sh = _bn(rng, cout)
    do, ho, wo = (d - 1) // s + 1, (h - 1) // s + 1, (w - 1) // s + 1
    r = _rand(rng, B, do, ho, wo, cout)
    if fmt == "f16":
        wp, un = H.pack_conv_weights_f16x3(wt)
        sc = sc * un
    else:
        wp = H.pack_conv_weights_bf16x3(wt)
    with arena.paused():
        y = H.conv3d(x, wt, wp, sc, sh, res=r, stride=s, impl=H.CONV_BF16X3 | (H.CONV_F16 if fmt == "f16" else 0))
        want = H.act_to_split(y, fmt=fmt).buf
    _check(arena, lambda x, wp, scale, shift, res: H.conv3d_out_split(x, wp, scale, shift, out=split_out(B, do, ho, wo, cout), res=res, stride=s, fmt=fmt),
           dict(x=x, wp=wp, scale=sc, shift=sh, res=r), lambda o: _assert_equal(o.buf, want))


# ------------------------------------------------------------------------------ split-padded formats and their kernels
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_split_format_conversions(arena, fmt):
    rng = np.random.default_rng(3)
    for shape in ((2, 3, 5, 7, 32), (3, 9, 7, 37, 16), (1, 1, 1, 1, 48)):
        x = _rand(rng, *shape, s=10.0)
        s = _check(arena, lambda x: H.act_to_split(x, out=split_out(*shape), fmt=fmt), dict(x=x))
        back = _check(arena, H.act_from_split, dict(x=s))
        if fmt == "f16":      # the bars of the round-trip tests in tests/test_gpu_parity.py: 22 significant bits of the tensor's maximum ...
            assert float((back - x).abs().max()) <= 2.0 ** -21 * float(x.abs().max())
        else:                 # ... 16-17 significant bits per element
            assert float(((back - x).abs() / x.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
        again = H.act_from_split(H.act_to_split(back, fmt=fmt))
        assert torch.equal(again, back)                               # the representable set is closed under the conversion


@pytest.mark.parametrize("shape", [(2, 5, 7, 37), (4, 9, 30, 70)])      # ragged in every axis; 800 ragged bricks: n > 1 per workgroup
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_conv3d_rs(arena, shape, fmt):
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x, r = _rand(rng, B, d, h, w, 32), _rand(rng, B, d, h, w, 32)
    wt = _w3(rng, 32, 32, s=0.02 if fmt == "f16" else 1.0)
    sc, sh = _bn(rng, 32)
    tol = 5e-6 if fmt == "f16" else 1e-4
    with arena.paused():
        xs, rs = H.act_to_split(x, fmt=fmt), H.act_to_split(r, fmt=fmt)
        xq, rq = H.act_from_split(xs), H.act_from_split(rs)
    if fmt == "f16":
        wp, un = H.pack_conv_weights_rs(wt, "f16")
        scale = sc * un
    else:
        wp, scale = H.pack_conv_weights_rs(wt), sc
    for res, slope, out_f32 in ((True, 0.01, False), (False, 0.01, True), (True, 0.0, True), (False, 1.0, False)):
        ref = _conv_ref64(xq, wt, sc, sh, slope, res=rq if res else None)
        ins = dict(x=xs, wp=wp, scale=scale, shift=sh)
        if res:
            ins["res"] = rs
        _check(arena, lambda x, wp, scale, shift, res=None: H.conv3d_rs(x, wp, scale, shift, res=res, neg_slope=slope,
                                                                        out=None if out_f32 else split_out(B, d, h, w, 32), out_f32=out_f32),
               ins, lambda y: _assert_rel(y, ref, tol))


@pytest.mark.parametrize("shape", [(2, 5, 7, 37), (3, 10, 30, 150)])    # ragged; 720 ragged bricks: masked stores mid-walk
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_conv3d_rs16(arena, shape, fmt):
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x, wt = _rand(rng, B, d, h, w, 16), _w3(rng, 16, 16)
    sc, sh = _bn(rng, 16)
    with arena.paused():
        xs = H.act_to_split(x, fmt=fmt)
        xq = H.act_from_split(xs)
    wp, scale = (H.pack_conv_weights_rs(wt), sc)
    if fmt == "f16":
        wp, un = H.pack_conv_weights_rs(wt, "f16")
        scale = sc * un
    ref = _conv_ref64(xq, wt, sc, sh, 0.01)
    y = _check(arena, lambda x, wp, scale, shift: H.conv3d_rs16(x, wp, scale, shift, neg_slope=0.01), dict(x=xs, wp=wp, scale=scale, shift=sh),
               lambda y: _assert_rel(y, ref, 5e-6 if fmt == "f16" else 1e-4))
    with arena.paused():
        want = H.act_to_split(y, fmt=fmt).buf
    _check(arena, lambda x, wp, scale, shift: H.conv3d_rs16(x, wp, scale, shift, neg_slope=0.01, out_split=split_out(B, d, h, w, 16)),
           dict(x=xs, wp=wp, scale=scale, shift=sh), lambda s: _assert_equal(s.buf, want))


@pytest.mark.parametrize("shape", [(1, 5, 7, 19), (3, 2, 9, 33), (4, 16, 80, 320)])     # odd sizes, ragged tiles; 3200 bricks: several per workgroup
def test_conv3d_s2rs(arena, shape):
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 4)
    x, wt = _rand(rng, B, d, h, w, 16), _w3(rng, 32, 16)
    sc, sh = _bn(rng, 32)
    do, ho, wo = (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for fmt in ("bf16", "f16"):
        with arena.paused():
            xs = H.act_to_split(x, fmt=fmt)
            xq = H.act_from_split(xs)
        ref = _conv_ref64(xq, wt, sc, sh, 0.01, stride=2)
        if fmt == "f16":
            wp, up, un = H.pack_conv_weights_s2rs(wt, sc, "f16")
            shift = sh * up
        else:
            wp, up, un, shift = H.pack_conv_weights_s2rs(wt, sc), 1.0, 1.0, sh
        z = _check(arena, lambda x, wp, shift: H.conv3d_s2rs(x, wp, shift, split_out(B, do, ho, wo, 32), neg_slope=0.01, unscale=un),
                   dict(x=xs, wp=wp, shift=shift), lambda y: _assert_rel(y, ref, 5e-6 if fmt == "f16" else 1e-4))
        if fmt == "f16":      # the fp32-padded output: the same values before the split
            z32 = _check(arena, lambda x, wp, shift: H.conv3d_s2rs(x, wp, shift, split_out(B, do, ho, wo, 32), neg_slope=0.01, unscale=un, out_f32p=True),
                         dict(x=xs, wp=wp, shift=shift))
            assert z32.fmt == "f32p" and torch.equal(H.act_to_split(H.act_from_f32p(z32), fmt="f16").buf, z.buf)


@pytest.mark.parametrize("shape", [(5, 8, 12, 32), (3, 8, 40, 160), (2, 16, 4, 32)])    # one workgroup per unit and several; 8 and 16 planes
@pytest.mark.parametrize("act32", [False, True])
def test_conv3d_wino(arena, shape, act32):
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 18)
    x, r = _rand(rng, B, d, h, w, 32), _rand(rng, B, d, h, w, 32)
    wt = _w3(rng, 32, 32, s=0.02)
    sc, sh = _bn(rng, 32)
    assert H.conv3d_wino_applies(32, 32, d, h, w, 1, 0.01)
    to_act, from_act = (H.act_to_f32p, H.act_from_f32p) if act32 else ((lambda t: H.act_to_split(t, fmt="f16")), H.act_from_split)
    with arena.paused():
        xs, rs = to_act(x), to_act(r)
        xq, rq = from_act(xs), from_act(rs)
        wp, un = H.pack_conv_weights_wino(wt)

    def out_buf():
        s = split_out(B, d, h, w, 32)
        return s
    for res, slope, out_f32 in ((True, 0.01, False), (False, 0.01, True), (True, 1.0, True), (False, 0.0, False)):
        ref = _conv_ref64(xq, wt, sc, sh, slope, res=rq if res else None)
        ins = dict(x=xs, wp=wp, scale=sc * un, shift=sh)
        if res:
            ins["res"] = rs
        _check(arena, lambda x, wp, scale, shift, res=None: H.conv3d_wino(x, wp, scale, shift, res=res, neg_slope=slope,
                                                                          out=None if out_f32 else out_buf(), out_f32=out_f32),
               ins, lambda y: _assert_rel(y if out_f32 else from_act(y), ref, 5e-6))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 5, 9, 33), (9, 3, 12, 40), (2, 8, 40, 160)])     # single-cell axes, odd and ragged, more bricks than workgroups
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_conv3d_up2_poly(arena, shape, fmt):
    """mvsgi_conv3d_up2_poly_fmt with y_is_split 0 (fp32), 3 (split, direct main kernel) and 5 (split, Winograd form where it applies)."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x, wt = _rand(rng, B, d, h, w, 32), _w3(rng, 16, 32)
    sc, sh = _bn(rng, 16)
    with arena.paused():
        xs = H.act_to_split(x, fmt=fmt)
        xq = H.act_from_split(xs)
    ref = _conv_ref64(xq, wt, sc, sh, 0.01, up2=True)
    if fmt == "f16":
        plan, un = H.conv3d_up2_poly_plan(wt, d, h, w, fmt="f16")
        scale = sc * un
    else:
        plan, scale = H.conv3d_up2_poly_plan(wt, d, h, w), sc
    tol = 5e-6 if fmt == "f16" else 1e-4
    ins = dict(x=xs, plan=plan, scale=scale, shift=sh)
    y = _check(arena, lambda x, plan, scale, shift: H.conv3d_up2_poly(x, plan, scale, shift, neg_slope=0.01), ins, lambda y: _assert_rel(y, ref, tol))
    with arena.paused():
        want = H.act_to_split(y, fmt=fmt).buf
    _check(arena, lambda x, plan, scale, shift: H.conv3d_up2_poly_split(x, plan, scale, shift, out=split_out(B, 2 * d, 2 * h, 2 * w, 16),
                                                                        neg_slope=0.01, direct=True),
           ins, lambda s: _assert_equal(s.buf, want))
    if fmt == "f16" and d == 8 and h % 2 == 0 and w % 32 == 0:
        _check(arena, lambda x, plan, scale, shift: H.conv3d_up2_poly_split(x, plan, scale, shift, out=split_out(B, 2 * d, 2 * h, 2 * w, 16),
                                                                            neg_slope=0.01, wino=True),
               ins, lambda s: _assert_rel(s, ref, 5e-6))


@pytest.mark.parametrize("shape", [(2, 16, 5, 9, 33), (2, 48, 5, 8, 32), (70, 16, 2, 8, 32), (3, 16, 16, 80, 320)])
def test_conv3d_head_split(arena, shape):
    B, cin, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x, wt = _rand(rng, B, d, h, w, cin), _w3(rng, 1, cin)
    for f16 in (False, True):
        with arena.paused():
            xs = H.act_to_split(x, fmt="f16" if f16 else "bf16")
            xq = H.act_from_split(xs)
        ref = F.conv3d(xq.cpu().double().permute(0, 4, 1, 2, 3), wt.cpu().double(), padding=1).permute(0, 2, 3, 4, 1).numpy() + 0.37
        if f16:
            wp, un = H.pack_head_split_weights_f16(wt)
        else:
            wp, un = H.pack_head_split_weights(wt), 1.0
        _check(arena, lambda x, wp: H.conv3d_head_split(x, wp, 1.0 * un, 0.37, f16=f16), dict(x=xs, wp=wp),
               lambda y: _assert_rel(y, ref, 5e-6 if f16 else 1e-4))


def test_weight_packers(arena):
    """Every packer's output is allocated at exactly the size its *_bytes / *_floats function states (hip_ops does; under the
    fixture that allocation has guards on both sides) and is bit-equal from guarded and from plain weights."""
    rng = np.random.default_rng(77)
    lib = _lib.load()
    w = lambda co, ci, *k: _g((rng.standard_normal((co, ci) + (k or (3, 3, 3))) * 0.1).astype(np.float32))
    sizes = []

    def chk(fn, ins, nbytes=None):
        r = _check(arena, fn, ins)
        first = _flat(r)[0][1]
        if nbytes is not None:
            assert first.numel() * first.element_size() == nbytes, (first.shape, nbytes)
        sizes.append(first.numel())
    chk(lambda w: H.pack_conv_weights(w), dict(w=w(48, 32)), 4 * lib.mvsgi_conv3d_packed_weight_floats(48, 32))
    chk(lambda w: H.pack_conv_weights(w), dict(w=w(1, 48)), 4 * lib.mvsgi_conv3d_packed_weight_floats(1, 48))
    chk(lambda w: H.pack_conv_weights_bf16x3(w), dict(w=w(48, 32)), lib.mvsgi_conv3d_packed_weight_bytes_bf16x3(48, 32))
    chk(lambda w: H.pack_conv_weights_bf16x3_d32(w), dict(w=w(48, 64)), lib.mvsgi_conv3d_packed_weight_bytes_bf16x3(48, 64))
    chk(lambda w: H.pack_conv_weights_bf16x3_v32(w), dict(w=w(96, 16)), lib.mvsgi_conv3d_packed_weight_bytes_bf16x3_v32(96, 16))
    chk(lambda w: H.pack_conv_weights_bf16x3_c16(w), dict(w=w(16, 48)), lib.mvsgi_conv3d_packed_weight_bytes_bf16x3_c16(48))
    for layout, (co, ci) in ((H.CONV_BF16X3, (48, 32)), (H.CONV_BF16X3_C16, (16, 48)), (H.CONV_BF16X3_V32, (96, 16)), (H.CONV_BF16X3_D32, (48, 64))):
        chk(lambda w: H.pack_conv_weights_f16x3(w, layout), dict(w=w(co, ci)))
    for co in (32, 16):
        chk(lambda w: H.pack_conv_weights_rs(w), dict(w=w(co, co)), lib.mvsgi_conv3d_rs_packed_weight_bytes(co, co))
        chk(lambda w: H.pack_conv_weights_rs(w, "f16"), dict(w=w(co, co)))
    sc32 = _g(rng.uniform(0.5, 1.5, 32).astype(np.float32))
    chk(lambda w, scale: H.pack_conv_weights_s2rs(w, scale), dict(w=w(32, 16), scale=sc32), lib.mvsgi_conv3d_s2rs_packed_weight_bytes())
    chk(lambda w, scale: H.pack_conv_weights_s2rs(w, scale, "f16")[0], dict(w=w(32, 16), scale=sc32), lib.mvsgi_conv3d_s2rs_packed_weight_bytes())
    chk(lambda w: H.pack_conv_weights_wino(w), dict(w=w(32, 32)), lib.mvsgi_conv3d_wino32_packed_weight_bytes())
    chk(lambda w: H.pack_head_split_weights(w), dict(w=w(1, 48)), lib.mvsgi_conv3d_head_split_packed_weight_bytes(48))
    chk(lambda w: H.pack_head_split_weights_f16(w)[0], dict(w=w(1, 48)), lib.mvsgi_conv3d_head_split_packed_weight_bytes(48))
    chk(lambda w: H.pack_conv2d_weights_bf16x3(w), dict(w=w(32, 16, 3, 3)), lib.mvsgi_conv2d_packed_weight_bytes_bf16x3(32, 16))
    chk(lambda w: H.pack_conv2d_weights_f32(w), dict(w=w(32, 16, 3, 3)), 4 * lib.mvsgi_conv2d_packed_weight_floats(32, 16))
    chk(lambda w: H.pack_conv2d_stem_weights(w), dict(w=w(16, 3, 5, 5)), lib.mvsgi_conv2d_stem_packed_weight_bytes())
    chk(lambda w, scale: H.pack_resblock2d_split_weights(w, scale), dict(w=w(16, 16, 3, 3), scale=sc32[:16].clone()),
        lib.mvsgi_resblock2d_split_packed_weight_bytes())
    chk(lambda w: H.pack_deform_conv2d_weights(w), dict(w=w(8, 5, 3, 3)))
    for fmt in ("bf16", "f16"):      # the plan is built on the host and uploaded: same bytes from a guarded weight
        chk(lambda w: (lambda p: p[0] if isinstance(p, tuple) else p)(H.conv3d_up2_poly_plan(w, 3, 5, 9, fmt=fmt)), dict(w=w(16, 32)),
            lib.mvsgi_conv3d_up2_poly_plan_bytes(3, 5, 9))
    assert all(n > 0 for n in sizes)
    # the 32-channel-slice layout fills 27 of the 28 k-steps its buffer is sized for: the packer zeroes the rest (it once left it unwritten)
    for wp in (H.pack_conv_weights_bf16x3_d32(w(48, 64)), H.pack_conv_weights_f16x3(w(48, 64), H.CONV_BF16X3_D32)[0]):
        used = wp.numel() // 28 * 27
        assert int(wp[used:].count_nonzero()) == 0 and int(wp[:used].count_nonzero()) > 0


# ------------------------------------------------------------------------------ 2-D
@pytest.mark.parametrize("shape", [(1, 16, 16, 33, 47, 1, False), (2, 16, 16, 23, 41, 2, True), (1, 32, 32, 17, 29, 1, True), (1, 16, 64, 15, 31, 2, False)])
def test_conv2d(arena, shape):
    B, Cin, Cout, Hh, W, stride, res = shape
    rng = np.random.default_rng(sum(shape))
    x, w = _rand(rng, B, Hh, W, Cin), _w3(rng, Cout, Cin, (3, 3))
    sc, sh = _bn(rng, Cout)
    ho, wo = (Hh - 1) // stride + 1, (W - 1) // stride + 1
    r = _rand(rng, B, ho, wo, Cout) if res else None
    yref = _conv_ref64(x, w, sc, sh, 0.01, stride, r, dims=2)

    def run(impl, wp, tol):
        ins = dict(x=x, w=w, scale=sc, shift=sh)
        if wp is not None:
            ins["wp"] = wp
        if res:
            ins["res"] = r
        return _check(arena, lambda x, w, scale, shift, wp=None, res=None: H.conv2d(x, w, wp, scale, shift, res=res, stride=stride, impl=impl),
                      ins, lambda y: _assert_rel(y, yref, tol))
    run(H.CONV_DIRECT, None, 2e-5)
    assert "bf16x3" in H.conv2d_variant(Cin, Cout, 3, stride, H.CONV_BF16X3)
    yb = run(H.CONV_BF16X3, H.pack_conv2d_weights_bf16x3(w), 1e-4)
    wpf = H.pack_conv2d_weights_f32(w)
    if wpf is not None:
        assert "conv3d_mfma_kernel" in H.conv2d_variant(Cin, Cout, 3, stride, H.CONV_MFMA)
        run(H.CONV_MFMA, wpf, 2e-5)
    if Cout == 16:      # mvsgi_conv2d_f32_out_split2d: the split (hi + lo: 16-17 bits) of the fp32 output of the same launch
        ins = dict(x=x, w=w, wp=H.pack_conv2d_weights_bf16x3(w), scale=sc, shift=sh)
        if res:
            ins["res"] = r
        s = _check(arena, lambda x, w, wp, scale, shift, res=None: Split2d(H.conv2d(x, w, wp, scale, shift, res=res, stride=stride, impl=H.CONV_BF16X3,
                                                                                  out_split=split2d_out(B, ho, wo))), ins)
        back = H.split2d_to_f32(s.buf)
        assert float(((back - yb).abs() / yb.abs().clamp_min(1e-20)).max()) <= 2.0 ** -15


@pytest.mark.parametrize("hw", [(37, 132), (21, 30), (5, 4)])      # W % 4 == 0: the matrix-core stem; W = 30: the fp32 stem
def test_conv2d_uint8_stem(arena, hw):
    rng = np.random.default_rng(21)
    Hh, Ww = hw
    u8 = _g(rng.integers(0, 256, (3, Hh, Ww, 3), dtype=np.uint8))
    w = _w3(rng, 16, 3, (5, 5))
    sc, sh = _bn(rng, 16)
    x64 = u8.cpu().permute(0, 3, 1, 2).double() / 255.0
    ref = F.conv2d(x64, w.cpu().double(), None, stride=2, padding=2)
    ref = F.leaky_relu(ref * sc.cpu().double().view(1, -1, 1, 1) + sh.cpu().double().view(1, -1, 1, 1), 0.01).permute(0, 2, 3, 1).numpy()
    fn = lambda x, w, scale, shift, wp=None: H.conv2d(x, w, wp, scale, shift, stride=2)
    _check(arena, fn, dict(x=u8, w=w, wp=H.pack_conv2d_stem_weights(w), scale=sc, shift=sh), lambda y: _assert_rel(y, ref, 5e-7))
    _check(arena, fn, dict(x=u8, w=w, scale=sc, shift=sh), lambda y: _assert_rel(y, ref, 5e-6))
    xn = _g(rng.random((2, 3, Hh, Ww)).astype(np.float32))          # the fp32 NCHW stem
    refn = _conv_ref64(xn.permute(0, 2, 3, 1), w, sc, sh, 0.01, 2, dims=2)
    _check(arena, lambda x, w, scale, shift: H.conv2d(x, w, None, scale, shift, stride=2, in_nchw=True), dict(x=xn, w=w, scale=sc, shift=sh),
           lambda y: _assert_rel(y, refn, 2e-5))


@pytest.mark.parametrize("shape", [(5, 29, 15), (1, 1, 1), (2, 15, 31), (3, 200, 500)])      # ragged, one pixel, several bricks per workgroup
def test_resblock2d_and_split2d(arena, shape):
    N, Hh, W = shape
    rng = np.random.default_rng(sum(shape) + 1)
    x = _rand(rng, N, Hh, W, 16)
    w1, w2 = _w3(rng, 16, 16, (3, 3)), _w3(rng, 16, 16, (3, 3))
    (sc1, sh1), (sc2, sh2) = _bn(rng, 16), _bn(rng, 16)

    def ref_of(xq):
        mid = torch.from_numpy(_conv_ref64(xq, w1, sc1, sh1, 0.01, dims=2))
        return _conv_ref64(mid, w2, sc2, sh2, 0.01, res=xq, dims=2)
    # mvsgi_resblock2d_f32 (bf16 split inside)
    ref = ref_of(x)
    _check(arena, lambda x, q1, s1, h1, q2, s2, h2: H.resblock2d(x, q1, s1, h1, q2, s2, h2, 0.01),
           dict(x=x, q1=H.pack_conv2d_weights_bf16x3(w1), s1=sc1, h1=sh1, q2=H.pack_conv2d_weights_bf16x3(w2), s2=sc2, h2=sh2),
           lambda y: _assert_rel(y, ref, 1e-4))
    # the 2-D split-padded format and the kernels on it
    xs = _check(arena, lambda x: Split2d(H.f32_to_split2d(x, out=split2d_out(N, Hh, W))), dict(x=x)).buf
    xq = _check(arena, H.split2d_to_f32, dict(x_split=xs))
    assert float(((xq - x).abs() / x.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
    q1, q2 = H.pack_resblock2d_split_weights(w1, sc1), H.pack_resblock2d_split_weights(w2, sc2)
    refq = ref_of(xq)
    ins = dict(x=xs, q1=q1, h1=sh1, q2=q2, h2=sh2)
    _check(arena, lambda x, q1, h1, q2, h2: H.resblock2d_split(x, q1, h1, q2, h2, 0.01), ins, lambda y: _assert_rel(y, refq, 1e-4))
    ys = _check(arena, lambda x, q1, h1, q2, h2: Split2d(H.resblock2d_split(x, q1, h1, q2, h2, 0.01, out_split=split2d_out(N, Hh, W))), ins)
    assert _rel(H.split2d_to_f32(ys.buf), refq) <= 1e-4
    ho, wo = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
    ref2 = _conv_ref64(xq, w1, sc1, sh1, 0.01, stride=2, dims=2)
    zs = _check(arena, lambda x, q1, h1: Split2d(H.conv2d_s2_split(x, q1, h1, split2d_out(N, ho, wo), 0.01)), dict(x=xs, q1=q1, h1=sh1))
    assert _rel(H.split2d_to_f32(zs.buf), ref2) <= 1e-4


# ------------------------------------------------------------------------------ resize, soft-argmin, layout, instance norm
@pytest.mark.parametrize("shape,size", [((2, 16, 3, 5, 7), (6, 10, 14)), ((1, 64, 4, 4, 10), (3, 3, 10)), ((1, 5, 2, 3, 5), (5, 6, 20)),
                                        ((3, 32, 5, 7, 9), (3, 4, 5))])
def test_resize_trilinear(arena, shape, size):
    rng = np.random.default_rng(9)
    x = _rand(rng, shape[0], *shape[2:], shape[1])
    ref = F.interpolate(x.cpu().permute(0, 4, 1, 2, 3), size=size, mode="trilinear", align_corners=False).permute(0, 2, 3, 4, 1).numpy()
    _check(arena, lambda x: H.resize_trilinear(x, size), dict(x=x), lambda y: _assert_rel(y, ref, 2e-6))


@pytest.mark.parametrize("shape", [(2, 5, 6, 9), (1, 48, 6, 10), (1, 16, 3, 700), (1, 20, 1, 4), (2, 16, 7, 13)])
def test_softargmin(arena, shape):
    """x1 / x2 (mvsgi_softargmin_div_f32) with and without norm_costs; mvsgi_softargmin_scaled_f32: the row-band kernel at 3 and 4,
    the thread-per-pixel kernel at 1.5 and 0.5; W % 4 != 0, odd W, H == 1, D in registers and the multi-pass form."""
    B, D, Hh, W = shape
    rng = np.random.default_rng(sum(shape))
    costs = _rand(rng, B, D, Hh, W, s=4.0)
    inv_idx = _g((96.0 / np.geomspace(0.5, 100.0, D)).astype(np.float32))
    for s, variant in ((1, H.SA_AUTO), (2, H.SA_AUTO), (3, H.SA_BAND), (4, H.SA_BAND), (4, H.SA_PIXEL), (1.5, H.SA_AUTO), (0.5, H.SA_AUTO)):
        if int(Hh * s) < 1 or int(W * s) < 1:
            continue
        up = F.interpolate(costs.cpu(), scale_factor=s, mode="bilinear") if s != 1 else costs.cpu()
        ref_pr = F.softmax(up.double(), 1)
        ref_inv = (ref_pr * inv_idx.cpu().double().view(1, -1, 1, 1)).sum(1, keepdim=True)

        def ref(out):
            inv, pr = out if isinstance(out, tuple) else (out, None)
            assert _rel(inv, ref_inv) <= 1e-5
            if pr is not None:
                assert _rel(pr, ref_pr) <= 1e-5
        inv, _ = _check(arena, lambda costs, inv_idx: H.softargmin(costs, inv_idx, s, True, variant=variant), dict(costs=costs, inv_idx=inv_idx), ref)
        only = _check(arena, lambda costs, inv_idx: H.softargmin(costs, inv_idx, s, False, variant=variant)[0], dict(costs=costs, inv_idx=inv_idx), ref)
        assert torch.equal(only, inv)


def test_layout(arena):
    rng = np.random.default_rng(4)
    for shape in ((2, 24, 3, 5, 70), (3, 5, 1, 7, 9), (1, 16, 2, 2, 1)):
        x = _rand(rng, *shape)
        y = _check(arena, H.ncdhw_to_ndhwc, dict(x=x), lambda y: _assert_equal(y, x.permute(0, 2, 3, 4, 1).contiguous()))
        _check(arena, H.ndhwc_to_ncdhw, dict(x=y.clone()), lambda z: _assert_equal(z, x))


@pytest.mark.parametrize("C,S", [(16, 7), (48, 1001), (32, 25600), (384, 3), (96, 5 * 9 * 33)])
def test_instance_norm(arena, C, S):
    """mvsgi_instance_norm_f32, workspace at exactly mvsgi_instance_norm_ws_bytes (hip_ops allocates max(that, 16) bytes; under
    the fixture that allocation is guarded); out of place and in place (y == x: the one entry that may write an input)."""
    g = torch.Generator().manual_seed(C * 7919 + S)
    B = 3
    x = (torch.randn(B, S, C, generator=g) * 2.0 + 0.5).to(DEV)
    res, gamma, beta = torch.randn(B, S, C, generator=g).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    assert _lib.load().mvsgi_instance_norm_ws_bytes(B, S, C) > 0
    xd = x.double().cpu().permute(0, 2, 1)
    y64 = F.instance_norm(xd, weight=gamma.double().cpu(), bias=beta.double().cpu(), eps=1e-5).permute(0, 2, 1) + res.double().cpu()
    ref = torch.where(y64 > 0, y64, y64 * 0.01)

    def close(y):
        assert float((y.double().cpu() - ref).abs().max()) <= 1e-5
    _check(arena, lambda x, res, gamma, beta: H.instance_norm(x, res, gamma, beta, eps=1e-5, neg_slope=0.01), dict(x=x, res=res, gamma=gamma, beta=beta), close)

    def in_place(x, res, gamma, beta):
        xx = torch.empty_like(x)            # the caller's own buffer: guarded under the fixture, plain in the plain twin
        xx.copy_(x)
        y = H.instance_norm(xx, res, gamma, beta, eps=1e-5, neg_slope=0.01, out=xx)
        assert y.data_ptr() == xx.data_ptr()
        return y
    _check(arena, in_place, dict(x=x, res=res, gamma=gamma, beta=beta), close)


# ------------------------------------------------------------------------------ second tier: grid generators, deform_conv2d
def test_grid_generators(arena, golden_dir):
    """rays_panorama, transform_points, grid_double_sphere, grid_equirect on guarded inputs: at the goldens' shapes against the
    reference's outputs (the bars of test_sweep_grid_generator_vs_reference_goldens), and at a shape odd in every axis (5
    candidates, 7 x 13, two poses) against float64 where a closed form is at hand (R p + t), bit-equal to the plain call everywhere.
    (Element for element: tests/test_gpu_grids_exact.py.)"""
    import os
    from mvs_gi_amd.dropin import sweep_grids as SG
    z = np.load(os.path.join(golden_dir, "sweep_grids.npz"))

    def rays_of(dist, lon, lat, shape):
        rm = SG.RayMaker_UEPanorama(np.zeros(1, np.float32), lon, lat, device=DEV)
        rm.dist = dist
        return rm.make_rays_for_candidates(shape)
    ds, eq = SG.DoubleSphereSampleGridMaker(), SG.EquirectangularSampleGridMaker()
    name = "g16"
    shape = tuple(int(v) for v in z[name + "_shape"])
    lon, lat = tuple(z[name + "_lon"]), tuple(z[name + "_lat"])
    ref_rays = z[name + "_rays"]
    _check(arena, lambda dist: rays_of(dist, lon, lat, shape), dict(dist=_g(z[name + "_dist"].astype(np.float32))), lambda r: _assert_rel(r, ref_rays, 2e-6))
    for i, pose in enumerate(z[name + "_poses"]):
        inv = torch.linalg.inv(torch.from_numpy(pose)).to(torch.float32)
        ref_pts = z[f"{name}_pts{i}"]
        _check(arena, SG.transform_3D_points_torch, dict(T=inv.unsqueeze(0).to(DEV), points=_g(ref_rays).unsqueeze(0)),
               lambda p: _assert_rel(p, ref_pts, 2e-6))
        x, y, zz = ref_pts[:, 0], ref_pts[:, 1], ref_pts[:, 2]
        g, m = _check(arena, ds.make_grid, dict(points=_g(ref_pts)))
        rg, rm_ = z[f"{name}_ds_grid{i}"], z[f"{name}_ds_mask{i}"]
        d1 = np.sqrt(x * x + y * y + zz * zz)
        edge = np.abs(zz + ds.w2 * d1) < 1e-5 * d1
        assert np.array_equal(m.cpu().numpy()[~edge], rm_[~edge])
        well = rm_ & (np.abs(rg).max(-1) < 4)
        assert well.sum() > 100 and np.abs(g.cpu().numpy() - rg)[well].max() <= 2e-5
        e = _check(arena, eq.make_grid, dict(points=_g(ref_pts))).cpu().numpy()
        cut = (x < 0) & (np.abs(zz) < 1e-4 * np.abs(x))
        assert np.abs(e - z[f"{name}_eq_grid{i}"])[~cut].max() <= 2e-6
    # odd in every axis
    rng = np.random.default_rng(5)
    rays = _check(arena, lambda dist: rays_of(dist, lon, lat, (7, 13)), dict(dist=_g(np.geomspace(0.5, 50.0, 5).astype(np.float32))))
    assert tuple(rays.shape) == (3, 5, 7, 13)
    T = torch.eye(4).repeat(2, 1, 1)
    T[:, :3, :3] = torch.linalg.qr(torch.from_numpy(rng.standard_normal((2, 3, 3)).astype(np.float32)))[0]
    T[:, :3, 3] = torch.from_numpy(rng.standard_normal((2, 3)).astype(np.float32))
    pts_in = rays.unsqueeze(0).repeat(2, 1, 1, 1, 1)
    ref = torch.einsum("bij,bjnhw->binhw", T[:, :3, :3].double(), pts_in.cpu().double()) + T[:, :3, 3].double().view(2, 3, 1, 1, 1)
    pts = _check(arena, SG.transform_3D_points_torch, dict(T=T.to(DEV), points=pts_in), lambda p: _assert_rel(p, ref, 2e-6))
    _check(arena, ds.make_grid, dict(points=pts))
    _check(arena, eq.make_grid, dict(points=pts))


@pytest.mark.parametrize("case", [
    # (N, Cin, Cout, H, W, k, stride, pad, dil, res, slope): from test_deform_conv2d_vs_oracle
    (2, 16, 16, 11, 39, 3, 1, 1, 1, True, 0.01),       # quad-lane kernel, odd sizes
    (1, 16, 16, 9, 21, 5, 2, 2, 1, False, 1.0),        # 5x5 stride 2, ragged pixel count
    (3, 8, 12, 7, 11, 3, 1, 1, 1, True, 0.01),         # generic kernel (other channel counts)
])
def test_deform_conv2d(arena, case):
    """mvsgi_deform_conv2d_f32: per-image and shared offsets; sub-pixel, a few pixels, far outside the image (-50, 1e4), exactly on
    the borders."""
    N, Cin, Cout, Hh, W, k, st, pad, dil, res, slope = case
    rng = np.random.default_rng(sum(case[:9]))
    x = rng.standard_normal((N, Cin, Hh, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(k * k * Cin)).astype(np.float32)
    sc, sh = _bn(rng, Cout)
    Ho = (Hh + 2 * pad - (dil * (k - 1) + 1)) // st + 1
    Wo = (W + 2 * pad - (dil * (k - 1) + 1)) // st + 1
    off = rng.normal(0, 1.5, (N, 2 * k * k, Ho, Wo)).astype(np.float32)
    off[:, :, 0, :] = np.round(off[:, :, 0, :])
    off[:, 0, 1, :] = -50.0
    off[:, 3, 2 % Ho, :] = 1e4
    r = rng.standard_normal((N, Cout, Ho, Wo)).astype(np.float32) if res else None

    def ref_of(o):
        y = O.deform_conv2d(torch.from_numpy(x), torch.from_numpy(o), torch.from_numpy(w), None, (st, st), (pad, pad), (dil, dil))
        y = y * sc.cpu().view(1, -1, 1, 1) + sh.cpu().view(1, -1, 1, 1)
        if res:
            y = y + torch.from_numpy(r)
        return torch.where(y > 0, y, y * slope).permute(0, 2, 3, 1).numpy()
    wp = H.pack_deform_conv2d_weights(_g(w))
    xg = _g(x).permute(0, 2, 3, 1).contiguous()
    fn = lambda x, offset, wp, scale, shift, res=None: H.deform_conv2d(x, offset, wp, scale, shift, (k, k), (st, st), (pad, pad), (dil, dil),
                                                                       res=res, neg_slope=slope)
    for o in (off, np.repeat(off[:1], N, 0), off[:1]):          # per image; the same field per image; ONE shared field
        ins = dict(x=xg, offset=_g(o), wp=wp, scale=sc, shift=sh)
        if res:
            ins["res"] = _g(r).permute(0, 2, 3, 1).contiguous()
        ref = ref_of(o if o.shape[0] == N else np.repeat(o, N, 0))
        _check(arena, fn, ins, lambda y: _assert_rel(y, ref, 2e-5))


# ------------------------------------------------------------------------------ 5. rejection leaves memory alone
def test_rejections_leave_memory_alone(arena):
    """The documented refusals return non-zero and enqueue nothing: the output arena is sentinel in every byte afterwards."""
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1)

    def untouched(t):
        torch.cuda.synchronize()
        e = arena.entry_of(t)
        return bool((e.arena == SENTINEL).all())

    def refused(rc, *needles):
        msg = lib.mvsgi_last_error().decode()
        assert rc != 0 and all(n in msg for n in needles), (rc, msg)
    # soft-argmin at a wrong OH / OW, a non-integer factor on the row-band kernel, bad factors
    B, D, Hh, W = 1, 8, 4, 6
    c, inv_idx = arena.guarded(_rand(rng, B, D, Hh, W)), arena.guarded(torch.ones(D, device=DEV))
    inv, pr = torch.empty((B, 1, 4 * Hh, 4 * W), device=DEV), torch.empty((B, D, 4 * Hh, 4 * W), device=DEV)

    def sa(scale, OH, OW, variant=H.SA_AUTO):
        return lib.mvsgi_softargmin_scaled_f32(c.data_ptr(), inv_idx.data_ptr(), inv.data_ptr(), pr.data_ptr(), B, D, Hh, W, scale, OH, OW, 1.0, variant, st)
    refused(sa(4.0, 16, 23), "16 x 23", "16 x 24")
    refused(sa(2.5, 10, 15, H.SA_BAND), "2.5")
    refused(sa(float("nan"), 16, 24), "nan")
    refused(sa(0.0, 16, 24), "scale 0")
    refused(sa(4.0, 16, 24, 7), "variant 7")
    assert untouched(inv) and untouched(pr)
    # a Winograd call on a refused geometry (D == 4)
    x4 = H.act_to_split(torch.ones((1, 4, 4, 32, 32), device=DEV), fmt="f16")
    wp, un = H.pack_conv_weights_wino(_w3(rng, 32, 32))
    y = torch.empty((1, 4, 4, 32, 32), device=DEV)
    refused(lib.mvsgi_conv3d_wino32_f16(x4.buf.data_ptr(), wp.data_ptr(), un.data_ptr(), un.data_ptr(), None, y.data_ptr(), 1, 0, 1, 4, 4, 32, 0.01, st),
            "needs D == 8")
    assert untouched(y)
    # MVSGI_CONV_F16 on an exact path
    x = _rand(rng, 1, 4, 6, 16, 16)
    w = _w3(rng, 16, 16)
    one = torch.ones(16, device=DEV)
    y2 = torch.empty((1, 4, 6, 16, 16), device=DEV)
    refused(lib.mvsgi_conv3d_f32(x.data_ptr(), w.data_ptr(), H.pack_conv_weights(w).data_ptr(), one.data_ptr(), one.data_ptr(), None, y2.data_ptr(),
                                 1, 16, 4, 6, 16, 16, 1, 0.01, H.CONV_MFMA | H.CONV_F16, st), "MVSGI_CONV_F16")
    assert untouched(y2)
    # the stride-2 kernel's fp32-padded output in the bf16 split
    xs = H.act_to_split(torch.ones((1, 4, 4, 32, 16), device=DEV))
    wps = H.pack_conv_weights_s2rs(_w3(rng, 32, 16), torch.ones(32, device=DEV))
    out = torch.empty((1, 4, 4, 18, 32), device=DEV, dtype=torch.int32)
    refused(lib.mvsgi_conv3d_s2rs_out_fmt(xs.buf.data_ptr(), wps.data_ptr(), torch.zeros(32, device=DEV).data_ptr(), out.data_ptr(), 1, 4, 4, 32,
                                          0.01, 1.0, 0, 1, st), "fp16 split only")
    assert untouched(out)
    # null pointers and bad sizes (tests/test_cabi_symbols.py exercises these without a device)
    y3 = torch.empty((1, 2, 4, 4, 8), device=DEV)
    assert lib.mvsgi_resize_trilinear_f32(None, y3.data_ptr(), 1, 8, 1, 2, 2, 2, 4, 4, st) != 0
    assert lib.mvsgi_resize_trilinear_f32(x.data_ptr(), y3.data_ptr(), 1, 8, 0, 2, 2, 2, 4, 4, st) != 0
    assert lib.mvsgi_ncv_to_nvc_f32(None, y3.data_ptr(), 1, 8, 32, st) != 0
    assert untouched(y3)


# ------------------------------------------------------------------------------ 6. the whole path
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x3"])
@pytest.mark.parametrize("name", ["std_d10_odd", "cat_d8"])
def test_whole_path_guarded(arena, golden_dir, name, mode):
    """SMALL_CASES through HotPath, eager, twice in a row (the second call reuses the module-owned split buffers), every library
    allocation and every input between guards, against the reference golden at the bars of test_small_cases_vs_reference_goldens."""
    import os
    case = SMALL_CASES[name]
    cfg = case["cfg"]
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    gain = case["gains"][0]
    w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
    H.set_conv_mode(mode)
    hp = HotPath(cfg, w, inp, device=DEV)
    feats = arena.guarded(_g(inp["feats"]))
    snap = arena.snapshot(feats)
    ref = z[f"inv_dist_g{gain:g}"]
    outs = []
    for _ in range(2):
        inv, _costs = hp(feats)
        assert bool(torch.isfinite(inv).all())
        err = _rel(inv, ref)
        assert err <= 1e-3, err                  # the north-star bar
        if mode == "f32":
            assert err <= 2e-4, err              # what the exact-fp32 path delivers
        outs.append(inv.clone())
    assert torch.equal(outs[0], outs[1])
    assert arena.unchanged(feats, snap)
    torch.cuda.synchronize()
    H.check_range("whole path")


@pytest.mark.parametrize("name", ["std_d8", "cat_d8"])
def test_graph_held_rig_constants_survive_another_batch_size(arena, name):
    """A captured hipGraph holds the addresses of the rig's validity byte (std builder) or of the replicated rig constants (concat
    builder), which an eager call at another batch size replaces in their caches: they must stay allocated for the replay.  (Found by
    the guarded allocator: torch's own allocator happened to leave the freed block alone.)"""
    import weakref
    from mvs_gi_amd.dropin import cost_volume_builder as cb
    case = SMALL_CASES[name]
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=7, batch=1)
    H.set_conv_mode("bf16x3")
    hp = HotPath(cfg, synth.make_weights(cfg, seed=7), inp, device=DEV)
    rng = np.random.default_rng(2)
    f2 = _g(rng.standard_normal((2, *inp["feats"].shape[1:]), dtype=np.float32))
    f3 = _g(rng.standard_normal((3, *inp["feats"].shape[1:]), dtype=np.float32))
    e2 = hp(f2)[0].clone()
    hp.capture(f2)
    if cfg.builder == "std":
        held = weakref.ref(cb._RIG_VALIDITY[hp.cv_builder][2])
    else:
        held = weakref.ref(hp._rig_views[1])
    assert torch.equal(hp.replay(f2)[0], e2)
    hp(f3)                                              # another batch size, eagerly: replaces the cache entries
    gc.collect()
    assert held() is not None, "a tensor the graph reads was freed"
    junk = [torch.full((1 << 20,), 7, device=DEV, dtype=torch.int32) for _ in range(8)]      # would land in freed blocks
    assert torch.equal(hp.replay(f2)[0], e2)
    del junk


# ------------------------------------------------------------------------------ C. frame bases beyond 2^31 elements
def _frames(t, n_frames):
    """first, second to last and last frame."""
    return [0, n_frames - 2, n_frames - 1]


def _big_randn(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, device=DEV, generator=g)


def _b_for(frame_elems):
    """The smallest B for which B * frame_elems exceeds 2^31 elements by at least two frames."""
    return (1 << 31) // frame_elems + 3


def _report_peak(tag):
    print(f"[large-offset] {tag}: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


@pytest.fixture
def big():
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def test_large_offsets_layout(arena, big):
    """ncv_to_nvc / nvc_to_ncv with B * C * V beyond 2^31 elements: first and last two frames bit-exact."""
    C, V = 16, 4 * 20 * 80                     # (the launcher's own limit is B < 65536: a level-1 frame)
    B = _b_for(C * V)
    assert B < 65536
    x = _big_randn((B, C, 4, 20, 80), 1)
    y = H.ncdhw_to_ndhwc(x)
    for b in _frames(x, B):
        assert torch.equal(y[b], x[b].permute(1, 2, 3, 0))
    z = H.ndhwc_to_ncdhw(y)
    del x
    for b in _frames(y, B):
        assert torch.equal(z[b], y[b].permute(3, 0, 1, 2))
    assert z.numel() >= (1 << 31) + 2 * C * V
    _report_peak(f"layout B={B}")


def test_large_offsets_split_format(arena, big):
    """act_f32_to_split_fmt / back: the split-padded side ([B][D+2][H+2][W+2][C] words) beyond 2^31 elements."""
    D, Hh, W, C = 2, 10, 40, 32
    B = _b_for((D + 2) * (Hh + 2) * (W + 2) * C)
    x = _big_randn((B, D, Hh, W, C), 2)
    for fmt in ("f16", "bf16"):
        s = H.act_to_split(x, fmt=fmt)
        assert s.buf.numel() > (1 << 31)
        back = H.act_from_split(s)
        for b in _frames(x, B):
            one = H.act_to_split(x[b:b + 1].clone(), fmt=fmt)
            assert torch.equal(s.buf[b], one.buf[0])
            assert torch.equal(back[b], H.act_from_split(one)[0])
            if fmt == "bf16":
                assert float(((back[b] - x[b]).abs() / x[b].abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
            else:
                assert float((back[b] - x[b]).abs().max()) <= 2.0 ** -21 * float(x[b].abs().max())
        del s, back
    _report_peak(f"split format B={B}")


def test_large_offsets_resize(arena, big):
    """resize_trilinear: B * Do < 65536 is the launcher's own limit, so the frame is a level-1 volume; output beyond 2^31 elements."""
    C, Di, Hi, Wi = 32, 2, 10, 40
    Do, Ho, Wo = 4, 20, 80
    B = _b_for(C * Do * Ho * Wo)
    assert B * Do < 65536
    x = _big_randn((B, Di, Hi, Wi, C), 3)
    y = H.resize_trilinear(x, (Do, Ho, Wo))
    assert y.numel() > (1 << 31)
    for b in _frames(x, B):
        ref = F.interpolate(x[b:b + 1].cpu().permute(0, 4, 1, 2, 3), size=(Do, Ho, Wo), mode="trilinear", align_corners=False).permute(0, 2, 3, 4, 1)
        assert _rel(y[b:b + 1], ref) <= 2e-6
    _report_peak(f"resize B={B}")


def test_large_offsets_instance_norm(arena, big):
    """instance_norm_f32: B < 65536 is the launcher's own limit; [B][S][C] beyond 2^31 elements, in place (one 8 GiB tensor)."""
    C, S = 64, 4 * 20 * 80
    B = _b_for(C * S)
    assert B < 65536
    x = _big_randn((B, S, C), 4)
    keep = {b: x[b:b + 1].clone() for b in _frames(x, B)}
    y = H.instance_norm(x, eps=1e-5, neg_slope=0.01, out=x)
    for b, xb in keep.items():
        y64 = F.instance_norm(xb.double().cpu().permute(0, 2, 1), eps=1e-5).permute(0, 2, 1)
        ref = torch.where(y64 > 0, y64, y64 * 0.01)
        assert float((y[b:b + 1].double().cpu() - ref).abs().max()) <= 1e-5
    _report_peak(f"instance norm B={B}")


def test_large_offsets_softargmin(arena, big):
    """softargmin_div_f32 (x2 with norm_costs) and softargmin_scaled_f32 (x4 with norm_costs): norm_costs beyond 2^31 elements."""
    D, Hh, W = 16, 10, 40
    inv_idx = _g((96.0 / np.geomspace(0.5, 100.0, D)).astype(np.float32))
    for s in (2, 4):
        B = _b_for(D * Hh * s * W * s)
        c = _big_randn((B, D, Hh, W), 5) * 4
        inv, pr = H.softargmin(c, inv_idx, s, True)
        assert pr.numel() > (1 << 31)
        for b in _frames(c, B):
            up = F.interpolate(c[b:b + 1].cpu(), scale_factor=s, mode="bilinear")
            ref_pr = F.softmax(up.double(), 1)
            ref_inv = (ref_pr * inv_idx.cpu().double().view(1, -1, 1, 1)).sum(1, keepdim=True)
            assert _rel(inv[b:b + 1], ref_inv) <= 1e-5 and _rel(pr[b:b + 1], ref_pr) <= 1e-5
        del c, inv, pr
        _report_peak(f"softargmin x{s} B={B}")


def _run_or_refused(run, B, what):
    """run(B); where the launcher refuses the size (MVSGI_REQUIRE) the refusal and its message are asserted and the largest
    accepted batch (by halving) is run instead -> the batch that ran."""
    nb = B
    while True:
        try:
            run(nb)
            if nb != B:
                print(f"[large-offset] {what}: largest batch tried and accepted {nb}")
            return nb
        except RuntimeError as e:
            msg = str(e)
            assert msg.startswith("mvsgi_") and ("<" in msg or "31" in msg or "large" in msg or "limit" in msg), msg
            print(f"[large-offset] {what}: B={nb} refused: {msg}")
            assert nb > 1, "no batch accepted"
            nb //= 2
            gc.collect()
            torch.cuda.empty_cache()


def _split_frame(s, b):
    t = H.SplitAct(1, s.D, s.H, s.W, s.C, DEV, buf=s.buf[b:b + 1])
    t.fmt = s.fmt
    return t


@pytest.mark.parametrize("impl", ["MFMA", "BF16X3", "F16"])
def test_large_offsets_conv3d(arena, big, impl):
    """mvsgi_conv3d_f32 with x, res and y beyond 2^31 elements each ([B][2][10][40][64]): first and last two frames against float64."""
    Cin = Cout = 64
    D, Hh, W = 2, 10, 40
    B = _b_for(D * Hh * W * Cout)
    rng = np.random.default_rng(6)
    w = _w3(rng, Cout, Cin, s=0.01 if impl == "F16" else 1.0)
    sc, sh = _bn(rng, Cout)
    code = {"MFMA": H.CONV_MFMA, "BF16X3": H.CONV_BF16X3, "F16": H.CONV_BF16X3 | H.CONV_F16}[impl]
    tol = {"MFMA": 2e-5, "BF16X3": 1e-4, "F16": 5e-6}[impl]
    scale = sc
    if impl == "MFMA":
        wp = H.pack_conv_weights(w)
    elif impl == "BF16X3":
        wp = H.pack_conv_weights_bf16x3(w)
    else:
        wp, un = H.pack_conv_weights_f16x3(w)
        scale = sc * un

    def run(nb):
        x, r = _big_randn((nb, D, Hh, W, Cin), 7), _big_randn((nb, D, Hh, W, Cout), 8)
        y = H.conv3d(x, w, wp, scale, sh, res=r, neg_slope=0.01, impl=code)
        assert nb != B or y.numel() > (1 << 31)
        for b in _frames(x, nb):
            err = _rel(y[b:b + 1], _conv_ref64(x[b:b + 1], w, sc, sh, 0.01, res=r[b:b + 1]))
            assert err <= tol, (b, err)
    _run_or_refused(run, B, f"conv3d {impl}")
    _report_peak(f"conv3d {impl} B={B}")


def test_large_offsets_conv3d_up2(arena, big):
    """mvsgi_conv3d_up2_f32: [B][1][5][20][64] -> [B][2][10][40][32] beyond 2^31 output elements."""
    Cin, Cout, Dl, Hl, Wl = 64, 32, 1, 5, 20
    B = _b_for(8 * Dl * Hl * Wl * Cout)
    rng = np.random.default_rng(8)
    w = _w3(rng, Cout, Cin)
    sc, sh = _bn(rng, Cout)
    wp = H.pack_conv_weights_bf16x3(w)

    def run(nb):
        x = _big_randn((nb, Dl, Hl, Wl, Cin), 9)
        y = H.conv3d_up2(x, wp, sc, sh, neg_slope=0.01)
        assert nb != B or y.numel() > (1 << 31)
        for b in _frames(x, nb):
            err = _rel(y[b:b + 1], _conv_ref64(x[b:b + 1], w, sc, sh, 0.01, up2=True))
            assert err <= 1e-4, (b, err)
    _run_or_refused(run, B, "conv3d_up2")
    _report_peak(f"conv3d_up2 B={B}")


def _big_split(shape, seed, fmt):
    """A split-padded volume filled from a seeded fp32 tensor that is freed again -> SplitAct."""
    x = _big_randn(shape, seed)
    s = H.act_to_split(x, fmt=fmt)
    del x
    return s


def test_large_offsets_conv3d_rs(arena, big):
    """mvsgi_conv3d_rs_split_fmt: split-padded input and output [B][4][12][42][32] words beyond 2^31 elements each."""
    D, Hh, W = 2, 10, 40
    B = _b_for((D + 2) * (Hh + 2) * (W + 2) * 32)
    rng = np.random.default_rng(10)
    w = _w3(rng, 32, 32, s=0.02)
    sc, sh = _bn(rng, 32)
    wp, un = H.pack_conv_weights_rs(w, "f16")

    def run(nb):
        xs = _big_split((nb, D, Hh, W, 32), 11, "f16")
        ys = H.conv3d_rs(xs, wp, sc * un, sh, neg_slope=0.01)
        assert nb != B or ys.buf.numel() > (1 << 31)
        for b in _frames(xs, nb):
            ref = _conv_ref64(H.act_from_split(_split_frame(xs, b)), w, sc, sh, 0.01)
            err = _rel(H.act_from_split(_split_frame(ys, b)), ref)
            assert err <= 5e-6, (b, err)
    _run_or_refused(run, B, "conv3d_rs")
    _report_peak(f"conv3d_rs B={B}")


def test_large_offsets_conv3d_rs16(arena, big):
    """mvsgi_conv3d_rs16_split_fmt, both outputs: split-padded [B][4][12][42][16] words beyond 2^31 elements."""
    D, Hh, W = 2, 10, 40
    B = _b_for((D + 2) * (Hh + 2) * (W + 2) * 16)
    rng = np.random.default_rng(12)
    w = _w3(rng, 16, 16)
    sc, sh = _bn(rng, 16)
    wp = H.pack_conv_weights_rs(w)

    def run(nb):
        xs = _big_split((nb, D, Hh, W, 16), 13, "bf16")
        y = H.conv3d_rs16(xs, wp, sc, sh, neg_slope=0.01)
        ys = H.conv3d_rs16(xs, wp, sc, sh, neg_slope=0.01, out_split=H.SplitAct(nb, D, Hh, W, 16, DEV))
        assert nb != B or ys.buf.numel() > (1 << 31)
        for b in _frames(xs, nb):
            ref = _conv_ref64(H.act_from_split(_split_frame(xs, b)), w, sc, sh, 0.01)
            err = _rel(y[b:b + 1], ref)
            assert err <= 1e-4, (b, err)
            assert torch.equal(ys.buf[b:b + 1], H.act_to_split(y[b:b + 1].clone()).buf)
    _run_or_refused(run, B, "conv3d_rs16")
    _report_peak(f"conv3d_rs16 B={B}")


def test_large_offsets_conv3d_s2rs(arena, big):
    """mvsgi_conv3d_s2rs_fmt: split-padded input [B][6][22][82][16] words beyond 2^31 elements."""
    D, Hh, W = 4, 20, 80
    B = _b_for((D + 2) * (Hh + 2) * (W + 2) * 16)
    rng = np.random.default_rng(14)
    w = _w3(rng, 32, 16)
    sc, sh = _bn(rng, 32)
    wp = H.pack_conv_weights_s2rs(w, sc)

    def run(nb):
        xs = _big_split((nb, D, Hh, W, 16), 15, "bf16")
        assert nb != B or xs.buf.numel() > (1 << 31)
        ys = H.conv3d_s2rs(xs, wp, sh, H.SplitAct(nb, D // 2, Hh // 2, W // 2, 32, DEV), neg_slope=0.01)
        for b in _frames(xs, nb):
            ref = _conv_ref64(H.act_from_split(_split_frame(xs, b)), w, sc, sh, 0.01, stride=2)
            err = _rel(H.act_from_split(_split_frame(ys, b)), ref)
            assert err <= 1e-4, (b, err)
    _run_or_refused(run, B, "conv3d_s2rs")
    _report_peak(f"conv3d_s2rs B={B}")


def test_large_offsets_conv3d_wino(arena, big):
    """mvsgi_conv3d_wino32_f16: split-padded input and output [B][10][4][34][32] words beyond 2^31 elements each."""
    D, Hh, W = 8, 2, 32
    B = _b_for((D + 2) * (Hh + 2) * (W + 2) * 32)
    rng = np.random.default_rng(16)
    w = _w3(rng, 32, 32, s=0.02)
    sc, sh = _bn(rng, 32)
    wp, un = H.pack_conv_weights_wino(w)

    def run(nb):
        xs = _big_split((nb, D, Hh, W, 32), 17, "f16")
        ys = H.conv3d_wino(xs, wp, sc * un, sh, neg_slope=0.01)
        assert nb != B or ys.buf.numel() > (1 << 31)
        for b in _frames(xs, nb):
            ref = _conv_ref64(H.act_from_split(_split_frame(xs, b)), w, sc, sh, 0.01)
            err = _rel(H.act_from_split(_split_frame(ys, b)), ref)
            assert err <= 5e-6, (b, err)
    _run_or_refused(run, B, "conv3d_wino")
    _report_peak(f"conv3d_wino B={B}")


def test_large_offsets_conv3d_up2_poly(arena, big):
    """mvsgi_conv3d_up2_poly_fmt: [B][2][5][20][32] split-padded -> fp32 [B][4][10][40][16] beyond 2^31 elements."""
    d, h, w_ = 2, 5, 20
    B = _b_for(8 * d * h * w_ * 16)
    rng = np.random.default_rng(18)
    w = _w3(rng, 16, 32)
    sc, sh = _bn(rng, 16)
    plan = H.conv3d_up2_poly_plan(w, d, h, w_)

    def run(nb):
        xs = _big_split((nb, d, h, w_, 32), 19, "bf16")
        y = H.conv3d_up2_poly(xs, plan, sc, sh, neg_slope=0.01)
        assert nb != B or y.numel() > (1 << 31)
        for b in _frames(xs, nb):
            ref = _conv_ref64(H.act_from_split(_split_frame(xs, b)), w, sc, sh, 0.01, up2=True)
            err = _rel(y[b:b + 1], ref)
            assert err <= 1e-4, (b, err)
    _run_or_refused(run, B, "conv3d_up2_poly")
    _report_peak(f"conv3d_up2_poly B={B}")


def test_large_offsets_sweep_one_rig(arena, big):
    """sweep_std_nhwc_valid_rig_f32 (vol [B][8][8][32][16] beyond 2^31 elements) and sweep_std_nhwc_valid_split_fmt with one rig
    (split-padded [B][10][10][34][16] words beyond 2^31): first and last two frames bit-exact against the CPU oracle."""
    cfg = PathConfig("rig", 3, "std", 16, 32, DIST_10[:8], feat_hw=(8, 32), mask_hw=(32, 128), cv_hw=(8, 32))
    inp = synth.make_inputs(cfg, seed=20, batch=1, grid_kind="random", grid_mask_dtype="bool")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in inp.items()}
    g, gm, m = (_g(inp[k]) for k in ("grids", "grid_masks", "masks"))
    vm = H.sweep_validity(g, gm, m)

    def want(fb):
        return O.sweep_std_masked(fb.cpu().permute(0, 1, 4, 2, 3).contiguous(), t["grids"], t["grid_masks"], t["masks"]).permute(0, 2, 3, 4, 1).contiguous()

    def run_f32(nb):
        f = _big_randn((nb, 3, 8, 32, 16), 21).permute(0, 1, 4, 2, 3)        # channels-last storage of [B, N, C, Hi, Wi]
        vol = H.sweep_std_valid(f, g, vm)
        assert nb != Bv or vol.numel() > (1 << 31)
        for b in _frames(f, nb):
            assert torch.equal(vol[b:b + 1].cpu(), want(f[b:b + 1].permute(0, 1, 3, 4, 2)))
    Bv = _b_for(8 * 8 * 32 * 16)
    _run_or_refused(run_f32, Bv, "sweep one rig")
    _report_peak(f"sweep_std_nhwc_valid_rig B={Bv}")
    gc.collect()
    torch.cuda.empty_cache()

    def run_split(nb):
        f = _big_randn((nb, 3, 8, 32, 16), 22).permute(0, 1, 4, 2, 3)
        vs = H.sweep_std_valid_split(f, g, vm, out=H.SplitAct(nb, 8, 8, 32, 16, DEV), fmt="f16")
        assert nb != Bs or vs.buf.numel() > (1 << 31)
        for b in _frames(f, nb):
            vol = want(f[b:b + 1].permute(0, 1, 3, 4, 2)).to(DEV)
            assert torch.equal(vs.buf[b:b + 1], H.act_to_split(vol, fmt="f16").buf)
    Bs = _b_for(10 * 10 * 34 * 16)
    _run_or_refused(run_split, Bs, "sweep one rig, split output")
    _report_peak(f"sweep_std_nhwc_valid_split B={Bs}")


def test_large_offsets_grid_generators(arena, big):
    """transform_points and grid_double_sphere with 3 B M (points) and 2 B M (grid) beyond 2^31 elements, a different transform
    per batch element: the first and the last window of 4096 points bit for bit against the host emulation
    (tests/grid_exact_cases.py).  rays_panorama with 3 N H W beyond 2^31 (the z plane starts at 2 N H W): the first and the last
    4096 elements of every plane within the per-element bounds of the float64 closed form.  Nothing between the windows is
    read back."""
    import grid_exact_cases as GC
    from mvs_gi_amd.dropin import sweep_grids as SG
    WIN = 4096
    M = (1 << 20) + 77                                       # points per batch element: odd, no multiple of the 256-thread block
    B = _b_for(2 * M)
    assert 2 * B * M >= (1 << 31) + 2 * WIN
    p = _big_randn((B, 3, 1, 1, M), 30)
    rng = np.random.default_rng(30)
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, :3, :3] = np.linalg.qr(rng.standard_normal((B, 3, 3)))[0].astype(np.float32)
    T[:, :3, 3] = rng.standard_normal((B, 3)).astype(np.float32)
    windows = [(0, slice(0, WIN)), (B - 1, slice(M - WIN, M))]
    q = SG.transform_3D_points_torch(_g(T), p)
    for b, sl in windows:
        got = q[b:b + 1, :, 0, 0, sl].cpu().numpy()
        want = GC.transform(T[b:b + 1], p[b:b + 1, :, 0, 0, sl].cpu().numpy())
        assert GC.same_bits(got, want), f"transform_points, batch element {b}: {GC.first_difference(got, want)}"
    del p
    _report_peak(f"transform_points B={B} M={M}")
    ds = SG.DoubleSphereSampleGridMaker()
    grid, mask = ds.make_grid(q)
    assert grid.numel() > (1 << 31) and tuple(mask.shape) == (B, 1, 1, M)
    for b, sl in windows:
        want_grid, want_mask = GC.double_sphere(q[b:b + 1, :, 0, 0, sl].cpu().numpy(), *GC.ds_args("default"))
        got_grid, got_mask = grid[b:b + 1, 0, 0, sl].cpu().numpy(), mask[b:b + 1, 0, 0, sl].cpu().numpy()
        assert np.array_equal(got_mask, want_mask), f"grid_double_sphere mask, batch element {b}: {GC.first_difference(got_mask, want_mask)}"
        assert GC.same_bits(got_grid, want_grid), f"grid_double_sphere, batch element {b}: {GC.first_difference(got_grid, want_grid)}"
    del q, grid, mask
    _report_peak(f"grid_double_sphere B={B} M={M}")
    gc.collect()
    torch.cuda.empty_cache()

    Hh, W = 257, 1021
    N = _b_for(3 * Hh * W)
    total = N * Hh * W
    assert 3 * total >= (1 << 31) + WIN and 2 * total < (1 << 31)             # the z plane crosses 2^31
    lat, lon = GC.PANORAMA_RANGES["full_sphere"]
    dist = np.geomspace(0.5, 100.0, N).astype(np.float32)
    rm = SG.RayMaker_UEPanorama(dist, lon, lat, device=DEV)
    rays = rm.make_rays_for_candidates((Hh, W))
    assert rays.numel() == 3 * total
    phi, theta = GC.panorama_args(N, Hh, W, lat, lon)
    flat = rays.view(3, total)
    for idx in (np.arange(WIN), np.arange(total - WIN, total)):
        got = flat[:, int(idx[0]):int(idx[-1]) + 1].cpu().numpy()
        exact = GC.panorama_exact_at(dist, phi, theta, idx)
        units = GC.UNITS_PANORAMA.reshape(3, 1)
        ok, worst = GC.check_bound(got, exact, units)
        print(f"[large-offset] rays_panorama elements {idx[0]}..{idx[-1]} of each plane: worst {worst:.2f} x 2^-23 |exact|")
        assert ok.all(), GC.describe_failures(ok, got, exact, units)
    _report_peak(f"rays_panorama N={N}")
