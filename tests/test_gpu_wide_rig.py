"""GPU (MI355X): the masked-variance sweep for rigs of 5 to 8 cameras on the channels-last fast path
(sweep_std_nhwc_v_kernel<N> with N > 4, csrc/sweep.hip) -- against the reference's own outputs (tests/golden/wide_rig.npz), bit for bit
against the plane-gather kernel sweep_std_kernel<N> (the same arithmetic in the same order: no tolerance), both output formats,
the divisions from subnormal to huge variances, several candidates per block, the range report, the whole path against the CPU
oracle, the drop-in's rig plumbing and the entry checks.  The kernel is one template for 1 to 8 cameras: every instantiation its
launch table can select, and the candidate walk of the rigs up to 4 cameras, are pinned here too."""
import ctypes
import os

import numpy as np
import pytest
import torch

import guard_arena
import wide_rig_cases as W
from mvs_gi_amd import _lib, hip_ops as H, synth
from mvs_gi_amd.pipeline import HotPath, build_modules
from oracle import mvsgi_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def arena(request):
    """Every device tensor the library allocates during a test of this module sits between NaN-sentinel guards, and unwritten
    fp32 outputs read as NaN (tests/guard_arena.py); the tests that call a kernel directly carve their inputs from it too."""
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


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "wide_rig.npz"))


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ncdhw(y_ndhwc):
    return y_ndhwc.permute(0, 4, 1, 2, 3).contiguous().cpu().numpy()


def _flags() -> int:
    torch.cuda.synchronize()
    return H.saturation_flags(clear=True)


class Case:
    """One seeded case on the device, inputs carved from the guarded arena: feats in NCHW planes (f) and channels-last storage
    (f_cl, presented with the NCHW shape), the rig tensors, and the plane-gather kernel's volume [B, D, Ho, Wo, C] (nchw) -- the
    bit-exact sibling -- computed once."""

    def __init__(self, ga, inp, scale=None):
        feats = inp["feats"] if scale is None else (inp["feats"].astype(np.float64) * scale).astype(np.float32)
        self.f = ga.guarded(_g(feats))
        self._cl = ga.guarded(self.f.permute(0, 1, 3, 4, 2).contiguous())
        self.f_cl = self._cl.permute(0, 1, 4, 2, 3)
        self.g, self.gm, self.m = (ga.guarded(_g(inp[k])) for k in ("grids", "grid_masks", "masks"))
        self.nchw = H.sweep_std(self.f, self.g, self.gm, self.m, layout="nchw")
        self.N = feats.shape[1]

    def rig0(self, ga):
        """frame 0's rig for every frame: (grids[:1], the plane-gather volume of all frames through rig 0)"""
        B = self.f.shape[0]
        exp = [t[:1].expand(B, *t.shape[1:]).contiguous() for t in (self.g, self.gm, self.m)]
        return ga.guarded(self.g[:1]), H.sweep_std(self.f, *exp, layout="nchw")


# ------------------------------------------------------------------------------ 4: the validity-byte sweep
@pytest.mark.parametrize("N", W.NS)
def test_sweep_std_valid_wide(arena, z, N):
    """NCHW and channels-last feature storage, bool / float / uint8 grid masks into the validity byte, per-frame rig and one rig
    for both frames: 1e-6 of the maximum and the same zeros against the reference's output (ATen may associate the camera sum
    differently from five addends on), and the bits of the plane-gather kernel."""
    inp = W.small_case(N)
    assert W.digest(inp) == str(z[f"inputs_sha256_{N}"])
    want = z[f"vol_raw_{N}"]
    c = Case(arena, inp)
    ref = _ncdhw(c.nchw)
    print(f"N = {N}: plane-gather kernel vs reference rel {_rel(ref, want):.3e}, {(ref != want).mean():.4f} of the elements differ")
    assert _rel(ref, want) <= 1e-6 and np.array_equal(ref == 0, want == 0) and (ref != want).mean() < 0.05
    for gmask in (c.gm, arena.guarded(c.gm.float()), arena.guarded(c.gm.to(torch.uint8))):
        vm = H.sweep_validity(c.g, gmask, c.m)
        assert vm.dtype == torch.uint8 and int(vm.max()) < (1 << N)
        for ft in (c.f, c.f_cl):
            got = H.sweep_std_valid(ft, c.g, vm)
            assert torch.equal(got, c.nchw)
            got = _ncdhw(got)
            assert _rel(got, want) <= 1e-6 and np.array_equal(got == 0, want == 0) and (got != want).mean() < 0.05
    g1, rig = c.rig0(arena)
    vm1 = arena.guarded(vm[:1])
    for ft in (c.f, c.f_cl):
        assert torch.equal(H.sweep_std_valid(ft, g1, vm1), rig)
    assert torch.equal(rig[0], c.nchw[0]) and not torch.equal(rig[1], c.nchw[1])


# ------------------------------------------------------------------------------ 5: layout="auto"
def test_sweep_std_auto_layout_six_cameras(arena):
    """sweep_std(layout='auto') with 6 cameras and C = 8: validity byte + the wide kernel, the bits of layout='nchw'."""
    c = Case(arena, W.small_case(6))
    assert c.f.shape[2] == 8
    for ft in (c.f, c.f_cl):
        for gmask in (c.gm, c.gm.float()):
            assert torch.equal(H.sweep_std(ft, c.g, gmask, c.m), c.nchw)


# ------------------------------------------------------------------------------ 6: split-padded output
@pytest.mark.parametrize("N", [5, 8])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_sweep_std_valid_split_wide(arena, N, fmt):
    """The split-padded output equals the format conversion of the fp32 volume, zero border included (the buffer is allocated
    zeroed inside guards; the kernel writes the interior only), per-frame rig and one rig."""
    c = Case(arena, W.small_case(N))
    B, _, C, _, _ = c.f.shape
    vm = H.sweep_validity(c.g, c.gm, c.m)
    g1, rig = c.rig0(arena)
    for gg, vv, vol in ((c.g, vm, c.nchw), (g1, arena.guarded(vm[:1]), rig)):
        want = H.act_to_split(vol, fmt=fmt)
        for ft in (c.f, c.f_cl):
            vs = H.sweep_std_valid_split(ft, gg, vv, out=H.SplitAct(B, W.D, W.HO, W.WO, C, DEV), fmt=fmt)
            assert vs.fmt == fmt and torch.equal(vs.buf, want.buf)
        border = want.buf.clone()
        border[:, 1:-1, 1:-1, 1:-1] = 0
        assert int(border.count_nonzero()) == 0 and int(want.buf.count_nonzero()) > 0
    assert _flags() == 0


# ------------------------------------------------------------------------------ 7: the divisions
@pytest.mark.parametrize("N", W.NS)
@pytest.mark.parametrize("scale", [1e-19, 1.0, 2e18])
def test_sweep_wide_divisions_exact_from_subnormal_to_huge(arena, N, scale):
    """The two divisions by the camera count are a reciprocal + two fmas inside [1e-30, 1e30] and the hardware division outside
    (tiny: x / 6 can be an exact tie between subnormals; huge: the residual overflows): the bits of the plane-gather kernel's
    IEEE divisions with variances down in the subnormals (1e-19) and past the switch (2e18 -> ~1e36)."""
    c = Case(arena, W.small_case(N), scale=scale)
    want = c.nchw.cpu().numpy()
    assert not np.isnan(want).any() and (want != 0).any()
    if scale < 1e-15:
        assert (np.abs(want[want != 0]) < 1.2e-38).any()            # some variances really are subnormal
    if scale > 1e15:
        assert want.max() > 1e30
    vm = H.sweep_validity(c.g, c.gm, c.m)
    for ft in (c.f, c.f_cl):
        assert torch.equal(H.sweep_std_valid(ft, c.g, vm), c.nchw)


# ------------------------------------------------------------------------------ 8: several candidates per block
@pytest.mark.parametrize("N", [8, 5])
def test_sweep_wide_walks_several_candidates(arena, N):
    """The launcher gives a block ceil(D / nd) candidates, nd = ceil(8192 / rows) capped at D, rows = ceil(Wo / 64) Ho B: one at
    the small shape.  B = 2, D = 10, Ho = 32, Wo = 2054 -> rows 2112, nd 4, chunks of 3, 3, 3, 1: the ping-pong pair, its odd tail
    and a one-candidate chunk.  (The rig is drawn for one frame and replicated on the device; the two frames' features differ.)"""
    shape = (1, W.HI, W.WI, 10, 32, 2054, W.HM, W.WM)
    inp = W.small_case(N, 16, shape)
    f2 = np.random.default_rng(200 + N).standard_normal(inp["feats"].shape).astype(np.float32)
    inp = dict(inp, feats=np.concatenate([inp["feats"], f2]),
               **{k: np.concatenate([inp[k]] * 2) for k in ("grids", "grid_masks", "masks")})
    c = Case(arena, inp)
    vm = H.sweep_validity(c.g, c.gm, c.m)
    assert int(vm.max()) < (1 << N) and len(torch.unique(vm)) > N
    assert torch.equal(H.sweep_std_valid(c.f_cl, c.g, vm), c.nchw)
    want = H.act_to_split(c.nchw, fmt="f16")
    vs = H.sweep_std_valid_split(c.f_cl, c.g, vm, out=H.SplitAct(2, 10, 32, 2054, 16, DEV), fmt="f16")
    assert torch.equal(vs.buf, want.buf)
    # one rig for both frames (the two frames' rigs are equal here): the same volume
    assert torch.equal(H.sweep_std_valid(c.f_cl, arena.guarded(c.g[:1]), arena.guarded(vm[:1])), c.nchw)
    assert _flags() == 0


@pytest.mark.parametrize("N", [1, 3, 4])
def test_sweep_narrow_walks_several_candidates(arena, N):
    """The same for rigs of up to 4 cameras (one grid point per lane): at the small shapes every block walks exactly one candidate,
    so this is the only test of their walk.  B = 2, D = 10, Ho = 32, Wo = 2054 -> rows 2112, nd 4, chunks of 3, 3, 3, 1: the
    ping-pong pair, its odd tail and a one-candidate chunk; fp32 volume, fp16 split output and one rig for both frames against the
    plane-gather kernel."""
    shape = (1, W.HI, W.WI, 10, 32, 2054, W.HM, W.WM)
    inp = W.small_case(N, 16, shape)
    f2 = np.random.default_rng(200 + N).standard_normal(inp["feats"].shape).astype(np.float32)
    inp = dict(inp, feats=np.concatenate([inp["feats"], f2]),
               **{k: np.concatenate([inp[k]] * 2) for k in ("grids", "grid_masks", "masks")})
    c = Case(arena, inp)
    vm = H.sweep_validity(c.g, c.gm, c.m)
    assert int(vm.max()) < (1 << N) and len(torch.unique(vm)) > N
    assert N == 1 or bool(c.nchw.any())                              # (one camera: fewer than two valid everywhere, all zeros)
    assert torch.equal(H.sweep_std_valid(c.f_cl, c.g, vm), c.nchw)
    want = H.act_to_split(c.nchw, fmt="f16")
    vs = H.sweep_std_valid_split(c.f_cl, c.g, vm, out=H.SplitAct(2, 10, 32, 2054, 16, DEV), fmt="f16")
    assert torch.equal(vs.buf, want.buf)
    assert torch.equal(H.sweep_std_valid(c.f_cl, arena.guarded(c.g[:1]), arena.guarded(vm[:1])), c.nchw)
    assert _flags() == 0


@pytest.mark.parametrize("C", [8, 16, 24])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 8])
def test_sweep_every_walking_instantiation(arena, N, C):
    """Every kernel the launch table of the validity-byte sweep can select, (N, C == 16, split format), at the small shape (Wo 70:
    a full 64-voxel tile and a 6-voxel tail) against the plane-gather kernel, no tolerance.  C = 8 leaves lanes 2 and 3 of a quad
    without channels, C = 24 gives lanes 0 and 1 two channel trips and lanes 2 and 3 one, C = 16 is the one-trip template; for
    C = 16 also both split formats, with per-frame rig and one rig for both frames, and no range flag."""
    c = Case(arena, W.small_case(N, C))
    assert c.f.shape[1:3] == (N, C)
    vm = H.sweep_validity(c.g, c.gm, c.m)
    assert int(vm.max()) < (1 << N)
    assert N == 1 or bool(c.nchw.any())
    for ft in (c.f, c.f_cl):
        assert torch.equal(H.sweep_std_valid(ft, c.g, vm), c.nchw)
    if C == 16:
        g1, rig = c.rig0(arena)
        for fmt in ("bf16", "f16"):
            for gg, vv, vol in ((c.g, vm, c.nchw), (g1, arena.guarded(vm[:1]), rig)):
                want = H.act_to_split(vol, fmt=fmt)
                vs = H.sweep_std_valid_split(c.f_cl, gg, vv, out=H.SplitAct(W.B, W.D, W.HO, W.WO, C, DEV), fmt=fmt)
                assert vs.fmt == fmt and torch.equal(vs.buf, want.buf)
        assert _flags() == 0


# ------------------------------------------------------------------------------ 9: range report
@pytest.mark.parametrize("N", [5, 8])
def test_sweep_wide_reports_a_cost_volume_beyond_fp16(arena, N):
    """Standard-normal features x 300: variances pass 65504 -> the fp16 split clamps and raises SAT_SWEEP, the bf16 split (fp32's
    range) raises nothing; the stored value is the clamped one."""
    inp = W.small_case(N)
    c1 = Case(arena, inp)
    c300 = Case(arena, inp, scale=300.0)
    assert float(c300.nchw.max()) > 65504.0 > float(c1.nchw.max())
    vm = H.sweep_validity(c1.g, c1.gm, c1.m)
    out = lambda: H.SplitAct(W.B, W.D, W.HO, W.WO, 16, DEV)
    for c, fmt, want in ((c1, "f16", 0), (c300, "f16", H.SAT_SWEEP), (c300, "bf16", 0)):
        vs = H.sweep_std_valid_split(c.f_cl, c.g, vm, out(), fmt=fmt)
        assert _flags() == want, (fmt, want)
        assert torch.equal(vs.buf, H.act_to_split(c.nchw, fmt=fmt).buf)
        _flags()                                                    # (the conversion clamps and reports too)
        back = H.act_from_split(vs)
        assert bool(torch.isfinite(back).all()) and (float(back.max()) == 65504.0) == bool(want)


# ------------------------------------------------------------------------------ 10: whole path
_ORACLE = {}


def _whole(N):
    if N not in _ORACLE:
        cfg = W.whole_path_cfg(N)
        inp = synth.make_inputs(cfg, seed=40 + N, batch=1)
        w = synth.make_weights(cfg, seed=40 + N, gain=1.0)
        t = O.to_torch(inp)
        ref = O.hot_path(t["feats"], t["grids"], t["grid_masks"], t["masks"], O.to_torch(w), cfg.builder, cfg.dist_cands, cfg.bf,
                         cfg.interp_scale_factor, cfg.pre_interp).numpy()
        _ORACLE[N] = (cfg, inp, w, ref)
    return _ORACLE[N]


@pytest.mark.parametrize("N", [6, 8])
def test_whole_path_wide_rig_vs_oracle(N, conv_mode):
    """PathConfig(num_cams = 6 / 8, builder 'std') through HotPath against the CPU oracle: 1e-3 on inv_dist, the project's bar.
    In the split modes the front end took the fast path (split-padded vol_raw in the module-owned buffer) and nothing clamped."""
    import parity_log
    cfg, inp, w, ref = _whole(N)
    hp = HotPath(cfg, w, inp, device=DEV)
    got = hp(_g(inp["feats"]))[0].cpu().numpy()
    err = _rel(got, ref)
    l1 = float(np.abs(got - ref).mean() / np.abs(ref).mean())
    parity_log.record(f"wide_rig_{N}cam", conv_mode, 1.0, err, l1, "oracle", float((np.abs(got - ref) / np.abs(ref)).max()))
    assert got.shape == ref.shape and err <= 1e-3, (N, conv_mode, err)
    if conv_mode != "f32":
        assert "_mvsgi_rs_vol" in hp.cv_builder.__dict__
    assert _flags() == 0


# ------------------------------------------------------------------------------ 11: rig plumbing
def test_rig_plumbing_six_cameras():
    """The drop-in with 6 cameras takes the path a 3-camera rig takes: front-end chunks over stride-0 rig views give the bits of
    the unchunked run; cache off gives the cached volume; an in-place edit of the masks is picked up; a captured graph replays
    the eager result."""
    from mvs_gi_amd.dropin import cost_volume_builder as cb
    cfg, inp, w, _ = _whole(6)
    old_chunk = cb._FRONT_CHUNK
    try:
        H.set_conv_mode("bf16x3")
        feats = _g(np.random.default_rng(6).standard_normal((5, *inp["feats"].shape[1:]), dtype=np.float32))
        cb._FRONT_CHUNK = 0
        hp0 = HotPath(cfg, w, inp, device=DEV)
        whole = hp0(feats)[0].clone()
        assert hp0._rig_views[1].stride(0) == 0
        cb._FRONT_CHUNK = 2                       # chunks of 2, 2 and a tail of 1
        hp = HotPath(cfg, w, inp, device=DEV)
        assert torch.equal(hp(feats)[0], whole)
        assert len(hp.cv_builder.__dict__["_mvsgi_rs_vol"]) == 1
        cb._FRONT_CHUNK = old_chunk
        eager = hp(feats)[0].clone()
        assert torch.equal(eager, whole)
        hp.capture(feats)
        assert torch.equal(hp.replay(feats)[0], eager)
        assert hp.cv_builder.__dict__.get("_mvsgi_graph_pins")
    finally:
        cb._FRONT_CHUNK = old_chunk
        H.set_conv_mode("f32")
    cvb, _, _ = build_modules(cfg, w, DEV)
    inp2 = synth.make_inputs(cfg, seed=46, batch=2)
    f, g, gm, m = (_g(inp2[k]) for k in ("feats", "grids", "grid_masks", "masks"))
    with torch.no_grad():
        cached = cvb.sweep(f, g, gm, m).clone()
        assert bool(cached.any()) and torch.equal(cvb.sweep(f, g, gm, m), cached)
        assert torch.equal(cached.permute(0, 2, 3, 4, 1), H.sweep_std(f, g, gm, m, layout="nchw"))
        cvb.cache_rig_constants = False
        assert torch.equal(cvb.sweep(f, g, gm, m), cached)
        cvb.cache_rig_constants = True
        m.zero_()                                 # in-place edit: every camera masked out
        assert not bool(cvb.sweep(f, g, gm, m).any())


# ------------------------------------------------------------------------------ 12: entry checks
def test_entry_checks_name_the_range():
    lib = _lib.load()
    assert lib.mvsgi_sweep_max_cams() == 8 == H.sweep_max_cams()
    p = ctypes.c_void_p(16)
    rc = lib.mvsgi_sweep_std_f32(p, p, p, 0, p, p, 1, 9, 16, 8, 8, 8, 8, 4, 4, 4, None)
    assert rc != 0 and b"num_cams 9 not in [1, 8]" in lib.mvsgi_last_error()
    rc = lib.mvsgi_sweep_std_nhwc_valid_f32(p, p, p, p, 1, 9, 16, 8, 8, 4, 4, 4, None)
    assert rc != 0 and b"num_cams 9 not in [1, 8]" in lib.mvsgi_last_error()
    rc = lib.mvsgi_sweep_std_nhwc_f32(p, p, p, 0, p, p, 1, 5, 16, 8, 8, 8, 8, 4, 4, 4, None)
    assert rc != 0 and b"not in [1, 4]" in lib.mvsgi_last_error()        # the mask-sampling channels-last kernel stays at 4
    f = torch.zeros((1, 9, 16, 8, 8), device=DEV)
    g = torch.zeros((1, 9, 4, 4, 4, 2), device=DEV)
    gm = torch.ones((1, 9, 4, 4, 4, 1), device=DEV, dtype=torch.bool)
    m = torch.ones((1, 9, 1, 8, 8), device=DEV)
    vm = torch.zeros((1, 4, 4, 4), device=DEV, dtype=torch.uint8)
    for call in (lambda: H.sweep_std_valid(f, g, vm), lambda: H.sweep_validity(g, gm, m), lambda: H.sweep_std(f, g, gm, m),
                 lambda: H.sweep_std(f, g, gm, m, layout="nchw"),
                 lambda: H.sweep_std_valid_split(f, g, vm, H.SplitAct(1, 4, 4, 4, 16, DEV))):
        with pytest.raises(AssertionError, match=r"\[1, 8\]|N<=8"):
            call()
