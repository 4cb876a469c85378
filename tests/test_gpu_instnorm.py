"""GPU (MI355X): norm_type='instance' on the HIP path -- the instance-norm kernels (csrc/instnorm.hip) against float64
F.instance_norm on the CPU, the conv blocks with instance norm against CPU float64 restatements, and whole paths against the
instnorm_* goldens made by the reference's own modules (tools/make_instnorm_goldens.py)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from instnorm_cases import EXTRACTOR_CASE, FULL_CASES, SMALL_CASES
import guard_arena
from mvs_gi_amd import dropin, hip_ops as H, synth
from mvs_gi_amd.pipeline import HotPath

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor the library allocates during a test of this module sits between NaN-sentinel guards, and unwritten
    fp32 outputs read as NaN (tests/guard_arena.py: what is guarded, guard sizes, exemptions)."""
    yield from guard_arena.fixture_body(request)
MODES = ["f16x3", "bf16x3", "f32"]


@pytest.fixture(autouse=True)
def _restore_mode():
    old = H.get_conv_mode()
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    H.set_conv_mode(old)
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)


@pytest.fixture(params=MODES)
def conv_mode(request):
    H.set_conv_mode(request.param)
    return request.param


def _rel(a, b):
    a, b = (t.detach().cpu() if isinstance(t, torch.Tensor) else t for t in (a, b))
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _ref_norm(x, res, gamma, beta, eps, slope):
    """float64 F.instance_norm on [B, S, C] channels-last data, + res, LeakyReLU(slope)."""
    xd = x.double().cpu().permute(0, 2, 1)
    y = F.instance_norm(xd, weight=None if gamma is None else gamma.double().cpu(),
                        bias=None if beta is None else beta.double().cpu(), eps=eps).permute(0, 2, 1)
    if res is not None:
        y = y + res.double().cpu()
    return torch.where(y > 0, y, y * slope)


_CS = [16, 32, 48, 64, 96, 128, 192, 384]
_SS = [2, 7, 1000, 16 * 20 * 80, 16 * 80 * 320]


@pytest.mark.parametrize("C", _CS)
@pytest.mark.parametrize("S", _SS)
def test_kernel_vs_float64_instance_norm(C, S):
    if S * C > 16 * 80 * 320 * 16:
        S = 16 * 80 * 320 * 16 // C          # keep the largest case at post_vol's size in bytes
    g = torch.Generator().manual_seed(C * 7919 + S)
    for i, (B, slope, inplace) in enumerate([(1, 0.01, False), (3, 0.0, True), (3, 1.0, False)]):
        x = (torch.randn(B, S, C, generator=g) * 2.0 + 0.5)
        with_res, with_affine = i != 0, i != 1
        res = torch.randn(B, S, C, generator=g) if with_res else None
        gamma = torch.rand(C, generator=g) + 0.5 if with_affine else None
        beta = torch.randn(C, generator=g) * 0.1 if with_affine else None
        xg = x.to(DEV)
        d = lambda t: None if t is None else t.to(DEV)
        y = H.instance_norm(xg, d(res), d(gamma), d(beta), eps=1e-5, neg_slope=slope, out=xg if inplace else None)
        if inplace:
            assert y.data_ptr() == xg.data_ptr()
        ref = _ref_norm(x, res, gamma, beta, 1e-5, slope)
        err = float((y.double().cpu() - ref).abs().max())
        assert err <= 1e-5, (B, slope, inplace, err)


def test_kernel_large_mean_and_constant_channel():
    """mean 1e3 and std 1 over S = 409600 (E[x^2] - E[x]^2 in fp32 loses every digit there); a constant channel (var = 0)
    comes out as beta."""
    B, S, C = 2, 16 * 80 * 320, 16
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, S, C, generator=g) + 1e3
    x[:, :, 3] = 7.25
    beta = torch.randn(C, generator=g)
    y = H.instance_norm(x.to(DEV), beta=beta.to(DEV), eps=1e-5, neg_slope=1.0).cpu()
    ref = _ref_norm(x, None, None, beta, 1e-5, 1.0)
    assert float((y.double() - ref).abs().max()) <= 1e-5
    assert torch.equal(y[:, :, 3], beta[3].expand(B, S))


def test_kernel_frame_independent_of_launch():
    """Frame b of a B = 4 launch is bit-identical to the same frame run alone: the chunking depends on S and C only."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 16 * 20 * 80, 32, generator=g).to(DEV) * 3 + 1
    res = torch.randn_like(x)
    y4 = H.instance_norm(x, res, eps=1e-5, neg_slope=0.01)
    for b in range(4):
        y1 = H.instance_norm(x[b:b + 1].clone(), res[b:b + 1].clone(), eps=1e-5, neg_slope=0.01)
        assert torch.equal(y1, y4[b:b + 1])


def test_spatial_size_one_raises():
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        H.instance_norm(torch.zeros(2, 1, 16, device=DEV))


# ---- blocks -------------------------------------------------------------------------------------------------------------
_BAR = {"f32": 2e-5, "bf16x3": 2e-3, "f16x3": 4e-4}


def _blk_ref(blk, x, res=None):
    """The block's own forward, restated in float64 on the CPU (the reference's conv -> norm -> (+res) -> act)."""
    b = copy.deepcopy(blk).double().cpu()
    return b, x.double().cpu(), None if res is None else res.double().cpu()


def _cpu_base3d(b, x, res=None):
    y = F.conv3d(x, b.conv_layer.weight, b.conv_layer.bias, stride=b.conv_layer.stride, padding=b.conv_layer.padding)
    y = b.norm_layer(y)
    if res is not None:
        y = y + res
    return b.activation(y)


def _mk3d(Cls, *a, affine=False, running=False, **k):
    norm = nn.InstanceNorm3d(k.pop("nchs"), affine=affine, track_running_stats=running)
    m = Cls(*a, activation=nn.LeakyReLU(), norm_layer=norm, **k)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.InstanceNorm3d):
                if mod.affine:
                    mod.weight.uniform_(0.5, 1.5)
                    mod.bias.normal_(0, 0.1)
                if mod.track_running_stats:
                    mod.running_mean.normal_(0, 0.1)
                    mod.running_var.uniform_(0.5, 1.5)
    return m


@pytest.mark.parametrize("affine", [False, True])
def test_conv_blocks_3d_with_instance_norm(conv_mode, affine):
    torch.manual_seed(3)
    bar = _BAR[conv_mode]
    x = torch.randn(2, 32, 6, 10, 20)
    # BaseConvBlk3d, stride 1 and 2, with a residual
    for stride in (1, 2):
        blk = _mk3d(dropin.BaseConvBlk3d, 32, 32, 3, stride=stride, nchs=32, affine=affine).eval()
        b, xd, _ = _blk_ref(blk, x)
        ref = _cpu_base3d(b, xd)
        res = torch.randn(ref.shape)
        ref_r = _cpu_base3d(b, xd, res.double())
        dev = blk.to(DEV)
        assert _rel(dev(x.to(DEV)).cpu(), ref) <= bar
        assert _rel(dev(x.to(DEV), res.to(DEV)).cpu(), ref_r) <= bar
    # ResConvBlk3d
    rb = _mk3d(dropin.ResConvBlk3d, 32, 32, 3, nchs=32, affine=affine).eval()
    b, xd, _ = _blk_ref(rb, x)
    ref = _cpu_base3d(b.blk2, _cpu_base3d(b.blk1, xd), xd)
    assert _rel(rb.to(DEV)(x.to(DEV)).cpu(), ref) <= bar
    # UNetDownBlk (16 -> 32, stride 2, two residual blocks): level 0 of the (16, 32) regulator
    db = _mk3d(dropin.UNetDownBlk, 16, 32, 3, 3, nchs=32, affine=affine).eval()
    b, xd, _ = _blk_ref(db, torch.randn(2, 16, 8, 16, 32))
    xin = xd.float()
    ref = _cpu_base3d(b.first, xd)
    for r in b.blks:
        ref = _cpu_base3d(r.blk2, _cpu_base3d(r.blk1, ref), ref)
    assert _rel(db.to(DEV)(xin.to(DEV)).cpu(), ref) <= bar
    # ResizeConv3d x2 with a skip, and with odd sizes (second resize to the skip's size)
    for lo, skip_sz in (((4, 5, 10), (8, 10, 20)), ((3, 3, 5), (5, 6, 10))):
        rc = _mk3d(dropin.ResizeConv3d, 32, 16, 3, stride=2, nchs=16, affine=affine).eval()
        b, xd, _ = _blk_ref(rc, torch.randn(2, 32, *lo))
        skip = torch.randn(2, 16, *skip_sz).double()
        up = F.interpolate(xd, size=[2 * s for s in lo], mode="trilinear", align_corners=False)
        if tuple(up.shape[2:]) != skip_sz:
            up = F.interpolate(up, size=skip_sz, mode="trilinear", align_corners=False)
        ref = _cpu_base3d(b.conv, up, skip)
        got = rc.to(DEV)(xd.float().to(DEV), skip.float().to(DEV)).cpu()
        assert _rel(got, ref) <= bar


def test_instance_norm_running_stats_folds_like_batch_norm():
    """track_running_stats=True in eval mode: the running statistics (the batch-norm fold, no norm launch); in train mode the
    'call model.eval()' error of batch norm."""
    torch.manual_seed(4)
    H.set_conv_mode("f32")
    blk = _mk3d(dropin.BaseConvBlk3d, 16, 32, 3, nchs=32, affine=True, running=True).eval()
    bn = dropin.BaseConvBlk3d(16, 32, 3, activation=nn.LeakyReLU(), norm_layer=nn.BatchNorm3d(32)).eval()
    bn.load_state_dict(blk.state_dict(), strict=False)
    for k in ("weight", "bias", "running_mean", "running_var"):
        getattr(bn.norm_layer, k).data.copy_(getattr(blk.norm_layer, k).data)
    x = torch.randn(1, 16, 4, 8, 16).to(DEV)
    blk, bn = blk.to(DEV), bn.to(DEV)
    from mvs_gi_amd.dropin import common_modules as cm
    assert cm.lower_conv_block(blk).inorm is None
    assert torch.equal(blk(x), bn(x))
    blk.train()
    with pytest.raises(RuntimeError, match="model.eval"):
        blk(x)


def _cpu_base2d(b, x, res=None):
    y = F.conv2d(x, b.conv_layer.weight, b.conv_layer.bias, stride=b.conv_layer.stride, padding=b.conv_layer.padding)
    y = b.norm_layer(y)
    if res is not None:
        y = y + res
    return b.activation(y)


def test_conv_blocks_2d_with_instance_norm(conv_mode):
    torch.manual_seed(5)
    bar = _BAR[conv_mode]
    x = torch.randn(3, 16, 32, 64)
    blk = dropin.BaseConvBlk2d(16, 16, 3, stride=2, activation=nn.LeakyReLU(), norm_layer=nn.InstanceNorm2d(16)).eval()
    ref = _cpu_base2d(copy.deepcopy(blk).double(), x.double())
    assert _rel(blk.to(DEV)(x.to(DEV)).cpu(), ref) <= bar
    rb = dropin.ResConvBlk2d(16, 16, 3, activation=nn.LeakyReLU(), norm_layer=nn.InstanceNorm2d(16, affine=True)).eval()
    with torch.no_grad():
        for m in rb.modules():
            if isinstance(m, nn.InstanceNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
    b = copy.deepcopy(rb).double()
    ref = _cpu_base2d(b.blk2, _cpu_base2d(b.blk1, x.double()), x.double())
    assert _rel(rb.to(DEV)(x.to(DEV)).cpu(), ref) <= bar


def test_sphere_block_with_instance_norm(conv_mode):
    """SphereConvBlk with InstanceNorm2d == the same block on NoOp followed by instance norm (+ res, act) on the CPU."""
    torch.manual_seed(6)
    blk = dropin.SphereConvBlk((32, 64), 16, 16, 3, norm_layer=nn.InstanceNorm2d(16), activation=nn.LeakyReLU()).eval().to(DEV)
    plain = dropin.SphereConvBlk((32, 64), 16, 16, 3, norm_layer=dropin.NoOp(), activation=dropin.NoOp()).eval().to(DEV)
    plain.load_state_dict(blk.state_dict(), strict=True)
    x = torch.randn(2, 16, 32, 64, device=DEV)
    res = torch.randn(2, 16, 32, 64, device=DEV)
    got = blk(x, res).cpu()
    y = plain(x).double().cpu()
    ref = F.leaky_relu(F.instance_norm(y, eps=1e-5) + res.double().cpu(), 0.01)
    assert _rel(got, ref) <= 1e-5


# ---- whole paths --------------------------------------------------------------------------------------------------------
def _case_run(name, case, conv_mode, full=False):
    import parity_log
    cfg = case["cfg"]
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["inputs_sha256"])
    feats = torch.from_numpy(inp["feats"]).to(DEV)
    for gain in case["gains"]:
        w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
        hp = HotPath(cfg, w, inp, device=DEV)
        inv, _ = hp(feats)
        ref = z[f"inv_dist_g{gain:g}"]
        got = inv.cpu().numpy()
        err = _rel(got, ref)
        parity_log.record(name, conv_mode, gain, err, float(np.abs(got - ref).mean() / np.abs(ref).mean()), "golden",
                          float((np.abs(got - ref) / np.abs(ref)).max()))
        assert err <= 1e-3, (gain, err)             # the north-star bar
        if conv_mode == "f32":
            assert err <= 2e-4, (gain, err)


@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_small_instance_norm_paths_vs_reference_goldens(name, conv_mode):
    _case_run(name, SMALL_CASES[name], conv_mode)


@pytest.mark.parametrize("name", list(FULL_CASES))
def test_full_size_instance_norm_path_vs_reference_golden(name, conv_mode):
    _case_run(name, FULL_CASES[name], conv_mode, full=True)


def test_extractor_and_pipeline_with_instance_norm(conv_mode):
    import parity_log
    from mvs_gi_amd.pipeline import InferencePipeline
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "instnorm_extractor.npz"))
    cfg, seed, batch = EXTRACTOR_CASE["cfg"], EXTRACTOR_CASE["seed"], EXTRACTOR_CASE["batch"]
    imgs = synth.make_images(cfg, seed=seed, batch=batch)
    inp = synth.make_inputs(cfg, seed=seed, batch=batch)
    assert synth.digest({"imgs": imgs}) == str(z["imgs_sha256"]) and synth.digest(inp) == str(z["inputs_sha256"])
    fw = synth.make_extractor_weights(seed, norm_type="instance")
    fe = dropin.SimpleFeatExtraction(in_size=(64, 256), in_chs=3, chs=16, k_sz=3, layers=[5, 10], norm_type="instance")
    fe.load_state_dict({k: torch.from_numpy(v) for k, v in fw.items()}, strict=True)
    hp = HotPath(cfg, synth.make_weights(cfg, seed=seed), inp, device=DEV)
    model = dropin.SphericalSweepStereoBase(fe.eval().to(DEV), hp.cv_builder, hp.cv_regulator, hp.dist_regressor)
    with torch.no_grad():
        feats = model.extract_features(torch.from_numpy(imgs).to(DEV))
        inv, _ = model(torch.from_numpy(imgs).to(DEV), hp.grids, hp.grid_masks, hp.masks)
    ferr = _rel(feats.contiguous().cpu().numpy(), z["feats"])
    ierr = _rel(inv.cpu().numpy(), z["inv_dist"])
    parity_log.record("instnorm_extractor(imgs->inv_dist)", conv_mode, 1.0, ierr,
                      float(np.abs(inv.cpu().numpy() - z["inv_dist"]).mean() / np.abs(z["inv_dist"]).mean()), "golden")
    assert ferr <= (2e-5 if conv_mode == "f32" else 2e-3), ferr
    assert ierr <= 1e-3, ierr
    # the same frames through InferencePipeline (float images -> the extractor's stem reads NCHW fp32) and its hipGraph
    w = synth.make_weights(cfg, seed=seed)
    w["feature_extractor"] = fw
    pipe = InferencePipeline(cfg, w, synth.make_inputs(cfg, seed=seed, batch=1), device=DEV)
    u8 = (np.random.default_rng(seed).random((cfg.num_cams, 64, 256, 3)) * 255).astype(np.uint8)
    out = pipe({"imgs": [im for im in u8]})
    t = torch.from_numpy(u8).to(DEV)
    pipe.capture(t)
    assert np.array_equal(pipe.replay(t).squeeze().cpu().numpy(), out)
    assert np.isfinite(out).all()


def test_graph_replay_and_streams_with_instance_norm():
    """hipGraph capture / replay equals eager, and StreamedHotPath equals one stream, for an instance-norm G16V model."""
    from mvs_gi_amd.pipeline import StreamedHotPath
    H.set_conv_mode("f16x3")
    case = SMALL_CASES["instnorm_std"]
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=4)
    w = synth.make_weights(cfg, seed=case["seed"], gain=4.0)
    hp = HotPath(cfg, w, inp, device=DEV)
    feats = torch.from_numpy(inp["feats"]).to(DEV)
    eager, _ = hp(feats)
    eager = eager.clone()
    hp.capture(feats)
    inv, _ = hp.replay(feats)
    assert torch.equal(inv, eager)
    sp = StreamedHotPath(cfg, w, inp, device=DEV, n_streams=2)
    parts = sp(feats)
    torch.cuda.synchronize()
    one = HotPath(cfg, w, inp, device=DEV)            # each part against the same frames through one stream
    for i, p in enumerate(parts):
        ref, _ = one(feats[2 * i:2 * i + 2])
        assert torch.equal(p[0], ref)


def test_batch_norm_path_never_calls_instance_norm(monkeypatch):
    """Batch-norm models take exactly the paths they took before: with the instance-norm op made to raise, a small case still
    runs and matches its golden."""
    from golden_cases import SMALL_CASES as BN_CASES

    def boom(*a, **k):
        raise AssertionError("instance_norm called on a batch-norm model")
    monkeypatch.setattr(H, "instance_norm", boom)
    H.set_conv_mode("f16x3")
    case = BN_CASES["std_d8"]
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "std_d8.npz"))
    inp = synth.make_inputs(case["cfg"], seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    hp = HotPath(case["cfg"], synth.make_weights(case["cfg"], seed=case["seed"]), inp, device=DEV)
    inv, _ = hp(torch.from_numpy(inp["feats"]).to(DEV))
    assert _rel(inv.cpu().numpy(), z["inv_dist_g1"]) <= 1e-3
