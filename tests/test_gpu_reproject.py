"""GPU (MI355X): the back-projection kernel (csrc/reproject.hip, dropin.Reprojector) -- bit for bit against the chain of existing
kernels it is defined by, pinned to tests/golden/reproject.npz (the reference's own closed forms,
tools/make_reproject_goldens.py), on values nobody should pass, with every tensor between guard bands, beyond 2^31 output
elements, and inside InferencePipeline's captured graph.  Every test runs with guarded allocations (tests/guard_arena.py)."""
import gc
import itertools
import os

import numpy as np
import pytest
import torch

import guard_arena
import reproject_cases as RC
from mvs_gi_amd import dropin, hip_ops as H, synth
from mvs_gi_amd.configs import CONFIGS
from mvs_gi_amd.dropin import sweep_grids as SG
from mvs_gi_amd.pipeline import InferencePipeline
from oracle import grid_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("xyz", "warped", "valid", "grid")


@pytest.fixture(autouse=True)
def arena(request):
    """The guarded allocator of tests/guard_arena.py, as in every GPU module; the tests here also carve their inputs from it."""
    yield from guard_arena.fixture_body(request)


@pytest.fixture(autouse=True)
def _restore_mode():
    old = H.get_conv_mode()
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    H.set_conv_mode(old)
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "reproject.npz"))


def _makers(n, all_eq=False):
    return [SG.EquirectangularSampleGridMaker() if all_eq or k % 2 else SG.DoubleSphereSampleGridMaker(RC.DS_PARAMS, RC.DS_CALIB)
            for k in range(n)]


def _reprojector(name, bf):
    c = RC.CASES[name]
    return dropin.Reprojector(_makers(c["N"], c["all_eq"]), RC.poses(name), c["hw"], RC.LON, RC.LAT, bf=bf, device=DEV)


def _same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Equal element for element, NaN positions included (a NaN where `want` holds a number -- an unwritten element -- fails)."""
    got, want = got.cpu(), want.cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not got.is_floating_point():
        return bool(torch.equal(got, want))
    return bool(torch.equal(torch.isnan(got), torch.isnan(want))) and \
        bool(torch.equal(torch.nan_to_num(got, nan=0.0, posinf=3e38, neginf=-3e38), torch.nan_to_num(want, nan=0.0, posinf=3e38, neginf=-3e38))) and \
        bool(torch.equal(torch.isinf(got), torch.isinf(want)))


def _inputs(arena, name, scale=1.0):
    inv, imgs = RC.make_inputs(name)
    return arena.guarded((inv / scale).to(DEV)), arena.guarded(imgs.to(DEV))


# ------------------------------------------------------------------------------ 1. exactness: the bits of the chain
@pytest.mark.parametrize("bf", [96.0, 1.0])
@pytest.mark.parametrize("name", list(RC.CASES))
def test_kernel_is_the_bits_of_the_chain(arena, name, bf):
    rp = _reprojector(name, bf)
    inv, imgs = _inputs(arena, name, scale=96.0 / bf)                   # bf = 1 runs on inv / 96, the pipeline's metric map
    with arena.paused():
        want = rp.reproject_chain(inv, imgs, want=OUTPUTS)
        want_neg = rp.reproject_chain(inv, imgs, RC.INVALID_OTHER, want=("warped",))["warped"]
    full = rp.reproject(inv, imgs, want=OUTPUTS)
    for k in OUTPUTS:
        assert full[k].dtype == want[k].dtype and torch.equal(full[k], want[k]), k
        assert not bool(torch.isnan(full[k]).any()), f"{k}: an element was not written"
    xyz, warped, valid = rp(inv, imgs, invalid_pixel_value=RC.INVALID_OTHER)
    assert torch.equal(xyz, want["xyz"]) and torch.equal(valid, want["valid"]) and torch.equal(warped, want_neg)
    assert torch.equal(rp.point_cloud(inv), want["xyz"]) and torch.equal(rp.point_cloud(inv.unsqueeze(1)), want["xyz"])
    # any subset of the outputs NULL: the others keep their bits; without 'warped' the call takes no images
    for r in range(1, len(OUTPUTS)):
        for sub in itertools.combinations(OUTPUTS, r):
            got = rp.reproject(inv, imgs if "warped" in sub else None, want=sub)
            assert tuple(got) == sub
            for k in sub:
                assert torch.equal(got[k], want[k]), (sub, k)
    # a caller's own output tensors are written in place; the [B, N, ...] image layout is the same call
    out = {k: arena.alloc(full[k].shape, full[k].dtype, DEV) for k in OUTPUTS}
    res = rp.reproject(inv, imgs.view(inv.shape[0], rp.num_cams, *imgs.shape[1:]), want=OUTPUTS, out=out)
    for k in OUTPUTS:
        assert res[k] is out[k] and torch.equal(out[k], want[k]), k


def test_chain_returns_the_dictionary_of_reproject(arena):
    """Reprojector.reproject_chain and Reprojector.reproject: the same keys in the same order, dtypes, shapes and device, for the
    default selection, for every output and without images (the bits are test_kernel_is_the_bits_of_the_chain's)."""
    rp = _reprojector("tail_u8", RC.BF)
    inv, imgs = _inputs(arena, "tail_u8")
    with arena.paused():
        pairs = [(rp.reproject_chain(inv, imgs), rp.reproject(inv, imgs), ("xyz", "warped", "valid")),
                 (rp.reproject_chain(inv, imgs, 7.25, want=OUTPUTS), rp.reproject(inv, imgs, 7.25, want=OUTPUTS), OUTPUTS),
                 (rp.reproject_chain(inv.unsqueeze(1), want=("grid", "xyz")), rp.reproject(inv.unsqueeze(1), want=("grid", "xyz")), ("grid", "xyz"))]
    for chain, fused, want in pairs:
        assert isinstance(chain, dict) and tuple(chain) == tuple(fused) == want
        for k in want:
            assert chain[k].dtype == fused[k].dtype and chain[k].shape == fused[k].shape and chain[k].device == fused[k].device, k


# ------------------------------------------------------------------------------ 2. pinned to the reference's closed forms
@pytest.mark.parametrize("name", list(RC.CASES))
def test_pinned_to_the_reference_goldens(arena, z, name):
    """The device sin / sqrt / atan2 are the only source of difference: the bars and masks of
    test_sweep_grid_generator_vs_reference_goldens."""
    c = RC.CASES[name]
    rp = _reprojector(name, RC.BF)
    inv, imgs = _inputs(arena, name)
    assert np.array_equal(inv.cpu().numpy(), z[f"{name}_inv"]) and np.array_equal(imgs.cpu().numpy(), z[f"{name}_imgs"])
    assert np.array_equal(rp.T.numpy(), z[f"{name}_T"])
    got = {k: v.cpu() for k, v in rp.reproject(inv, imgs, want=OUTPUTS).items()}
    g = {k: torch.from_numpy(z[f"{name}_{k}"]) for k in ("xyz", "grid", "in_fov", "valid", "warped")}
    err = float((got["xyz"] - g["xyz"]).abs().max() / g["xyz"].abs().max())
    print(f"[reproject] {name}: xyz max error / max {err:.2e} (bar 2e-6)")
    assert err <= 2e-6
    fov, unit, _ = RC.edge_bands(name, g["xyz"], g["grid"])
    for n in range(c["N"]):
        well = g["in_fov"][:, n] & (g["grid"][:, n].abs().amax(-1) < 4)
        band = fov[:, n] | unit[:, n]
        left_out = 1 - float((well & ~band).float().mean())              # what the two masks together leave unchecked
        gerr = float((got["grid"][:, n] - g["grid"][:, n]).abs().amax(-1)[well].max())
        print(f"[reproject] {name} camera {n}: grid error {gerr:.2e} (bar 5e-5); masks leave out {left_out:.3f} of the pixels")
        assert left_out <= (0.25 if RC.is_double_sphere(name, n) else 0.02)
        assert gerr <= 5e-5
        assert torch.equal(got["valid"][:, n][~band], g["valid"][:, n][~band])
    # the sampler on the kernel's own coordinates: bit for bit
    for invalid in (0.0, RC.INVALID_OTHER):
        w = rp.reproject(inv, imgs, invalid, want=("warped",))["warped"].cpu()
        assert torch.equal(w, RC.sample(imgs.cpu(), got["grid"], got["valid"], invalid))
    assert bool(got["valid"].any()) and (c["all_eq"] or not bool(got["valid"].all()))          # both branches of step 6 ran


# ------------------------------------------------------------------------------ 3. values nobody should pass
@pytest.mark.parametrize("bf", [96.0, 1.0])
@pytest.mark.parametrize("name", ["tail_u8", "vec_f32c1", "eq_f32c3"])
def test_values_nobody_should_pass(arena, name, bf):
    rp = _reprojector(name, bf)
    inv, imgs = RC.make_inputs(name)
    bad = torch.tensor([0.0, -1.0, float("nan"), float("inf"), 1e-38, 1e38])
    flat = inv.view(-1)
    pos = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(7))[:4 * len(bad)]
    flat[pos] = bad.repeat(4)
    inv, imgs = arena.guarded(inv.to(DEV)), arena.guarded(imgs.to(DEV))
    with arena.paused():
        want = rp.reproject_chain(inv, imgs, 7.25, want=OUTPUTS)
    got = rp.reproject(inv, imgs, 7.25, want=OUTPUTS)
    torch.cuda.synchronize()                                            # no HIP error
    for k in OUTPUTS:
        assert _same_bits(got[k], want[k]), k
    finite = torch.isfinite(got["grid"]).all(dim=-1)
    assert not bool(finite.all()) and not bool(got["valid"][~finite].any())
    assert bool((got["warped"].movedim(2, -1)[~got["valid"]] == 7.25).all())
    assert bool(torch.isnan(got["xyz"]).any()) and bool(torch.isinf(got["xyz"]).any())


# ------------------------------------------------------------------------------ 4. address safety
@pytest.mark.parametrize("name", list(RC.CASES))
def test_address_safety(arena, name):
    """Every input in a guarded allocation, outputs pre-filled with the NaN sentinel: every output element is overwritten,
    the inputs and their guard bands are intact (the outputs' bands are checked at teardown)."""
    rp = _reprojector(name, RC.BF)
    inv, imgs = _inputs(arena, name)
    rays = arena.guarded(rp.rays)
    rp.rays = rays
    snaps = [(t, arena.snapshot(t)) for t in (inv, imgs, rays)]
    B, N, (Ho, Wo), C = RC.CASES[name]["B"], rp.num_cams, rp.out_shape, RC.CASES[name]["C"]
    out = dict(xyz=arena.alloc((B, 3, Ho, Wo), torch.float32, DEV), warped=arena.alloc((B, N, C, Ho, Wo), torch.float32, DEV),
               valid=arena.alloc((B, N, Ho, Wo), torch.bool, DEV), grid=arena.alloc((B, N, Ho, Wo, 2), torch.float32, DEV))
    for t in out.values():
        assert bool((t.view(torch.uint8).view(-1, 4) == torch.tensor(guard_arena.SENTINEL_BYTES, dtype=torch.uint8, device=DEV)).all())
    rp.reproject(inv, imgs, want=OUTPUTS, out=out)
    lib_made = rp.reproject(inv, imgs, want=OUTPUTS)                     # the library's own allocations are guarded and pre-filled too
    torch.cuda.synchronize()
    for res in (out, lib_made):
        for k in ("xyz", "warped", "grid"):
            assert not bool((res[k].view(torch.int32) == guard_arena.SENTINEL).any()), f"{k}: an element was never stored"
        assert bool((res["valid"].view(torch.uint8) <= 1).all()), "valid: a byte was never stored"
    for k in OUTPUTS:
        assert torch.equal(out[k], lib_made[k])
    for t, snap in snaps:
        assert arena.unchanged(t, snap)


# ------------------------------------------------------------------------------ 5. beyond 2^31 output elements
@pytest.fixture
def big():
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def test_large_offsets_reproject(arena, big):
    """warped [B][8][3][64][256] beyond 2^31 elements on 8 x 8 uint8 images: the first and the last two frames equal the chain."""
    N, C, Ho, Wo = 8, 3, 64, 256
    B = (1 << 31) // (N * C * Ho * Wo) + 3
    rp = dropin.Reprojector(_makers(N), G.ring_poses(N), (Ho, Wo), RC.LON, RC.LAT, bf=RC.BF, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(9)
    imgs = torch.randint(0, 256, (B * N, 8, 8, 3), device=DEV, generator=g, dtype=torch.uint8)
    inv = RC.BF / torch.exp(torch.rand((B, Ho, Wo), device=DEV, generator=g) * float(np.log(200.0)) + float(np.log(0.5)))
    res = rp.reproject(inv, imgs, -2.0, want=("warped", "valid"))
    warped, valid = res["warped"], res["valid"]
    assert warped.numel() >= (1 << 31) + 2 * N * C * Ho * Wo
    for b in (0, B - 2, B - 1):
        with arena.paused():
            want = rp.reproject_chain(inv[b:b + 1].clone(), imgs[b * N:(b + 1) * N].clone(), -2.0, want=("warped", "valid"))
        assert not bool(torch.isnan(warped[b]).any())
        assert torch.equal(warped[b:b + 1], want["warped"]) and torch.equal(valid[b:b + 1], want["valid"])
        assert 0.5 < float(want["valid"].float().mean()) < 1.0
    print(f"[large-offset] reproject B={B}: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ------------------------------------------------------------------------------ 6. the pipeline
def _tiny_rig(with_samplers):
    """extractor_small's geometry: 64 x 256 views, 16 x 64 output, three cameras."""
    from resample_cases import CASES as RAW, rotation
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32))
    w = synth.make_weights(cfg, seed=21)
    w["feature_extractor"] = synth.make_extractor_weights(21)
    inp = synth.make_inputs(cfg, seed=21, batch=1)
    rng = np.random.default_rng(22)
    poses = G.ring_poses(3)
    if with_samplers:
        yprs = [(0.0, 0.0, 0.0), (2.1, 0.3, 0.1), (-2.0, -0.2, 0.3)]
        samplers = [dropin.DoubleSphereToEquirectSampler(RAW["a"]["params"], (40, 56), (64, 256), rotation(*a), device=DEV) for a in yprs]
        imgs = [torch.from_numpy(rng.integers(0, 256, (3, 40, 56, 3), dtype=np.uint8)).to(DEV) for _ in range(2)]
        rp = dropin.Reprojector.from_samplers(samplers, poses, (16, 64), RC.LON, RC.LAT, bf=1.0, device=DEV)
        assert [gm.calib_shape for gm in rp.grid_makers] == [[40, 56]] * 3 and not torch.equal(rp.T[1], dropin.Reprojector(
            rp.grid_makers, poses, (16, 64), RC.LON, RC.LAT, bf=1.0, device=DEV).T[1])
    else:
        samplers = None
        imgs = [torch.from_numpy(rng.integers(0, 256, (3, 64, 256, 3), dtype=np.uint8)).to(DEV) for _ in range(2)]
        rp = dropin.Reprojector(_makers(3), poses, (16, 64), RC.LON, RC.LAT, bf=1.0, device=DEV)
    return cfg, w, inp, samplers, imgs, rp


@pytest.mark.parametrize("with_samplers", [False, True], ids=["views", "raw"])
def test_pipeline_with_reprojector(arena, with_samplers):
    H.set_conv_mode("f32")
    cfg, w, inp, samplers, (img_a, img_b), rp = _tiny_rig(with_samplers)
    plain = InferencePipeline(cfg, w, inp, device=DEV, samplers=samplers)
    pipe = InferencePipeline(cfg, w, inp, device=DEV, samplers=samplers, reprojector=rp)
    assert plain.reprojection is None and pipe.reprojection is None
    want_inv = plain.forward_device(img_a).clone()
    assert tuple(want_inv.shape) == (1, 1, 16, 64) and bool(torch.isfinite(want_inv).all()) and bool((want_inv > 0).all())
    want = [t.clone() for t in rp(want_inv, img_a)]
    assert tuple(want[0].shape) == (1, 3, 16, 64) and tuple(want[1].shape) == (1, 3, 3, 16, 64) and tuple(want[2].shape) == (1, 3, 16, 64)
    assert bool(want[2].any()) and not bool(want[2].all())

    def check(inv, expect_inv, expect):
        assert torch.equal(inv, expect_inv)                             # inv_dist: the bits of a pipeline without a reprojector
        assert len(pipe.reprojection) == 3
        for got, e in zip(pipe.reprojection, expect):
            assert got.dtype == e.dtype and torch.equal(got, e)
    check(pipe.forward_device(img_a), want_inv, want)
    pipe.capture(img_a)
    check(pipe.replay(img_a), want_inv, want)
    # other images: the replay's results follow
    other_inv = plain.forward_device(img_b).clone()
    other = [t.clone() for t in rp(other_inv, img_b)]
    assert not torch.equal(other[1], want[1]) and not torch.equal(other[0], want[0])
    check(pipe.replay(img_b), other_inv, other)
    check(pipe.replay(img_a), want_inv, want)
    with pytest.raises(ValueError, match="cameras"):
        InferencePipeline(cfg, w, inp, device=DEV, samplers=samplers,
                          reprojector=dropin.Reprojector(_makers(2), G.ring_poses(2), (16, 64), RC.LON, RC.LAT, bf=1.0, device=DEV))


def test_pipeline_without_reprojector_launches_no_reproject_kernel(arena, monkeypatch):
    """reprojector=None is the path as it was: the new symbol is not called."""
    H.set_conv_mode("f32")
    cfg, w, inp, _, (img_a, _), rp = _tiny_rig(False)
    called = []
    real = H._call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(H, "_call", spy)
    InferencePipeline(cfg, w, inp, device=DEV).forward_device(img_a)
    assert called and "mvsgi_reproject_f32" not in called
    called.clear()
    InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp).forward_device(img_a)
    assert called.count("mvsgi_reproject_f32") == 1 and called[-1] == "mvsgi_reproject_f32"          # one launch, behind the soft-argmin
