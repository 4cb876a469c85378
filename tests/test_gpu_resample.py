"""GPU (MI355X): the fisheye -> surrogate-view resampler -- the kernel (csrc/resample.hip) bit for bit against
tests/golden/resample.npz (the reference's own closed forms, tools/make_resample_goldens.py) and the CPU restatement pinned to
it (tests/resample_cases.py), the sampler with its table built on the device, the pipeline with samplers, and image bases
beyond 2^31 elements.  Every test runs with guarded allocations: NaN-filled outputs between guard bands."""
import gc
import os

import numpy as np
import pytest
import torch

import guard_arena
import resample_cases as RC
from mvs_gi_amd import dropin, hip_ops as H, synth
from mvs_gi_amd.configs import CONFIGS
from mvs_gi_amd.pipeline import InferencePipeline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return np.load(os.path.join(ROOT, "tests", "golden", "resample.npz"))


@pytest.fixture(scope="module")
def extra():
    """fp32 CHW images with C = 1 and 5 per case and their restated outputs (computed once, shared, never modified)."""
    zz = np.load(os.path.join(ROOT, "tests", "golden", "resample.npz"))
    out = {}
    for name, c in RC.CASES.items():
        g = torch.Generator().manual_seed(RC.SEEDS[name])
        grid, valid = torch.from_numpy(zz[f"{name}_grid"]), torch.from_numpy(zz[f"{name}_valid"])
        for C in (1, 5):
            img = torch.randn((C, *c["raw"]), generator=g)
            out[name, C] = (img, RC.resample(img, grid, valid), RC.resample(img, grid, valid, RC.INVALID_OTHER))
    return out


def _t(z, name, key):
    return torch.from_numpy(z[f"{name}_{key}"])


def _table(arena, z, name):
    return arena.guarded(_t(z, name, "grid").unsqueeze(0).to(DEV)), arena.guarded(_t(z, name, "valid").unsqueeze(0).to(DEV))


def _bits_equal(got: torch.Tensor, want: torch.Tensor) -> bool:
    """torch.equal, with NaNs equal to NaNs (a NaN in `got` where `want` is a number -- an unwritten element -- fails)."""
    got, want = got.cpu(), want.cpu()
    return got.shape == want.shape and bool(torch.equal(torch.isnan(got), torch.isnan(want))) and \
        bool(torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)))


# ------------------------------------------------------------------------------ 0. the validity rule
def test_resample_validity_on_the_edges_of_the_rule(arena):
    """hip_ops.resample_validity on a 1 x 8 table: in_fov & |gx| <= 1 & |gy| <= 1 with the bounds included, one ulp beyond them
    excluded, NaN and inf invalid -- equal to the same expression evaluated by torch on the CPU."""
    up, down = float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(-1), np.float32(-2)))
    grid = torch.tensor([[[1.0, 0.0], [-1.0, 0.0], [up, 0.0], [0.0, down], [float("nan"), 0.0], [0.0, float("inf")], [0.25, -0.5],
                          [0.25, -0.5]]], dtype=torch.float32)
    in_fov = torch.tensor([[1, 1, 1, 1, 1, 1, 0, 1]], dtype=torch.bool)
    assert up > 1.0 and down < -1.0 and tuple(grid.shape) == (1, 8, 2)
    want = (in_fov & (grid[..., 0].abs() <= 1) & (grid[..., 1].abs() <= 1)).to(torch.uint8)
    assert want.tolist() == [[1, 1, 0, 0, 0, 0, 0, 1]]
    for fov in (in_fov, in_fov.to(torch.uint8)):
        got = H.resample_validity(arena.guarded(grid.to(DEV)), arena.guarded(fov.to(DEV)))
        assert got.dtype == torch.uint8 and got.device.type == "cuda" and torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------ 1. the kernel, bit-exact
@pytest.mark.parametrize("name", list(RC.CASES))
def test_kernel_is_bit_exact_against_the_goldens(arena, z, extra, name):
    grid, valid = _table(arena, z, name)
    img, smooth = _t(z, name, "img"), _t(z, name, "smooth")
    for invalid, key in ((0.0, "out"), (RC.INVALID_OTHER, "out_neg")):
        got = H.resample_bilinear(arena.guarded(img.unsqueeze(0).to(DEV)), grid, valid, invalid_value=invalid)
        assert not bool(torch.isnan(got).any()), "an output element was not written"
        assert torch.equal(got.cpu(), _t(z, name, key))
        # the same image as fp32 CHW (C = 3), converted by hand
        f = arena.guarded(RC.as_f32_chw(img).unsqueeze(0).contiguous().to(DEV))
        assert torch.equal(H.resample_bilinear(f, grid, valid, invalid_value=invalid).cpu(), _t(z, name, key))
    assert torch.equal(H.resample_bilinear(arena.guarded(smooth.unsqueeze(0).to(DEV)), grid, valid).cpu(), _t(z, name, "out_smooth"))
    # C = 1: the mask path (sample_masks' input is mask * 255), then C = 1 and 5 of arbitrary fp32 data
    m = H.resample_bilinear(arena.guarded((_t(z, name, "mask") * 255).view(1, 1, *img.shape[:2]).to(DEV)), grid, valid)
    m[m > 0] = 1.0
    assert torch.equal(m[0].cpu(), _t(z, name, "out_mask"))
    for C in (1, 5):
        x, want0, want_neg = extra[name, C]
        xd = arena.guarded(x.unsqueeze(0).to(DEV))
        assert torch.equal(H.resample_bilinear(xd, grid, valid).cpu(), want0)
        assert torch.equal(H.resample_bilinear(xd, grid, valid, invalid_value=RC.INVALID_OTHER).cpu(), want_neg)
    # a caller's own output tensor is written in place
    out = arena.alloc((1, 3, *valid.shape[1:]), torch.float32, DEV)
    assert H.resample_bilinear(arena.guarded(img.unsqueeze(0).to(DEV)), grid, valid, out=out) is out
    assert torch.equal(out.cpu(), _t(z, name, "out"))


def test_image_m_uses_table_m_mod_t(arena, z):
    """M = 6, T = 3: cases a, b, c stacked (raw sizes differ, so every image is cropped to the common 37 x 45 and the expected
    outputs come from the restatement), then again with other images."""
    names = ("a", "b", "c")
    grids = torch.stack([_t(z, n, "grid") for n in names])
    valids = torch.stack([_t(z, n, "valid") for n in names])
    imgs = torch.stack([_t(z, n, "img")[:37, :45] for n in names] + [_t(z, n, "smooth")[:37, :45] for n in names]).contiguous()
    want = RC.resample_batch(imgs, grids, valids, RC.INVALID_OTHER)
    gd, vd = arena.guarded(grids.to(DEV)), arena.guarded(valids.to(DEV))
    got = H.resample_bilinear(arena.guarded(imgs.to(DEV)), gd, vd, invalid_value=RC.INVALID_OTHER)
    assert tuple(got.shape) == (6, 3, 16, 64) and torch.equal(got.cpu(), want)
    # case c's own image is uncropped: frame 0 of camera 2 is the golden itself
    assert torch.equal(got[2].cpu(), _t(z, "c", "out_neg")[0])
    f = arena.guarded(RC.as_f32_chw(imgs).contiguous().to(DEV))
    assert torch.equal(H.resample_bilinear(f, gd, vd, invalid_value=RC.INVALID_OTHER).cpu(), want)
    with pytest.raises(RuntimeError, match="no multiple of T"):
        H.resample_bilinear(arena.guarded(imgs[:4].to(DEV)), gd, vd)


# ------------------------------------------------------------------------------ 2. degenerate tables
@pytest.mark.parametrize("hw", [(16, 64), (7, 30)])
def test_degenerate_tables(arena, z, hw):
    Ho, Wo = hw
    img = _t(z, "c", "img")
    imgd = arena.guarded(img.unsqueeze(0).to(DEV))
    f = torch.randn((1, 2, 37, 45), generator=torch.Generator().manual_seed(5))
    fd = arena.guarded(f.to(DEV))
    # all invalid: the constant, whatever the grid holds
    grid = torch.full((1, Ho, Wo, 2), float("nan"))
    grid[0, ::2] = 1e30
    grid[0, :, ::3] = -float("inf")
    none = torch.zeros((1, Ho, Wo), dtype=torch.bool)
    for x, C in ((imgd, 3), (fd, 2)):
        got = H.resample_bilinear(x, arena.guarded(grid.to(DEV)), arena.guarded(none.to(DEV)), invalid_value=7.25)
        assert torch.equal(got.cpu(), torch.full((1, C, Ho, Wo), 7.25))
    # all valid with grids at exactly +-1, far outside and NaN, among ordinary ones
    g = torch.Generator().manual_seed(6)
    grid = torch.rand((1, Ho, Wo, 2), generator=g) * 2.4 - 1.2
    flat = grid.view(-1, 2)
    special = torch.tensor([[1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [-1.0, 0.3], [0.2, 1.0], [37.0, 0.0], [0.0, -37.0], [-37.0, 37.0],
                            [float("nan"), 0.0], [0.0, float("nan")], [float("nan"), float("nan")], [float("inf"), 0.1],
                            [3e38, -3e38]])
    pos = torch.randperm(flat.shape[0], generator=g)[:3 * len(special)]
    flat[pos] = special.repeat(3, 1)
    every = torch.ones((1, Ho, Wo), dtype=torch.bool)
    gd, vd = arena.guarded(grid.to(DEV)), arena.guarded(every.to(DEV))
    snaps = [(t, arena.snapshot(t)) for t in (imgd, fd, gd, vd)]
    assert _bits_equal(H.resample_bilinear(imgd, gd, vd), RC.resample(img, grid[0], every[0]))
    assert _bits_equal(H.resample_bilinear(fd, gd, vd, invalid_value=-1.0), RC.resample(f[0], grid[0], every[0]))
    torch.cuda.synchronize()
    for t, snap in snaps:                                   # inputs and their guard bands untouched; the outputs' bands are checked at teardown
        assert arena.unchanged(t, snap)


# ------------------------------------------------------------------------------ 3. the sampler, table built on the device
@pytest.mark.parametrize("name", list(RC.CASES))
def test_sampler_end_to_end(arena, z, name):
    c = RC.CASES[name]
    Ho, Wo = c["out"]
    Hr, Wr = c["raw"]
    s = dropin.DoubleSphereToEquirectSampler(c["params"], c["raw"], c["out"], z[f"{name}_R"], device=DEV)
    grid, valid = s.table
    assert tuple(grid.shape) == (Ho, Wo, 2) and tuple(valid.shape) == (Ho, Wo) and valid.dtype == torch.bool
    assert float((s.rays.cpu() - _t(z, name, "rays")).abs().max()) <= 1e-6          # unit vectors; device sin / cos within an ulp or two
    edge = RC.edge_set(name, z)
    n_edge = int(edge.sum())
    print(f"[resample] {name}: edge set {n_edge} of {Ho * Wo} pixels")
    assert n_edge <= 0.02 * Ho * Wo
    gv = _t(z, name, "valid")
    assert torch.equal(valid.cpu()[~edge], gv[~edge])
    keep = gv & ~edge
    gerr = float((grid.cpu() - _t(z, name, "grid")).abs()[keep].max())
    smooth = _t(z, name, "smooth")
    Gs = RC.largest_step(smooth)
    bound = 2e-5 * (Wr + Hr) / 2 * Gs
    out, v2 = s(smooth.to(DEV))
    assert v2 is valid and tuple(out.shape) == (1, 3, Ho, Wo)
    err = float((out.cpu() - _t(z, name, "out_smooth"))[0][:, keep].abs().max())
    print(f"[resample] {name}: device grid error {gerr:.2e} (bar 2e-5), smooth-image error {err:.2e} (bound {bound:.2e}, G = {Gs:.4f})")
    assert gerr <= 2e-5
    assert err <= bound
    # a given ray table (the golden's own) and the default one agree; a batch and a float image go through the same call
    s2 = dropin.DoubleSphereToEquirectSampler(c["params"], c["raw"], c["out"], z[f"{name}_R"], rays=_t(z, name, "rays"), device=DEV)
    assert float((s2.table[0] - grid).abs()[keep.to(DEV)].max()) <= 2e-5
    both, _ = s(torch.stack([smooth, _t(z, name, "img")]).to(DEV), invalid_pixel_value=RC.INVALID_OTHER)
    assert tuple(both.shape) == (2, 3, Ho, Wo) and torch.equal(both[0][:, valid], out[0][:, valid])
    assert bool((both[:, :, ~valid] == RC.INVALID_OTHER).all())
    fl, _ = s(RC.as_f32_chw(smooth).contiguous().to(DEV))
    assert torch.equal(fl, out)
    # the rig's masks
    m = dropin.sample_masks([s], [_t(z, name, "mask").to(DEV)])
    assert tuple(m.shape) == (1, 1, 1, Ho, Wo)
    assert torch.equal(m[0, 0, 0].cpu()[~edge], _t(z, name, "out_mask")[0][~edge])
    raw = torch.rand((Ho, Wo))
    assert torch.equal(dropin.sample_masks([dropin.NoOpSampler()], [raw])[0, 0, 0], raw)


def test_stack_tables(arena, z):
    ss = [dropin.DoubleSphereToEquirectSampler(RC.CASES[n]["params"], RC.CASES[n]["raw"], (16, 64), z[f"{n}_R"], device=DEV) for n in "ab"]
    grid, valid = dropin.stack_tables(ss)
    assert tuple(grid.shape) == (2, 16, 64, 2) and tuple(valid.shape) == (2, 16, 64)
    imgs = torch.stack([_t(z, "a", "img"), _t(z, "b", "img")]).to(DEV)
    got = H.resample_bilinear(imgs, grid, valid)
    for k, s in enumerate(ss):
        assert torch.equal(got[k:k + 1], s(imgs[k])[0])
    with pytest.raises(ValueError):
        dropin.stack_tables([ss[0], dropin.NoOpSampler()])


# ------------------------------------------------------------------------------ 4. the pipeline
def _tiny_rig():
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32))
    w = synth.make_weights(cfg, seed=21)
    w["feature_extractor"] = synth.make_extractor_weights(21)
    inp = synth.make_inputs(cfg, seed=21, batch=1)
    yprs = [(0.0, 0.0, 0.0), (2.1, 0.3, 0.1), (-2.0, -0.2, 0.3)]
    samplers = [dropin.DoubleSphereToEquirectSampler(RC.CASES["a"]["params"], (40, 56), (64, 256), RC.rotation(*a), device=DEV) for a in yprs]
    rng = np.random.default_rng(21)
    raw = torch.from_numpy(rng.integers(0, 256, (3, 40, 56, 3), dtype=np.uint8))
    raw_masks = [torch.from_numpy((rng.random((40, 56)) < 0.8).astype(np.float32)) for _ in range(3)]
    return cfg, w, inp, samplers, raw, raw_masks


def test_pipeline_with_samplers(arena):
    H.set_conv_mode("f32")
    cfg, w, inp, samplers, raw, raw_masks = _tiny_rig()
    assert cfg.num_cams == 3
    consts = {k: v for k, v in inp.items() if k != "masks"}
    pipe = InferencePipeline(cfg, w, consts, device=DEV, samplers=samplers, raw_masks=raw_masks)
    masks = dropin.sample_masks(samplers, raw_masks)
    assert tuple(masks.shape) == (1, 3, 1, 64, 256) and torch.equal(pipe.hot.masks, masks)
    plain = InferencePipeline(cfg, w, dict(consts, masks=masks.cpu().numpy()), device=DEV)
    rawd = raw.to(DEV)
    by_hand = H.resample_bilinear(rawd, *dropin.stack_tables(samplers))               # fp32 [3, 3, 64, 256]
    want = plain.forward_device(by_hand)
    got = pipe.forward_device(rawd)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    host = pipe({"imgs": [im for im in raw.numpy()]})
    assert np.array_equal(host, want.squeeze(0).squeeze(0).cpu().numpy())
    # the whole chain, resample included, as one hipGraph
    pipe.capture(rawd)
    assert torch.equal(pipe.replay(rawd), want)
    other = rawd.flip(0).contiguous()
    eager = pipe.forward_device(other).clone()
    assert not torch.equal(eager, want) and torch.equal(pipe.replay(other), eager)
    with pytest.raises(ValueError):
        InferencePipeline(cfg, w, consts, device=DEV, samplers=samplers)             # no masks and no raw masks
    with pytest.raises(ValueError):
        InferencePipeline(cfg, w, inp, device=DEV, samplers=samplers[:2])


def test_pipeline_without_samplers_launches_no_resample_kernel(arena, monkeypatch):
    """samplers=None is the path as it was: no resample symbol is called."""
    H.set_conv_mode("f32")
    cfg, w, inp, _, _, _ = _tiny_rig()
    called = []
    real = H._call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(H, "_call", spy)
    pipe = InferencePipeline(cfg, w, inp, device=DEV)
    imgs = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, 64, 256, 3), dtype=np.uint8)).to(DEV)
    out = pipe.forward_device(imgs)
    assert bool(torch.isfinite(out).all())
    assert called and not [n for n in called if "resample" in n or "rays_equirect" in n]
    called.clear()
    s = dropin.DoubleSphereToEquirectSampler(RC.CASES["a"]["params"], (40, 56), (16, 64), np.eye(3), device=DEV)
    s(torch.zeros((40, 56, 3), dtype=torch.uint8, device=DEV))
    assert "mvsgi_resample_bilinear_u8_f32" in called                   # the spy does see the resampler when it runs


# ------------------------------------------------------------------------------ 5. image bases beyond 2^31 elements
@pytest.fixture
def big():
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
def test_large_offsets_resample(arena, big, u8):
    """Output [M, 3, 64, 256] beyond 2^31 elements, T = 1: the first, second to last and last image equal a one-image launch."""
    Ho, Wo, C = 64, 256, 3
    M = (1 << 31) // (C * Ho * Wo) + 3
    g = torch.Generator(device=DEV).manual_seed(9)
    if u8:
        imgs = torch.randint(0, 256, (M, 8, 12, 3), device=DEV, generator=g, dtype=torch.uint8)
    else:
        imgs = torch.rand((M, C, 8, 12), device=DEV, generator=g)
    grid = arena.guarded(torch.rand((1, Ho, Wo, 2), device=DEV, generator=g) * 2.2 - 1.1)
    valid = arena.guarded(torch.rand((1, Ho, Wo), device=DEV, generator=g) < 0.8)
    out = H.resample_bilinear(imgs, grid, valid, invalid_value=-2.0)
    assert out.numel() >= (1 << 31) + 2 * C * Ho * Wo
    for m in (0, M - 2, M - 1):
        one = H.resample_bilinear(imgs[m:m + 1].clone(), grid, valid, invalid_value=-2.0)
        assert not bool(torch.isnan(one).any()) and torch.equal(out[m:m + 1], one)
    print(f"[large-offset] resample M={M}: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
