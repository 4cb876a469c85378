"""CPU: the fisheye -> surrogate-view resampler's definition (tests/resample_cases.py) against tests/golden/resample.npz
(the reference's own torch_cuda_sweep.py and backports.py, tools/make_resample_goldens.py), the surrogate rays against the
equirect projection the sweep uses, the uint8 conversion table, and the argument checks of the new C symbols."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resample_cases as RC
from mvs_gi_amd import _lib
from oracle import grid_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "resample.npz"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _same(a: torch.Tensor, b) -> bool:
    b = torch.from_numpy(np.asarray(b))
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_golden_file_is_complete_and_small(z):
    assert sorted(z.files) == sorted(f"{n}_{k}" for n in RC.CASES for k in RC.STORED)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "resample.npz")) < 200 * 1024
    for name, c in RC.CASES.items():
        assert z[f"{name}_grid"].shape == (*c["out"], 2) and z[f"{name}_img"].shape == (*c["raw"], 3)
        assert np.isfinite(z[f"{name}_grid"]).all()
        assert np.array_equal(z[f"{name}_img"].reshape(-1, 3)[:256, 0], np.arange(256))
        assert np.array_equal(z[f"{name}_R"], RC.rotation(*c["ypr"]))


@pytest.mark.parametrize("name", list(RC.CASES))
def test_restatement_reproduces_the_goldens_bit_for_bit(z, name):
    c = RC.CASES[name]
    g = {k: z[f"{name}_{k}"] for k in RC.STORED}
    assert _same(RC.surrogate_rays(*c["out"]), g["rays"])
    grid, ds, valid = RC.sampler_table(torch.from_numpy(g["rays"]), g["R"], c["params"], c["raw"])
    assert _same(grid, g["grid"]) and _same(ds, g["ds_mask"]) and _same(valid, g["valid"])
    img, smooth, mask = RC.make_images(name)
    assert _same(img, g["img"]) and _same(smooth, g["smooth"]) and _same(mask, g["mask"])
    assert _same(RC.resample(img, grid, valid), g["out"])
    assert _same(RC.resample(img, grid, valid, RC.INVALID_OTHER), g["out_neg"])
    assert _same(RC.resample(smooth, grid, valid), g["out_smooth"])
    assert _same(RC.sample_mask(mask, grid, valid), g["out_mask"])
    # the invalid value is what separates the two outputs, and only off the valid set
    v = torch.from_numpy(g["valid"])
    assert bool((torch.from_numpy(g["out_neg"])[0, :, ~v] == RC.INVALID_OTHER).all())
    assert _same(torch.from_numpy(g["out_neg"])[0, :, v], g["out"][0][:, g["valid"]])


def test_cases_cover_what_they_are_for(z):
    """Valid shares, valid pixels whose taps straddle the raw image border, both w1 branches, an odd row length in bytes."""
    shares = {n: float(z[f"{n}_valid"].mean()) for n in ("a", "b", "c")}
    assert shares == pytest.approx({"a": 0.55, "b": 0.60, "c": 0.39}, abs=0.006)
    for n in ("a", "b", "c"):
        Hr, Wr = RC.CASES[n]["raw"]
        g = torch.from_numpy(z[f"{n}_grid"])
        x, y = ((g[..., 0] + 1) * Wr - 1) / 2, ((g[..., 1] + 1) * Hr - 1) / 2
        straddle = torch.from_numpy(z[f"{n}_valid"]) & ((x < 0) | (x > Wr - 1) | (y < 0) | (y > Hr - 1))
        assert 12 <= int(straddle.sum()) <= 22
        assert int(RC.edge_set(n, z).sum()) <= 0.02 * g.shape[0] * g.shape[1]
    assert RC.CASES["a"]["params"][1] > 0.5 >= RC.CASES["c"]["params"][1]
    assert (RC.CASES["c"]["raw"][1] * 3) % 2 == 1


@pytest.mark.parametrize("hw", [(16, 64), (7, 30), (5, 4), (512, 2048)])
def test_surrogate_rays_are_the_pixel_centres_of_the_equirect_projection(hw):
    H, W = hw
    uv = G.grid_equirect(RC.surrogate_rays(H, W).view(1, 3, 1, H, W))[0, 0]
    u = (2 * torch.arange(W) + 1).float() / W - 1
    v = (2 * torch.arange(H) + 1).float() / H - 1
    assert float((uv[..., 0] - u.view(1, W)).abs().max()) <= 2e-7
    assert float((uv[..., 1] - v.view(H, 1)).abs().max()) <= 2e-7


def test_u8_table_is_torch_division_bit_for_bit(lib):
    t = torch.empty(256, dtype=torch.float32)
    assert lib.mvsgi_resample_u8_table_f32(ctypes.c_void_p(t.data_ptr())) == 0
    assert torch.equal(t.view(torch.int32), (torch.arange(256).float() / 255).view(torch.int32))
    assert lib.mvsgi_resample_u8_table_f32(None) != 0 and b"null pointer" in lib.mvsgi_last_error()


def test_new_symbols_reject_bad_arguments_before_any_launch(lib):
    p = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
    u8, f32 = lib.mvsgi_resample_bilinear_u8_f32, lib.mvsgi_resample_bilinear_f32

    def err():
        return lib.mvsgi_last_error()
    assert u8(None, p, p, p, 3, 3, 8, 12, 16, 64, 0.0, None) != 0 and b"null pointer" in err()
    assert u8(p, p, p, None, 3, 3, 8, 12, 16, 64, 0.0, None) != 0 and b"null pointer" in err()
    assert f32(p, None, p, p, 3, 3, 1, 8, 12, 16, 64, 0.0, None) != 0 and b"null pointer" in err()
    assert f32(p, p, None, p, 3, 3, 1, 8, 12, 16, 64, 0.0, None) != 0 and b"null pointer" in err()
    assert u8(p, p, p, p, 3, 0, 8, 12, 16, 64, 0.0, None) != 0 and b"T >= 1" in err()
    assert f32(p, p, p, p, 3, -1, 1, 8, 12, 16, 64, 0.0, None) != 0 and b"T >= 1" in err()
    assert u8(p, p, p, p, 7, 3, 8, 12, 16, 64, 0.0, None) != 0 and b"no multiple of T" in err()
    assert f32(p, p, p, p, 4, 3, 1, 8, 12, 16, 64, 0.0, None) != 0 and b"no multiple of T" in err()
    assert u8(p, p, p, p, 0, 3, 8, 12, 16, 64, 0.0, None) != 0 and b"no multiple of T" in err()
    assert f32(p, p, p, p, 3, 3, 0, 8, 12, 16, 64, 0.0, None) != 0 and b"non-positive" in err()
    assert u8(p, p, p, p, 3, 3, 8, 12, 0, 64, 0.0, None) != 0 and b"non-positive" in err()
    # row bytes: 3 Wr (uint8) and 4 Wr (fp32) must stay below 2^23; the whole image within the 32-bit tap offsets
    assert u8(p, p, p, p, 3, 3, 8, (1 << 23) // 3 + 1, 16, 64, 0.0, None) != 0 and b"row bytes" in err()
    assert f32(p, p, p, p, 3, 3, 1, 8, 1 << 21, 16, 64, 0.0, None) != 0 and b"row bytes" in err()
    assert f32(p, p, p, p, 3, 3, 1, 1 << 12, 1 << 20, 16, 64, 0.0, None) != 0 and b"row bytes" in err()
    # 16-byte tables and output for rows of whole quads
    q = ctypes.c_void_p(264)
    assert u8(p, q, p, p, 3, 3, 8, 12, 16, 64, 0.0, None) != 0 and b"aligned" in err()
    assert u8(p, p, p, q, 3, 3, 8, 12, 16, 64, 0.0, None) != 0 and b"aligned" in err()
    assert lib.mvsgi_rays_equirect_surrogate_f32(None, 16, 64, None) != 0 and b"null pointer" in err()
    assert lib.mvsgi_rays_equirect_surrogate_f32(p, 0, 64, None) != 0 and b"bad dimension" in err()
    assert lib.mvsgi_resample_validity_u8(p, None, p, 16, None) != 0 and b"null pointer" in err()
    assert lib.mvsgi_resample_validity_u8(p, p, p, 0, None) != 0 and b"bad element count" in err()


def test_hip_ops_entry_raises_on_cpu_tensors():
    from mvs_gi_amd import hip_ops as H
    with pytest.raises(RuntimeError, match="GPU only"):
        H.resample_bilinear(torch.zeros((1, 8, 12, 3), dtype=torch.uint8), torch.zeros((1, 4, 4, 2)), torch.ones((1, 4, 4), dtype=torch.bool))
    with pytest.raises(TypeError):
        H.resample_bilinear(torch.zeros((1, 8, 12, 3), dtype=torch.int16), torch.zeros((1, 4, 4, 2)), torch.ones((1, 4, 4), dtype=torch.bool))


def test_resample_validity_wrapper_rejects_bad_arguments():
    """hip_ops.resample_validity: a CPU tensor, a wrong dtype of either argument, a mask that is not the grid's leading shape."""
    from mvs_gi_amd import hip_ops as H
    grid, fov = torch.zeros((1, 8, 2)), torch.ones((1, 8), dtype=torch.bool)
    with pytest.raises(RuntimeError, match="GPU only"):          # there is no CPU fallback
        H.resample_validity(grid, fov)
    for bad in (grid.double(), grid.to(torch.uint8), None):
        with pytest.raises(TypeError, match="grid: expected a fp32 tensor"):
            H.resample_validity(bad, fov)
    for bad in (fov.float(), fov.to(torch.int32), [[True] * 8]):
        with pytest.raises(TypeError, match="in_fov: expected a bool or uint8 tensor"):
            H.resample_validity(grid, bad)
    for bad_grid, bad_fov in ((grid, fov[:, :7]), (grid, fov[0]), (torch.zeros((1, 8, 3)), fov), (torch.zeros((2,)), torch.ones((), dtype=torch.bool))):
        with pytest.raises(AssertionError, match="grid must be"):
            H.resample_validity(bad_grid, bad_fov)
