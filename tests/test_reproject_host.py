"""CPU: the back-projection's definition (tests/reproject_cases.py) against tests/golden/reproject.npz (the reference's own
torch_cuda_sweep.py and backports.py, tools/make_reproject_goldens.py), what the cases are for, the argument checks of
mvsgi_reproject_f32, and the host side of dropin.Reprojector (transforms composed in float64, the camera table)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import reproject_cases as RC
from mvs_gi_amd import _lib
from oracle import grid_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reproject.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def composed():
    """The CPU restatement of every case (computed once, shared, never modified)."""
    out = {}
    for name in RC.CASES:
        inv, imgs = RC.make_inputs(name)
        out[name] = (inv, imgs, RC.compose(name, inv, imgs), RC.compose(name, inv, imgs, invalid=RC.INVALID_OTHER)["warped"])
    return out


def test_abi_version_and_symbol(lib):
    assert _lib.ABI_VERSION == 8 and lib.mvsgi_abi_version() == 8
    assert "mvsgi_reproject_f32" in _lib.SIGNATURES and lib.mvsgi_reproject_f32.restype is ctypes.c_int
    decl = open(os.path.join(ROOT, "include", "mvsgi.h")).read()
    assert "#define MVSGI_ABI_VERSION 8" in decl and "int mvsgi_reproject_f32(" in decl


def test_golden_file_is_complete_and_small(z):
    assert sorted(z.files) == sorted(f"{n}_{k}" for n in RC.CASES for k in RC.STORED)
    assert os.path.getsize(GOLDEN) < 400 * 1024
    for name, c in RC.CASES.items():
        B, N, (H, W) = c["B"], c["N"], c["hw"]
        assert z[f"{name}_inv"].shape == (B, H, W) and z[f"{name}_xyz"].shape == (B, 3, H, W)
        assert z[f"{name}_grid"].shape == (B, N, H, W, 2) and z[f"{name}_valid"].shape == (B, N, H, W)
        assert z[f"{name}_warped"].shape == (B, N, c["C"], H, W)
        assert z[f"{name}_imgs"].shape == ((B * N, *c["img"], 3) if c["u8"] else (B * N, c["C"], *c["img"]))


@pytest.mark.parametrize("name", list(RC.CASES))
def test_restatement_reproduces_the_goldens(z, composed, name):
    """The comparison of test_grid_oracle_matches_reference_closed_forms: np.array_equal, array by array."""
    inv, imgs, r, warped_neg = composed[name]
    assert np.array_equal(inv.numpy(), z[f"{name}_inv"]) and np.array_equal(imgs.numpy(), z[f"{name}_imgs"])
    assert np.array_equal(RC.rays(name).numpy(), z[f"{name}_rays"])
    assert np.array_equal(RC.transforms(name).numpy(), z[f"{name}_T"])
    for k in ("xyz", "grid", "in_fov", "valid", "warped"):
        assert np.array_equal(r[k].numpy(), z[f"{name}_{k}"]), k
    assert np.array_equal(warped_neg.numpy(), z[f"{name}_warped_neg"])
    v = r["valid"].unsqueeze(2).expand_as(r["warped"])
    assert bool((warped_neg[~v] == RC.INVALID_OTHER).all()) and torch.equal(warped_neg[v], r["warped"][v])


def test_cases_cover_what_they_are_for(composed):
    """Both branches of step 6 run on every double-sphere camera, every equirectangular pixel is valid, at most one pixel per
    camera sits in an edge band, none on the atan2 branch cut, and fp32 is within 3e-7 of a float64 evaluation."""
    assert [(c["B"], c["N"], *c["hw"], c["u8"], c["C"], *c["img"]) for c in RC.CASES.values()] == \
        [(2, 3, 6, 10, True, 3, 9, 13), (1, 1, 8, 16, False, 1, 12, 20), (2, 8, 1, 7, True, 3, 5, 7), (1, 4, 8, 16, False, 3, 12, 20)]
    for name, c in RC.CASES.items():
        inv, _, r, _ = composed[name]
        d = RC.BF / inv
        assert 0.5 * (1 - 1e-6) <= float(d.min()) and float(d.max()) <= 100.0 * (1 + 1e-6)
        fov, unit, cut = RC.edge_bands(name, r["xyz"], r["grid"])
        r64 = RC.compose(name, inv, None, dtype=torch.float64)
        for n in range(c["N"]):
            share = float(r["valid"][:, n].float().mean())
            if RC.is_double_sphere(name, n):
                assert 0.78 <= share <= 0.86, (name, n, share)
            else:
                assert share == 1.0 and bool(r["in_fov"][:, n].all())
            assert int(fov[:, n].sum()) <= 1 and int(unit[:, n].sum()) <= 1 and int(cut[:, n].sum()) == 0
            well = r["in_fov"][:, n] & (r["grid"][:, n].abs().amax(-1) < 4)
            assert float((r["grid"][:, n].double() - r64["grid"][:, n]).abs().amax(-1)[well].max()) <= 3e-7
    assert all(RC.is_double_sphere("tail_u8", n) == (n % 2 == 0) for n in range(3))
    assert not any(RC.is_double_sphere("eq_f32c3", n) for n in range(4))


# ------------------------------------------------------------------------------ the C entry point's checks
def test_reproject_rejects_bad_arguments_before_any_launch(lib):
    f = lib.mvsgi_reproject_f32
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(264)          # never dereferenced: every call below fails its checks first
    T = torch.eye(4).repeat(8, 1, 1).contiguous()
    cams = torch.zeros((8, 10))
    cams[:, 0] = 1.0                                            # equirectangular
    ds = torch.tensor([[0.0, -0.203, 0.589, 232.0, 232.0, 611.5, 513.5, 0.9, 1027.0, 1223.0]])
    Tp, Cp = ctypes.c_void_p(T.data_ptr()), ctypes.c_void_p(cams.data_ptr())

    def call(inv=p, rays=p, imgs=p, kind=0, T=Tp, cams=Cp, xyz=p, warped=p, valid=p, grid=p, B=2, N=3, C=3, Hr=9, Wr=13, H=6, W=10):
        return f(inv, rays, imgs, kind, T, cams, xyz, warped, valid, grid, B, N, C, Hr, Wr, H, W, 96.0, 0.0, None)

    def err():
        return lib.mvsgi_last_error()
    for kw in (dict(inv=None), dict(rays=None), dict(T=None), dict(cams=None)):
        assert call(**kw) != 0 and b"null pointer" in err(), kw
    assert call(xyz=None, warped=None, valid=None, grid=None, imgs=None) != 0 and b"null pointer" in err()
    assert call(imgs=None) != 0 and b"warped without imgs" in err()
    assert call(warped=None) != 0 and b"imgs without warped" in err()
    for n in (0, -1, 9):
        assert call(N=n) != 0 and b"cameras" in err(), n
    bad = cams.clone()
    bad[1, 0] = 2.0
    assert call(cams=ctypes.c_void_p(bad.data_ptr())) != 0 and b"unknown model id" in err() and b"camera 1" in err()
    bad[1, 0] = 0.5
    assert call(cams=ctypes.c_void_p(bad.data_ptr())) != 0 and b"unknown model id" in err()
    assert call(C=1) != 0 and b"uint8 images have C = 3" in err()
    assert call(C=4) != 0 and b"uint8 images have C = 3" in err()
    assert call(kind=1, C=0) != 0 and b"C >= 1" in err()
    assert call(kind=2) != 0 and b"unknown image kind" in err()
    for kw in (dict(B=0), dict(H=0), dict(W=-3), dict(Hr=0), dict(Wr=0)):
        assert call(**kw) != 0 and b"non-positive" in err(), kw
    for hm1, wm1 in ((0.0, 1223.0), (1027.0, 0.0), (-1.0, 5.0)):
        d = ds.clone()
        d[0, 8], d[0, 9] = hm1, wm1
        assert call(N=1, cams=ctypes.c_void_p(d.data_ptr())) != 0 and b"calib" in err()
    for k in ("xyz", "warped", "valid", "grid"):
        assert call(**{k: q}) != 0 and b"outputs must be 16-byte aligned" in err(), k
    assert call(W=12, inv=q) != 0 and b"aligned" in err()
    assert call(W=12, rays=q) != 0 and b"aligned" in err()
    assert call(Wr=(1 << 23) // 3 + 1) != 0 and b"row bytes" in err()


# ------------------------------------------------------------------------------ dropin.Reprojector, host side
def _makers(n):
    from mvs_gi_amd.dropin import sweep_grids as SG
    return [SG.DoubleSphereSampleGridMaker() if k % 2 == 0 else SG.EquirectangularSampleGridMaker() for k in range(n)]


def test_reprojector_composes_transforms_in_float64(lib):
    from mvs_gi_amd import dropin
    from resample_cases import rotation
    poses = G.ring_poses(3)
    R_raw = [rotation(2.1, 0.3, 0.1), None, rotation(-1.0, -0.4, 0.5)]
    r = dropin.Reprojector(_makers(3), poses, (4, 8), bf=1.0, rays=torch.zeros((3, 4, 8)), R_raw=R_raw, device="cpu")
    assert r.T.dtype == torch.float32 and tuple(r.T.shape) == (3, 4, 4) and not r.T.is_cuda and r.bf == 1.0
    for n, (pose, R) in enumerate(zip(poses, R_raw)):
        want = np.linalg.inv(pose.numpy().astype(np.float64))
        if R is not None:
            R4 = np.eye(4)
            R4[:3, :3] = R
            want = R4 @ want
        # entries are at most 1 in magnitude: float64 algebra rounded once to fp32 is within one fp32 ulp of 1 of numpy's
        assert np.abs(r.T[n].numpy().astype(np.float64) - want).max() <= 2.0 ** -23
        assert np.array_equal(r.T[n, 3].numpy(), [0, 0, 0, 1])
    # without raw rotations: make_sweep_grid's own transform, bit for bit; rounding first and multiplying in fp32 is another number
    plain = dropin.Reprojector(_makers(3), poses, (4, 8), rays=torch.zeros((3, 4, 8)), device="cpu")
    assert plain.bf == 96.0
    for n, pose in enumerate(poses):
        assert torch.equal(plain.T[n], torch.linalg.inv(pose.to(torch.float64)).to(torch.float32))
    R4 = torch.eye(4, dtype=torch.float64)
    R4[:3, :3] = torch.from_numpy(R_raw[0])
    assert torch.equal(r.T[0], (R4 @ torch.linalg.inv(poses[0].to(torch.float64))).to(torch.float32))
    assert not torch.equal(r.T[0], R4.float() @ plain.T[0])


def test_reprojector_packs_the_camera_table(lib):
    from mvs_gi_amd import dropin, hip_ops as H
    from mvs_gi_amd.dropin import sweep_grids as SG
    ds2 = SG.DoubleSphereSampleGridMaker(params=[0.1, 0.45, 300.0, 310.0, 320.0, 240.0], calib_shape=[480, 640])
    makers = [SG.DoubleSphereSampleGridMaker(), SG.EquirectangularSampleGridMaker(), ds2]
    r = dropin.Reprojector(makers, G.ring_poses(3), (4, 8), rays=torch.zeros((3, 4, 8)), device="cpu")
    assert r.cams.dtype == torch.float32 and tuple(r.cams.shape) == (3, H.REPROJECT_CAM_FLOATS) and H.REPROJECT_CAM_FLOATS == 10
    w2 = G.double_sphere_w2(-0.203, 0.589)
    assert np.array_equal(r.cams[0].numpy(), np.array([0, -0.203, 0.589, 232.0, 232.0, 611.5, 513.5, w2, 1027, 1223], np.float64).astype(np.float32))
    assert np.array_equal(r.cams[1].numpy(), np.array([1] + [0] * 9, np.float32))
    assert np.array_equal(r.cams[2].numpy(), np.array([0, 0.1, 0.45, 300.0, 310.0, 320.0, 240.0, G.double_sphere_w2(0.1, 0.45), 479, 639],
                                                      np.float64).astype(np.float32))
    with pytest.raises(TypeError, match="grid maker"):
        dropin.Reprojector([object()], G.ring_poses(1), (4, 8), rays=torch.zeros((3, 4, 8)), device="cpu")


def test_reprojector_raises_on_cpu_tensors_shape_mismatches_and_wide_rigs(lib):
    from mvs_gi_amd import dropin, hip_ops as H
    rays = torch.zeros((3, 4, 8))
    r = dropin.Reprojector(_makers(2), G.ring_poses(2), (4, 8), rays=rays, device="cpu")
    inv = torch.ones((1, 4, 8))
    imgs = torch.zeros((2, 5, 6, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):          # there is no CPU fallback
        r.point_cloud(inv)
    with pytest.raises(RuntimeError, match="GPU only"):
        r(inv, imgs)
    with pytest.raises(RuntimeError, match="GPU only"):
        H.reproject(inv, rays, r.T, r.cams, 96.0, want=("xyz",))
    with pytest.raises(AssertionError, match="inv must be"):
        r.point_cloud(torch.ones((1, 4, 9)))
    with pytest.raises(AssertionError, match="imgs must"):
        r(inv, torch.zeros((3, 5, 6, 3), dtype=torch.uint8))
    with pytest.raises(AssertionError, match="imgs must"):
        r(inv, torch.zeros((1, 3, 5, 6, 3), dtype=torch.uint8))
    with pytest.raises(AssertionError, match="rays must be"):
        dropin.Reprojector(_makers(2), G.ring_poses(2), (4, 8), rays=torch.zeros((3, 4, 9)), device="cpu")
    with pytest.raises(AssertionError, match="poses"):
        dropin.Reprojector(_makers(2), G.ring_poses(3), (4, 8), rays=rays, device="cpu")
    with pytest.raises(AssertionError, match="rotations"):
        dropin.Reprojector(_makers(2), G.ring_poses(2), (4, 8), rays=rays, R_raw=[np.eye(3)], device="cpu")
    assert H.sweep_max_cams() == 8
    with pytest.raises(ValueError, match="9 cameras"):
        dropin.Reprojector(_makers(9), G.ring_poses(9), (4, 8), rays=rays, device="cpu")
    with pytest.raises(ValueError, match="0 cameras"):
        dropin.Reprojector([], [], (4, 8), rays=rays, device="cpu")
    with pytest.raises(ValueError, match="long_range"):
        dropin.Reprojector(_makers(2), G.ring_poses(2), (4, 8), device="cpu")
