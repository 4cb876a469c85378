"""Cases and CPU restatement (torch fp32) of the back-projection (mvs_gi_amd/dropin/reproject.py, csrc/reproject.hip).
TEST INFRASTRUCTURE ONLY.  The restatement composes the pinned restatements of the reference's closed forms
(oracle.grid_oracle, oracle.mvsgi_oracle.bilinear_sample_zeros); tests/test_reproject_host.py pins it to
tests/golden/reproject.npz, which tools/make_reproject_goldens.py makes with the reference's own torch_cuda_sweep.py and
backports.py.

Definition (SphericalSweepStereo._create_warped_inputs, spherical_sweep_stereo.py:417-471), frame b, pixel (i, j), camera n:
  1. d = bf / inv[b, i, j]                       IEEE single division (the reference's `bf / outputs` is reciprocal * bf in torch)
  2. p = rays[:, i, j] * d                       rays = RayMaker_UEPanorama([1.0], lon, lat) at (H, W); -> xyz
  3. q = T_n p                                   transform_3D_points_torch, T_n = float32(inverse(pose_n) in float64)
  4. g, in_fov = camera n's make_grid(q)         double sphere, or equirectangular with in_fov = 1
  5. valid = in_fov & |gx| <= 1 & |gy| <= 1
  6. warped = valid ? bilinear_grid_sample(img[b, n], g, align_corners=False) : invalid_value
"""
import math

import numpy as np
import torch

from oracle import grid_oracle as G
from oracle.mvsgi_oracle import bilinear_sample_zeros

LON = (0.0, 2 * math.pi)                     # the rig camera of the g16 golden (tools/make_grid_goldens.py)
LAT = (-math.pi / 2, 0.0)
DS_PARAMS = (-0.203, 0.589, 232.0, 232.0, 611.5, 513.5)
DS_CALIB = (1028, 1224)
BF = 96.0
INVALID_OTHER = -3.5

CASES = {
    # name: frames B, cameras N, map (H, W), image dtype / channels / size, every camera equirectangular?
    "tail_u8": dict(B=2, N=3, hw=(6, 10), u8=True, C=3, img=(9, 13), all_eq=False),          # row tail, odd image
    "vec_f32c1": dict(B=1, N=1, hw=(8, 16), u8=False, C=1, img=(12, 20), all_eq=False),      # vector form, mask-like
    "eight_u8": dict(B=2, N=8, hw=(1, 7), u8=True, C=3, img=(5, 7), all_eq=False),           # eight cameras, one row
    "eq_f32c3": dict(B=1, N=4, hw=(8, 16), u8=False, C=3, img=(12, 20), all_eq=True),
}
# eight_u8 has 14 pixels per camera: its seed is one at which every double-sphere camera keeps 11 or 12 of them (0.78 ... 0.86)
SEEDS = {"tail_u8": 300, "vec_f32c1": 301, "eight_u8": 306, "eq_f32c3": 303}
# arrays stored per case in reproject.npz (prefix "<case>_"); grid / in_fov / valid / warped are [B, N, ...]
STORED = ("inv", "imgs", "rays", "T", "xyz", "grid", "in_fov", "valid", "warped", "warped_neg")


def is_double_sphere(name: str, n: int) -> bool:
    return not CASES[name]["all_eq"] and n % 2 == 0


def poses(name: str):
    return G.ring_poses(CASES[name]["N"])


def transforms(name: str) -> torch.Tensor:
    """Step 3's T [N, 4, 4] fp32 (make_sweep_grid_cuda, multi_view_camera_model_dataset.py:505)."""
    return torch.stack([torch.linalg.inv(p.to(torch.float64)).to(torch.float32) for p in poses(name)])


def make_inputs(name: str):
    """The seeded inputs of a case -> (inv [B, H, W] fp32 = 96 / d with d log-uniform in 0.5 ... 100 m, imgs uint8
    [B*N, Hr, Wr, 3] or fp32 [B*N, C, Hr, Wr])."""
    c = CASES[name]
    rng = np.random.default_rng(SEEDS[name])
    H, W = c["hw"]
    d = np.exp(rng.uniform(np.log(0.5), np.log(100.0), size=(c["B"], H, W))).astype(np.float32)
    inv = torch.from_numpy(np.float32(BF) / d)
    M = c["B"] * c["N"]
    if c["u8"]:
        imgs = torch.from_numpy(rng.integers(0, 256, size=(M, *c["img"], 3), dtype=np.uint8))
    else:
        imgs = torch.from_numpy(rng.standard_normal((M, c["C"], *c["img"])).astype(np.float32))
        if c["C"] == 1:
            imgs = (imgs > -0.5).to(torch.float32) * 255                 # mask-like: sample_masks' input is mask * 255
    return inv, imgs


def rays(name: str) -> torch.Tensor:
    """Step 2's table [3, H, W]."""
    H, W = CASES[name]["hw"]
    return G.rays_panorama(np.ones(1, np.float32), LON, LAT, (H, W))[:, 0]


def distance(inv: torch.Tensor, bf: float) -> torch.Tensor:
    """Step 1 as an IEEE division of two tensors (a Python scalar over a tensor is reciprocal * scalar in torch)."""
    return torch.full_like(inv, bf) / inv


def as_f32_chw(imgs: torch.Tensor) -> torch.Tensor:
    """uint8 [M, Hr, Wr, 3] -> fp32 [M, 3, Hr, Wr] as inference_pytorch.py:58-59 converts (.float() / 255.0); fp32 as is."""
    if imgs.dtype == torch.uint8:
        return imgs.movedim(-1, -3).float() / 255.0
    return imgs


def sample(imgs: torch.Tensor, grid: torch.Tensor, valid: torch.Tensor, invalid: float = 0.0) -> torch.Tensor:
    """Step 6: imgs [B*N, ...], grid [B, N, H, W, 2], valid [B, N, H, W] -> warped [B, N, C, H, W]."""
    B, N, H, W, _ = grid.shape
    s = bilinear_sample_zeros(as_f32_chw(imgs), grid.reshape(B * N, H, W, 2))
    s = torch.where(valid.reshape(B * N, 1, H, W), s, torch.tensor(invalid, dtype=torch.float32))
    return s.reshape(B, N, -1, H, W)


def compose(name: str, inv: torch.Tensor, imgs, bf: float = BF, invalid: float = 0.0, ray_table=None, T=None, dtype=torch.float32,
            makers=None):
    """Steps 1-6 on the CPU -> dict(xyz [B, 3, H, W], grid [B, N, H, W, 2], in_fov, valid [B, N, H, W], warped [B, N, C, H, W]).
    dtype=torch.float64 evaluates steps 1-4 in double from the same fp32 inputs (no warped).  makers: (transform_points,
    grid_double_sphere(points, params, calib), grid_equirect) -- the oracle's by default, the reference's own in
    tools/make_reproject_goldens.py."""
    c = CASES[name]
    tp, gds, geq = makers or (G.transform_points, G.grid_double_sphere, G.grid_equirect)
    r = (rays(name) if ray_table is None else ray_table).to(dtype)
    T = (transforms(name) if T is None else T).to(dtype)
    B, H, W = inv.shape
    xyz = r.unsqueeze(0) * distance(inv.to(dtype), bf).unsqueeze(1)                        # [B, 3, H, W]
    grids, fovs = [], []
    for n in range(c["N"]):
        q = tp(T[n].unsqueeze(0).expand(B, 4, 4).contiguous(), xyz.unsqueeze(2))           # [B, 3, 1, H, W]
        if is_double_sphere(name, n):
            g, m = gds(q, DS_PARAMS, DS_CALIB)
        else:
            g, m = geq(q), torch.ones((B, 1, H, W), dtype=torch.bool)
        grids.append(g[:, 0])
        fovs.append(m[:, 0])
    grid, in_fov = torch.stack(grids, dim=1), torch.stack(fovs, dim=1)
    valid = in_fov & (grid[..., 0].abs() <= 1) & (grid[..., 1].abs() <= 1)
    out = dict(xyz=xyz, grid=grid, in_fov=in_fov, valid=valid)
    if imgs is not None and dtype == torch.float32:
        out["warped"] = sample(imgs, grid, valid, invalid)
    return out


def edge_bands(name: str, xyz: torch.Tensor, grid: torch.Tensor, T=None):
    """Pixels [B, N, H, W] where two evaluations of the closed forms may legitimately disagree on validity:
    (fov) the double-sphere field-of-view test within 1e-5 |q| of its threshold, (unit) a |g| within 1e-4 of 1,
    (cut) an equirectangular camera's atan2 branch cut (x < 0, |z| < 1e-4 |x|: u flips between -1 and +1).  The rules of
    test_sweep_grid_generator_vs_reference_goldens."""
    c = CASES[name]
    T = transforms(name) if T is None else T
    B = xyz.shape[0]
    w2 = G.double_sphere_w2(DS_PARAMS[0], DS_PARAMS[1])
    fov, cut = [], []
    for n in range(c["N"]):
        q = G.transform_points(T[n].unsqueeze(0).expand(B, 4, 4).contiguous(), xyz.unsqueeze(2))[:, :, 0]
        d1 = torch.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2)
        ds = is_double_sphere(name, n)
        fov.append(((q[:, 2] + w2 * d1).abs() < 1e-5 * d1) & ds)
        cut.append((q[:, 0] < 0) & (q[:, 2].abs() < 1e-4 * q[:, 0].abs()) & (not ds))
    unit = ((grid.abs() - 1).abs() < 1e-4).any(dim=-1)
    return torch.stack(fov, dim=1), unit, torch.stack(cut, dim=1)
