"""Cases and CPU restatement (torch fp32) of the fisheye -> surrogate-view resampler (mvs_gi_amd/dropin/image_sampler.py,
csrc/resample.hip).  TEST INFRASTRUCTURE ONLY.  The restatement composes the pinned restatements of the reference's closed
forms (oracle.grid_oracle, oracle.mvsgi_oracle.bilinear_sample_zeros); tests/test_resample_host.py pins it bit for bit to
tests/golden/resample.npz, which tools/make_resample_goldens.py makes with the reference's own torch_cuda_sweep.py and
backports.py.

Definition, for one camera:
  1. surrogate ray of output pixel (i, j) of an H x W view: u = (2j+1)/W - 1, v = (2i+1)/H - 1, lon = pi u, lat = pi v / 2,
     p = (cos lat cos lon, sin lat, -cos lat sin lon), fp32 (the inverse of grid_equirect at the pixel centre)
  2. q = R p, R given as a 4 x 4 transform to transform_3D_points_torch
  3. (grid, ds_mask) = DoubleSphereSampleGridMaker(params, calib_shape).make_grid(q)
  4. valid = ds_mask & |gx| <= 1 & |gy| <= 1
  5. sampled = bilinear_grid_sample(img, grid, align_corners=False); a uint8 image is .float() / 255.0 first
  6. out = valid ? sampled : invalid_pixel_value
"""
import math

import numpy as np
import torch

from oracle import grid_oracle as G
from oracle.mvsgi_oracle import bilinear_sample_zeros

_P_AB = (-0.203, 0.589, 11.0, 11.0, 27.5, 19.5)
_P_C = (0.1, 0.45, 14.0, 15.0, 22.0, 18.0)            # alpha <= 0.5 branch of w1; 45 * 3 = 135 bytes per row
CASES = {
    # name: raw (Hr, Wr) = calib_shape, double-sphere params, (yaw, pitch, roll), out (H, W)
    "a": dict(raw=(40, 56), params=_P_AB, ypr=(0.0, 0.0, 0.0), out=(16, 64)),
    "b": dict(raw=(40, 56), params=_P_AB, ypr=(2.1, 0.3, 0.1), out=(16, 64)),
    "c": dict(raw=(37, 45), params=_P_C, ypr=(-1.0, -0.4, 0.5), out=(16, 64)),
    "b_7x30": dict(raw=(40, 56), params=_P_AB, ypr=(2.1, 0.3, 0.1), out=(7, 30)),
    "c_5x4": dict(raw=(37, 45), params=_P_C, ypr=(-1.0, -0.4, 0.5), out=(5, 4)),
}
SEEDS = {name: 100 + k for k, name in enumerate(CASES)}
INVALID_OTHER = -3.5
# arrays stored per case in resample.npz (prefix "<case>_")
STORED = ("rays", "R", "grid", "ds_mask", "valid", "img", "out", "out_neg", "smooth", "out_smooth", "mask", "out_mask")


def rotation(yaw: float, pitch: float, roll: float) -> np.ndarray:
    """R = Ry(yaw) Rx(pitch) Rz(roll), float64."""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def surrogate_rays(H: int, W: int) -> torch.Tensor:
    """Step 1 -> [3, H, W] fp32."""
    pi = torch.tensor(np.pi, dtype=torch.float32)
    u = (2 * torch.arange(W) + 1).to(torch.float32) / W - 1
    v = (2 * torch.arange(H) + 1).to(torch.float32) / H - 1
    lat, lon = torch.meshgrid(v * pi / 2, u * pi, indexing="ij")
    cl = torch.cos(lat)
    return torch.stack((cl * torch.cos(lon), torch.sin(lat), -(cl * torch.sin(lon))), dim=0)


def transform4(R) -> torch.Tensor:
    """The 3 x 3 rotation as the fp32 [1, 4, 4] transform handed to transform_3D_points_torch."""
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = torch.as_tensor(np.asarray(R, dtype=np.float64))
    return T.to(torch.float32).unsqueeze(0)


def raw_points(rays: torch.Tensor, R) -> torch.Tensor:
    """Step 2 -> [1, 3, 1, H, W]."""
    return G.transform_points(transform4(R), rays.unsqueeze(0).unsqueeze(2))


def sampler_table(rays: torch.Tensor, R, params, calib_shape):
    """Steps 2-4 -> (grid [H, W, 2], ds_mask [H, W] bool, valid [H, W] bool)."""
    grid, ds = G.grid_double_sphere(raw_points(rays, R), params, calib_shape)
    grid, ds = grid[0, 0], ds[0, 0]
    valid = ds & (grid[..., 0].abs() <= 1) & (grid[..., 1].abs() <= 1)
    return grid, ds, valid


def as_f32_chw(img: torch.Tensor) -> torch.Tensor:
    """uint8 [..., Hr, Wr, 3] -> fp32 [..., 3, Hr, Wr] as inference_pytorch.py:58-59 converts (.float() / 255.0); fp32 CHW as is."""
    if img.dtype == torch.uint8:
        return img.movedim(-1, -3).float() / 255.0
    return img


def resample(img: torch.Tensor, grid: torch.Tensor, valid: torch.Tensor, invalid: float = 0.0) -> torch.Tensor:
    """Steps 5-6 for one image (uint8 [Hr, Wr, 3] or fp32 [C, Hr, Wr]) -> [1, C, H, W]."""
    x = as_f32_chw(img).unsqueeze(0)
    s = bilinear_sample_zeros(x, grid.unsqueeze(0))
    return torch.where(valid.unsqueeze(0).unsqueeze(0), s, torch.tensor(invalid, dtype=torch.float32))


def resample_batch(imgs: torch.Tensor, grids: torch.Tensor, valids: torch.Tensor, invalid: float = 0.0) -> torch.Tensor:
    """imgs [M, ...], tables [T, ...]: image m through table m % T -> [M, C, H, W]."""
    T = grids.shape[0]
    return torch.cat([resample(imgs[m], grids[m % T], valids[m % T], invalid) for m in range(imgs.shape[0])])


def sample_mask(mask: torch.Tensor, grid: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    """sample_masks (multi_view_camera_model_dataset.py:424-438) for one fp32 [Hr, Wr] mask -> [1, H, W]."""
    m = resample((mask * 255).unsqueeze(0), grid, valid, 0.0)
    m[m > 0] = 1.0
    return m.squeeze(0)


def make_images(name: str):
    """The seeded raw inputs of a case -> (img uint8 [Hr, Wr, 3], smooth uint8 [Hr, Wr, 3], mask fp32 [Hr, Wr])."""
    Hr, Wr = CASES[name]["raw"]
    rng = np.random.default_rng(SEEDS[name])
    img = rng.integers(0, 256, size=(Hr, Wr, 3), dtype=np.uint8)
    img.reshape(-1, 3)[:256, 0] = np.arange(256, dtype=np.uint8)          # every byte value goes through the /255 table
    yy, xx = np.meshgrid(np.arange(Hr), np.arange(Wr), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, size=3)
    smooth = np.stack([127.5 + 60.0 * np.sin(2 * np.pi * xx / Wr + ph[c]) + 60.0 * np.cos(2 * np.pi * yy / Hr * (1 + 0.5 * c) + ph[c])
                       for c in range(3)], axis=-1)
    smooth = np.clip(np.rint(smooth), 0, 255).astype(np.uint8)
    mask = (rng.random((Hr, Wr)) < 0.7).astype(np.float32)
    return torch.from_numpy(img), torch.from_numpy(smooth), torch.from_numpy(mask)


def largest_step(img_u8: torch.Tensor) -> float:
    """G: the largest step between horizontally or vertically neighbouring pixels of a uint8 HWC image, / 255."""
    x = img_u8.to(torch.int32)
    return float(max((x[1:] - x[:-1]).abs().max(), (x[:, 1:] - x[:, :-1]).abs().max())) / 255.0


def edge_set(name: str, z) -> torch.Tensor:
    """Pixels [H, W] whose validity may legitimately differ between two evaluations of the closed forms: the double-sphere
    field-of-view test within 1e-5 d1 of its threshold (the rule of test_grid_generators) or a stored |g| within 1e-4 of 1."""
    c = CASES[name]
    q = raw_points(torch.from_numpy(z[f"{name}_rays"]), z[f"{name}_R"])[0, :, 0]
    d1 = torch.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    w2 = G.double_sphere_w2(c["params"][0], c["params"][1])
    g = torch.from_numpy(z[f"{name}_grid"])
    return ((q[2] + w2 * d1).abs() < 1e-5 * d1) | (((g.abs() - 1).abs() < 1e-4).any(dim=-1))
