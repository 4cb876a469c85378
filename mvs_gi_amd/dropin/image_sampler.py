"""Raw fisheye image -> equirectangular surrogate view, the `sample_input=True` step of the reference's facade
(api/inference_pytorch.py:61-74) and the source of the rig's image-resolution masks
(support/dataset/multi_view_camera_model_dataset.py:424-438).

The reference does this with its `image_sampler` package, an empty submodule in the vendored tree.  The sampler here
is therefore DEFINED as a composition of closed forms the reference does ship, each pinned by goldens of its own code:

    surrogate ray of output pixel (i, j)        the inverse of EquirectangularSampleGridMaker.make_grid at the pixel centre
    q = R_raw_fisheye p                         transform_3D_points_torch (torch_cuda_sweep.py:385-408)
    grid, ds_mask = DoubleSphereSampleGridMaker(params, calib_shape).make_grid(q)        (torch_cuda_sweep.py:235-298)
    valid = ds_mask & |gx| <= 1 & |gy| <= 1
    out = valid ? bilinear_grid_sample(img, grid, align_corners=False) : invalid_pixel_value       (backports.py:11-86)

Bit parity with the absent package cannot be claimed (as for the camera models).  The table (grid, valid)
is built once per camera by the grid-generator kernels; the per-frame work is one launch of the resample kernel
(csrc/resample.hip) for all cameras of all frames.  No stand-in is registered under dsta_mvs.image_sampler: that
package's constructors take mvs_utils camera-model objects, which this build cannot honour.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import hip_ops as H
from .sweep_grids import DoubleSphereSampleGridMaker, transform_3D_points_torch


def equirect_surrogate_rays(H_out: int, W_out: int, device="cuda") -> torch.Tensor:
    """Rays [3, H, W] of the pixel centres of an H x W surrogate view: u = (2j+1)/W - 1, v = (2i+1)/H - 1, lon = pi u,
    lat = pi v / 2, p = (cos lat cos lon, sin lat, -cos lat sin lon); grid_equirect(p) = (u, v)."""
    rays = torch.empty((3, int(H_out), int(W_out)), device=torch.device(device), dtype=torch.float32)
    H._arg(rays, "rays", None)            # a CPU `device` ends here: the kernel takes device addresses only
    H._call("mvsgi_rays_equirect_surrogate_f32", rays.data_ptr(), int(H_out), int(W_out), H._stream_ptr(rays))
    return rays


def _as_device_image(img, device) -> torch.Tensor:
    """uint8 HWC / fp32 CHW image or a batch of either -> 4-D tensor on the device."""
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img)).to(device)
    if not isinstance(img, torch.Tensor) or img.dtype not in (torch.uint8, torch.float32):
        raise TypeError("image sampler: expected a uint8 HWC or fp32 CHW image (or a batch of either), got "
                        f"{getattr(img, 'dtype', type(img))}")
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4:
        raise AssertionError(f"image sampler: expected a 3-D image or a 4-D batch, got {tuple(img.shape)}")
    return img


class DoubleSphereToEquirectSampler:
    """sampler(img, invalid_pixel_value=0.0) -> (sampled [B, C, H, W] fp32, valid [H, W] bool) for one double-sphere camera.

    params = (xi, alpha, fx, fy, cx, cy) and calib_shape = (Hr, Wr) of the raw camera; out_shape = (H, W) of the surrogate
    view; R_raw_fisheye: 3x3 rotation taking surrogate-frame rays into the raw camera's frame; rays: any [3, H, W] ray
    table instead of the equirectangular pixel centres."""

    def __init__(self, params, calib_shape, out_shape, R_raw_fisheye, rays: Optional[torch.Tensor] = None, device="cuda"):
        self.device = torch.device(device)
        self.out_shape = (int(out_shape[0]), int(out_shape[1]))
        self.grid_maker = DoubleSphereSampleGridMaker(params, calib_shape)
        Ho, Wo = self.out_shape
        if rays is None:
            rays = equirect_surrogate_rays(Ho, Wo, self.device)
        else:
            rays = torch.as_tensor(rays).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(rays.shape) != (3, Ho, Wo):
                raise AssertionError(f"rays must be [3, {Ho}, {Wo}], got {tuple(rays.shape)}")
        R = torch.as_tensor(np.asarray(R_raw_fisheye, dtype=np.float64))
        if tuple(R.shape) != (3, 3):
            raise AssertionError(f"R_raw_fisheye must be 3 x 3, got {tuple(R.shape)}")
        T = torch.eye(4, dtype=torch.float64)
        T[:3, :3] = R
        pts = transform_3D_points_torch(T.to(torch.float32).unsqueeze(0).to(self.device), rays.view(1, 3, 1, Ho, Wo))
        grid, ds_mask = self.grid_maker.make_grid(pts)
        grid = grid.view(Ho, Wo, 2)
        valid = H.resample_validity(grid, ds_mask.view(Ho, Wo))
        self.rays, self.R, self.ds_mask = rays, R, ds_mask.view(Ho, Wo)
        self._grid, self._valid = grid, valid.view(torch.bool)
        self._table1 = (grid.unsqueeze(0), self._valid.unsqueeze(0))

    @property
    def table(self):
        """(grid [H, W, 2] fp32, valid [H, W] bool), rig constants on the device."""
        return self._grid, self._valid

    def __call__(self, img, invalid_pixel_value: float = 0.0):
        x = _as_device_image(img, self.device)
        return H.resample_bilinear(x, *self._table1, invalid_value=invalid_pixel_value), self._valid


class NoOpSampler:
    """Identity, for a camera that already delivers its surrogate view: (img, None)."""

    def __call__(self, img, invalid_pixel_value: float = 0.0):
        return img, None


def stack_tables(samplers: Sequence[DoubleSphereToEquirectSampler]):
    """(grid [T, H, W, 2], valid [T, H, W] bool) of a rig's samplers, so that one launch serves all cameras of all frames
    (hip_ops.resample_bilinear: image m uses table m % T)."""
    if not samplers or any(not isinstance(s, DoubleSphereToEquirectSampler) for s in samplers):
        raise ValueError("stack_tables: every camera needs a DoubleSphereToEquirectSampler (a rig mixing raw and surrogate "
                         "cameras is sampled camera by camera)")
    if len({(s.out_shape, s._grid.device) for s in samplers}) != 1:
        raise ValueError("stack_tables: the samplers differ in out_shape or device")
    return torch.stack([s._grid for s in samplers]).contiguous(), torch.stack([s._valid for s in samplers]).contiguous()


def sample_masks(samplers, raw_masks) -> torch.Tensor:
    """MultiViewCameraModelDataset.sample_masks (:424-438) for a rig: raw_masks[k] [Hr, Wr] (0 / 1) per camera ->
    masks [1, N, 1, H, W] fp32: m, _ = sampler(mask * 255, invalid_pixel_value=0); m[m > 0] = 1.  A NoOpSampler's mask is
    taken as it is."""
    if len(samplers) != len(raw_masks):
        raise AssertionError(f"{len(samplers)} samplers for {len(raw_masks)} masks")
    out = []
    for s, m in zip(samplers, raw_masks):
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(np.ascontiguousarray(m))
        dev = s.device if isinstance(s, DoubleSphereToEquirectSampler) else m.device
        m = m.to(device=dev, dtype=torch.float32)
        m = m.reshape(1, 1, *m.shape[-2:])
        if not isinstance(s, NoOpSampler):
            m, _ = s(m * 255, invalid_pixel_value=0)
            m[m > 0] = 1.0
        out.append(m[0])
    return torch.stack(out).unsqueeze(0)
