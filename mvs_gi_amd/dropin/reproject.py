"""Back-projection of the predicted inverse distance: SphericalSweepStereo._create_warped_inputs
(dsta_mvs/model/mvs_model/spherical_sweep_stereo.py:417-471) for a rig of double-sphere / equirectangular cameras.

    dist = bf / inv_dist                              :422
    xyz = rays of the rig camera * dist               :435      the point cloud, in the rig camera's frame
    q = T_n xyz                                       :450-451  T_n = inverse camera pose (x [R_raw_fisheye | 0] for a raw fisheye camera)
    grid = camera n's projection of q                 :454      the grid makers of dropin/sweep_grids.py
    valid = in the field of view & |gx| <= 1 & |gy| <= 1        the rule of the image sampler (dropin/image_sampler.py)
    warped = valid ? bilinear_grid_sample(img_n, grid) : invalid_pixel_value            :461-465

One launch of csrc/reproject.hip for all frames and cameras; its result is the bits of the chain of the separate kernels
(mvsgi_rays_panorama_f32 -> multiply -> mvsgi_transform_points_f32 -> make_grid -> mvsgi_resample_validity_u8 ->
mvsgi_resample_bilinear_*), which Reprojector.reproject_chain executes: the definition the tests and tools/reproject_probe.py
compare the kernel with.  The reference projects through mvs_utils camera models and samples with F.grid_sample; here the
projection is the reference's own grid makers and the sampler its backports.bilinear_grid_sample, as everywhere in this build.

The rig (poses, camera parameters, rays) is fixed at construction: the transforms and the camera table travel in the kernel's
arguments, so a captured graph holds their values.  Another rig is another Reprojector, and a new capture.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import hip_ops as H
from .sweep_grids import DoubleSphereSampleGridMaker, EquirectangularSampleGridMaker, RayMaker_UEPanorama, transform_3D_points_torch

MODEL_DOUBLE_SPHERE, MODEL_EQUIRECT = 0, 1


def compose_transforms(poses, R_raw=None) -> torch.Tensor:
    """-> T [N, 4, 4] fp32 on the host: the fp32 image of the float64 inverse camera pose (make_sweep_grid,
    multi_view_camera_model_dataset.py:505), left-multiplied in float64 by [R_raw_fisheye | 0] where R_raw[n] is given."""
    N = len(poses)
    if R_raw is None:
        R_raw = [None] * N
    if len(R_raw) != N:
        raise AssertionError(f"{len(R_raw)} raw-camera rotations for {N} poses")
    out = []
    for pose, R in zip(poses, R_raw):
        pose = torch.as_tensor(np.asarray(pose, dtype=np.float64)) if not isinstance(pose, torch.Tensor) else pose.detach().cpu()
        if tuple(pose.shape) != (4, 4):
            raise AssertionError(f"a camera pose must be 4 x 4, got {tuple(pose.shape)}")
        T = torch.linalg.inv(pose.to(torch.float64))
        if R is not None:
            R = torch.as_tensor(np.asarray(R.detach().cpu() if isinstance(R, torch.Tensor) else R, dtype=np.float64))
            if tuple(R.shape) != (3, 3):
                raise AssertionError(f"R_raw_fisheye must be 3 x 3, got {tuple(R.shape)}")
            R4 = torch.eye(4, dtype=torch.float64)
            R4[:3, :3] = R
            T = R4 @ T
        out.append(T.to(torch.float32))
    return torch.stack(out).contiguous()


def camera_table(grid_makers) -> torch.Tensor:
    """-> [N, hip_ops.REPROJECT_CAM_FLOATS] fp32 on the host: model id, xi, alpha, fx, fy, cx, cy, w2, calib_h - 1, calib_w - 1
    (zeros behind the id of an equirectangular camera)."""
    rows = []
    for gm in grid_makers:
        if isinstance(gm, DoubleSphereSampleGridMaker):
            rows.append([MODEL_DOUBLE_SPHERE, gm.xi, gm.alpha, gm.fx, gm.fy, gm.cx, gm.cy, gm.w2, gm.calib_shape[0] - 1, gm.calib_shape[1] - 1])
        elif isinstance(gm, EquirectangularSampleGridMaker):
            rows.append([MODEL_EQUIRECT] + [0.0] * (H.REPROJECT_CAM_FLOATS - 1))
        else:
            raise TypeError(f"grid maker {type(gm).__name__}: expected a DoubleSphereSampleGridMaker or an EquirectangularSampleGridMaker")
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32).contiguous()


def pose_arg(T, B=None, name: str = "T") -> torch.Tensor:
    """A pose argument of the stages that read it from device memory: [B, 4, 4] fp32, or [4, 4] for every one of B (default 1)
    sequences; name: the argument's letter in the messages"""
    T = torch.as_tensor(T)
    if T.dim() == 2 and tuple(T.shape) == (4, 4):
        T = T.unsqueeze(0).expand(1 if B is None else int(B), 4, 4)
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4) or (B is not None and T.shape[0] != B):
        raise AssertionError(f"{name} must be [{'B' if B is None else B}, 4, 4] (or [4, 4]), got {list(T.shape)}")
    if T.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {T.dtype}")
    return T


def panorama_cell(g: torch.Tensor, affine, hw) -> tuple:
    """The cell of the rig panorama (H, W) = hw an equirectangular grid coordinate g [..., 2] lands in (include/mvsgi.h, "temporal
    fusion", step A4; csrc/panorama_map.hpp), one operation per line: the affine map of hip_ops.temporal_affine(), floor, the column
    wrapped once where the longitude closes, the test.  -> fx, fy (whole floats; column, row), inside"""
    Ho, Wo = hw
    au, bu, av, bv = (torch.full((), c, device=g.device, dtype=torch.float32) for c in affine[:4])   # each rounded to fp32 once
    u = g[..., 0] * au + bu
    v = g[..., 1] * av + bv
    fx = torch.floor(u)
    fy = torch.floor(v)
    if affine[4]:
        fx = torch.where(fx < 0, fx + float(Wo), torch.where(fx >= float(Wo), fx - float(Wo), fx))
    inside = (fx >= 0) & (fx < float(Wo)) & (fy >= 0) & (fy < float(Ho))
    return fx, fy, inside


class Reprojector:
    """reprojector(inv, imgs, invalid_pixel_value=0.0) -> (xyz [B, 3, H, W], warped [B, N, C, H, W], valid [B, N, H, W] bool);
    reprojector.point_cloud(inv) -> xyz.

    grid_makers: one DoubleSphereSampleGridMaker / EquirectangularSampleGridMaker per camera; poses: the cameras' 4 x 4 poses in
    the rig camera's frame; out_shape = (H, W) of the inverse-distance map; long_range / lat_range: the rig camera's ranges in
    radians (its rays are RayMaker_UEPanorama([1.0], ...) at out_shape); bf: 96 for the regressor's raw output, 1 for
    InferencePipeline's metric map; rays: any [3, H, W] table instead; R_raw: per camera None or the 3 x 3 R_raw_fisheye of a
    camera whose images are its raw frames (DoubleSphereToEquirectSampler)."""

    def __init__(self, grid_makers, poses, out_shape, long_range=None, lat_range=None, bf: float = 96.0,
                 rays: Optional[torch.Tensor] = None, R_raw: Optional[Sequence] = None, device="cuda"):
        self.device = torch.device(device)
        self.grid_makers = list(grid_makers)
        N = len(self.grid_makers)
        if len(poses) != N:
            raise AssertionError(f"{len(poses)} poses for {N} grid makers")
        if not 1 <= N <= H.sweep_max_cams():
            raise ValueError(f"Reprojector: {N} cameras (1 ... {H.sweep_max_cams()} are supported)")
        self.num_cams = N
        self.out_shape = (int(out_shape[0]), int(out_shape[1]))
        self.bf = float(bf)
        self.cams = camera_table(self.grid_makers)
        self.T = compose_transforms(poses, R_raw)
        self._T_dev = None               # reproject_chain's device copy, made at its first call
        Ho, Wo = self.out_shape
        # the ranges the rays were made from (TemporalFusion inverts them in closed form); None with a caller's ray table
        self.long_range = self.lat_range = None
        if rays is None:
            if long_range is None or lat_range is None:
                raise ValueError("Reprojector: long_range and lat_range of the rig camera, or a ray table")
            rm = RayMaker_UEPanorama(np.ones(1, np.float32), long_range, lat_range, device=self.device)
            self.long_range, self.lat_range = rm.long_range, rm.lat_range
            rays = rm.make_rays_for_candidates(self.out_shape).view(3, Ho, Wo)
        else:
            rays = torch.as_tensor(rays).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(rays.shape) != (3, Ho, Wo):
                raise AssertionError(f"rays must be [3, {Ho}, {Wo}], got {tuple(rays.shape)}")
        self.rays = rays

    @classmethod
    def from_samplers(cls, samplers, poses, out_shape, long_range=None, lat_range=None, bf: float = 96.0, rays=None, device="cuda"):
        """The rig of InferencePipeline(samplers=...): camera parameters, calib_shape and R_raw_fisheye of each
        DoubleSphereToEquirectSampler; the images are then the cameras' raw frames."""
        from .image_sampler import DoubleSphereToEquirectSampler
        if any(not isinstance(s, DoubleSphereToEquirectSampler) for s in samplers):
            raise TypeError("Reprojector.from_samplers: every camera needs a DoubleSphereToEquirectSampler")
        return cls([s.grid_maker for s in samplers], poses, out_shape, long_range, lat_range, bf, rays=rays,
                   R_raw=[s.R for s in samplers], device=device)

    def _inv(self, inv: torch.Tensor) -> torch.Tensor:
        if not isinstance(inv, torch.Tensor):
            raise TypeError(f"inv: expected a torch.Tensor, got {type(inv)}")
        if inv.dim() == 4 and inv.shape[1] == 1:
            inv = inv.squeeze(1)
        if inv.dim() != 3 or tuple(inv.shape[1:]) != self.out_shape:
            raise AssertionError(f"inv must be [B, {self.out_shape[0]}, {self.out_shape[1]}] or [B, 1, ...], got {tuple(inv.shape)}")
        return inv

    def _imgs(self, imgs: torch.Tensor, B: int) -> torch.Tensor:
        if not isinstance(imgs, torch.Tensor):
            raise TypeError(f"imgs: expected a torch.Tensor, got {type(imgs)}")
        if imgs.dim() == 5:
            if tuple(imgs.shape[:2]) != (B, self.num_cams):
                raise AssertionError(f"imgs must be [{B}, {self.num_cams}, ...], got {tuple(imgs.shape)}")
            imgs = imgs.flatten(0, 1)
        if imgs.dim() != 4 or imgs.shape[0] != B * self.num_cams:
            raise AssertionError(f"imgs must hold {B} x {self.num_cams} images ([B*N, Hr, Wr, 3] uint8 or [B*N, C, Hr, Wr] fp32), got "
                                 f"{tuple(imgs.shape)}")
        return imgs

    def reproject(self, inv, imgs=None, invalid_pixel_value: float = 0.0, want=("xyz", "warped", "valid"), out=None) -> dict:
        """The general form: any selection of 'xyz', 'warped', 'valid', 'grid'; `out` tensors are written in place."""
        inv = self._inv(inv)
        if imgs is not None:
            imgs = self._imgs(imgs, inv.shape[0])
        return H.reproject(inv, self.rays, self.T, self.cams, self.bf, imgs=imgs, invalid_value=invalid_pixel_value, want=want, out=out)

    def reproject_chain(self, inv, imgs=None, invalid_pixel_value: float = 0.0, want=("xyz", "warped", "valid")) -> dict:
        """The definition of reproject(), executed: the separate launches whose bits the fused kernel returns, same arguments
        (but `out`) and same dictionary.  Its first call copies the transforms to the device; later calls can be captured."""
        inv = H._dev(self._inv(inv), "inv")
        B, (Ho, Wo), N = inv.shape[0], self.out_shape, self.num_cams
        if self._T_dev is None:
            self._T_dev = self.T.to(self.device)
        xyz = self.rays.unsqueeze(0) * (torch.full_like(inv, self.bf) / inv).unsqueeze(1)          # an IEEE division, then :435
        grids, valids = [], []
        for n, gm in enumerate(self.grid_makers):
            g = gm.make_grid(transform_3D_points_torch(self._T_dev[n].expand(B, 4, 4).contiguous(), xyz.unsqueeze(2)))
            g, fov = g if isinstance(g, tuple) else (g, torch.ones((B, 1, Ho, Wo), dtype=torch.bool, device=self.device))
            grids.append(g[:, 0])
            valids.append(H.resample_validity(g, fov)[:, 0].view(torch.bool))
        res = dict(xyz=xyz, grid=torch.stack(grids, dim=1), valid=torch.stack(valids, dim=1))
        if "warped" in want:
            warped = H.resample_bilinear(self._imgs(imgs, B), res["grid"].view(B * N, Ho, Wo, 2), res["valid"].view(B * N, Ho, Wo),
                                         invalid_value=invalid_pixel_value)
            res["warped"] = warped.view(B, N, -1, Ho, Wo)
        return {k: res[k] for k in want}

    def point_cloud(self, inv) -> torch.Tensor:
        return self.reproject(inv, want=("xyz",))["xyz"]

    def __call__(self, inv, imgs, invalid_pixel_value: float = 0.0):
        r = self.reproject(inv, imgs, invalid_pixel_value)
        return r["xyz"], r["warped"], r["valid"]
