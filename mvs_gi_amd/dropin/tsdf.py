"""Volumetric fusion of the predicted inverse distance: every prediction of a sequence integrated into a world-fixed truncated
signed distance volume that rolls with the rig, and that volume ray-cast back into the rig's view.

    state vol [B, Nz, Ny, Nx, 2]       per voxel (f, w): the truncated signed distance in units of trunc (positive in front of the
                                       surface) and the accumulated weight; TOROIDAL: world voxel i lives in slot i mod N, the volume
                                       covers origin <= i < origin + N, and re-centring is a change of origin, not a copy
    integrate                          per slot: its world voxel, cleared if it scrolled in since the last integrate; the centre in
                                       the rig frame, its cell of the panorama (the temporal splat's step 4), sdf = bf / inv - r,
                                       a running weighted mean with weight trunc^2 / (trunc^2 + sigma_d^2)          (csrc/tsdf.hip)
    raycast                            per pixel of the panorama: a fixed-step march through the nearest voxels, the first front-face
                                       zero crossing between two valid samples, interpolated linearly -> inv = bf / t*

The definition is stated in include/mvsgi.h ("volumetric fusion") and DESIGN.md section 24, which also says what the method cannot
do: nearest-cell and nearest-voxel look-ups (no bilinear or trilinear interpolation), one truncation band at every range, free space
carved along every ray (a wrong near prediction erases what lies behind it until it is observed again), no occlusion test (pass the
visibility stage's `visible` as `mask` if wanted).  TsdfVolume.integrate_chain / raycast_chain execute the definition in torch, one
operation per line, and tests/test_gpu_tsdf.py compares the bits.

The pose and the origins are read from device memory by the launches: set_pose() before a replay moves the rig of a captured step.
"""
from __future__ import annotations

import math

import torch

from .. import hip_ops as H
from .reproject import panorama_cell, pose_arg

_FLT_MAX = H.TSDF_FLT_MAX


class TsdfVolume:
    """vol = TsdfVolume(reprojector, dims=(Nx, Ny, Nz), voxel=0.1); vol.integrate(inv, std=None, mask=None, P=None);
    vol.raycast(P=None, want=("inv", "weight", "steps")) -> dict of inv, weight [B, H, W] fp32 and steps [B, H, W] int32.

    reprojector: the dropin.Reprojector of the rig at the map's resolution, built from the rig camera's long_range / lat_range (its
    rays, bf and out_shape are used; one built from a bare ray table is refused: the inverse of the ray table has no closed form
    then); dims: voxels per axis; voxel: their edge; trunc: the truncation band (default 4 voxel); w_max: where the weight saturates;
    r_range: the ranges a voxel is integrated at; w_min: the weight a sample needs to count in the ray-cast; march = (t0, t_max,
    step): the ray-cast's samples t0, t0 + step, ... <= t_max (default: from one voxel to half the volume's diagonal in steps of
    voxel / 2; at most 4096 samples).

    B independent sequences.  The volume owns, per (B, device), vol, the poses P (rig -> world) and T (its rigid inverse), origin,
    origin_prev and the ray-cast's outputs, made at the first use and never replaced: a captured graph holds their addresses.
    |origin| < 2^23 voxels is the caller's to keep."""

    OUTPUTS = H.TSDF_OUTPUTS

    def __init__(self, reprojector, dims, voxel: float, trunc=None, w_max: float = 64.0, r_range=(0.0, float("inf")), w_min: float = 1.0,
                 march=None):
        for a in ("rays", "bf", "out_shape", "reproject", "long_range", "lat_range"):
            if not hasattr(reprojector, a):
                raise TypeError(f"TsdfVolume: expected a dropin.Reprojector, got {type(reprojector)}")
        if reprojector.long_range is None or reprojector.lat_range is None:
            raise ValueError("TsdfVolume: the reprojector was built from a ray table; the stage needs the rig camera's long_range and "
                             "lat_range (the inverse of an arbitrary ray table has no closed form)")
        self.reprojector = reprojector
        self.out_shape = tuple(reprojector.out_shape)
        self.device = reprojector.rays.device
        self.affine = H.temporal_affine(reprojector.long_range, reprojector.lat_range, self.out_shape)
        try:
            self.dims = tuple(int(v) for v in dims)
            if len(self.dims) != 3 or any(int(v) != v for v in dims):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"TsdfVolume: dims = (Nx, Ny, Nz), whole numbers, got {dims!r}") from None
        H.tsdf_dims(1, *self.dims)
        H._pano_map("volumetric fusion", 31, 1, *self.out_shape)
        self.voxel = H._tsdf_scalar(voxel, "voxel")
        self.trunc = H._tsdf_scalar(4.0 * self.voxel if trunc is None else trunc, "trunc")
        H._tsdf_scalar(self.trunc * self.trunc, "trunc^2")
        self.w_max = H._tsdf_scalar(w_max, "w_max")
        try:
            r_min, r_max = (float(v) for v in r_range)
        except (TypeError, ValueError):
            raise ValueError(f"TsdfVolume: r_range = (r_min, r_max), got {r_range!r}") from None
        r_max = min(r_max, _FLT_MAX)
        if not 0.0 <= r_min < r_max:
            raise ValueError(f"TsdfVolume: r_range: 0 <= r_min < r_max, got {r_range!r}")
        self.r_range = (r_min, r_max)
        self.w_min = float(w_min)
        if not math.isfinite(self.w_min):
            raise ValueError(f"TsdfVolume: w_min must be finite, got {w_min!r}")
        if march is None:
            march = (self.voxel, 0.5 * self.voxel * math.sqrt(sum(n * n for n in self.dims)), None)
        try:
            t0, t_max, step = march
            t0, t_max, step = float(t0), float(t_max), 0.5 * self.voxel if step is None else float(step)
        except (TypeError, ValueError):
            raise ValueError(f"TsdfVolume: march = (t0, t_max, step), got {march!r}") from None
        if not (0.0 <= t0 <= t_max < float("inf") and 0.0 < step < float("inf")):
            raise ValueError(f"TsdfVolume: march: 0 <= t0 <= t_max < inf and 0 < step < inf, got {march!r}")
        self.t0, self.step, self.K = t0, step, int(math.floor((t_max - t0) / step)) + 1
        if not 1 <= self.K <= H.TSDF_MAX_STEPS:
            raise ValueError(f"TsdfVolume: march: {self.K} samples (at most {H.TSDF_MAX_STEPS}); a larger step or a nearer t_max")
        self._bufs = {}          # (B, device) -> dict: made at first use, NEVER replaced (a captured graph holds them)

    # ---- what the volume owns ----
    def buffers(self, B: int, device=None) -> dict:
        """-> dict(vol; P, T [B, 4, 4]; origin, origin_prev [B, 3] int32; out: the ray-cast's outputs; half, dims: N // 2 and N as
        device constants)"""
        device = torch.device(self.device if device is None else device)
        key = (int(B), device)
        got = self._bufs.get(key)
        if got is None:
            Nx, Ny, Nz = self.dims
            Hh, W = self.out_shape
            H.tsdf_dims(int(B), Nx, Ny, Nz)
            eye = torch.eye(4, device=device, dtype=torch.float32).repeat(int(B), 1, 1)
            half = torch.tensor([Nx // 2, Ny // 2, Nz // 2], device=device, dtype=torch.int32)
            kinds = dict(inv=torch.float32, weight=torch.float32, steps=torch.int32)
            got = self._bufs[key] = dict(
                vol=torch.empty((int(B), Nz, Ny, Nx, 2), device=device, dtype=torch.float32), P=eye.clone(), T=eye.clone(),
                origin=(-half).repeat(int(B), 1).contiguous(), origin_prev=(-half).repeat(int(B), 1).contiguous(), half=half,
                dims=torch.tensor([Nx, Ny, Nz], device=device, dtype=torch.int32),
                out={k: torch.empty((int(B), Hh, W), device=device, dtype=d) for k, d in kinds.items()})
            self._clear(got)
        return got

    @staticmethod
    def _clear(bufs) -> None:
        bufs["vol"][..., 0] = 1.0
        bufs["vol"][..., 1] = 0.0

    def release(self) -> None:
        """Drop every buffer, the volumes with them.  Not while a captured graph that holds their addresses is still to be replayed."""
        self._bufs = {}

    def reset(self) -> None:
        """Every sequence starts over: every voxel holds (1, 0), free and never observed."""
        for bufs in self._bufs.values():
            self._clear(bufs)

    @staticmethod
    def origin_of(t: torch.Tensor, voxel: float, half: torch.Tensor) -> torch.Tensor:
        """The coverage that centres the volume on the rig: floor(t / voxel) - N // 2 per axis, t [B, 3] fp32 -> [B, 3] int32 (torch
        operations on t's device; the floor makes a negative position round away from zero, as the floored modulus needs)."""
        return torch.floor(t / voxel).to(torch.int32) - half

    def set_pose(self, P, B=None) -> None:
        """Stage the rig's pose in the world for the next integrate(P=None) / raycast(P=None) -- the calls a captured graph replays.
        P: [B, 4, 4], or [4, 4] for every sequence (then B, default 1, names the buffers), on the host or the device.  Writes P, its
        rigid inverse T (R^T, -R^T t) and origin = floor(t / voxel) - N // 2 with torch operations on the device only."""
        P = pose_arg(P, B, "P")
        bufs = self.buffers(P.shape[0])
        Pd = bufs["P"]
        Pd.copy_(P, non_blocking=True)
        Rt = Pd[:, :3, :3].transpose(1, 2)
        t = Pd[:, :3, 3]
        bufs["T"][:, :3, :3] = Rt
        bufs["T"][:, :3, 3] = -(Rt * t.unsqueeze(1)).sum(-1)
        bufs["origin"].copy_(self.origin_of(t, self.voxel, bufs["half"]))

    def _want(self, want) -> tuple:
        return H._wanted(want, self.OUTPUTS)

    def _measurement(self, inv, std, mask):
        rp = self.reprojector
        inv = H._pano_plane(rp._inv(inv), "inv", None, None)
        shape = tuple(int(v) for v in inv.shape)
        if std is not None:
            std = H._pano_plane(std, "std", shape, inv.device)
        if mask is not None:
            mask = H._pano_plane(mask, "mask", shape, inv.device, torch.uint8)
        return inv, std, mask

    # ---- the stage ----
    def integrate(self, inv, std=None, mask=None, P=None, r_out=None) -> torch.Tensor:
        """One prediction of every sequence into the volume: P (None: the pose set_pose() staged, identity before any), the launch,
        then origin_prev := origin.  inv [B, H, W] or [B, 1, H, W]; std likewise (its standard deviation) or None; mask [B, H, W]
        uint8 / bool or None.  After the first call at a batch size nothing is allocated, and a call with P=None can be captured.
        -> vol"""
        inv, std, mask = self._measurement(inv, std, mask)
        B = int(inv.shape[0])
        bufs = self.buffers(B, inv.device)
        if P is not None:
            self.set_pose(pose_arg(P, B, "P"))
        H.tsdf_integrate(bufs["vol"], inv, bufs["T"], bufs["origin"], bufs["origin_prev"], self.reprojector.bf, self.affine, self.voxel,
                         self.trunc, self.w_max, self.r_range, std=std, mask=mask, r_out=r_out)
        bufs["origin_prev"].copy_(bufs["origin"])
        return bufs["vol"]

    def raycast(self, P=None, want=OUTPUTS, B: int = 1) -> dict:
        """The volume ray-cast into the view of the rig at P (None: the staged pose; B names the buffers then).  The coverage is the
        one of the last integrate (origin_prev): a pose staged since then moves the rays, not the volume.  -> dict of `want`, the
        volume's own tensors, valid until the next raycast at this batch size."""
        want = self._want(want)
        if P is not None:
            P = pose_arg(P, None if torch.as_tensor(P).dim() == 3 else B, "P")
            B = int(P.shape[0])
            self.set_pose(P)
        bufs = self.buffers(B)
        return H.tsdf_raycast(bufs["vol"], self.reprojector.rays, bufs["P"], bufs["origin_prev"], self.reprojector.bf, self.voxel, self.t0,
                              self.step, self.K, self.w_min, want=want, out=bufs["out"])

    # ---- the definition, executed ----
    def integrate_chain(self, vol, inv, std=None, mask=None, T=None, origin=None, origin_prev=None, r=None) -> dict:
        """mvsgi_tsdf_integrate_f32's definition, executed: the voxel centres as a dense tensor through the transform kernel and the
        equirectangular grid kernel, then torch, one operation per line.  vol is not written.  T, origin, origin_prev default to the
        staged ones; r [B, Nz, Ny, Nx] replaces the chain's own root (torch's stands in for the correctly rounded one, so the tests
        feed the device's).  -> dict(vol: the new volume; r; cx, cy: the cell of every voxel as floats; hit: the voxels updated)"""
        from .sweep_grids import EquirectangularSampleGridMaker, transform_3D_points_torch
        inv, std, mask = self._measurement(inv, std, mask)
        dev = inv.device
        B, (Ho, Wo), (Nx, Ny, Nz) = int(inv.shape[0]), self.out_shape, self.dims
        bufs = self.buffers(B, dev)
        T = bufs["T"] if T is None else pose_arg(T, B, "P").to(dev).contiguous()
        origin = (bufs["origin"] if origin is None else origin).to(dev)
        origin_prev = (bufs["origin_prev"] if origin_prev is None else origin_prev).to(dev)
        c32 = lambda c: torch.full((), c, device=dev, dtype=torch.float32)              # each rounded to fp32 once
        vs, trunc, t2, w_max, bf = c32(self.voxel), c32(self.trunc), c32(self.trunc * self.trunc), c32(self.w_max), c32(self.reprojector.bf)
        r_min, r_max = c32(self.r_range[0]), c32(self.r_range[1])
        full = (B, Nz, Ny, Nx)
        views = ((1, 1, 1, Nx), (1, 1, Ny, 1), (1, Nz, 1, 1))
        fresh = torch.zeros(full, device=dev, dtype=torch.bool)
        centre = []
        for a, N in enumerate(self.dims):                                               # step 1
            s = torch.arange(N, device=dev, dtype=torch.int32).view(views[a])
            o = origin[:, a].view(B, 1, 1, 1)
            op = origin_prev[:, a].view(B, 1, 1, 1)
            i = o + torch.remainder(s - o, N)
            fresh = fresh | (i < op) | (i >= op + N)
            c = i.to(torch.float32) + 0.5                                               # step 2
            c = c * vs
            centre.append(c.expand(full))
        f = torch.where(fresh, torch.ones_like(vol[..., 0]), vol[..., 0])
        w = torch.where(fresh, torch.zeros_like(vol[..., 1]), vol[..., 1])
        pts = torch.stack(centre, 1).reshape(B, 3, 1, Nz, Ny * Nx).contiguous()
        q = transform_3D_points_torch(T, pts)
        g = EquirectangularSampleGridMaker().make_grid(q)[:, 0].reshape(B, Nz, Ny, Nx, 2)
        qx, qy, qz = (q[:, k, 0].reshape(full) for k in range(3))
        r2 = (qx * qx + qy * qy) + qz * qz
        ok = (r2 > 0) & (r2 <= _FLT_MAX)
        rr = torch.sqrt(r2) if r is None else r
        ok = ok & (rr >= r_min) & (rr <= r_max)
        fx, fy, inside = panorama_cell(g, self.affine, self.out_shape)                  # step 3
        ok = ok & inside
        zero = torch.zeros_like(fx)
        cell = (torch.where(ok, fy, zero).to(torch.int64) * Wo + torch.where(ok, fx, zero).to(torch.int64)).view(B, -1)
        m = torch.gather(inv.reshape(B, -1), 1, cell).view(full)                        # step 4
        if mask is not None:
            ok = ok & (torch.gather(mask.reshape(B, -1), 1, cell).view(full) != 0)
        d = bf / m
        ok = ok & (m > 0) & (m <= _FLT_MAX) & (d <= _FLT_MAX)
        sdf = d - rr                                                                    # step 5
        ok = ok & ~(sdf < -trunc)
        obs = torch.minimum(sdf, trunc) / trunc
        if std is not None:                                                             # step 6
            sd = torch.gather(std.reshape(B, -1), 1, cell).view(full)
            sig = sd * d / m
            w_obs = t2 / (t2 + sig * sig)
            ok = ok & (w_obs > 0) & (w_obs <= 1)
        else:
            w_obs = torch.ones_like(w)
        Wn = w + w_obs                                                                  # step 7
        f_new = (f * w + obs * w_obs) / Wn
        w_new = torch.minimum(Wn, w_max)
        out = torch.stack([torch.where(ok, f_new, f), torch.where(ok, w_new, w)], -1)   # step 8
        return dict(vol=out, r=rr, cx=fx, cy=fy, hit=ok)

    def raycast_chain(self, vol, P=None, origin=None) -> dict:
        """mvsgi_tsdf_raycast_f32's definition, executed in torch: the rays moved by the transform kernel (P without its translation),
        then a Python loop over the K samples on dense planes, one operation per line.  -> dict of OUTPUTS"""
        from .sweep_grids import transform_3D_points_torch
        dev = vol.device
        B, (Ho, Wo), (Nx, Ny, Nz) = int(vol.shape[0]), self.out_shape, self.dims
        bufs = self.buffers(B, dev)
        P = bufs["P"] if P is None else pose_arg(P, B, "P").to(dev).contiguous()
        origin = (bufs["origin_prev"] if origin is None else origin).to(dev)
        c32 = lambda c: torch.full((), c, device=dev, dtype=torch.float32)
        t0, step, inv_vs, w_min, bf = c32(self.t0), c32(self.step), c32(1.0 / self.voxel), c32(self.w_min), c32(self.reprojector.bf)
        R = P.clone()
        R[:, :3, 3] = 0.0
        rays = self.reprojector.rays.to(dev).unsqueeze(0).expand(B, 3, Ho, Wo).unsqueeze(2).contiguous()
        dirs = transform_3D_points_torch(R, rays)[:, :, 0]                               # step 1
        o = P[:, :3, 3].reshape(B, 3, 1, 1)
        lo = origin.to(torch.float32).view(B, 3, 1, 1)
        hi = (origin + bufs["dims"]).to(torch.float32).view(B, 3, 1, 1)
        n = bufs["dims"].to(torch.int64).view(1, 3, 1, 1)
        pairs = vol.reshape(B, -1, 2)
        plane = (B, Ho, Wo)
        inv = torch.zeros(plane, device=dev, dtype=torch.float32)
        weight = torch.zeros(plane, device=dev, dtype=torch.float32)
        steps = torch.full(plane, self.K, device=dev, dtype=torch.int32)
        done = torch.zeros(plane, device=dev, dtype=torch.bool)
        pf = torch.zeros(plane, device=dev, dtype=torch.float32)
        pv = torch.zeros(plane, device=dev, dtype=torch.bool)
        for k in range(self.K):                                                         # step 2
            tk = t0 + c32(float(k)) * step
            p = o + dirs * tk
            g = torch.floor(p * inv_vs)
            inside = ((g >= lo) & (g < hi)).all(1)
            s = torch.remainder(torch.where(inside.unsqueeze(1), g, torch.zeros_like(g)).to(torch.int64), n)
            slot = ((s[:, 2] * Ny + s[:, 1]) * Nx + s[:, 0]).view(B, -1)
            f = torch.gather(pairs[..., 0], 1, slot).view(plane)
            w = torch.gather(pairs[..., 1], 1, slot).view(plane)
            valid = inside & (w >= w_min)
            cross = valid & pv & (pf > 0) & (f <= 0) & ~done                            # step 3
            tp = t0 + c32(float(k - 1)) * step
            ts = tp + step * (pf / (pf - f))
            inv = torch.where(cross, bf / ts, inv)
            weight = torch.where(cross, w, weight)
            steps = torch.where(cross, torch.full_like(steps, k), steps)
            done = done | cross
            pf, pv = f, valid
        return dict(inv=inv, weight=weight, steps=steps)
