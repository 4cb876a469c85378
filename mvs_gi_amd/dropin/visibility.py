"""Camera range images and visibility of the prediction: the predicted surface forward-rendered into each camera of the rig, the
nearest point kept per cell (a z-buffer), and per pixel and camera whether the pixel's own point is the one that camera sees.

    v, d, p, q = T_n p, g, valid_n     Reprojector's steps 1-5 for camera n at the pixel                  (csrc/reproject.hip)
    live = 0 < v <= FLT_MAX and d <= FLT_MAX
    r2 = (qx qx + qy qy) + qz qz       the squared range from camera n
    cell = the cell of camera n's Hz x Wz buffer that holds g (nearest; footprint 2: the four around it)
    z2[b, n, cell] = min over the live, valid, unmasked pixels that land there of r2;  +inf where none does
    visible_n = live and valid_n and r2 <= z2[b, n, nearest cell] * fp32((1 + tol)^2)
    n_visible = sum_n visible_n;  range = sqrt(z2)

Two calls of csrc/visibility.hip (fill + splat; test + root).  The minimum is the package's one atomic: an integer minimum on the bit
pattern of a non-negative float, which does not depend on the order the points arrive in, so the same inputs give the same bits in
every run and a captured graph replays the eager bits (include/mvsgi.h, "camera range images and visibility").
Visibility.evaluate_chain executes the definition in torch and tests/test_gpu_visibility.py compares the two bit for bit.

What the method cannot do is in DESIGN.md section 20: a cell holds the minimum over everything that lands in it, so a slanted surface
reads nearer than its own points (tol answers that, and a buffer no coarser than the map's angular sampling); single-cell splats
leave holes, and an empty cell occludes nothing; footprint 2 closes holes and occludes more; the footprint clamps at the buffer's
edge, equirectangular longitude does not wrap.

Consumers: PhotoConsistency(..., visibility=vis) keeps hidden cameras out of the fusion; `visible` goes where `valid` goes in
hip_ops.pack_cloud / CloudPacker.pack(valid=...): the colour of the lowest camera that actually sees the point, and require_colour
as "some camera sees it"; InferencePipeline(..., visibility=vis) runs the stage behind the soft-argmin, inside the captured graph.
"""
from __future__ import annotations

import torch

from .. import hip_ops as H

_FLT_MAX = float(torch.finfo(torch.float32).max)


class Visibility:
    """vis.evaluate(inv, want=hip_ops.VISIBILITY_OUTPUTS + ("z2",), out=None) -> dict of visible [B, N, H, W] bool, n_visible
    [B, H, W] uint8, range [B, N, Hz, Wz] fp32 and z2 [B, N, Hz, Wz] fp32 (the squared range image itself).

    reprojector: the dropin.Reprojector of the rig at the map's resolution (its rays, transforms, camera table and bf are used);
    zshape = (Hz, Wz) of every camera's buffer, default (2 H, W) of the map: one rule for both camera models, because the buffers of a
    rig are one tensor -- the full sphere of an equirectangular camera then has the angular sampling of the half-sphere rig map, and a
    double-sphere image, which spans less, is sampled finer; tol: the relative range a point may lie behind its cell's nearest and
    still count as seen; footprint 1 or 2; mask uint8 / bool [H, W] or [B, H, W]: the pixels that are rendered (all are tested).

    The evaluator owns one z2 per (B, H, W, device), made at the first evaluation of that shape and never replaced: a captured graph
    holds its address.  A z2 returned without `out` is valid until the next evaluation at its shape."""

    OUTPUTS = H.VISIBILITY_OUTPUTS + ("z2",)

    def __init__(self, reprojector, zshape=None, tol: float = H.VISIBILITY_TOL, footprint: int = 1, mask=None):
        for a in ("rays", "T", "cams", "bf", "out_shape", "num_cams", "reproject"):
            if not hasattr(reprojector, a):
                raise TypeError(f"Visibility: expected a dropin.Reprojector, got {type(reprojector)}")
        self.reprojector = reprojector
        self.out_shape = tuple(reprojector.out_shape)
        self.num_cams = reprojector.num_cams
        self.device = reprojector.rays.device
        self.zshape = H._zshape((2 * self.out_shape[0], self.out_shape[1]) if zshape is None else zshape)
        self.tol = float(tol)
        H.visibility_k2(self.tol)
        if footprint not in (1, 2):
            raise ValueError(f"Visibility: footprint 1 or 2, got {footprint!r}")
        self.footprint = int(footprint)
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
                raise TypeError("Visibility: mask must be a bool or uint8 tensor")
            if tuple(mask.shape[-2:]) != self.out_shape or mask.dim() not in (2, 3):
                raise AssertionError(f"Visibility: mask must be [H, W] or [B, H, W] with (H, W) = {self.out_shape}, got {tuple(mask.shape)}")
            mask = mask.to(self.device).contiguous()
        self.mask = mask
        self._bufs = {}          # (B, H, W, device) -> z2: made at first use, NEVER replaced (a captured graph holds it)

    def buffers(self, B: int, device) -> torch.Tensor:
        Hh, W = self.out_shape
        key = (B, Hh, W, torch.device(device))
        got = self._bufs.get(key)
        if got is None:
            got = self._bufs[key] = torch.empty((B, self.num_cams) + self.zshape, device=device, dtype=torch.float32)
        return got

    def release(self) -> None:
        """Drop every buffer.  Not while a captured graph that holds their addresses is still to be replayed."""
        self._bufs = {}

    def _want(self, want) -> tuple:
        want = tuple(want)
        if not want or set(want) - set(self.OUTPUTS) or len(set(want)) != len(want):
            raise ValueError(f"want: a non-empty selection of {', '.join(repr(k) for k in self.OUTPUTS)}, got {want}")
        return want

    def evaluate(self, inv, want=OUTPUTS, out=None) -> dict:
        rp = self.reprojector
        want = self._want(want)
        inv = H._dev(rp._inv(inv), "inv")
        z2 = None if out is None else out.get("z2")
        if z2 is None:
            z2 = self.buffers(int(inv.shape[0]), inv.device)
        H.camera_range(inv, rp.rays, rp.T, rp.cams, rp.bf, self.zshape, mask=self.mask, footprint=self.footprint, out=z2)
        res = {}
        rest = tuple(k for k in want if k != "z2")
        if rest:
            res = H.visibility(inv, rp.rays, rp.T, rp.cams, rp.bf, z2, tol=self.tol, want=rest, out=out)
        if "z2" in want:
            res["z2"] = z2
        return {k: res[k] for k in want}

    def evaluate_chain(self, inv, want=OUTPUTS) -> dict:
        """The definition of evaluate(), executed: Reprojector.reproject()'s xyz, grid and valid, the transform kernel for q, then
        torch, one operation per line: the squared range, the cell, scatter_reduce(amin) into a buffer of +inf (a pixel that is
        not splatted contributes +inf, which changes nothing) and the comparison.  The bits evaluate() returns, but for range,
        where torch's root stands in for the correctly rounded one.  Its first call copies the transforms to the device."""
        rp = self.reprojector
        want = self._want(want)
        inv = H._dev(rp._inv(inv), "inv")
        B, (Ho, Wo), N, (Hz, Wz) = int(inv.shape[0]), self.out_shape, self.num_cams, self.zshape
        dev = inv.device
        from .sweep_grids import transform_3D_points_torch
        r = rp.reproject(inv, want=("xyz", "grid", "valid"))
        if rp._T_dev is None:
            rp._T_dev = rp.T.to(rp.device)
        d = torch.full_like(inv, rp.bf) / inv
        live = (inv > 0) & (inv <= _FLT_MAX) & (d <= _FLT_MAX)
        inf = torch.full((), float("inf"), device=dev, dtype=torch.float32)
        mask = None if self.mask is None else (self.mask != 0).expand(B, Ho, Wo)
        k2 = torch.full((), H.visibility_k2(self.tol), device=dev, dtype=torch.float32)         # rounded to fp32 once

        def cell(g, n):
            return torch.clamp(torch.floor(((g + 1.0) * float(n)) * 0.5), 0, n - 1).to(torch.int64)

        def lower(g, n):
            return torch.floor(((g + 1.0) * float(n) - 1.0) * 0.5)

        z2 = torch.full((B * N * Hz * Wz,), float("inf"), device=dev, dtype=torch.float32)
        frame = torch.arange(B, device=dev, dtype=torch.int64).view(B, 1, 1)
        tests = []
        for n in range(N):
            q = transform_3D_points_torch(rp._T_dev[n].expand(B, 4, 4).contiguous(), r["xyz"].unsqueeze(2))[:, :, 0]
            qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
            r2 = (qx * qx + qy * qy) + qz * qz
            ok = live & r["valid"][:, n]
            gx, gy = r["grid"][:, n, ..., 0], r["grid"][:, n, ..., 1]
            zero = torch.zeros_like(gx)
            gx, gy = torch.where(ok, gx, zero), torch.where(ok, gy, zero)                        # a cell index is taken of a valid coordinate only
            base = (frame * N + n) * (Hz * Wz)
            splat = ok if mask is None else ok & mask
            src = torch.where(splat, r2, inf).reshape(-1)
            if self.footprint == 1:
                cells = [(cell(gx, Wz), cell(gy, Hz))]
            else:
                x0, y0 = lower(gx, Wz), lower(gy, Hz)
                cells = [(torch.clamp(x0 + float(dx), 0, Wz - 1).to(torch.int64), torch.clamp(y0 + float(dy), 0, Hz - 1).to(torch.int64))
                         for dy in (0, 1) for dx in (0, 1)]
            for cx, cy in cells:
                z2.scatter_reduce_(0, (base + cy * Wz + cx).reshape(-1), src, "amin", include_self=True)
            tests.append((ok, r2, base + cell(gy, Hz) * Wz + cell(gx, Wz)))
        res = dict(z2=z2.view(B, N, Hz, Wz))
        visible = torch.stack([ok & (r2 <= z2[at] * k2) for ok, r2, at in tests], dim=1)
        res["visible"] = visible
        cnt = torch.zeros((B, Ho, Wo), device=dev, dtype=torch.uint8)
        for n in range(N):
            cnt = cnt + visible[:, n].to(torch.uint8)
        res["n_visible"] = cnt
        res["range"] = torch.sqrt(res["z2"])
        return {k: res[k] for k in want}
