"""Temporal fusion of the predicted inverse distance: the last fused map of a sequence warped to the rig's new pose and fused with the
new prediction, per pixel.

    state (inv, var, age)              the previous fused inverse distance, its variance, and for how many steps the pixel has been
                                       confirmed (0: it holds nothing)
    A, splat                           Reprojector's back-projection of the state, q = T p, the equirectangular projection of q into
                                       the rig panorama's own cells; per cell the nearest source survives, WITH ITS INDEX:
                                       zkey = min((bits(r2) << 32) | source index), an integer minimum            (csrc/temporal.hip)
    B, resolve and fuse                warped_inv = bf / sqrt(r2), var_w = var[src] (warped_inv / inv[src])^4 + q_var; with the
                                       measurement m, var_m = std^2: a Kalman update where (m - warped_inv)^2 <= gate^2 (var_w + var_m),
                                       the measurement alone where not (occlusion, motion, a wrong prediction) or where no source
                                       landed, the prior alone (age not incremented) where the measurement is not usable

The definition is stated in include/mvsgi.h ("temporal fusion") and DESIGN.md section 23, which also says what the method cannot do:
single-cell splats leave holes when the rig moves towards a surface (such a pixel takes the measurement alone), a cell holds the
nearest of everything that lands in it, the variance is carried along the ray only (the cosine between the old and the new ray is
dropped), and the prior is as wrong as the previous prediction was.  TemporalFusion.evaluate_chain executes the definition in torch
and tests/test_gpu_temporal.py compares the two bit for bit.

The integer minimum does not depend on the order the points arrive in, so the same inputs give the same bits in every run, and a
captured graph replays the eager bits.  The pose is read from device memory by the launch: set_pose() before a replay moves the map.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip_ops as H
from .reproject import panorama_cell, pose_arg

_FLT_MAX = float(torch.finfo(torch.float32).max)
_LOW32 = 0xFFFFFFFF


class TemporalFusion:
    """tf.step(inv, std=None, T=None, want=("fused", "var", "age")) -> dict of fused, var [B, H, W] fp32, age [B, H, W] uint8 (the new
    state), and on request warped_inv, warped_var fp32, src int32 (the prior and the pixel it came from) and zkey int64.

    reprojector: the dropin.Reprojector of the rig at the map's resolution, built from the rig camera's long_range / lat_range (its rays,
    bf and out_shape are used; one built from a bare ray table is refused: the inverse of the ray table has no closed form then);
    gate: how many standard deviations prior and measurement may differ and still be fused; q_var >= 0: the process noise added to
    the warped variance every step; meas_std > 0: the measurement's standard deviation where step() gets no `std` map.

    B independent sequences, one step per call.  The evaluator owns one state (inv, var, age), one zkey, one pose tensor and one set of
    outputs per (B, H, W, device), made at the first use of that shape and never replaced: a captured graph holds their addresses.
    Returned tensors are valid until the next step at their shape."""

    OUTPUTS = H.TEMPORAL_OUTPUTS + ("zkey",)
    STATE = ("fused", "var", "age")

    def __init__(self, reprojector, gate: float = H.TEMPORAL_GATE, q_var: float = 0.0, meas_std=None):
        for a in ("rays", "bf", "out_shape", "reproject", "long_range", "lat_range"):
            if not hasattr(reprojector, a):
                raise TypeError(f"TemporalFusion: expected a dropin.Reprojector, got {type(reprojector)}")
        if reprojector.long_range is None or reprojector.lat_range is None:
            raise ValueError("TemporalFusion: the reprojector was built from a ray table; the stage needs the rig camera's long_range and "
                             "lat_range (the inverse of an arbitrary ray table has no closed form)")
        self.reprojector = reprojector
        self.out_shape = tuple(reprojector.out_shape)
        self.device = reprojector.rays.device
        self.affine = H.temporal_affine(reprojector.long_range, reprojector.lat_range, self.out_shape)
        self.gate = float(gate)
        H.temporal_gate2(self.gate)
        self.q_var = float(q_var)
        if not 0.0 <= self.q_var < float("inf"):
            raise ValueError(f"TemporalFusion: q_var: 0 <= q_var < inf, got {q_var!r}")
        if meas_std is not None:
            meas_std = float(meas_std)
            if not 0.0 < meas_std < float("inf"):
                raise ValueError(f"TemporalFusion: meas_std: 0 < meas_std < inf, got {meas_std!r}")
        self.meas_std = meas_std
        H._pano_map("temporal fusion", 32, 1, *self.out_shape)
        self._bufs = {}          # (B, H, W, device) -> dict: made at first use, NEVER replaced (a captured graph holds them)

    # ---- what the evaluator owns ----
    def buffers(self, B: int, device=None) -> dict:
        """-> dict(inv, var, age: the state; zkey; T [B, 4, 4]: the pose the next step(T=None) uses; out: the outputs)"""
        Hh, W = self.out_shape
        device = torch.device(self.device if device is None else device)
        key = (int(B), Hh, W, device)
        got = self._bufs.get(key)
        if got is None:
            shape = (int(B), Hh, W)
            kinds = dict(fused=torch.float32, var=torch.float32, age=torch.uint8, warped_inv=torch.float32, warped_var=torch.float32,
                         src=torch.int32)
            got = self._bufs[key] = dict(
                inv=torch.zeros(shape, device=device, dtype=torch.float32), var=torch.zeros(shape, device=device, dtype=torch.float32),
                age=torch.zeros(shape, device=device, dtype=torch.uint8), zkey=torch.empty(shape, device=device, dtype=torch.int64),
                T=torch.eye(4, device=device, dtype=torch.float32).repeat(int(B), 1, 1),
                out={k: torch.empty(shape, device=device, dtype=d) for k, d in kinds.items()})
        return got

    def release(self) -> None:
        """Drop every buffer, the states with them.  Not while a captured graph that holds their addresses is still to be replayed."""
        self._bufs = {}

    def reset(self) -> None:
        """Every sequence starts over: age = 0 everywhere, so nothing of the state is live and the next step takes the measurement."""
        for bufs in self._bufs.values():
            bufs["age"].zero_()

    def set_pose(self, T, B=None) -> None:
        """Stage the pose of the previous rig frame in the current one for the next step(T=None) -- the step a captured graph replays.
        T: [B, 4, 4], or [4, 4] for every sequence (then B, default 1, names the buffers), on the host or the device; written into the
        evaluator's own device tensor with copy_."""
        T = pose_arg(T, B)
        self.buffers(T.shape[0])["T"].copy_(T, non_blocking=True)

    def _want(self, want) -> tuple:
        return H._wanted(want, self.OUTPUTS)

    def _measurement(self, inv, std):
        rp = self.reprojector
        inv = H._dev(rp._inv(inv), "inv")
        if std is not None:
            std = H._dev(rp._inv(std), "std")
            if std.shape != inv.shape or std.device != inv.device:
                raise AssertionError(f"std must be {list(inv.shape)} on {inv.device}, got {list(std.shape)} on {std.device}")
        elif self.meas_std is None:
            raise ValueError("TemporalFusion: no std map and no meas_std: the measurement's standard deviation is needed")
        return inv, std

    # ---- the stage ----
    def step(self, inv, std=None, T=None, want=STATE) -> dict:
        """One step of every sequence: T (None: the pose set_pose() staged, identity before any) into the evaluator's pose tensor, the
        splat from the state, the fuse into the outputs, and fused / var / age copied into the state (stage B gathers the state at
        the source index, so it cannot write it in place).  inv [B, H, W] or [B, 1, H, W]: the new measurement; std likewise, or
        None for meas_std.  Five launches on the current stream; after the first step at a shape nothing is allocated, and a step with
        T=None can be captured."""
        want = self._want(want)
        inv, std = self._measurement(inv, std)
        B = int(inv.shape[0])
        bufs = self.buffers(B, inv.device)
        if T is not None:
            bufs["T"].copy_(pose_arg(T, B), non_blocking=True)
        rp = self.reprojector
        H.temporal_splat(bufs["inv"], bufs["age"], rp.rays, bufs["T"], rp.bf, self.affine, out=bufs["zkey"])
        sel = tuple(k for k in H.TEMPORAL_OUTPUTS if k in want or k in self.STATE)
        res = H.temporal_fuse(bufs["zkey"], bufs["inv"], bufs["var"], bufs["age"], inv, rp.bf, gate=self.gate, q_var=self.q_var,
                              cur_std=std, meas_std=None if std is not None else self.meas_std, want=sel, out=bufs["out"])
        bufs["inv"].copy_(res["fused"])
        bufs["var"].copy_(res["var"])
        bufs["age"].copy_(res["age"])
        res["zkey"] = bufs["zkey"]
        return {k: res[k] for k in want}

    # ---- the definition, executed ----
    def splat_chain(self, state_inv, state_age, T) -> torch.Tensor:
        """Stage A of the definition, executed: Reprojector.reproject()'s xyz of the state, the transform kernel with T, the
        equirectangular grid kernel, then torch, one operation per line: the squared range, panorama_cell(), the keys
        and scatter_reduce(amin) into a buffer of EMPTY (a pixel that is not splatted contributes EMPTY, which changes nothing; on a
        build whose scatter_reduce refuses int64 the minimum is numpy's minimum.at on the host).  -> zkey [B, H, W] int64, the bits
        temporal_splat() returns."""
        from .sweep_grids import EquirectangularSampleGridMaker, transform_3D_points_torch
        rp = self.reprojector
        v = H._dev(rp._inv(state_inv), "state_inv")
        dev = v.device
        B, (Ho, Wo) = int(v.shape[0]), self.out_shape
        T = pose_arg(T, B).to(dev).contiguous()
        xyz = rp.reproject(v, want=("xyz",))["xyz"]
        q = transform_3D_points_torch(T, xyz.unsqueeze(2))
        g = EquirectangularSampleGridMaker().make_grid(q)[:, 0]
        qx, qy, qz = q[:, 0, 0], q[:, 1, 0], q[:, 2, 0]
        d = torch.full_like(v, rp.bf) / v
        live = (state_age != 0) & (v > 0) & (v <= _FLT_MAX) & (d <= _FLT_MAX)
        r2 = (qx * qx + qy * qy) + qz * qz
        near = (r2 > 0) & (r2 <= _FLT_MAX)
        fx, fy, inside = panorama_cell(g, self.affine, self.out_shape)
        splat = live & near & inside
        zero = torch.zeros_like(fx)
        cell = torch.where(splat, fy, zero).to(torch.int64) * Wo + torch.where(splat, fx, zero).to(torch.int64)
        s = torch.arange(Ho * Wo, device=dev, dtype=torch.int64).view(1, Ho, Wo)
        key = (r2.contiguous().view(torch.int32).to(torch.int64) << 32) | s
        key = torch.where(splat, key, torch.full_like(key, H.TEMPORAL_EMPTY))
        at = (torch.arange(B, device=dev, dtype=torch.int64).view(B, 1, 1) * (Ho * Wo) + cell).reshape(-1)
        zkey = torch.full((B * Ho * Wo,), H.TEMPORAL_EMPTY, device=dev, dtype=torch.int64)
        try:
            zkey.scatter_reduce_(0, at, key.reshape(-1), "amin", include_self=True)
        except RuntimeError:
            host = np.full(B * Ho * Wo, H.TEMPORAL_EMPTY, np.uint64)
            np.minimum.at(host, at.cpu().numpy(), key.reshape(-1).cpu().numpy().view(np.uint64))
            zkey = torch.from_numpy(host.view(np.int64)).to(dev)
        return zkey.view(B, Ho, Wo)

    def fuse_chain(self, zkey, state, inv, std=None, warped=None) -> dict:
        """Stage B of the definition in torch, one operation per line.  state = (inv, var, age); warped = (warped_inv, src) replaces
        the chain's own resolution of zkey -- torch's root stands in for the correctly rounded one there, so the tests feed the
        device's prior and compare everything behind it bit for bit.  -> dict of TemporalFusion.OUTPUTS."""
        inv, std = self._measurement(inv, std)
        p_inv, p_var, p_age = state
        dev = inv.device
        B, (Ho, Wo) = int(inv.shape[0]), self.out_shape
        last = Ho * Wo - 1
        inf = torch.full_like(inv, float("inf"))
        if warped is None:
            filled = zkey != H.TEMPORAL_EMPTY
            r2 = (zkey >> 32).to(torch.int32).view(torch.float32)
            s = torch.clamp(zkey & _LOW32, max=last)
            w_inv = torch.full_like(r2, self.reprojector.bf) / torch.sqrt(r2)
        else:
            w_inv, src = warped
            filled = src >= 0
            s = torch.where(filled, src.to(torch.int64), torch.full_like(src, last, dtype=torch.int64))
        s = s.view(B, -1)
        s_inv = torch.gather(p_inv.reshape(B, -1), 1, s).view(B, Ho, Wo)
        s_var = torch.gather(p_var.reshape(B, -1), 1, s).view(B, Ho, Wo)
        s_age = torch.gather(p_age.reshape(B, -1), 1, s).view(B, Ho, Wo).to(torch.int32)
        ratio = w_inv / s_inv
        g = ratio * ratio
        g = g * g
        var_w = s_var * g
        var_w = var_w + torch.full((), self.q_var, device=dev, dtype=torch.float32)
        prior = filled & (var_w >= 0) & (var_w <= _FLT_MAX)
        m = inv
        sd = std if std is not None else torch.full_like(inv, self.meas_std)
        var_m = sd * sd
        meas = (m > 0) & (m <= _FLT_MAX) & (var_m > 0) & (var_m <= _FLT_MAX)
        e = m - w_inv
        S = var_w + var_m
        gate2 = torch.full((), H.temporal_gate2(self.gate), device=dev, dtype=torch.float32)          # rounded to fp32 once
        agree = (e * e) <= (gate2 * S)
        K = var_w / S
        upd = w_inv + K * e
        upd_var = var_w - K * var_w
        both = prior & meas & agree
        only_prior = prior & ~meas
        take_meas = meas & ~both
        fused = torch.where(both, upd, torch.where(only_prior, w_inv, m))
        var = torch.where(both, upd_var, torch.where(only_prior, var_w, torch.where(take_meas, var_m, inf)))
        one = torch.ones_like(s_age)
        age = torch.where(both, torch.clamp(s_age + 1, max=255), torch.where(only_prior, s_age, torch.where(take_meas, one, one - 1)))
        res = dict(fused=fused, var=var, age=age.to(torch.uint8), warped_inv=torch.where(filled, w_inv, torch.zeros_like(w_inv)),
                   warped_var=torch.where(filled, var_w, inf), src=torch.where(filled, s.view(B, Ho, Wo), -one.to(torch.int64)).to(torch.int32),
                   zkey=zkey)
        return res

    def evaluate_chain(self, inv, std=None, T=None, state=None, want=OUTPUTS) -> dict:
        """The definition of one step, executed in torch on `state` = (inv, var, age) (default: the evaluator's own at this batch
        size) and the pose T (default: the staged one); the state is not advanced.  The bits step() returns, but for what depends on
        the root in warped_inv (see fuse_chain)."""
        want = self._want(want)
        m, _ = self._measurement(inv, std)
        bufs = self.buffers(int(m.shape[0]), m.device)
        if state is None:
            state = (bufs["inv"], bufs["var"], bufs["age"])
        zkey = self.splat_chain(state[0], state[2], bufs["T"] if T is None else T)
        res = self.fuse_chain(zkey, state, inv, std)
        return {k: res[k] for k in want}
