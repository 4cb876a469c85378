"""Photometric consistency of the prediction: do the cameras agree on the colour of the point a pixel's predicted distance puts in
front of them?

    valid_n, w_n = Reprojector's validity and warped colours of camera n at the pixel       (csrc/reproject.hip, steps 1-6)
    seen_n = valid_n (& the camera's mask, sampled like its image, > 0)                      spherical_sweep_avg.py:92-102
    cnt = sum_n seen_n;  ok = cnt > 1;  k = ok ? cnt : 1                                     :106-111
    avg_c = sum_n w_n[c] seen_n / k                                                          :114
    var_c = ok ? sum_n (x_n - avg_c)^2 / k : 0,  x_n = seen_n ? w_n[c] : avg_c               :119-125
    photo_var = sum_c var_c / C;  photo_std = sqrt(photo_var)

the cost volume's own fusion rule (SphericalSweepStdMasked) on the images at the predicted distance, and per frame the scores of
hip_ops.PHOTO_COLUMNS over the pixels at least two cameras see.  One launch of csrc/photo.hip (two with the table) computes it without
storing the warped views: no atomics, no host synchronisation, the same bits every run and, with the evaluator's own workspace and
table, no allocation -- so the stage can follow the soft-argmin inside a captured graph (InferencePipeline(..., photo=...)).  It
needs no labels.  Not part of the reference's interface (install() does not serve it): the definition is a composition of operations
this package already has (include/mvsgi.h, "photometric consistency"), which PhotoConsistency.evaluate_chain
executes in torch and tests/test_gpu_photo.py compares bit for bit.

Occlusion is not reasoned about by this stage alone: a point hidden from one camera but inside its field of view reads high.  The
rig's baseline bounds how often that happens.  PhotoConsistency(..., visibility=dropin.Visibility(...)) keeps
the cameras a nearer predicted surface hides the point from out of the fusion.
"""
from __future__ import annotations

import torch

from .. import hip_ops as H


class PhotoConsistency:
    """pc.evaluate(inv, imgs, want=hip_ops.PHOTO_OUTPUTS, out=None) -> dict of n_views [B, H, W] uint8, photo_var / photo_std
    [B, H, W], mean_colour [B, C, H, W] and table float64 [B + 1, 14] (hip_ops.PHOTO_COLUMNS, row B pooled).

    reprojector: the dropin.Reprojector of the rig at the map's resolution (its rays, transforms, camera table and bf are used);
    cam_masks: fp32 [N, 1, Hr, Wr] (or [1, N, 1, Hr, Wr], as sample_masks takes them), the size of the images: a camera sees a point
    only where its mask, sampled like its image, is > 0; mask: uint8 / bool [H, W] or [B, H, W], the pixels the table scores; thresh:
    the table's bad-pixel threshold on photo_std; visibility: a dropin.Visibility built on the same reprojector -- a camera then also
    has to see the point (its `visible`, evaluated first, or the cam_seen= plane handed to evaluate()).

    The evaluator owns one workspace and one table per (B, H, W, device), made at the first evaluation of that shape and never
    replaced: a captured graph holds their addresses.  A table returned without `out` is valid until the next evaluation at its shape."""

    def __init__(self, reprojector, cam_masks=None, mask=None, thresh: float = 0.1, visibility=None):
        for a in ("rays", "T", "cams", "bf", "out_shape", "num_cams", "reproject"):
            if not hasattr(reprojector, a):
                raise TypeError(f"PhotoConsistency: expected a dropin.Reprojector, got {type(reprojector)}")
        self.reprojector = reprojector
        self.out_shape = tuple(reprojector.out_shape)
        self.num_cams = reprojector.num_cams
        self.device = reprojector.rays.device
        if cam_masks is not None:
            if not isinstance(cam_masks, torch.Tensor) or cam_masks.dtype != torch.float32:
                raise TypeError("PhotoConsistency: cam_masks must be an fp32 tensor [N, 1, Hr, Wr]")
            if cam_masks.dim() == 5 and cam_masks.shape[0] == 1:
                cam_masks = cam_masks[0]
            if cam_masks.dim() != 4 or cam_masks.shape[0] != self.num_cams or cam_masks.shape[1] != 1:
                raise AssertionError(f"PhotoConsistency: cam_masks must be [{self.num_cams}, 1, Hr, Wr], got {tuple(cam_masks.shape)}")
            cam_masks = cam_masks.to(self.device).contiguous()
        self.cam_masks = cam_masks
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
                raise TypeError("PhotoConsistency: mask must be a bool or uint8 tensor")
            if tuple(mask.shape[-2:]) != self.out_shape or mask.dim() not in (2, 3):
                raise AssertionError(f"PhotoConsistency: mask must be [H, W] or [B, H, W] with (H, W) = {self.out_shape}, got {tuple(mask.shape)}")
            mask = mask.to(self.device).contiguous()
        self.mask = mask
        self.thresh = float(thresh)
        if self.thresh != self.thresh:
            raise ValueError("PhotoConsistency: thresh must not be a NaN")
        if visibility is not None and getattr(visibility, "reprojector", None) is not reprojector:
            raise ValueError("PhotoConsistency: visibility= must be a dropin.Visibility built on the same reprojector")
        self.visibility = visibility
        self._bufs = {}          # (B, H, W, device) -> (workspace, table): made at first use, NEVER replaced (a captured graph holds them)
        self._seen = {}          # (B, H, W, device) -> the visibility stage's `visible`, likewise

    def buffers(self, B: int, device) -> tuple:
        Hh, W = self.out_shape
        key = (B, Hh, W, torch.device(device))
        got = self._bufs.get(key)
        if got is None:
            got = self._bufs[key] = (H.photo_ws(B, Hh, W, device),
                                     torch.empty((B + 1, len(H.PHOTO_COLUMNS)), device=device, dtype=torch.float64))
        return got

    def release(self) -> None:
        """Drop every workspace and table.  Not while a captured graph that holds their addresses is still to be replayed."""
        self._bufs = {}
        self._seen = {}

    def evaluate(self, inv, imgs, want=H.PHOTO_OUTPUTS, out=None, cam_seen=None) -> dict:
        """cam_seen: bool / uint8 [B, N, H, W], the cameras that may see each pixel (a Visibility's `visible`); None with a
        visibility= stage: that stage is evaluated first, into a buffer this evaluator owns."""
        rp = self.reprojector
        inv = rp._inv(inv)
        imgs = rp._imgs(imgs, inv.shape[0])
        want = tuple(want)
        if cam_seen is None and self.visibility is not None:
            H._dev(inv, "inv")
            key = (int(inv.shape[0]),) + self.out_shape + (inv.device,)
            got = self.visibility.evaluate(inv, want=("visible",), out=self._seen.get(key))
            self._seen[key] = {"visible": got["visible"]}
            cam_seen = got["visible"]
        ws = None
        if "table" in want:
            H._dev(inv, "inv")
            ws, table = self.buffers(int(inv.shape[0]), inv.device)
            if out is None or out.get("table") is None:
                out = dict(out or {}, table=table)
        return H.photo_consistency(inv, rp.rays, rp.T, rp.cams, rp.bf, imgs, cam_masks=self.cam_masks, mask=self.mask, thresh=self.thresh,
                                   want=want, out=out, ws=ws, cam_seen=cam_seen)

    def evaluate_chain(self, inv, imgs, want=H.PHOTO_OUTPUTS, cam_seen=None) -> dict:
        """The definition of evaluate(), executed: Reprojector.reproject()'s valid and warped (and, with camera masks, its grid
        through hip_ops.resample_bilinear), then the fusion rule in torch, one operation per line, sums over cameras and channels
        started at zero and taken in index order.  The planes are the bits evaluate() returns, but for photo_std, where torch's
        root stands in for the correctly rounded one.  The table is summed by torch in float64, uncompensated: it agrees with
        evaluate()'s to rounding (the tests restate it with math.fsum instead).
        Captured into a graph, the planes replay as they should; the TABLE is for eager calls only.  At 16 frames of 160 x 640 its
        pooled row stopped being right in replays that followed eager work on the same device (one frame, and every eager call, are
        right; the cause lies among the replayed torch reductions on zero-dimensional tensors and is not known).  A table inside a
        graph is evaluate()'s."""
        rp = self.reprojector
        inv = H._dev(rp._inv(inv), "inv")
        B, (Ho, Wo), N = int(inv.shape[0]), self.out_shape, self.num_cams
        imgs = rp._imgs(imgs, B)
        r = rp.reproject(inv, imgs, 0.0, want=("warped", "valid") + (("grid",) if self.cam_masks is not None else ()))
        w, seen = r["warped"], r["valid"]
        if self.cam_masks is not None:
            m = H.resample_bilinear(self.cam_masks.repeat(B, 1, 1, 1), r["grid"].view(B * N, Ho, Wo, 2), r["valid"].view(B * N, Ho, Wo))
            seen = seen & (m.view(B, N, Ho, Wo) > 0)
        if cam_seen is None and self.visibility is not None:
            cam_seen = self.visibility.evaluate_chain(inv, want=("visible",))["visible"]
        if cam_seen is not None:
            seen = seen & (cam_seen != 0)
        C = int(w.shape[2])
        seen_f = seen.to(torch.float32)
        cnt = torch.zeros((B, Ho, Wo), device=inv.device, dtype=torch.float32)
        for n in range(N):
            cnt = cnt + seen_f[:, n]
        ok = cnt > 1
        k = torch.where(ok, cnt, torch.ones_like(cnt))
        vsum = torch.zeros_like(cnt)
        avgs = []
        for c in range(C):
            acc = torch.zeros_like(cnt)
            for n in range(N):
                acc = acc + w[:, n, c] * seen_f[:, n]
            avg = acc / k
            dev2 = torch.zeros_like(cnt)
            for n in range(N):
                d = torch.where(seen[:, n], w[:, n, c], avg) - avg
                dev2 = dev2 + d * d
            vsum = vsum + torch.where(ok, dev2 / k, torch.zeros_like(cnt))
            avgs.append(avg)
        var = vsum / torch.full_like(vsum, float(C))
        std = torch.sqrt(var)
        res = dict(n_views=cnt.to(torch.uint8), photo_var=var, photo_std=std, mean_colour=torch.stack(avgs, dim=1))
        if "table" in want:
            masked = torch.ones_like(ok) if self.mask is None else (self.mask != 0).expand(B, Ho, Wo)
            scored = ok & masked
            rows = []
            for sel in [slice(b, b + 1) for b in range(B)] + [slice(0, B)]:
                s, mk = scored[sel], masked[sel]
                n = s.to(torch.float64).sum()
                nan = torch.full((), float("nan"), device=inv.device, dtype=torch.float64)
                some = n > 0
                zero = torch.zeros_like(std[sel])
                row = [n, torch.where(some, torch.where(s, std[sel], zero).double().sum() / n, nan),
                       torch.where(some, torch.sqrt(torch.where(s, var[sel], zero).double().sum() / n), nan),
                       torch.where(some, (s & (std[sel] > self.thresh)).to(torch.float64).sum() / n, nan),      # a Python scalar compares in fp32
                       n / mk.to(torch.float64).sum()]
                row += [((cnt[sel] == v) & mk).to(torch.float64).sum() for v in range(9)]
                rows.append(torch.stack(row))
            res["table"] = torch.stack(rows)
        return {key: res[key] for key in want}
