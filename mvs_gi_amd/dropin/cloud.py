"""The prediction as a packed point cloud: what a PointCloud2 publisher, an occupancy mapper or a planner takes.

    xyz = rays * (bf / inv_dist)                      the bits of Reprojector.point_cloud (csrc/reproject.hip)
    keep = on the step's lattice & mask & d finite and inside d_range & every gate's plane inside its interval
           (& seen by some camera, with require_colour)
    record = [x, y, z, colour of the first valid camera .., attributes ..]
    points[b] = the records of the kept pixels of frame b, in the order of the pixels

Three launches of csrc/cloud.hip (flags, scan, scatter): no atomics, no host synchronisation, the same bits every run, and no
allocation after the first call at a shape -- so the stage can follow the back-projection inside a captured graph
(InferencePipeline(..., cloud=packer)).  Not part of the reference's interface: the definition is a composition of operations this
package already has (include/mvsgi.h, "packed point cloud"), and tests/test_gpu_cloud.py compares with that
composition bit for bit.

Gates and attributes are confidence maps, named as in hip_ops.CONFIDENCE_MAPS:
    CloudPacker(reprojector, gates={"max_prob": (0.5, inf), "spread": (-inf, 2.0)}, attrs=("max_prob",))
`argmax` is an int map and is refused as either.  One more name is legal in both places: "photo_std", the photometric spread of
dropin.PhotoConsistency (do the cameras agree on the point's colour?); its plane arrives through pack(..., photo=...).
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import hip_ops as H

_FLOAT_MAPS = tuple(n for n in H.CONFIDENCE_MAPS if n != "argmax")
_PHOTO_MAPS = ("photo_std",)          # planes of dropin.PhotoConsistency, given to pack() as photo=


class CloudPacker:
    """packer.pack(inv, confidence=None, warped=None, valid=None, out=None, photo=None) -> dict(points [B, capacity, R], counts [B, 2], index
    [B, capacity] with want_index); packer.to_host(result) -> list of [written_b, R] arrays.

    source: a dropin.Reprojector (its rays, bf and out_shape are used) or a ray table [3, H, W] (then bf: 96 for the regressor's raw
    output, 1 for InferencePipeline's metric map).  gates: {map name: (lo, hi)}, closed intervals, at most hip_ops.CLOUD_MAX_GATES;
    attrs: map names appended to each record, in this order; mask: uint8 / bool [H, W] or [B, H, W]; step: (sy, sx), every sy-th
    row and sx-th column; d_range: (d_min, d_max) on d = bf / inv, default every positive finite distance; colour: records carry the
    colour of the first valid camera (pack() then needs warped and valid); require_colour: points no camera sees are dropped instead
    of coloured no_colour; capacity: rows per frame, default the pixels the step leaves.

    The packer owns one workspace and one set of outputs per (B, H, W, device), made at the first pack() of that shape and never
    replaced: a captured graph holds their addresses.  A result without `out` is valid until the next pack() at its shape."""

    def __init__(self, source, bf: Optional[float] = None, *, gates=None, attrs=(), mask=None, step=(1, 1), d_range=H.CLOUD_D_RANGE,
                 colour: bool = True, require_colour: bool = False, no_colour: float = 0.0, capacity: Optional[int] = None,
                 want_index: bool = False):
        if hasattr(source, "rays") and hasattr(source, "out_shape"):
            if bf is not None and float(bf) != float(source.bf):
                raise ValueError(f"CloudPacker: bf = {bf} given beside a Reprojector whose bf is {source.bf}")
            rays, bf = source.rays, source.bf
        elif isinstance(source, torch.Tensor):
            if bf is None:
                raise ValueError("CloudPacker: a ray table needs bf (96 for the regressor's raw output, 1 for a metric map)")
            rays = source
        else:
            raise TypeError(f"CloudPacker: expected a Reprojector or a ray table [3, H, W], got {type(source)}")
        if rays.dim() != 3 or rays.shape[0] != 3 or rays.dtype != torch.float32:
            raise AssertionError(f"CloudPacker: rays must be fp32 [3, H, W], got {rays.dtype} {tuple(rays.shape)}")
        self.rays = rays.contiguous()
        self.bf = float(bf)
        self.out_shape = (int(rays.shape[1]), int(rays.shape[2]))
        self.device = rays.device
        gates = dict(gates or {})
        attrs = (attrs,) if isinstance(attrs, str) else tuple(attrs)
        for name in list(gates) + list(attrs):
            if name == "argmax":
                raise ValueError("CloudPacker: 'argmax' is an int map; gates and attributes are the fp32 maps " + ", ".join(_FLOAT_MAPS))
            if name not in _FLOAT_MAPS + _PHOTO_MAPS:
                raise ValueError(f"CloudPacker: unknown confidence map {name!r} (gates and attributes: {', '.join(_FLOAT_MAPS + _PHOTO_MAPS)})")
        if len(set(attrs)) != len(attrs):
            raise ValueError(f"CloudPacker: attrs without repeats, got {attrs}")
        if len(gates) > H.CLOUD_MAX_GATES:
            raise ValueError(f"CloudPacker: {len(gates)} gates (at most {H.CLOUD_MAX_GATES})")
        self.gates = {}
        for name, iv in gates.items():
            lo, hi = (float(v) for v in iv)
            if lo != lo or hi != hi:
                raise ValueError(f"CloudPacker: gate {name!r}: the interval's ends must not be NaN")
            self.gates[name] = (lo, hi)
        self.attrs = attrs
        self.colour = bool(colour)
        self.require_colour = bool(require_colour)
        if self.require_colour and not self.colour:
            raise ValueError("CloudPacker: require_colour needs colour=True")
        if 3 + len(attrs) + (1 if self.colour else 0) > H.CLOUD_MAX_RECORD:
            raise ValueError(f"CloudPacker: a record of more than {H.CLOUD_MAX_RECORD} floats (3 + colour channels + {len(attrs)} attributes)")
        self.no_colour = float(no_colour)
        sy, sx = (int(v) for v in step)
        if sy < 1 or sx < 1:
            raise ValueError(f"CloudPacker: step (sy, sx) >= 1, got {tuple(step)}")
        self.step = (sy, sx)
        self.d_range = (float(d_range[0]), float(d_range[1]))
        self.capacity = H.cloud_capacity(*self.out_shape, self.step) if capacity is None else int(capacity)
        if not 1 <= self.capacity < 1 << 31:
            raise ValueError(f"CloudPacker: 1 <= capacity < 2^31, got {capacity}")
        self.want_index = bool(want_index)
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
                raise TypeError("CloudPacker: mask must be a bool or uint8 tensor")
            if tuple(mask.shape[-2:]) != self.out_shape or mask.dim() not in (2, 3):
                raise AssertionError(f"CloudPacker: mask must be [H, W] or [B, H, W] with (H, W) = {self.out_shape}, got {tuple(mask.shape)}")
            mask = mask.to(self.device).contiguous()
        self.mask = mask
        self.channels = None     # colour channels of the records: those of the first warped tensor packed
        self._bufs = {}          # (B, H, W, device) -> (workspace, outputs): made at first use, NEVER replaced (a captured graph holds them)

    @property
    def maps(self) -> tuple:
        """The confidence maps pack() needs, gates first."""
        return tuple(n for n in dict.fromkeys(list(self.gates) + list(self.attrs)) if n not in _PHOTO_MAPS)

    @property
    def photo_maps(self) -> tuple:
        """The planes of dropin.PhotoConsistency pack() needs (through photo=), gates first."""
        return tuple(n for n in dict.fromkeys(list(self.gates) + list(self.attrs)) if n in _PHOTO_MAPS)

    def record_width(self, channels: Optional[int] = None) -> int:
        c = (self.channels if channels is None else channels) if self.colour else 0
        if c is None:
            raise RuntimeError("CloudPacker: the record width is known after the first pack() (the colour channels are warped's)")
        return 3 + c + len(self.attrs)

    def buffers(self, B: int, R: int, device) -> tuple:
        Hh, W = self.out_shape
        key = (B, Hh, W, torch.device(device))
        got = self._bufs.get(key)
        if got is None:
            out = dict(points=torch.empty((B, self.capacity, R), device=device, dtype=torch.float32),
                       counts=torch.empty((B, 2), device=device, dtype=torch.int32))
            if self.want_index:
                out["index"] = torch.empty((B, self.capacity), device=device, dtype=torch.int32)
            got = self._bufs[key] = (H.cloud_ws(B, Hh, W, device), out)
        return got

    def release(self) -> None:
        """Drop every workspace and output set.  Not while a captured graph that holds their addresses is still to be replayed."""
        self._bufs = {}

    def _plane(self, confidence, name: str, B: int, photo=None) -> torch.Tensor:
        if name in _PHOTO_MAPS:
            if photo is None or name not in photo:
                raise ValueError(f"CloudPacker.pack: {name!r} is a gate or an attribute of this packer and was not given (photo=, the "
                                 "result of dropin.PhotoConsistency.evaluate)")
            confidence = photo
        elif confidence is None or name not in confidence:
            raise ValueError(f"CloudPacker.pack: the confidence map {name!r} is a gate or an attribute of this packer and was not given")
        t = confidence[name]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"CloudPacker.pack: confidence[{name!r}] must be an fp32 tensor")
        if t.dim() == 4 and t.shape[1] == 1:
            t = t[:, 0]
        if tuple(t.shape) != (B,) + self.out_shape:
            raise AssertionError(f"CloudPacker.pack: confidence[{name!r}] must be [{B}, 1, {self.out_shape[0]}, {self.out_shape[1]}] "
                                 f"(or without the 1), got {tuple(confidence[name].shape)}")
        return t

    def pack(self, inv, confidence=None, warped=None, valid=None, out=None, photo=None) -> dict:
        if not isinstance(inv, torch.Tensor):
            raise TypeError(f"inv: expected a torch.Tensor, got {type(inv)}")
        if inv.dim() == 4 and inv.shape[1] == 1:
            inv = inv[:, 0]
        if inv.dim() != 3 or tuple(inv.shape[1:]) != self.out_shape:
            raise AssertionError(f"inv must be [B, {self.out_shape[0]}, {self.out_shape[1]}] or [B, 1, ...], got {tuple(inv.shape)}")
        B = int(inv.shape[0])
        if self.colour:
            if warped is None or valid is None:
                raise ValueError("CloudPacker.pack: this packer colours its points: warped and valid (Reprojector's) are needed")
            if not isinstance(warped, torch.Tensor) or warped.dim() != 5:
                raise AssertionError("CloudPacker.pack: warped must be [B, N, C, H, W]")
            C = int(warped.shape[2])
            if self.channels is None:
                if self.record_width(C) > H.CLOUD_MAX_RECORD:
                    raise ValueError(f"CloudPacker.pack: a record of {self.record_width(C)} floats (at most {H.CLOUD_MAX_RECORD})")
                self.channels = C
            elif C != self.channels:
                raise ValueError(f"CloudPacker.pack: warped has {C} channels, this packer's records hold {self.channels}")
        elif warped is not None or valid is not None:
            raise ValueError("CloudPacker.pack: warped / valid given to a packer built with colour=False")
        gates = [(self._plane(confidence, n, B, photo),) + self.gates[n] for n in self.gates]
        attrs = [self._plane(confidence, n, B, photo) for n in self.attrs]
        H._cloud_plane(inv, "inv", None, None)
        ws, own = self.buffers(B, self.record_width(), inv.device)
        return H.pack_cloud(inv, self.rays, self.bf, d_range=self.d_range, gates=gates, mask=self.mask, step=self.step, warped=warped,
                            valid=valid, require_colour=self.require_colour, no_colour=self.no_colour, attrs=attrs,
                            capacity=self.capacity, want_index=self.want_index, ws=ws, out=own if out is None else out)

    @staticmethod
    def to_host(result) -> list:
        """-> one [written_b, R] float32 array per frame.  The one place that synchronises the host (it reads counts): for use
        outside graphs."""
        counts = result["counts"].cpu().numpy()
        points = result["points"]
        return [points[b, :int(counts[b, 0])].cpu().numpy() for b in range(points.shape[0])]
