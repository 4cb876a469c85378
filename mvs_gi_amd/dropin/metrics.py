"""Validation metrics: the classes of dsta_mvs/support/loss_function/metrics.py (the `validation_metrics` of
configs/base_model.yaml:40-79, applied by validation_step, model/mvs_model/spherical_sweep_stereo_2024.py:145-231) with the
reference's constructors, buffers and forward(preds, target, valid_mask=None), on one HIP evaluation (csrc/metrics.hip).

    Evaluator.evaluate(preds, target, ...) -> float64 [B + 1, 9]: hip_ops.METRICS_COLUMNS for every frame, row B pooled

is the product: all eight numbers (and the valid count) of every frame from at most four launches, no host synchronisation, no
allocation after the first call at a shape, the same bits on every run.  Per frame, because the reference evaluates one frame per
step and averages the steps (offline_validation.py:33-42): at many frames per launch its epoch figure is the mean of the rows
b < B, not the pooled row.  The definition is stated in include/mvsgi.h ("validation metrics") and DESIGN.md section 15.

A metric module asked for its one number runs the whole evaluation and returns the pooled row's entry (range of the SSIM over
the batch: what one call of the reference's class on these tensors computes) as an fp32 scalar on the device.  Modules built with
the same (bf, dist_list, thresholds) share one Evaluator, and an evaluation is reused while the tensors are the same objects at the same
_version (the evaluator holds them until its next evaluation, so a freed block handed to new tensors cannot pass for them): the
six metrics of base_model.yaml cost one evaluation.  What remains: a tensor OBJECT that is reused and rewritten through a raw
pointer (a module-owned output buffer, the static output of a replayed graph) keeps its identity and its _version -- call
Evaluator.invalidate() between such evaluations, or use evaluate() itself, which never reuses.

preds is the regressor's raw output (not divided by bf): Evaluator goes behind HotPath or the drop-in model.  There is no CPU
path: CPU tensors raise.
"""
from __future__ import annotations

import weakref
from typing import Optional, Sequence, Tuple

import torch
from torch import nn, Tensor

from .. import hip_ops as H
from .common_modules import module_getstate

DEFAULT_BF = 96
DEFAULT_DIST_LIST = [0.5, 1, 1.5, 2, 5, 10, 20, 30, 50, 100]

_COL = {name: i for i, name in enumerate(H.METRICS_COLUMNS)}


def clamp_range(bf: float, dist_list: Sequence[float]) -> Tuple[Tensor, Tensor]:
    """(clamp_min, clamp_max): 0-dim fp32 tensors on the host, by the reference's own torch ops (metrics.py:23-25)."""
    inv = bf / torch.Tensor(dist_list)
    return torch.min(inv), torch.max(inv)


class _OwnRange:
    """The default of Evaluator.evaluate(label_range=...): the evaluator's own label range."""

    def __repr__(self):
        return "OWN_RANGE"


OWN_RANGE = _OwnRange()


class Evaluator:
    """evaluate(preds, target, valid_mask=None, label_range=OWN_RANGE, out=None) -> the table.

    bf, dist_list: the metric classes' arguments (the clamp range of the labels is min / max of bf / dist_list), or the clamp range
    itself as clamp_min / clamp_max; delta_thresh / delta_thresh_dist: the bad-pixel thresholds of the direct and the distance
    form; range_scope: 'frame' (each frame's SSIM with its own data range: the reference at one frame per step) or 'batch' (one call
    of the reference on the whole batch); label_range: the evaluator's own (lo, hi) on the raw label, validation_step's mask_labels,
    or None."""

    def __init__(self, bf: float = DEFAULT_BF, dist_list: Sequence[float] = DEFAULT_DIST_LIST, delta_thresh: float = 0.1,
                 delta_thresh_dist: Optional[float] = None, range_scope: str = "frame", label_range=None,
                 clamp_min: Optional[float] = None, clamp_max: Optional[float] = None):
        if range_scope not in H.METRICS_RANGE_SCOPES:
            raise ValueError(f"range_scope: 'frame' or 'batch', got {range_scope!r}")
        if (clamp_min is None) != (clamp_max is None):
            raise ValueError("clamp_min and clamp_max: both or neither")
        self.bf = float(bf)
        if clamp_min is None:
            clamp_min, clamp_max = clamp_range(bf, dist_list)
        self.clamp_min, self.clamp_max = float(clamp_min), float(clamp_max)
        self.delta_thresh = float(delta_thresh)
        self.delta_thresh_dist = float(delta_thresh if delta_thresh_dist is None else delta_thresh_dist)
        self.range_scope = range_scope
        self.label_range = None if label_range is None else (float(label_range[0]), float(label_range[1]))
        self._bufs = {}          # (B, H, W, device) -> (workspace, table): made at first use, NEVER replaced (a captured graph holds them)
        self._last = None        # ((preds, target, valid_mask), their _versions, table) of the last evaluation through shared()

    @classmethod
    def from_regressor(cls, dist_regressor, **kw):
        """bf, the clamp range and the label range of a DistanceRegressorWithFixedCandidates: both ranges are its
        [inv_dist_idx_min, inv_dist_idx_max], the fp32 min / max of bf / dist_cands that the metric classes compute too."""
        lo, hi = float(dist_regressor.inv_dist_idx_min), float(dist_regressor.inv_dist_idx_max)
        kw.setdefault("label_range", (lo, hi))
        return cls(bf=dist_regressor.bf, clamp_min=lo, clamp_max=hi, **kw)

    @staticmethod
    def _shape(preds: Tensor) -> tuple:
        if not isinstance(preds, torch.Tensor):
            raise TypeError(f"preds: expected a torch.Tensor, got {type(preds)}")
        if preds.dim() == 4 and preds.shape[1] == 1:
            return int(preds.shape[0]), int(preds.shape[2]), int(preds.shape[3])
        if preds.dim() == 3:
            return tuple(int(v) for v in preds.shape)
        raise AssertionError(f"preds must be [B, 1, H, W] or [B, H, W], got {tuple(preds.shape)}")

    def buffers(self, B: int, Hh: int, W: int, device) -> tuple:
        key = (B, Hh, W, torch.device(device))
        got = self._bufs.get(key)
        if got is None:
            ws = H.metrics_ws(B, Hh, W, device)
            table = torch.empty((B + 1, len(H.METRICS_COLUMNS)), device=device, dtype=torch.float64)
            got = self._bufs[key] = (ws, table)
        return got

    def release(self) -> None:
        """Drop every workspace and table (one pair is kept per (B, H, W, device) ever evaluated) and the remembered evaluation.
        Not while a captured graph that holds their addresses is still to be replayed."""
        self._bufs = {}
        self._last = None

    def evaluate(self, preds: Tensor, target: Tensor, valid_mask: Optional[Tensor] = None, label_range=OWN_RANGE,
                 out: Optional[Tensor] = None, range_scope: Optional[str] = None) -> Tensor:
        """-> float64 [B + 1, 9].  valid_mask [B, 1, H, W] bool / uint8, or label_range: (lo, hi), None (every pixel), or left
        at OWN_RANGE (the evaluator's own; ignored when a mask is given).  Without `out` the result is the evaluator's own table
        for this shape, overwritten by the next evaluation at this shape."""
        B, Hh, W = self._shape(preds)
        self._last = None                  # the table that shared() may have handed out is about to be overwritten
        if label_range is OWN_RANGE:
            label_range = None if valid_mask is not None else self.label_range
        H._dev(preds, "preds")
        ws, table = self.buffers(B, Hh, W, preds.device)
        return H.metrics(preds, target, self.bf, self.clamp_min, self.clamp_max, valid_mask=valid_mask, label_range=label_range,
                         thresh=self.delta_thresh, thresh_dist=self.delta_thresh_dist, range_scope=range_scope or self.range_scope,
                         ws=ws, out=table if out is None else out)

    def invalidate(self) -> None:
        self._last = None

    def shared(self, preds: Tensor, target: Tensor, valid_mask: Optional[Tensor]) -> Tensor:
        """The table of the metric modules (mask as given, no label range, batch scope): evaluated once per set of tensors.
        The same set: the same tensor OBJECTS at the same _version.  The remembered tensors are held until the next evaluation, so
        their storage cannot be freed and handed to other tensors that would then look the same by address."""
        tensors = (preds, target, valid_mask)
        versions = tuple(None if t is None else t._version for t in tensors)
        last = self._last
        if last is not None and all(a is b for a, b in zip(last[0], tensors)) and last[1] == versions:
            return last[2]
        table = self.evaluate(preds, target, valid_mask=valid_mask, label_range=None, range_scope="batch")
        self._last = (tensors, versions, table)
        return table


# One Evaluator per distinct parameter set: what lets separately constructed modules share an evaluation.  Weak: an evaluator,
# with its workspaces, lives as long as a metric object that resolved to it.
_EVALUATORS = weakref.WeakValueDictionary()


def _evaluator_for(bf, clamp_min: float, clamp_max: float, thresh: float, thresh_dist: float) -> Evaluator:
    key = (float(bf), clamp_min, clamp_max, thresh, thresh_dist)
    ev = _EVALUATORS.get(key)
    if ev is None:
        ev = _EVALUATORS[key] = Evaluator(bf=bf, clamp_min=clamp_min, clamp_max=clamp_max, delta_thresh=thresh,
                                          delta_thresh_dist=thresh_dist, range_scope="batch")
    return ev


def _resolve_evaluator(obj, column: str, inverse: bool) -> Evaluator:
    """The evaluator of a metric object: the one set by use_evaluator(), else the shared one for the object's parameters.  The
    resolution is remembered on the object (reading the clamp buffers of a module on the device synchronises the host: once per
    set of buffers, not once per call)."""
    ev = obj.__dict__.get("_mvsgi_evaluator")
    if ev is not None:
        return ev
    # a bad-pixel threshold other than the default evaluates apart from the other metrics: an evaluator holds one per form
    thr = float(getattr(obj, "delta_thresh", 0.1)) if column == "bad" else 0.1
    cmin, cmax = obj.clamp_min, obj.clamp_max
    sig = (obj.bf, thr, id(cmin), getattr(cmin, "_version", None), id(cmax), getattr(cmax, "_version", None))
    cache = obj.__dict__.setdefault("_mvsgi_resolved", {})
    got = cache.get(inverse)
    if got is None or got[0] != sig:
        got = cache[inverse] = (sig, _evaluator_for(obj.bf, float(cmin), float(cmax), 0.1 if inverse else thr, thr if inverse else 0.1),
                                cmin, cmax)          # (the buffers themselves: an id stays theirs while they live)
    return got[1]


def _metric_value(obj, column: Optional[str], preds: Tensor, target: Tensor, valid_mask: Optional[Tensor], inverse: bool) -> Tensor:
    """The pooled row's entry for a metric object (a class below, or the reference's own class behind install()'s patch): reads
    bf, clamp_min / clamp_max, delta_thresh and the evaluator set by use_evaluator() from the object."""
    if column is None:
        raise NotImplementedError()
    H._dev(preds, "preds")
    H._dev(target, "target")
    table = _resolve_evaluator(obj, column, inverse).shared(preds, target, valid_mask)
    return table[-1, _COL[column + ("_dist" if inverse else "")]].to(torch.float32)


class MVSMetric(nn.Module):
    _column = None            # the table column of the direct form; the distance form is "<column>_dist"

    def __init__(self, bf: float = DEFAULT_BF, dist_list: Sequence[float] = DEFAULT_DIST_LIST):
        super().__init__()
        self.bf = bf
        lo, hi = clamp_range(bf, dist_list)
        self.register_buffer("clamp_min", lo, persistent=False)
        self.register_buffer("clamp_max", hi, persistent=False)

    __getstate__ = module_getstate

    def clamp_and_scale(self, preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
        """(preds / bf, clamp(target) / bf) with torch ops: the reference's helper, kept for callers; forward does not use it."""
        return preds / self.bf, torch.clamp(target, self.clamp_min, self.clamp_max) / self.bf

    def use_evaluator(self, evaluator: Optional[Evaluator]) -> "MVSMetric":
        """Evaluate through this Evaluator (its bf, clamp range and thresholds then hold), or None: back to the shared default."""
        self.__dict__["_mvsgi_evaluator"] = evaluator
        return self

    def forward(self, preds: Tensor, target: Tensor, valid_mask: Tensor = None) -> Tensor:
        return _metric_value(self, self._column, preds, target, valid_mask, False)


class SSIMMetric(MVSMetric):
    """valid_mask is accepted and not used, as in the reference."""
    _column = "ssim"

    def __init__(self, bf: float = DEFAULT_BF, dist_list: Sequence[float] = DEFAULT_DIST_LIST):
        super().__init__(bf=bf, dist_list=dist_list)


class RMSEMetric(MVSMetric):
    _column = "rmse"

    def __init__(self, bf: float = DEFAULT_BF, dist_list: Sequence[float] = DEFAULT_DIST_LIST):
        super().__init__(bf=bf, dist_list=dist_list)


class MAEMetric(MVSMetric):
    _column = "mae"

    def __init__(self, bf: float = DEFAULT_BF, dist_list: Sequence[float] = DEFAULT_DIST_LIST):
        super().__init__(bf=bf, dist_list=dist_list)


class BadPixelRatioMetric(MVSMetric):
    _column = "bad"

    def __init__(self, bf: float = DEFAULT_BF, dist_list: Sequence[float] = DEFAULT_DIST_LIST, delta_thresh: float = 0.1):
        super().__init__(bf=bf, dist_list=dist_list)
        self.delta_thresh = delta_thresh


_COLUMN_OF = {"SSIMMetric": "ssim", "RMSEMetric": "rmse", "MAEMetric": "mae", "BadPixelRatioMetric": "bad"}


class InverseMetricWrapper(nn.Module):
    """metric(1 / preds, 1 / target, valid_mask): the distance form of the wrapped metric, from the same evaluation.  (The
    reference turns any exception of the wrapped metric into 0.0; here an error is an error.)"""

    def __init__(self, metric: nn.Module):
        super().__init__()
        self.metric = metric

    def forward(self, preds: Tensor, target: Tensor, valid_mask: Tensor = None) -> Tensor:
        return inverse_forward(self, preds, target, valid_mask)


def metric_forward(self, preds: Tensor, target: Tensor, valid_mask: Tensor = None) -> Tensor:
    """forward of the reference's own metric classes once install() has patched them (matched by class name)."""
    return _metric_value(self, _COLUMN_OF.get(type(self).__name__), preds, target, valid_mask, False)


def inverse_forward(self, preds: Tensor, target: Tensor, valid_mask: Tensor = None) -> Tensor:
    m = self.metric
    column = getattr(m, "_column", None) or _COLUMN_OF.get(type(m).__name__)
    if column is not None and hasattr(m, "clamp_min") and hasattr(m, "bf"):
        return _metric_value(m, column, preds, target, valid_mask, True)
    return m(1.0 / preds, 1.0 / target, valid_mask)          # a metric of another kind: the wrapper's own definition
