"""Loss functions, forward values only: the classes of dsta_mvs/support/loss_function/distance_loss.py (VolumeCrossEntropy,
MaskedSmoothL1Loss, InBoundsBCEDistanceLoss, NearFocusDistanceLoss; named by configs/base_model.yaml:83-92 and configs/loss/*.yaml) with the
reference's constructors, buffers and forward signatures, on one HIP evaluation (csrc/losses.hip).

    LossEvaluator.evaluate(labels, ...) -> float64 [B + 1, 5]: hip_ops.LOSSES_COLUMNS for every frame, row B pooled

is the product: `vol_loss` and `distance_loss` of every frame of a validation batch from two launches, no host synchronisation, no
allocation after the first call at a shape, the same bits on every run.  With `costs` (the regulator's output) and the regressor's
scale the volume loss walks the soft-argmin's softmax itself: norm_costs [B, D, OH, OW] is never stored, the regressor may keep
return_norm_costs = False.  The definition is stated in include/mvsgi.h ("loss functions") and DESIGN.md section 18.

There is no backward: this path has no autograd anywhere, the values are for laying a validation run over a training curve.  A loss
module asked for its number runs an evaluation and returns the pooled row's entry as an fp32 0-dim tensor on the device.  There is no
CPU path: CPU tensors raise.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import nn, Tensor

from .. import hip_ops as H
from .common_modules import module_getstate

DEFAULT_BF = 96
DEFAULT_DIST_LIST = [0.5, 1, 1.5, 2, 5, 10, 20, 30, 50, 100]

_COL = {name: i for i, name in enumerate(H.LOSSES_COLUMNS)}


def check_inv_list(inv_list: Tensor) -> Tensor:
    """inv_list = bf / dist_list as an fp32 tensor -> the same, flat, on the host; ValueError unless it has at least two entries, all
    positive and finite, strictly decreasing (dist_list strictly increasing and positive): a zero bin width has no meaning."""
    v = inv_list.detach().reshape(-1).to("cpu", torch.float32)
    if v.numel() < 2:
        raise ValueError(f"dist_list: the volume labels need at least two candidates, got {v.numel()}")
    if not bool(torch.isfinite(v).all()) or not bool((v > 0).all()) or not bool((v[1:] < v[:-1]).all()):
        raise ValueError(f"dist_list must be positive and strictly increasing (bf / dist_list strictly decreasing in fp32), got "
                         f"bf / dist_list = {v.tolist()}")
    return v


class LossEvaluator:
    """evaluate(labels, pred=None, norm_costs=None, costs=None, scale=None, vol_mask=None, px_mask=None, label_max=None, out=None)
    -> the table.

    bf, dist_list: VolumeCrossEntropy's arguments (or inv_dist_idx: bf / dist_list itself, as the regressor holds it); scale: the
    regressor's up-sampling factor for `costs`; near_dist_threshold / far_dist_threshold: InBoundsBCEDistanceLoss's (both or neither;
    neither: the inbounds column is NaN); label_max: the default selection of the image losses, labels <= label_max (the training step
    uses 191), or None."""

    def __init__(self, bf: float = DEFAULT_BF, dist_list: Sequence[float] = DEFAULT_DIST_LIST, scale: float = 1.0,
                 near_dist_threshold: Optional[float] = None, far_dist_threshold: Optional[float] = None,
                 label_max: Optional[float] = None, inv_dist_idx: Optional[Tensor] = None):
        if (near_dist_threshold is None) != (far_dist_threshold is None):
            raise ValueError("near_dist_threshold and far_dist_threshold: both or neither")
        self.bf = float(bf)
        inv = bf / torch.Tensor(list(dist_list)) if inv_dist_idx is None else inv_dist_idx
        self.inv_list = check_inv_list(inv)
        self.scale = float(scale)
        self.inbounds = None if near_dist_threshold is None else (1.0 / near_dist_threshold, 1.0 / far_dist_threshold)
        self.label_max = None if label_max is None else float(label_max)
        self._lists = {}         # device -> the list there
        self._bufs = {}          # (B, OH, OW, device) -> (workspace, table): made at first use, NEVER replaced (a captured graph holds them)

    @classmethod
    def from_regressor(cls, dist_regressor, **kw):
        """bf, the candidate list and the scale rule (pre_interp / interp_scale_factor) of a DistanceRegressorWithFixedCandidates."""
        scale = 1.0
        if getattr(dist_regressor, "pre_interp", False) and getattr(dist_regressor, "interp_scale_factor", 0) > 0:
            scale = dist_regressor.interp_scale_factor
        return cls(bf=dist_regressor.bf, inv_dist_idx=dist_regressor.inv_dist_idx, scale=scale, **kw)

    def list_on(self, device) -> Tensor:
        device = torch.device(device)
        got = self._lists.get(device)
        if got is None:
            got = self._lists[device] = self.inv_list.to(device)
        return got

    def buffers(self, B: int, OH: int, OW: int, device) -> tuple:
        key = (B, OH, OW, torch.device(device))
        got = self._bufs.get(key)
        if got is None:
            ws = H.losses_ws(B, OH, OW, device)
            table = torch.empty((B + 1, len(H.LOSSES_COLUMNS)), device=device, dtype=torch.float64)
            got = self._bufs[key] = (ws, table)
        return got

    def release(self) -> None:
        """Drop every workspace and table.  Not while a captured graph that holds their addresses is still to be replayed."""
        self._bufs = {}

    def evaluate(self, labels: Tensor, pred: Optional[Tensor] = None, norm_costs: Optional[Tensor] = None,
                 costs: Optional[Tensor] = None, scale: Optional[float] = None, vol_mask: Optional[Tensor] = None,
                 px_mask: Optional[Tensor] = None, label_max: Optional[float] = None, out: Optional[Tensor] = None,
                 true_cost: Optional[Tensor] = None) -> Tensor:
        """-> float64 [B + 1, 5].  labels [B, 1, OH, OW]; pred [B, 1, OH, OW] (the image losses); norm_costs [B, D, OH, OW] or
        costs [B, 1(+), D, H, W] / [B, D, H, W] with scale (default: the evaluator's) for the volume loss; vol_mask [B, 1, OH, OW] or
        [B, D, OH, OW]; px_mask [B, 1, OH, OW] or label_max (default: the evaluator's, ignored when a mask is given).  Without `out`
        the result is the evaluator's own table for this shape, overwritten by the next evaluation at this shape."""
        lab = H._dev(labels, "labels")
        if lab.dim() not in (3, 4) or (lab.dim() == 4 and lab.shape[1] != 1):
            raise AssertionError(f"labels must be [B, 1, OH, OW] or [B, OH, OW], got {tuple(lab.shape)}")
        B, OH, OW = int(lab.shape[0]), int(lab.shape[-2]), int(lab.shape[-1])
        if costs is not None and isinstance(costs, torch.Tensor) and costs.dim() == 5:
            costs = costs[:, 0]
        if label_max is None and px_mask is None:
            label_max = self.label_max
        ws, table = self.buffers(B, OH, OW, lab.device)
        return H.losses(lab, self.list_on(lab.device), pred=pred, pred_cost=norm_costs, costs=costs,
                        scale=self.scale if scale is None else scale, vol_mask=vol_mask, px_mask=px_mask, label_max=label_max,
                        inbounds=self.inbounds, true_cost=true_cost, ws=ws, out=table if out is None else out)

    def volume_labels(self, labels: Tensor, out: Optional[Tensor] = None) -> Tensor:
        """VolumeCrossEntropy's two-hot true_cost [B, D, OH, OW] for these labels."""
        lab = H._dev(labels, "labels")
        return H.volume_labels(lab, self.list_on(lab.device), out=out)


def _own_evaluator(obj, make) -> LossEvaluator:
    """The evaluator of a loss object (a class below, or the reference's own class behind install()'s patch), made at first use
    from the object's parameters; an `_mvsgi_*` entry: it does not travel with a pickled module."""
    key = getattr(obj, "inv_dist_list", None)
    sig = None if key is None else (id(key), key._version)
    got = obj.__dict__.get("_mvsgi_evaluator")
    if got is None or got[0] != sig:
        got = obj.__dict__["_mvsgi_evaluator"] = (sig, make(), key)
    return got[1]


def _entry(table: Tensor, column: str) -> Tensor:
    return table[-1, _COL[column]].to(torch.float32)


def _image_only(pred_costs: Tensor, what: str) -> None:
    if not isinstance(pred_costs, torch.Tensor):
        raise TypeError(f"pred_costs: expected a torch.Tensor, got {type(pred_costs)}")
    if pred_costs.dim() != 4:
        raise AssertionError(f"pred_costs must be [B, 1, H, W], got {tuple(pred_costs.shape)}")
    if pred_costs.shape[1] > 1:
        raise NotImplementedError(
            f"{what}: pred_costs with shape[1] > 1 is the branch that regresses the volume first; the reference raises TypeError "
            "there (it calls dist_regressor, which returns a tuple, and indexes the tuple with a mask).  Regress the image yourself and "
            "pass it as [B, 1, H, W].")


def volume_forward(self, pred_cost: Tensor, inv_dist_true: Tensor, mask: Tensor = None) -> Tensor:
    """VolumeCrossEntropy.forward, also of the reference's class once install() has patched it.  mask: [B, D, H, W] as the
    reference takes it, or [B, 1, H, W] (an extension: the pixel across all D)."""
    ev = _own_evaluator(self, lambda: LossEvaluator(inv_dist_idx=self.inv_dist_list))      # ValueError on a list without bins
    H._dev(pred_cost, "pred_cost")
    H._dev(inv_dist_true, "inv_dist_true")
    return _entry(ev.evaluate(inv_dist_true, norm_costs=pred_cost, vol_mask=mask), "vol")


def smooth_l1_forward(self, pred_costs: Tensor, labels: Tensor, mask: Tensor = None):
    """MaskedSmoothL1Loss.forward on an image; mask None, [B, 1, H, W] or [B, D, H, W] (its channel 0 is used, as in the
    reference)."""
    _image_only(pred_costs, "MaskedSmoothL1Loss")
    H._dev(pred_costs, "pred_costs")
    H._dev(labels, "labels")
    if mask is not None:
        mask = mask[:, 0, ...].unsqueeze(1)
    ev = _own_evaluator(self, _image_evaluator)
    return _entry(ev.evaluate(labels, pred=pred_costs, px_mask=mask), "smooth_l1")


def inbounds_forward(self, pred_costs: Tensor, labels: Tensor, mask: Tensor = None):
    """InBoundsBCEDistanceLoss.forward on an image; mask None or [B, 1, H, W]."""
    _image_only(pred_costs, "InBoundsBCEDistanceLoss")
    H._dev(pred_costs, "pred_costs")
    H._dev(labels, "labels")
    ev = _own_evaluator(self, _image_evaluator)
    ev.inbounds = (self.near_inv_dist_thresh, self.far_inv_dist_thresh)
    return _entry(ev.evaluate(labels, pred=pred_costs, px_mask=mask), "inbounds")


def near_focus_forward(self, pred_cost: Tensor, inv_dist_true: Tensor):
    """NearFocusDistanceLoss.forward, composed literally; a loss function of this package gets the far / near mask as
    [B, 1, H, W] instead of the reference's repeat over the candidates (the same selection, D times fewer bytes)."""
    far_mask = inv_dist_true < self.inv_near_dist_thresh
    pixel_ok = all(getattr(type(f), "forward", None) is volume_forward for f in (self.near_loss_func, self.far_loss_func))
    far_vol_mask = far_mask if pixel_ok else far_mask.repeat(1, self.num_cands, 1, 1)
    far_loss = self.far_loss_func(pred_cost, inv_dist_true, mask=far_vol_mask)
    near_loss = self.near_loss_func(pred_cost, inv_dist_true, mask=~far_vol_mask)
    return (self.near_weight * near_loss) + (self.far_weight * far_loss)


def _image_evaluator() -> LossEvaluator:
    return LossEvaluator()          # the image losses read neither bf nor the list


class VolumeCrossEntropy(nn.Module):
    def __init__(self, bf: float = DEFAULT_BF, dist_list: Sequence[float] = DEFAULT_DIST_LIST):
        super().__init__()
        self.register_buffer("inv_dist_list", bf / torch.Tensor(dist_list), persistent=False)
        self.register_buffer("inv_dist_list_flipped", torch.flip(self.inv_dist_list, [0]), persistent=False)
        self.register_buffer("bin_widths", torch.diff(self.inv_dist_list), persistent=False)

    __getstate__ = module_getstate
    forward = volume_forward


class MaskedSmoothL1Loss(nn.Module):
    def __init__(self, dist_regressor: nn.Module):
        super().__init__()
        self.loss = torch.nn.SmoothL1Loss()
        self.dist_regressor = dist_regressor

    __getstate__ = module_getstate
    forward = smooth_l1_forward


class InBoundsBCEDistanceLoss(nn.Module):
    def __init__(self, dist_regressor: nn.Module, far_dist_threshold: float, near_dist_threshold: float):
        super().__init__()
        self.loss = torch.nn.BCELoss(reduction="mean")
        self.dist_regressor = dist_regressor
        self.far_inv_dist_thresh = 1.0 / far_dist_threshold
        self.near_inv_dist_thresh = 1.0 / near_dist_threshold

    __getstate__ = module_getstate
    forward = inbounds_forward


class NearFocusDistanceLoss(nn.Module):
    def __init__(self, near_loss_func: nn.Module, far_loss_func: nn.Module, near_dist_thresh: float,
                 loss_weights: Tuple[float, float], dist_list: Sequence):
        super().__init__()
        self.near_loss_func = near_loss_func
        self.far_loss_func = far_loss_func
        self.inv_near_dist_thresh = 1.0 / near_dist_thresh
        self.near_weight = loss_weights[0]
        self.far_weight = loss_weights[1]
        self.num_cands = len(dist_list)

    __getstate__ = module_getstate
    forward = near_focus_forward
