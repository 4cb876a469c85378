"""The loss-function cases and the definition they are checked against (include/mvsgi.h "loss functions"):
seeded inputs, and `restate`, the definition in plain torch / NumPy on the CPU.  tests/test_losses_host.py,
tests/test_gpu_losses.py and tools/make_losses_goldens.py all call this one restatement.  The fused chain (blend, softmax) is not
restated again: it is softargmin_cases.ref64, with its per-element bounds.

Inputs.  Low-resolution costs: Gaussian, sigma = SIGMA.  softargmin_cases' tolerance regime uses sigma 4 and 10; at sigma 4 the
operating shape has a winner with p > 0.999 at 1.2e-4 of its pixels (measured; largest p 0.99982), and a wider sigma has more:
there log1p(-p) amplifies the error of p by 1 / (1 - p) and condition (b) below fails.  SIGMA = 1 keeps every case inside the
conditions with the reference's own fp32 softmax as well as with ref64 (largest p 0.85; check_conditions asserts them).  Labels [B, 1, OH, OW]: uniform over [0.2, 230]; planted at the head of every frame, as far as the frame has
pixels: every candidate exactly, list[0] and list[D-1] again, values outside the range on both sides, values on both sides of 191;
and every fourth pixel after those lies within ~1 of the prediction, so that the quadratic branch of smooth-L1 is populated beside
the linear one (branches() counts both).  pred: the float64 expectation of ref64 rounded to fp32 plus N(0, 0.3) noise.

`restate`: the label stage in fp32 with the reference's own torch ops (clamp, bucketize, index, diff, divide, scatter_); the
cross-entropy addend per element from the fp32 two-hot t and the given p in float64, (t - 1) * max(log1p(-p), -100) -
t * max(log(p), -100), unrounded; the smooth-L1 addend in fp32 as ATen computes it; sums by math.fsum; the final divisions float64.

Bars.
  smooth_l1, inbounds, n_vol, n_px: 1 ulp of float64 (the same fp32 addends on both sides, both sums rounded once, one division).
  vol, given p (VOL_BAR): relative (U_LOG + 2) * 2^-23.  The kernel's addend is fl(fl(t - 1) * lq) - fl(t * lp) rounded, with lq, lp
      the device's log1pf(-p), logf(p).  U_LOG = 1: the documented maximum error, in ulp, of logf and of log1pf in HIP's math
      API (1 ulp <= 2^-23 relative).  The restatement's logs are float64.  (1 - t) * (-lq) carries U_LOG * 2^-23 (log) + 2^-24 (t - 1) +
      2^-24 (product); t * (-lp) carries U_LOG * 2^-23 + 2^-24; the subtraction 2^-24 on their sum: at most (U_LOG + 1.5) * 2^-23,
      taken as U_LOG + 2.  Both products are non-negative (0 <= t <= 1, both logs <= 0): no cancellation in an addend, none in the
      sum, so the bar holds for the mean.  The -100 clamp must engage on both sides alike: condition (a) below.
  vol, fused (fused_bar): propagated per case from softargmin_cases.bounds: per element t * dp / p + (1 - t) * dp / (1 - p) with
      dp = rel_p * p, plus VOL_BAR times the addend; summed over the selection and divided by the count.
Conditions (check_conditions): (a) every p is exactly 0 or >= 1e-30 (log p >= -69.1: the clamp engages at p = 0 only);
(b) max p <= 0.999; (c) the fused bar is <= 1e-4 of the case's loss.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import softargmin_cases as SC

BF = 96.0
DEFAULT_DIST_LIST = [0.5, 1, 1.5, 2, 5, 10, 20, 30, 50, 100]
COLUMNS = ("vol", "smooth_l1", "inbounds", "n_vol", "n_px")
SIGMA = 1.0
LABEL_MAX = 191.0
NEAR_DIST, FAR_DIST = 0.02, 0.2           # InBoundsBCEDistanceLoss: in(v) = 5 < v < 50 on the raw values
U_LOG = 1
VOL_BAR = (U_LOG + 2) * 2.0 ** -23
REDUCE_CAP_PIXELS = 256 * 256             # above this many pixels per frame the reduce grid is capped and strides further

# name -> (B, D, H, W low-resolution, scale, selection): 'none' | 'label_max' (labels <= 191: the image losses by label_max, the
# volume by the equal pixel mask) | 'volume' (a [B, D, OH, OW] mask, 70 % true; the image losses by its channel 0) | 'pixel'
# (a [B, 1, OH, OW] mask, 70 % true, for both) | 'frames' (a pixel mask: frame 1 all false, frame 2 all true, random elsewhere)
CASES = {
    "tiny": (1, 2, 1, 1, 1, "none"),
    "d10_x2": (2, 10, 7, 13, 2, "label_max"),
    "d33_x2": (1, 33, 6, 10, 2, "none"),
    "d16_x1.5": (2, 16, 7, 13, 1.5, "volume"),
    "d16_x4": (2, 16, 7, 13, 4, "pixel"),
    "frames": (5, 8, 9, 17, 1, "frames"),
    "operating": (1, 16, 80, 320, 2, "none"),
    "reduce_strided": (1, 8, 132, 500, 2, "label_max"),
}
assert CASES["reduce_strided"][2] * 2 * CASES["reduce_strided"][3] * 2 > REDUCE_CAP_PIXELS
STORED_INPUTS = ("tiny", "d10_x2", "d33_x2", "d16_x1.5", "d16_x4", "frames")      # inputs and true_cost kept in the golden file


def dist_list(D):
    """The candidates of a case: the reference's default at D = 10, else geomspace(0.5, 100, D)."""
    return list(DEFAULT_DIST_LIST) if D == 10 else [float(v) for v in np.geomspace(0.5, 100.0, D)]


def inv_list(D, bf=BF):
    """bf / Tensor(dist_list): VolumeCrossEntropy's inv_dist_list, fp32 [D], strictly decreasing"""
    return bf / torch.Tensor(dist_list(D))


def out_shape(name):
    B, D, H, W, s, _ = CASES[name]
    return B, D, math.floor(H * s), math.floor(W * s)


def planted(lst):
    lst = [float(v) for v in lst]
    return lst + [lst[0], lst[-1], 0.1, 0.5, 200.0, 229.0, 190.99, 191.0, 191.01]


def make_labels(shape, lst, pred, seed):
    """labels [B, 1, OH, OW] fp32 for candidates lst and the prediction pred (see the module's text)"""
    B, _, OH, OW = shape
    g = torch.Generator().manual_seed(seed)
    lab = (0.2 + 229.8 * torch.rand(B, OH * OW, generator=g, dtype=torch.float64)).to(torch.float32)
    near = (pred.reshape(B, -1).double() + 0.6 * torch.randn(B, OH * OW, generator=g, dtype=torch.float64)).to(torch.float32)
    pl = torch.tensor(planted(lst), dtype=torch.float32)
    n = min(len(pl), OH * OW)
    idx = torch.arange(OH * OW)
    take = (idx >= n) & ((idx - n) % 4 == 0)
    lab[:, take] = near[:, take].clamp(min=0.2)
    lab[:, :n] = pl[:n]
    return lab.reshape(B, 1, OH, OW).contiguous()


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """-> dict(costs np fp32 [B, D, H, W], scale, inv_idx np fp32 [D] (the regressor's candidates for ref64), inv_list fp32 tensor
    [D], labels, pred [B, 1, OH, OW] fp32 tensors, vol_mask, px_mask bool tensors or None, label_max or None, r: ref64's namespace)"""
    B, D, H, W, s, kind = CASES[name]
    seed = 2000 + sorted(CASES).index(name)
    costs = SC.gauss_costs((B, D, H, W), SIGMA, seed=seed)
    inv_idx = SC.stock_candidates(D)
    r = SC.ref64(costs, inv_idx, s)
    _, _, OH, OW = r.shape
    g = torch.Generator().manual_seed(seed)
    pred = (torch.from_numpy(r.inv).double() + 0.3 * torch.randn(B, 1, OH, OW, generator=g, dtype=torch.float64)).to(torch.float32)
    lst = inv_list(D)
    labels = make_labels((B, 1, OH, OW), lst.tolist(), pred, seed + 1)
    vol_mask = px_mask = label_max = None
    if kind == "label_max":
        label_max = LABEL_MAX
        vol_mask = labels <= LABEL_MAX
    elif kind == "volume":
        vol_mask = torch.rand(B, D, OH, OW, generator=g) < 0.7
        px_mask = vol_mask[:, :1].contiguous()
    elif kind in ("pixel", "frames"):
        px_mask = torch.rand(B, 1, OH, OW, generator=g) < 0.7
        if kind == "frames":
            px_mask[1] = False
            px_mask[2] = True
        vol_mask = px_mask
    return dict(costs=costs, scale=s, inv_idx=inv_idx, inv_list=lst, labels=labels, pred=pred.contiguous(), vol_mask=vol_mask,
                px_mask=px_mask, label_max=label_max, r=r)


def px_selection(inp):
    """The image losses' selection of a case as a mask tensor (what the reference's classes take), or None."""
    if inp["px_mask"] is not None:
        return inp["px_mask"]
    if inp["label_max"] is not None:
        return inp["labels"] <= inp["label_max"]
    return None


def true_cost(labels, lst, D=None):
    """VolumeCrossEntropy.forward's label stage, op for op (distance_loss.py:22-41) -> fp32 [B, D, OH, OW]"""
    lst = torch.as_tensor(lst, dtype=torch.float32)
    flipped, widths = torch.flip(lst, [0]), torch.diff(lst)
    x = torch.clamp(labels, lst[-1], lst[0])
    bin_idx = len(lst) - torch.bucketize(x, flipped)
    bin_idx = torch.clamp(bin_idx - 1, min=0, max=len(lst) - 2).to(torch.long)
    flat = bin_idx.flatten()
    lb = lst[flat].view_as(bin_idx)
    bw = widths[flat].view_as(bin_idx)
    d = (x - lb) / bw
    t = torch.zeros(labels.shape[0], len(lst), labels.shape[2], labels.shape[3], dtype=torch.float32)
    t.scatter_(1, bin_idx, 1 - d)
    t.scatter_(1, bin_idx + 1, d)
    return t


def vol_addends(t, p):
    """float64 [B, D, OH, OW]: ATen's binary_cross_entropy per element on the fp32 two-hot t and probabilities p, unrounded"""
    t = np.asarray(t, np.float64)
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.maximum(np.log(p), -100.0)
        lq = np.maximum(np.log1p(-p), -100.0)
        return (t - 1.0) * lq - t * lp


def _fsum(a):
    return math.fsum(np.asarray(a, np.float64).ravel().tolist())


def _div(s, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(s) / np.float64(n))


def restate(labels, lst, p=None, pred=None, vol_mask=None, px_mask=None, label_max=None, inbounds=None):
    """-> (np.float64 [B + 1, 5]: COLUMNS for every frame, row B pooled; the two-hot true_cost fp32 [B, D, OH, OW]).
    p: probabilities [B, D, OH, OW] (fp32 or float64) or None; pred [B, 1, OH, OW] fp32 or None; vol_mask [B, 1, OH, OW] or
    [B, D, OH, OW] bool; px_mask [B, 1, OH, OW] bool or label_max; inbounds: (near_inv, far_inv) as fp32 numbers or None."""
    B, _, OH, OW = labels.shape
    t = true_cost(labels, lst)
    D = t.shape[1]
    out = np.full((B + 1, 5), np.nan, np.float64)
    if px_mask is not None:
        spx = px_mask.reshape(B, 1, OH, OW).bool().numpy()
    elif label_max is not None:
        spx = (labels <= label_max).numpy()
    else:
        spx = np.ones((B, 1, OH, OW), bool)
    n_px = [int(spx[b].sum()) for b in range(B)]
    out[:B, 4], out[B, 4] = n_px, sum(n_px)
    if pred is not None:
        z = (pred - labels).abs()
        a = torch.where(z < 1.0, 0.5 * z * z, z - 0.5).numpy()
        S = [_fsum(a[b][spx[b]]) for b in range(B)]
        for b in range(B):
            out[b, 1] = _div(S[b], n_px[b])
        out[B, 1] = _div(_fsum(a[spx]), sum(n_px))
        if inbounds is not None:
            near, far = np.float32(inbounds[0]), np.float32(inbounds[1])
            pn, ln = pred.numpy(), labels.numpy()
            mm = ((pn < near) & (pn > far)) != ((ln < near) & (ln > far))
            M = [int(mm[b][spx[b]].sum()) for b in range(B)]
            for b in range(B):
                out[b, 2] = _div(100.0 * M[b], n_px[b])
            out[B, 2] = _div(100.0 * sum(M), sum(n_px))
    if p is not None:
        a = vol_addends(t.numpy(), p)
        sel = np.ones((B, D, OH, OW), bool) if vol_mask is None else np.broadcast_to(vol_mask.bool().numpy(), (B, D, OH, OW))
        n_vol = [int(sel[b].sum()) for b in range(B)]
        for b in range(B):
            out[b, 0] = _div(_fsum(a[b][sel[b]]), n_vol[b])
        out[B, 0] = _div(_fsum(a[sel]), sum(n_vol))
        out[:B, 3], out[B, 3] = n_vol, sum(n_vol)
    return out, t


def restate_case(inp, p, with_pred=True):
    near, far = np.float32(1.0 / NEAR_DIST), np.float32(1.0 / FAR_DIST)
    return restate(inp["labels"], inp["inv_list"], p=p, pred=inp["pred"] if with_pred else None, vol_mask=inp["vol_mask"],
                   px_mask=inp["px_mask"], label_max=inp["label_max"], inbounds=(near, far))


def fused_bar(r, t, p, vol_mask=None):
    """The bar of the fused volume loss against ref64 -> restate, per row: np.float64 [B + 1] (absolute, on the mean).
    r: ref64's namespace, t: the two-hot labels, p = r.p."""
    rel_p, _ = SC.bounds(r)
    t = np.asarray(t, np.float64)
    B, D, OH, OW = t.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        per = t * rel_p + (1.0 - t) * rel_p * p / (1.0 - p) + VOL_BAR * vol_addends(t, p)
    sel = np.ones(t.shape, bool) if vol_mask is None else np.broadcast_to(vol_mask.bool().numpy(), t.shape)
    bar = np.full(B + 1, np.nan)
    n = [int(sel[b].sum()) for b in range(B)]
    for b in range(B):
        bar[b] = _div(_fsum(per[b][sel[b]]), n[b])
    bar[B] = _div(_fsum(per[sel]), sum(n))
    return bar


def check_conditions(p):
    """(a) and (b) of the module's text for probabilities p -> (smallest non-zero p, largest p)"""
    p = np.asarray(p, np.float64)
    nz = p[p != 0]
    lo, hi = float(nz.min()), float(p.max())
    assert lo >= 1e-30, lo
    assert hi <= 0.999, hi
    return lo, hi


def branches(inp):
    """-> (pixels on the quadratic branch of smooth-L1, pixels on the linear one) among the selected pixels"""
    z = (inp["pred"] - inp["labels"]).abs()
    sel = px_selection(inp)
    if sel is not None:
        z = z[sel]
    return int((z < 1).sum()), int((z >= 1).sum())


def exact_inputs(shape, s):
    """softargmin_cases.exact_case at (shape, s) with labels for its D -> (case, dict(labels, inv_list, pred)); there p is exactly
    fl32(1 / |T|) or +0."""
    c = SC.exact_case(shape, s)
    B, D, OH, OW = c.want_p.shape
    lst = inv_list(D)
    g = torch.Generator().manual_seed(sum(shape) + int(8 * s))
    pred = (30.0 + 20.0 * torch.randn(B, 1, OH, OW, generator=g)).to(torch.float32)
    labels = make_labels((B, 1, OH, OW), lst.tolist(), pred, sum(shape) + int(8 * s) + 1)
    return c, dict(labels=labels, inv_list=lst, pred=pred)
