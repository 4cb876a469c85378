"""The validation-metric cases and the definition they are checked against (include/mvsgi.h "validation
metrics"): seeded inputs, and `restate`, the definition in plain torch on the CPU.  tests/test_metrics_host.py,
tests/test_gpu_metrics.py and tools/make_metrics_goldens.py all call this one restatement.

Inputs: the label is a smooth field that spans [2, 62] in every frame (a coarse uniform grid, bilinearly enlarged, normalised
and cubed: the distance form's range comes from the smallest predictions, so every frame needs labels near 2), the prediction the label with 5 %
multiplicative and 0.3 additive Gaussian noise, floored at 0.3; bf = 96 and the reference's default dist_list.

`restate(..., dtype=torch.float64)`: per pixel the reference's fp32 arithmetic; S2 and S1 are the correctly rounded sums of their
fp32 addends (math.fsum), the final division / root and the whole SSIM (separable filter) float64.  dtype=torch.float32 is the same
formula with fp32 sums and an fp32 SSIM: the noise level of an fp32 evaluation such as the reference's own, from which the host
test derives its bars.

SSIM_CONDITION: for every case, frame and form max(|P|, |T|) <= 2 R, R the frame's data range -- the condition under which the
1e-9 bar of the GPU test is derived (moments up to (2 R)^2 against c2 = 9e-4 R^2); check_condition() asserts it, the largest ratio
over the table is 1.68 (the distance form of 'no_ssim'; 1.59 where an SSIM is computed).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

BF = 96.0
DIST_LIST = [0.5, 1, 1.5, 2, 5, 10, 20, 30, 50, 100]
COLUMNS = ("rmse", "mae", "bad", "ssim", "rmse_dist", "mae_dist", "bad_dist", "ssim_dist", "n")
LABEL_RANGE = (5.0, 40.0)
# bad-pixel thresholds of the table: at the reference's default of 0.1 (in 1 / m after the division by bf) no pixel of these inputs
# is bad and the column would be 0 whatever the kernel counted; with these about a third and a half of the pixels are
THRESH, THRESH_DIST = 0.005, 0.008
SSIM_TILE = (16, 32)          # output pixels per block of the SSIM kernel (csrc/metrics.hip)
REDUCE_CAP_PIXELS = 64 * 4096  # above this many pixels per frame the reduce grid is capped and strides further

# name -> (B, H, W, validity): 'none' | 'mask' (random, 70 % valid) | 'range' (LABEL_RANGE) | 'frames' (frame 1 all false, frame 2
# all true, random elsewhere)
CASES = {
    "one_window": (1, 11, 11, "none"),
    "no_ssim": (1, 10, 40, "range"),
    "row_tail": (2, 12, 75, "mask"),
    "odd": (3, 37, 130, "range"),
    "operating": (1, 160, 640, "none"),
    "tile_plus_one": (2, SSIM_TILE[0] + 11, SSIM_TILE[1] + 11, "mask"),
    "reduce_strided": (1, 264, 1000, "range"),
    "masked_frames": (5, 33, 67, "frames"),
}
assert CASES["reduce_strided"][1] * CASES["reduce_strided"][2] > REDUCE_CAP_PIXELS
STORED_INPUTS = ("one_window", "no_ssim", "row_tail", "odd", "tile_plus_one", "masked_frames")      # inputs kept in the golden file


def clamp_range(bf=BF, dist_list=DIST_LIST):
    inv = bf / torch.Tensor(dist_list)
    return float(torch.min(inv)), float(torch.max(inv))


def make_inputs(name):
    """-> dict(preds, target [B, 1, H, W] fp32, mask [B, 1, H, W] bool or None, label_range (lo, hi) or None)"""
    B, H, W, kind = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    coarse = torch.rand(B, 1, -(-H // 8) + 2, -(-W // 8) + 2, generator=g, dtype=torch.float64)
    field = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    lo, hi = field.amin((1, 2, 3), keepdim=True), field.amax((1, 2, 3), keepdim=True)
    field = ((field - lo) / (hi - lo)) ** 3              # every frame spans the whole of [2, 62], with room near 2: SSIM_CONDITION
    target = (2.0 + 60.0 * field).to(torch.float32)
    noise_m = torch.randn(B, 1, H, W, generator=g, dtype=torch.float32)
    noise_a = torch.randn(B, 1, H, W, generator=g, dtype=torch.float32)
    preds = torch.clamp(target * (1.0 + 0.05 * noise_m) + 0.3 * noise_a, min=0.3)
    mask, label_range = None, None
    if kind in ("mask", "frames"):
        mask = torch.rand(B, 1, H, W, generator=g) < 0.7
        if kind == "frames":
            mask[1] = False
            mask[2] = True
    elif kind == "range":
        label_range = LABEL_RANGE
    return dict(preds=preds.contiguous(), target=target.contiguous(), mask=mask, label_range=label_range)


def validity(inp):
    """The case's validity as a mask tensor (what the reference's classes take), or None."""
    if inp["mask"] is not None:
        return inp["mask"]
    if inp["label_range"] is not None:
        lo, hi = inp["label_range"]
        return (inp["target"] >= lo) & (inp["target"] <= hi)
    return None


def gauss_taps(dtype=torch.float64):
    k = torch.arange(-5, 6, dtype=dtype)
    g = torch.exp(-((k / 1.5) ** 2) / 2)
    return g / g.sum()


def forms(preds, target, bf, cmin, cmax):
    """-> [(P, T) direct, (P, T) distance], fp32, the reference's arithmetic element by element"""
    out = []
    for inverse in (False, True):
        p, t = (1.0 / preds, 1.0 / target) if inverse else (preds, target)
        out.append((p / bf, torch.clamp(t, cmin, cmax) / bf))
    return out


def _ssim_maps(P, T, c1, c2, dtype):
    """P, T [B, H, W] in dtype, c1 / c2 [B] -> the map [B, H - 10, W - 10]"""
    g = gauss_taps(dtype)
    Wn, Hn = P.shape[2] - 10, P.shape[1] - 10

    def filt(X):
        h = sum(g[k] * X[:, :, k:k + Wn] for k in range(11))
        return sum(g[k] * h[:, k:k + Hn, :] for k in range(11))
    muP, muT, mPP, mTT, mPT = filt(P), filt(T), filt(P * P), filt(T * T), filt(P * T)
    sP, sT, sPT = mPP - muP * muP, mTT - muT * muT, mPT - muP * muT
    c1, c2 = c1.view(-1, 1, 1), c2.view(-1, 1, 1)
    return ((2 * muP * muT + c1) * (2 * sPT + c2)) / ((muP * muP + muT * muT + c1) * (sP + sT + c2))


def _sum(x, dtype):
    if dtype == torch.float64:
        return math.fsum(x.to(torch.float64).flatten().tolist())
    return float(torch.sum(x.to(dtype)))


def restate(preds, target, mask=None, label_range=None, bf=BF, cmin=None, cmax=None, thresh=THRESH, thresh_dist=THRESH_DIST, scope="frame",
            dtype=torch.float64):
    """-> np.float64 [B + 1, 9]: COLUMNS for every frame, row B pooled."""
    if cmin is None:
        cmin, cmax = clamp_range(bf)
    B, H, W = preds.shape[0], preds.shape[-2], preds.shape[-1]
    preds, target = preds.reshape(B, H, W), target.reshape(B, H, W)
    if mask is not None:
        v = mask.reshape(B, H, W).bool()
    elif label_range is not None:
        v = (target >= label_range[0]) & (target <= label_range[1])
    else:
        v = torch.ones(B, H, W, dtype=torch.bool)
    unmasked = mask is None and label_range is None
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    out = np.full((B + 1, 9), np.nan, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for f, ((P, T), th) in enumerate(zip(forms(preds, target, bf, cmin, cmax), (thresh, thresh_dist))):
            e = P - T
            a, s = e.abs(), e * e
            bad = a > th                                      # the fp32 tensor against fp32(thresh)
            S2 = [_sum(s[b][v[b]], dtype) for b in range(B)]
            S1 = [_sum(a[b][v[b]], dtype) for b in range(B)]
            NB = [int(bad[b][v[b]].sum()) for b in range(B)]
            n = [int(v[b].sum()) for b in range(B)]
            S2.append(_sum(s[v], dtype)), S1.append(_sum(a[v], dtype))
            NB.append(sum(NB)), n.append(sum(n))
            for r in range(B + 1):
                nn = np_dt(n[r])
                out[r, 4 * f + 0] = np.sqrt(np_dt(S2[r]) / nn)
                out[r, 4 * f + 1] = np_dt(S1[r]) / nn
                out[r, 4 * f + 2] = np_dt(NB[r]) / np_dt(H * W) if unmasked else (np_dt(NB[r]) / nn if n[r] > 0 else 1.0)
                out[r, 8] = n[r]
            if H >= 11 and W >= 11:
                Pd, Td = P.to(dtype), T.to(dtype)
                if scope == "batch":
                    R = torch.maximum(Pd.max() - Pd.min(), Td.max() - Td.min()).expand(B)
                else:
                    R = torch.maximum(Pd.amax((1, 2)) - Pd.amin((1, 2)), Td.amax((1, 2)) - Td.amin((1, 2)))
                m = _ssim_maps(Pd, Td, (0.01 * R) ** 2, (0.03 * R) ** 2, dtype)
                per = m.mean((1, 2))
                out[:B, 4 * f + 3] = per.to(torch.float64).numpy()
                out[B, 4 * f + 3] = float(per.mean())
    return out


def check_condition(preds, target, bf=BF, cmin=None, cmax=None):
    """SSIM_CONDITION for one set of inputs -> the largest max(|P|, |T|) / R over frames and forms (asserted <= 2)."""
    if cmin is None:
        cmin, cmax = clamp_range(bf)
    B, H, W = preds.shape[0], preds.shape[-2], preds.shape[-1]
    worst = 0.0
    for P, T in forms(preds.reshape(B, H, W), target.reshape(B, H, W), bf, cmin, cmax):
        P, T = P.double(), T.double()
        R = torch.maximum(P.amax((1, 2)) - P.amin((1, 2)), T.amax((1, 2)) - T.amin((1, 2)))
        ratio = torch.maximum(P.abs().amax((1, 2)), T.abs().amax((1, 2))) / R
        worst = max(worst, float(ratio.max()))
    assert worst <= 2.0, worst
    return worst


def exact_inputs(B=2, H=24, W=52, seed=7):
    """The exact-operand case: bf = 64, a dist_list of powers of two, every value a multiple of 1/8 in [1, 64].  P - T is then a
    multiple of 2^-9 below 1 in the direct form, so e * e and every partial sum are exact in any order.
    -> dict(preds, target, mask, bf, dist_list)"""
    g = torch.Generator().manual_seed(seed)
    target = torch.randint(8, 513, (B, 1, H, W), generator=g).to(torch.float32) / 8
    preds = torch.randint(8, 513, (B, 1, H, W), generator=g).to(torch.float32) / 8
    mask = torch.rand(B, 1, H, W, generator=g) < 0.6
    return dict(preds=preds, target=target, mask=mask, bf=64.0, dist_list=[1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0])
