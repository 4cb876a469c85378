"""Exact-arithmetic operands for the convolution kernels (no GPU needed).

The split kernels compute x = hi + lo per operand and hi*hi + hi*lo + lo*hi with fp32 accumulation (csrc/split_fmt.hpp).  On
operands for which every product and every partial sum is exactly representable, any correct kernel -- whatever its summation
order, with or without FMA, direct, polyphase or Winograd -- returns the bits of a float64 reference.  This module builds such
operands, the float64 reference, and asserts the conditions that make the claim true (they are conditions, not tolerances):

  (a) conv(|x_hi| + |x_lo|, |w_hi| + |w_lo|).max() < 2^24 in units of the operands' common lsb: every partial sum of every
      product stream, in any order, is an integer below 2^24 (x the lsb) and so an fp32 number;
  (b) the accumulator and its scaled, shifted, residual-added and activated values are fp32 numbers: v == v.float().double();
  (c) outputs stay inside the range of the format they are delivered in (+-65504 for fp16 pieces, +-16376 for fp32-padded
      records); the per-channel power-of-two scale is picked for that.

Recipes.  "narrow": integers of at most 3 bits (bf16 split, fp32 kernels: |v| <= 7; fp16 split: |v| <= 3).  "wide": integers with
more significant bits than `hi` holds (bf16: |v| <= 1023, fp16: |v| <= 4095), so that lo != 0.  The dropped lo*lo term must be
zero, so every split case exists in two regimes, `x_wide` (w narrow) and `w_wide` (x narrow): together both cross terms.  A wide
operand is wide at a `density` of its elements and narrow elsewhere; the density starts at 1 and is halved until (a) holds, so that
(a) is met by construction on deep layers and trilinear forms.  Trilinear forms (fused x2 upsample, polyphase) have coefficients
k/64: the x_wide regime keeps w a multiple of 64, the w_wide regime keeps x a multiple of 64 (the upsampled activation then has
no lo part).  Winograd F(2x2, 3x3) carries 1/2 per axis in G: w is a multiple of 4 and (a) and the split are checked on the
transformed operands.  The Winograd form of the polyphase layer has a domain of its own (V_up, U: polywino_operands) in which
the split and (a) are asserted as well, with narrower wide operands.  The 2-D residual block has a third regime, w2_wide.  Epilogue: per-channel scale a power of two that varies by channel, integer shift and residual, neg_slope
in {0, 1, 0.25, 0.5}.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

TWO24 = float(1 << 24)
F16_MAX = 65504.0
F32P_MAX = 16376.0
SPLIT_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
WIDE_MAX = {"bf16": 1023, "f16": 4095, "f32": 1023}
NARROW_MAX = {"bf16": 7, "f16": 3, "f32": 7}
REGIMES = ("x_wide", "w_wide")
SLOPES = (0.25, 0.0, 1.0, 0.5)


# ------------------------------------------------------------------------------------------------ the split, emulated with torch
def split(y: torch.Tensor, fmt: str):
    """(hi, lo) of csrc/split_fmt.hpp with torch on the CPU: hi = dt(y), lo = dt(y - hi), the fp16 clamp first."""
    y = y.float()
    if fmt == "f16":
        y = y.clamp(-F16_MAX, F16_MAX)
    hi = y.to(SPLIT_DT[fmt]).float()
    lo = (y - hi).to(SPLIT_DT[fmt]).float()
    return hi, lo


def split_join(y: torch.Tensor, fmt: str) -> torch.Tensor:
    """What a reader of a split output sees: hi + lo (fp32)."""
    hi, lo = split(y, fmt)
    return hi + lo


# ------------------------------------------------------------------------------------------------ operand recipes
def narrow(rng, shape, amax: int) -> torch.Tensor:
    return torch.from_numpy(rng.integers(-amax, amax + 1, shape).astype(np.float64))


def wide(rng, shape, fmt: str, density: float, amax=None) -> torch.Tensor:
    """Integers up to WIDE_MAX[fmt] (or `amax`) at `density` of the elements, narrow ones elsewhere (the same draws at every density)."""
    amax = amax or WIDE_MAX[fmt]
    big = rng.integers(-amax, amax + 1, shape).astype(np.float64)
    small = rng.integers(-NARROW_MAX[fmt], NARROW_MAX[fmt] + 1, shape).astype(np.float64)
    pick = rng.random(shape) < density
    return torch.from_numpy(np.where(pick, big, small))


def representable(v: torch.Tensor) -> bool:
    return bool(torch.equal(v.float().double(), v))


def _conv(x, w, stride):
    return (F.conv3d if x.dim() == 5 else F.conv2d)(x, w, None, stride=stride, padding=w.shape[-1] // 2)


def _up2(x):
    return F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=False)


# ------------------------------------------------------------------------------------------------ Winograd F(2x2, 3x3) x direct D
_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
_G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def wino_operands(x, w, absolute=False):
    """The transformed operands of conv3d_wino: V = B^T d B per 4x4 (H, W) tile of the padded input [B, C, D+2, H/2, W/2, 4, 4] and
    U = G g G^T [O, I, 3, 4, 4].  `absolute`: |B^T| |d| |B| and |G| |g| |G^T|, which bound every partial sum of the transforms."""
    bt, g = (_BT.abs(), _G.abs()) if absolute else (_BT, _G)
    xp = F.pad(x.abs() if absolute else x, (1, 1, 1, 1, 1, 1))
    tiles = xp.unfold(3, 4, 2).unfold(4, 4, 2)
    V = torch.einsum("ai,bcdhwij,ej->bcdhwae", bt, tiles, bt)
    U = torch.einsum("ah,oidhw,bw->oidab", g, w.abs() if absolute else w, g)
    return V, U


def wino_abs_sum(x, w) -> float:
    """max over outputs of |A^T| (sum_cin,kd |V| |U|) |A|: the bound of condition (a) in the transformed domain."""
    V, U = wino_operands(x, w, absolute=True)
    D = x.shape[2]
    M = sum(torch.einsum("bcdhwae,ocae->bodhwae", V[:, :, kd:kd + D], U[:, :, kd]) for kd in range(3))
    return float(torch.einsum("pa,bodhwae,qe->bodhwpq", _AT.abs(), M, _AT.abs()).max())


# ------------------------------------------------------------------------------------------------ polyphase ResizeConv3d
# The polyphase kernels never upsample: they multiply the LOW-resolution x with folded weights W_eff = (M_d x M_h x M_w) w, where
# the 3x3 matrices M[t][k] hold the coefficient of x[i + t - 1] in up[2 i + p + k - 1] (restated here from first principles: the
# 0.25 / 0.75 blend, ATen's source-index clamp, the zero padding of the upsampled grid).  The split is taken of the FOLDED
# weights, so "exactly one operand has a lo part" must hold for them: every set a matrix-core kernel multiplies is built below --
# (pd, D class) x interior matrices along H and W (main kernel), and the centre-row differences on the H and W faces.
def _axis_matrix(p: int, i: int, n: int) -> np.ndarray:
    M = np.zeros((3, 3))
    for k in range(3):
        v = 2 * i + p + k - 1
        if 0 <= v < 2 * n:
            m = v >> 1
            for s, c in (((m - 1, 0.25), (m, 0.75)) if v % 2 == 0 else ((m, 0.75), (m + 1, 0.25))):
                M[min(max(s, 0), n - 1) - i + 1][k] += c
    return M


@functools.lru_cache(maxsize=None)
def _poly_fold_matrices() -> torch.Tensor:
    """[sets, 27 folded taps, 27 taps]: every (M_d x M_h x M_w) of the main and face kernels."""
    cls = {"first": (0, 4), "int": (1, 4), "last": (3, 4), "only": (0, 1)}
    cm = {(p, c): _axis_matrix(p, *cls[c]) for p in range(2) for c in cls}

    def delta(p, c):
        d = np.zeros((3, 3))
        d[1] = (cm[p, c] - cm[p, "int"])[1]
        return d
    out = []
    for pd in range(2):
        for cd in cls:
            for ph in range(2):
                for pw in range(2):
                    trip = [(cm[ph, "int"], cm[pw, "int"])]
                    trip += [(delta(ph, c), cm[pw, "int"]) for c in ("first", "last", "only")]
                    trip += [(cm[ph, "int"], delta(pw, c)) for c in ("first", "last", "only")]
                    out += [np.einsum("ak,bl,cm->abcklm", cm[pd, cd], mh, mw).reshape(27, 27) for mh, mw in trip]
    return torch.from_numpy(np.stack(out))


def poly_folded(w: torch.Tensor) -> torch.Tensor:
    """w [O, I, 3, 3, 3] -> every folded weight the polyphase kernels split: [sets, O, I, 27] (float64, exact: dyadic)."""
    return torch.einsum("sqk,oik->soiq", _poly_fold_matrices(), w.reshape(*w.shape[:2], 27))


def _poly_bad_filters(w, fmt, regime):
    """(o, i) filters whose folded weights break the split's conditions: a lo part where w is the narrow operand, more bits than
    hi + lo holds where it is the wide one."""
    f = poly_folded(w)
    hi, lo = split(f, fmt)
    bad = (lo != 0) if regime == "x_wide" else ((hi + lo).double() != f)
    return bad.any(dim=3).any(dim=0)


# ---- the Winograd form of the polyphase layer (csrc/conv3d_wino_up2.hip) multiplies neither of the above.  Per (H, W) phase
# (ph, pw) it multiplies V_up, the trilinear blend ALONG D of the transformed low-resolution planes X_j = B^T x_j B
# (V_up[0] = X_0, V_up[2j+1] = 0.75 X_j + 0.25 X_(j+1), V_up[2j+2] = 0.25 X_j + 0.75 X_(j+1), V_up[2D-1] = X_(D-1), zero planes
# outside), split in fp16, by U = G ((M_h x M_w) w[kd]) G^T with the INTERIOR matrices (the faces arrive as corrections from the
# face kernels above), and takes y = A^T [sum_cin,kd U_kd (.) V_up[o + kd - 1]] A.  V_up is a multiple of 1/4 (x_wide) or of 16
# (w_wide, x = 64 j) and U an integer or a multiple of 1/64: the products' lsb is 1/4 in both regimes.
POLYWINO_LSB = 0.25
# wide operands of this form: |x| <= 767 (one wide voxel alone gives V_up = 0.75 x = n / 4 with n up to 2301: 12 bits, a lo part),
# |w| <= 255 (U has 6 more fractional bits); the 12 bits of the other fp16 cases put ONE product stream (12 + 2 bits of V_up, 7 of
# U, 3 of A^T . A) beyond 2^24 lsb in this domain.  In the x_wide regime half of the narrow weights are zero for the same reason.
POLYWINO_WIDE_MAX = {"x_wide": 767, "w_wide": 255}


def polywino_operands(x, w, absolute=False):
    """-> V_up [B, C, 2D + 2, H/2, W/2, 4, 4], U [ph, pw, O, I, 3, 4, 4] (float64, exact).  `absolute`: every transform and blend on
    absolute values with absolute coefficients, which bounds every partial sum."""
    X = wino_operands(x, w, absolute)[0][:, :, 1:-1]
    D = X.shape[2]
    planes = [X[:, :, 0]]
    for j in range(D - 1):
        planes += [0.75 * X[:, :, j] + 0.25 * X[:, :, j + 1], 0.25 * X[:, :, j] + 0.75 * X[:, :, j + 1]]
    planes.append(X[:, :, D - 1])
    zero = torch.zeros_like(planes[0])
    V = torch.stack([zero] + planes + [zero], dim=2)
    g = _G.abs() if absolute else _G
    M = [torch.from_numpy(_axis_matrix(p, 1, 4)) for p in range(2)]      # interior class, [t][k]
    ww = w.abs() if absolute else w
    U = torch.stack([torch.stack([torch.einsum("ab,ec,bl,cm,oidlm->oidae", g, g, M[ph], M[pw], ww) for pw in range(2)])
                     for ph in range(2)])
    return V, U


def _polywino_y(V, U, at):
    """y[ph, pw] = A^T (sum_cin,kd U_kd (.) V_up[o + kd - 1]) A -> [2, 2, B, O, 2D, H/2, W/2, 2, 2]."""
    n = V.shape[2] - 2
    return torch.stack([torch.stack([
        torch.einsum("pa,bodhwae,qe->bodhwpq", at, sum(torch.einsum("bcdhwae,ocae->bodhwae", V[:, :, kd:kd + n], U[ph, pw][:, :, kd])
                                                       for kd in range(3)), at) for pw in range(2)]) for ph in range(2)])


def polywino_abs_sum(x, w) -> float:
    """The bound of condition (a) in the domain of the Winograd-form polyphase kernel, in real units (lsb POLYWINO_LSB)."""
    V, U = polywino_operands(x, w, absolute=True)
    return float(_polywino_y(V, U, _AT.abs()).max())


def polywino_to_volume(y):
    """[ph, pw, B, O, 2D, H/2, W/2, 2, 2] (cell (2r + p, 2n + q) of phase (ph, pw)) -> [B, O, 2D, 2H, 2W]."""
    _, _, B, O, D2, hh, wh, _, _ = y.shape
    y = y.permute(2, 3, 4, 5, 7, 0, 6, 8, 1)          # B, O, d, r, p, ph, n, q, pw
    return y.reshape(B, O, D2, 4 * hh, 4 * wh)


# ------------------------------------------------------------------------------------------------ one case
def _at_most_one_lo(a, b, fmt):
    (ahi, alo), (bhi, blo) = split(a, fmt), split(b, fmt)
    assert torch.equal((ahi + alo).double(), a) and torch.equal((bhi + blo).double(), b), "hi + lo != operand"
    assert not (bool(alo.any()) and bool(blo.any())), "both operands have a lo part: the dropped lo*lo term is not zero"
    return ahi.double(), alo.double(), bhi.double(), blo.double()


def _exactly_one_lo(a, b, fmt):
    (ahi, alo), (bhi, blo) = split(a, fmt), split(b, fmt)
    assert torch.equal((ahi + alo).double(), a) and torch.equal((bhi + blo).double(), b), "hi + lo != operand"
    assert bool(alo.any()) != bool(blo.any()), f"lo parts: x {bool(alo.any())}, w {bool(blo.any())} (exactly one must be non-zero)"
    return ahi.double(), alo.double(), bhi.double(), blo.double()


def frame_index(B: int, F: int, seed: int) -> np.ndarray:
    """A length-B sequence over range(F), drawn from the seed (redrawn until the conditions hold; asserted):
      - idx[b] != idx[b - 1] for every b: neighbouring frames always differ, so a read across a frame boundary, or a shift by ANY
        fixed number of frames, cannot land on an identical frame everywhere (the sequence is not periodic);
      - every frame occurs;
      - for B >= 32 (and F <= 4: 12 ordered pairs at most), every ordered pair of distinct frames occurs as neighbours."""
    assert 1 <= F <= B
    if F == 1:
        assert B == 1, "a sequence over one frame repeats it"
        return np.zeros(1, dtype=np.int64)
    rng = np.random.default_rng([seed, B, F])
    want_pairs = B >= 32 and F <= 4
    for _ in range(10000):
        idx = np.empty(B, dtype=np.int64)
        idx[:F] = rng.permutation(F)
        for b in range(F, B):
            idx[b] = (idx[b - 1] + 1 + rng.integers(0, F - 1)) % F
        pairs = set(zip(idx[:-1].tolist(), idx[1:].tolist()))
        periodic = any(np.array_equal(idx[p:], idx[:-p]) for p in range(1, B // 2 + 1)) if B > F >= 3 else False
        if (not want_pairs or len(pairs) == F * (F - 1)) and not periodic:
            break
    else:
        raise AssertionError(f"no frame sequence for B = {B}, F = {F}")
    check_frame_index(idx, B, F)
    return idx


def check_frame_index(idx, B: int, F: int) -> None:
    idx = np.asarray(idx)
    assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < F
    assert bool((idx[1:] != idx[:-1]).all()), "two neighbouring frames are the same frame"
    assert set(idx.tolist()) == set(range(F)), "a frame does not occur"
    if B >= 32 and F <= 4:
        pairs = set(zip(idx[:-1].tolist(), idx[1:].tolist()))
        assert len(pairs) == F * (F - 1), "an ordered pair of distinct frames never occurs as neighbours"
    for p in range(1, B // 2 + 1) if B > F >= 3 else ():      # (two frames can only alternate)
        assert not np.array_equal(idx[p:], idx[:-p]), f"the sequence repeats with period {p}"


def make_case(fmt, regime, B, Cin, Cout, dims, stride=1, res=False, slope=0.25, up2=False, wino=False, poly=False, polywino=False,
              bound=None, k=3, shift=True, fold_scale=False, seed=0, frames=None):
    """Operands, float64 reference and conditions (a)-(c) of act(conv(x [, upsampled x2]) * scale + shift (+ res)).

    fmt: 'bf16' | 'f16' (the split the kernel multiplies in) | 'f32' (an fp32 kernel: no split, no regimes needed but both run).
    bound: range of the delivered output (F16_MAX, F32P_MAX) or None for plain fp32.  fold_scale: the kernel's packer folds the
    scale into the weights (exact: a power of two).  poly: a polyphase kernel multiplies the case -- the filters whose FOLDED weights
    break the split's conditions are drawn again (a few in a million folded weights need 9 bits).  polywino: the Winograd form of
    the polyphase layer multiplies the case: wide operands of 8 bits, and (a) and the split are ALSO met in its own domain
    (polywino_operands).  Returns a namespace of float32 tensors in NC(D)HW order (x, w, scale, shift,
    r) plus `acc` and `ref` (float64) and the figures of the conditions.

    frames=F: a launch-size case.  Operands, the convolution and every condition above are built and asserted for min(F, B) DISTINCT
    frames; the kernel sees them B times in the irregular order `idx` (frame_index), x = x_F[idx], and the reference is expanded by
    the same index.  Frames of a batch are independent and (a)-(c), the split identities and "ATen fp32 == float64" are per-frame
    properties: they hold for the batch when they hold for the F frames.  The residual is NOT periodic: it is drawn for all B
    frames and added to the expanded accumulator (a frame mix-up in the residual's addressing shows); (b) and (c) are asserted on
    the expanded stages.  The case also carries idx, n_frames and the F-frame operands x_frames."""
    assert regime in REGIMES and slope in SLOPES
    nd = len(dims)
    idx = None
    if frames is not None:
        idx = frame_index(B, min(frames, B), seed)
        B_all, B = B, min(frames, B)
    xshape, wshape = (B, Cin, *dims), (Cout, Cin) + (k,) * nd
    w_unit = 4 if wino else 1
    wmax = POLYWINO_WIDE_MAX[regime] if polywino else None
    for halvings in range(9):
        density = 0.5 ** halvings
        rng = np.random.default_rng(seed)
        if regime == "x_wide":
            x = wide(rng, xshape, fmt, density, wmax)
            w = narrow(rng, wshape, 1 if up2 else NARROW_MAX[fmt]) * (64 if up2 else w_unit)
            if polywino:
                w = w * torch.from_numpy((rng.random(wshape) < 0.5).astype(np.float64))
        else:
            x = narrow(rng, xshape, 3 if up2 else NARROW_MAX[fmt]) * (64 if up2 else 1)      # (x_up <= 192: 8 bits)
            w = wide(rng, wshape, fmt, density, wmax) * w_unit
        for _ in range(50 if poly else 0):
            bad = _poly_bad_filters(w, fmt, regime)
            if not bool(bad.any()):
                break
            fresh = narrow(rng, wshape, 1) * 64 if regime == "x_wide" else wide(rng, wshape, fmt, density, wmax)
            w = torch.where(bad.view(Cout, Cin, 1, 1, 1), fresh, w)
        if wino:
            abs_sum = wino_abs_sum(x, w)
        else:
            abs_sum = float(_conv(_up2(x.abs()) if up2 else x.abs(), w.abs(), stride).max())
        if polywino:
            abs_sum = max(abs_sum, polywino_abs_sum(x, w) / POLYWINO_LSB)
        if abs_sum < 0.7 * TWO24:       # head room for |hi| + |lo| >= |x| and for the epilogue's adds
            break
    else:
        raise AssertionError(f"condition (a) not reachable: {abs_sum / TWO24:.2f} x 2^24 at density {density}")
    xin = _up2(x) if up2 else x                      # what the convolution multiplies
    if up2:
        assert torch.equal(_up2(x.float()).double(), xin), "trilinear x2 is not exact in fp32 on these operands"
    acc = _conv(xin, w, stride)
    c = types.SimpleNamespace(fmt=fmt, regime=regime, density=density, stride=stride, slope=slope, up2=up2, wino=wino, polywino=polywino, bound=bound,
                              x=x.float(), w=w.float(), xin=xin, w64=w, acc=acc)
    # ---- the split: hi + lo == operand, exactly one operand has a lo part; (a) on |hi| + |lo|; the three-product formula
    if fmt != "f32":
        a, b = wino_operands(x, w) if wino else (xin, w)
        if wino:
            assert float(a.abs().max()) <= F16_MAX      # (U is pre-scaled by the packer with a power of two per cout: the same lo bits)
        # (8-bit operands of the Winograd-form polyphase cases have no lo part before the transforms: checked in its domain below)
        ahi, alo, bhi, blo = (_at_most_one_lo if polywino else _exactly_one_lo)(a, b, fmt)
        if polywino:
            # the face and edge kernels multiply the low-resolution x with the 3-D folded weights (8-bit x has no lo part in fp16) ...
            _at_most_one_lo(x, poly_folded(w), fmt)
            # ... the main kernel V_up with U: split conditions, (a) in lsb units, and the domain itself against the reference
            V, U = polywino_operands(x, w)
            assert float(V.abs().max()) <= F16_MAX
            Vh, Vl, Uh, Ul = _exactly_one_lo(V, U, fmt)
            c.polywino_abs_sum = float(_polywino_y(Vh.abs() + Vl.abs(), Uh.abs() + Ul.abs(), _AT.abs()).max()) / POLYWINO_LSB
            assert c.polywino_abs_sum < TWO24, f"condition (a), Winograd-form polyphase domain: {c.polywino_abs_sum / TWO24:.3f} x 2^24"
            y3 = _polywino_y(Vh, Uh, _AT) + _polywino_y(Vh, Ul, _AT) + _polywino_y(Vl, Uh, _AT)
            assert torch.equal(y3, _polywino_y(V, U, _AT)) and torch.equal(torch.round(y3 / POLYWINO_LSB), y3 / POLYWINO_LSB)
            inner = (slice(None), slice(None), slice(None), slice(2, -2), slice(2, -2))      # cells off the H and W faces
            assert torch.equal(polywino_to_volume(y3)[inner], acc[inner]), "Winograd-form polyphase domain != interpolate -> conv"
        elif poly:      # the operands the polyphase kernels split: the low-resolution x and the folded weights
            _exactly_one_lo(x, poly_folded(w), fmt)
        if wino:
            c.abs_sum = abs_sum * (1 + 2.0 ** -10)      # the transformed domain; |hi| + |lo| <= |v| (1 + 2^-10) in the fp16 split
            Vh, Vl, Uh, Ul = ahi, alo, bhi, blo
            D = x.shape[2]

            def m(vv, uu):
                return sum(torch.einsum("bcdhwae,ocae->bodhwae", vv[:, :, kd:kd + D], uu[:, :, kd]) for kd in range(3))
            three = torch.einsum("pa,bodhwae,qe->bodhwpq", _AT, m(Vh, Uh) + m(Vh, Ul) + m(Vl, Uh), _AT)
            three = three.permute(0, 1, 2, 3, 5, 4, 6).reshape(acc.shape)
        else:
            c.abs_sum = float(_conv(ahi.abs() + alo.abs(), bhi.abs() + blo.abs(), stride).max())
            three = _conv(ahi, bhi, stride) + _conv(ahi, blo, stride) + _conv(alo, bhi, stride)
        assert torch.equal(three, acc), "hi*hi + hi*lo + lo*hi != the full convolution"
    else:
        c.abs_sum = abs_sum
    if polywino:
        c.abs_sum = max(c.abs_sum, c.polywino_abs_sum)
    c.abs_sum_frac = c.abs_sum / TWO24
    assert c.abs_sum < TWO24, f"condition (a): {c.abs_sum_frac:.3f} x 2^24"
    assert torch.equal(torch.round(acc), acc), "products are not integers (x_up = m / 64 against w = 64 j in the trilinear forms)"
    # ---- ATen in fp32 (another summation order) returns the float64 bits
    aten = _conv(_up2(x.float()) if up2 else x.float(), w.float(), stride)
    assert torch.equal(aten.double(), acc), "ATen fp32 != float64"
    if idx is not None:      # the batch the kernel sees: the F frames in the order idx (the residual below is drawn for all B frames)
        c.idx, c.n_frames, c.x_frames = idx, B, c.x
        sel = torch.from_numpy(idx)
        c.x, c.acc = c.x[sel], acc[sel]
        c.xin = None                     # (per-frame intermediates are not expanded)
        acc, B = c.acc, B_all
    # ---- epilogue: power-of-two scale per channel, integer shift / residual; (b) at every stage, (c) on the result
    amax = float(acc.abs().max())
    k2 = 0
    if bound is not None:
        while (amax + 64.0) * 2.0 ** (1 - k2) >= bound:
            k2 += 1
    rng = np.random.default_rng(seed + 1)
    scale = torch.tensor([2.0 ** (1 - (ch % 3) - k2) for ch in range(Cout)], dtype=torch.float64)
    shift_v = narrow(rng, (Cout,), 15) if shift else torch.zeros(Cout, dtype=torch.float64)
    r = narrow(rng, tuple(acc.shape), 31) if res else None
    bc = (1, -1) + (1,) * nd
    stages = [acc, acc * scale.view(bc)]
    stages.append(stages[-1] + shift_v.view(bc))
    if res:
        stages.append(stages[-1] + r)
    stages.append(torch.where(stages[-1] > 0, stages[-1], stages[-1] * slope))
    for i, v in enumerate(stages):
        assert representable(v), f"condition (b): epilogue stage {i} is not an fp32 number"
    if fold_scale:      # scale folded into the weights: w * scale must be exact too (it is: a power of two)
        assert representable(w * scale.view((-1, 1) + (1,) * nd))
    c.ref = stages[-1]
    c.out_max = float(c.ref.abs().max())
    if bound is not None:
        assert c.out_max < bound, f"condition (c): |out| {c.out_max} reaches {bound}"
        if r is not None:
            assert float(r.abs().max()) < bound
    c.scale, c.shift, c.r = scale.float(), shift_v.float(), (None if r is None else r.float())
    return c


def expected_split(ref64: torch.Tensor, fmt: str) -> np.ndarray:
    """An output delivered in split form: hi + lo of the exact reference, by the torch emulation (not the library's converter)."""
    assert representable(ref64)
    return split_join(ref64.float(), fmt).numpy()


# ------------------------------------------------------------------------------------------------ comparison
def mismatch_report(got, want, lsb: float = 1.0) -> str:
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = ~(got == want)
    if not bad.any():
        return ""
    first = tuple(int(i) for i in np.argwhere(bad)[0])
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = np.nanmax(np.where(bad, d, 0.0)) / lsb
    return (f"{int(bad.sum())} of {bad.size} elements differ; first at {first}: got {got[first]!r}, want {want[first]!r}; "
            f"largest difference {worst:g} lsb (lsb {lsb:g})" + ("; NaN in the output" if np.isnan(got).any() else ""))


def assert_exact(got, want, lsb: float = 1.0, what: str = "") -> None:
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(got, want), f"{what}: {mismatch_report(got, want, lsb)}"


# ------------------------------------------------------------------------------------------------ the case table
# family -> list of (case id, make_case keyword arguments).  Shapes: the two or three smallest ragged shapes of each family's
# oracle test in tests/test_gpu_parity.py.  tests/test_exact_cases_host.py walks the whole table on the CPU;
# tests/test_gpu_exact.py builds the same cases (cached) before it calls the kernels.
def _c3(B, Cin, Cout, D, H, W, stride=1, res=False, **kw):
    return dict(B=B, Cin=Cin, Cout=Cout, dims=(D, H, W), stride=stride, res=res, **kw)


def _c2(B, Cin, Cout, H, W, stride=1, res=False, **kw):
    return dict(B=B, Cin=Cin, Cout=Cout, dims=(H, W), stride=stride, res=res, **kw)


CONV3D_SHAPES = [(2, 16, 16, 5, 9, 11, 1, True), (1, 16, 32, 7, 9, 13, 2, False), (1, 32, 32, 4, 6, 10, 1, True),
                 (1, 64, 16, 4, 8, 32, 1, False), (1, 48, 96, 4, 8, 12, 2, False), (1, 128, 128, 2, 5, 9, 1, True),
                 (1, 32, 384, 1, 10, 40, 1, True)]
CONV3D_DIRECT_ODD = [(2, 5, 3, 5, 7, 9, 1, False), (2, 4, 8, 5, 7, 9, 1, True)]          # odd Cin / Cout: the direct kernel only
CONV3D_V32_SHAPES = [(3, 32, 32, 9, 37, 70, 1, False), (17, 16, 96, 4, 12, 32, 1, False)]   # the two smallest the 32x32x16 schedule takes
CONV3D_OUT_SPLIT_SHAPES = [(2, 16, 32, 7, 9, 13, 2, False), (1, 32, 32, 4, 6, 10, 1, True), (1, 16, 16, 5, 9, 11, 1, False)]
UP2_SHAPES = [(2, 32, 16, 3, 5, 9, False), (1, 128, 64, 1, 3, 5, True), (1, 64, 32, 2, 6, 8, True),
              # the smallest launches that reach the 32-channel-slice forms (d32u, and d32u_dk out of a one-plane level) and the 32x32x16 schedule
              (1, 32, 96, 3, 10, 24, True), (3, 32, 96, 1, 10, 24, False), (6, 16, 64, 4, 8, 32, False)]
RS_SHAPES = [(1, 2, 4, 16), (2, 5, 7, 37), (3, 3, 9, 16)]
RS16_SHAPES = [(1, 4, 4, 16), (2, 5, 7, 37)]
S2RS_SHAPES = [(1, 2, 2, 16), (1, 5, 7, 19), (3, 2, 9, 33)]
WINO_SHAPES = [(1, 8, 2, 32), (2, 8, 6, 64), (2, 16, 4, 32)]
POLY_SHAPES = [(1, 1, 1, 1), (1, 2, 2, 2), (1, 3, 5, 7), (3, 5, 9, 33)]
POLY_WINO_SHAPES = [(1, 8, 2, 32), (3, 8, 6, 32)]
HEAD_F32_SHAPES = [(2, 16, 5, 7, 9, False), (2, 64, 5, 7, 9, True)]          # the fp32 LDS-tiled cost head behind H.conv3d at Cout = 1
HEAD_SHAPES = [(1, 16, 1, 1, 1), (1, 16, 3, 5, 7), (1, 32, 4, 9, 33)]
CONV2D_SHAPES = [(2, 16, 16, 20, 36, 1, True), (1, 16, 16, 33, 47, 1, False), (2, 16, 16, 24, 40, 2, False)]
# channel counts whose Cout / 16 leaves a remainder against the two-tile templates of the split kernel (3 under D2_N32 and its
# stride-2 form, 5 under D2_N64), and 16 -> 32; the fp32 MFMA kernel takes the rows with Cout in (16, 32), out_split those with 16
CONV2D_WIDE_SHAPES = [(1, 32, 32, 9, 21, 2, False), (1, 48, 48, 9, 21, 1, True), (1, 48, 48, 10, 22, 2, False), (1, 80, 80, 5, 19, 1, False),
                      (1, 16, 32, 9, 21, 1, False)]
# (B, Cin, Cout, H, W, stride, res, k, NCHW input): the direct kernel alone -- a Cout % 4 != 0 tail group, k of 1, 5 and 7, and the
# generic NCHW stem (in_chs of 1 and 4)
CONV2D_DIRECT_ROWS = [(2, 6, 6, 9, 13, 1, True, 3, False), (1, 8, 8, 9, 13, 2, False, 3, False), (1, 16, 16, 9, 13, 1, True, 1, False),
                      (1, 16, 16, 9, 13, 1, True, 5, False), (1, 16, 16, 9, 13, 1, True, 7, False), (2, 1, 16, 11, 14, 2, False, 5, True),
                      (2, 4, 16, 11, 14, 2, False, 5, True)]
RESBLOCK2D_SHAPES = [(1, 1, 1), (2, 15, 31), (1, 9, 100)]
S2_2D_SHAPES = [(1, 2, 2), (3, 17, 33)]


def _slope(i):
    return SLOPES[i % len(SLOPES)]


def _table():
    t = {}

    def add(family, name, **kw):
        t.setdefault(family, []).append((name, kw))
    for i, (B, ci, co, d, h, w, s, res) in enumerate(CONV3D_SHAPES + CONV3D_DIRECT_ODD):
        for rg in REGIMES:
            add("conv3d_f32", f"{(B, ci, co, d, h, w, s)}-{rg}", fmt="f32", regime=rg, slope=_slope(i), seed=100 + i, **_c3(B, ci, co, d, h, w, s, res))
    for i, (B, ci, d, h, w, res) in enumerate(HEAD_F32_SHAPES):
        for rg in REGIMES:
            add("conv3d_head_f32", f"{(B, ci, d, h, w)}-{rg}", fmt="f32", regime=rg, slope=_slope(i + 2), seed=150 + i, **_c3(B, ci, 1, d, h, w, 1, res))
    for fmt in ("bf16", "f16"):
        for i, (B, ci, co, d, h, w, s, res) in enumerate(CONV3D_SHAPES + CONV3D_V32_SHAPES):
            for rg in REGIMES:
                add(f"conv3d_{fmt}", f"{(B, ci, co, d, h, w, s)}-{rg}", fmt=fmt, regime=rg, slope=_slope(i + 1), seed=200 + i, **_c3(B, ci, co, d, h, w, s, res))
        for i, (B, ci, co, d, h, w, s, res) in enumerate(CONV3D_OUT_SPLIT_SHAPES):
            for rg in REGIMES:
                add(f"conv3d_out_split_{fmt}", f"{(B, ci, co, d, h, w, s)}-{rg}", fmt=fmt, regime=rg, slope=_slope(i), seed=300 + i,
                    bound=F16_MAX if fmt == "f16" else None, **_c3(B, ci, co, d, h, w, s, res))
        for i, (B, ci, co, d, h, w, res) in enumerate(UP2_SHAPES):
            for rg in REGIMES:
                add(f"conv3d_up2_{fmt}", f"{(B, ci, co, d, h, w)}-{rg}", fmt=fmt, regime=rg, slope=_slope(i + 2), seed=400 + i, up2=True,
                    bound=F16_MAX if fmt == "f16" else None, **_c3(B, ci, co, d, h, w, 1, res))
        for i, (B, d, h, w) in enumerate(RS_SHAPES):
            for rg in REGIMES:
                for j, res in enumerate((True, False)):
                    add(f"conv3d_rs_{fmt}", f"{(B, d, h, w)}-{rg}-res{int(res)}", fmt=fmt, regime=rg, slope=_slope(i + j), seed=500 + i,
                        bound=F16_MAX if fmt == "f16" else None, **_c3(B, 32, 32, d, h, w, 1, res))
        for i, (B, d, h, w) in enumerate(RS16_SHAPES):
            for rg in REGIMES:
                add(f"conv3d_rs16_{fmt}", f"{(B, d, h, w)}-{rg}", fmt=fmt, regime=rg, slope=_slope(i + 3), seed=600 + i,
                    bound=F16_MAX if fmt == "f16" else None, **_c3(B, 16, 16, d, h, w))
        for i, (B, d, h, w) in enumerate(S2RS_SHAPES):
            for rg in REGIMES:
                add(f"conv3d_s2rs_{fmt}", f"{(B, d, h, w)}-{rg}", fmt=fmt, regime=rg, slope=_slope(i), seed=700 + i, fold_scale=True,
                    bound=F32P_MAX if fmt == "f16" else None, **_c3(B, 16, 32, d, h, w, 2))      # (F32P_MAX: the fp32-padded output too)
        for i, (B, d, h, w) in enumerate(POLY_SHAPES):
            for rg in REGIMES:
                add(f"conv3d_up2_poly_{fmt}", f"{(B, d, h, w)}-{rg}", fmt=fmt, regime=rg, slope=_slope(i), seed=800 + i, up2=True, poly=True,
                    bound=F16_MAX if fmt == "f16" else None, **_c3(B, 32, 16, d, h, w))
        for i, (B, ci, d, h, w) in enumerate(HEAD_SHAPES):
            for rg in REGIMES:
                add(f"conv3d_head_split_{fmt}", f"{(B, ci, d, h, w)}-{rg}", fmt=fmt, regime=rg, slope=1.0, seed=900 + i, **_c3(B, ci, 1, d, h, w))
    for i, (B, d, h, w) in enumerate(WINO_SHAPES):
        for rg in REGIMES:
            for j, res in enumerate((True, False)):
                add("conv3d_wino", f"{(B, d, h, w)}-{rg}-res{int(res)}", fmt="f16", regime=rg, slope=_slope(i + j), seed=1000 + i, wino=True,
                    bound=F32P_MAX, **_c3(B, 32, 32, d, h, w, 1, res))
    for i, (B, d, h, w) in enumerate(POLY_WINO_SHAPES):
        for rg in REGIMES:
            add("conv3d_up2_poly_wino", f"{(B, d, h, w)}-{rg}", fmt="f16", regime=rg, slope=_slope(i), seed=1100 + i, up2=True, poly=True, polywino=True,
                bound=F16_MAX, **_c3(B, 32, 16, d, h, w))
    for i, (B, ci, co, h, w, s, res) in enumerate(CONV2D_SHAPES + CONV2D_WIDE_SHAPES):
        for rg in REGIMES:
            add("conv2d_f32", f"{(B, ci, co, h, w, s)}-{rg}", fmt="f32", regime=rg, slope=_slope(i), seed=1200 + i, **_c2(B, ci, co, h, w, s, res))
            add("conv2d_bf16", f"{(B, ci, co, h, w, s)}-{rg}", fmt="bf16", regime=rg, slope=_slope(i + 1), seed=1300 + i, **_c2(B, ci, co, h, w, s, res))
    for rg in REGIMES:
        add("conv2d_stem_f32", f"(2, 3, 16, 30, 52, 2)-{rg}", fmt="f32", regime=rg, slope=0.25, seed=1400, k=5, **_c2(2, 3, 16, 30, 52, 2))
    for i, (B, ci, co, h, w, s, res, k, nchw) in enumerate(CONV2D_DIRECT_ROWS):
        for rg in REGIMES:
            add("conv2d_direct", f"{(B, ci, co, h, w, s)}-k{k}-{'nchw' if nchw else 'nhwc'}-{rg}", fmt="f32", regime=rg, slope=_slope(i), seed=1600 + i,
                k=k, **_c2(B, ci, co, h, w, s, res))
    for i, (B, h, w) in enumerate(S2_2D_SHAPES):
        for rg in REGIMES:
            add("conv2d_s2_split", f"{(B, h, w)}-{rg}", fmt="bf16", regime=rg, slope=_slope(i), seed=1500 + i, fold_scale=True, **_c2(B, 16, 16, h, w, 2))
    return t


TABLE = _table()


@functools.lru_cache(maxsize=None)
def case(family: str, name: str):
    """The built case (operands, reference, conditions asserted), cached: computed once, shared, never modified."""
    kw = dict(TABLE[family])[name]
    return make_case(**kw)


def ids(family: str):
    return [n for n, _ in TABLE[family]]


# ------------------------------------------------------------------------------------------------ the extractor's residual block
RESBLOCK_REGIMES = REGIMES + ("w2_wide",)


def make_resblock_case(B, H, W, regime, seed, slope=0.25, frames=None):
    """ResConvBlk2d on 16 channels in the bf16 split: y = act(conv2(m) * s2 + b2 + x), m = act(conv1(x) * s1 + b1).  The kernels
    hold m in 16-bit pieces, so m must be a bf16 hi + lo pair itself (asserted: split_join(m) == m).  Three regimes:
      x_wide, w_wide   conv1's wide operand; m comes out wide (a lo part), so w2 is narrow: the cross terms lo(x) hi(w1), hi(x) lo(w1)
                       and lo(m) hi(w2);
      w2_wide          x and w1 of one bit, s1 = 1 and slope in {0, 1}: m is an integer of at most 8 bits (|m| <= 144 + 15) without a
                       lo part, and w2 is wide: the cross term hi(m) lo(w2), the lo stream of conv2's weights."""
    assert regime in RESBLOCK_REGIMES and (regime != "w2_wide" or slope in (0.0, 1.0))
    bc = (1, -1, 1, 1)
    idx = None
    if frames is not None:      # a launch-size case (make_case): built and asserted on F frames, presented B times in the order idx
        idx = torch.from_numpy(frame_index(B, min(frames, B), seed))
        B = min(frames, B)
    for halvings in range(9):
        density = 0.5 ** halvings
        rng = np.random.default_rng(seed)
        if regime == "x_wide":
            x, w1 = wide(rng, (B, 16, H, W), "bf16", density), narrow(rng, (16, 16, 3, 3), 1)
        elif regime == "w_wide":
            x, w1 = narrow(rng, (B, 16, H, W), 1), wide(rng, (16, 16, 3, 3), "bf16", density)
        else:
            x, w1 = narrow(rng, (B, 16, H, W), 1), narrow(rng, (16, 16, 3, 3), 1)
        w2 = wide(rng, (16, 16, 3, 3), "bf16", density) if regime == "w2_wide" else narrow(rng, (16, 16, 3, 3), 3)
        s1 = torch.tensor([1.0 if regime == "w2_wide" else 2.0 ** -(ch % 3) for ch in range(16)], dtype=torch.float64)
        s2 = torch.tensor([2.0 ** -((ch + 1) % 3) for ch in range(16)], dtype=torch.float64)
        b1, b2 = narrow(rng, (16,), 15), narrow(rng, (16,), 15)
        a1 = _conv(x, w1, 1)
        m = a1 * s1.view(bc) + b1.view(bc)
        m = torch.where(m > 0, m, m * slope)
        # m's lsb: 2^-2 from the scale, 2^-2 from the slope (1 in the w2_wide regime)
        lsb_m = 1.0 if regime == "w2_wide" else 1.0 / 16
        sums = (float(_conv(x.abs(), w1.abs(), 1).max()), float(_conv(m.abs(), w2.abs(), 1).max()) / lsb_m)
        ok_m = representable(m) and torch.equal(split_join(m.float(), "bf16").double(), m)
        if max(sums) < 0.7 * TWO24 and ok_m:
            break
    else:
        raise AssertionError(f"resblock case not reachable: sums {sums}, m in 16 bits {ok_m}")
    (_at_most_one_lo if regime == "w2_wide" else _exactly_one_lo)(x, w1 * s1.view(-1, 1, 1, 1), "bf16")
    mh, ml, w2h, w2l = _exactly_one_lo(m, w2 * s2.view(-1, 1, 1, 1), "bf16")
    assert (bool(w2l.any()) and not bool(ml.any())) if regime == "w2_wide" else (bool(ml.any()) and not bool(w2l.any()))
    assert torch.equal(_conv(x.float(), w1.float(), 1).double(), a1), "ATen fp32 != float64 (conv1)"
    a2 = _conv(m, w2, 1)
    u2h, u2l = (t.double() for t in split(w2, "bf16"))
    assert torch.equal(_conv(mh, u2h, 1) + _conv(ml, u2h, 1) + _conv(mh, u2l, 1), a2), "hi*hi + lo*hi + hi*lo != the full convolution (conv2)"
    assert torch.equal(_conv(m.float(), w2.float(), 1).double(), a2), "ATen fp32 != float64 (conv2)"
    assert torch.equal(torch.round(m / lsb_m), m / lsb_m)
    assert float(_conv(mh.abs() + ml.abs(), u2h.abs() + u2l.abs(), 1).max()) / lsb_m < TWO24, "condition (a), conv2"
    assert sums[0] < TWO24, "condition (a), conv1"
    stages = [a1, a1 * s1.view(bc), a2, a2 * s2.view(bc), a2 * s2.view(bc) + b2.view(bc), a2 * s2.view(bc) + b2.view(bc) + x]
    y = torch.where(stages[-1] > 0, stages[-1], stages[-1] * slope)
    for i, v in enumerate(stages + [y]):
        assert representable(v), f"condition (b): resblock stage {i}"
    c = types.SimpleNamespace(regime=regime, density=density, x=x.float(), w1=w1.float(), w2=w2.float(), s1=s1.float(), s2=s2.float(),
                              b1=b1.float(), b2=b2.float(), ref=y, slope=slope, abs_sum_frac=max(sums) / TWO24,
                              m_has_lo=bool(ml.any()), w2_has_lo=bool(w2l.any()))
    if idx is not None:         # (the block's residual is its own input: it follows the frame)
        c.idx, c.n_frames, c.x_frames, c.x, c.ref = idx.numpy(), B, c.x, c.x[idx], y[idx]
    return c


RESBLOCK_IDS = [f"{s}-{rg}" for s in RESBLOCK2D_SHAPES for rg in RESBLOCK_REGIMES]


@functools.lru_cache(maxsize=None)
def resblock_case(name: str):
    shape, rg = name.rsplit("-", 1)
    i = [str(s) for s in RESBLOCK2D_SHAPES].index(shape)
    return make_resblock_case(*RESBLOCK2D_SHAPES[i], rg, 1600 + i, slope=(0.0, 1.0)[i % 2] if rg == "w2_wide" else 0.25)


# ------------------------------------------------------------------------------------------------ deformable conv, resize
DEFORM_ROWS = [
    # (N, Cin, Cout, H, W, k, stride, pad, dil, res, slope): the rows of test_deform_conv2d_vs_oracle, slopes from SLOPES
    (2, 16, 16, 12, 40, 3, 1, 1, 1, True, 0.25),
    (1, 16, 16, 9, 21, 5, 2, 2, 1, False, 1.0),
    (1, 16, 16, 10, 16, 3, 1, 2, 2, False, 0.0),
    (2, 8, 12, 7, 11, 3, 1, 1, 1, True, 0.5),
]


@functools.lru_cache(maxsize=None)
def deform_case(i: int):
    """Integer x and w, offsets that are multiples of 0.25 (bilinear weights k/16): sub-pixel, whole numbers, exactly on the -1 / H
    borders, far outside.  Reference: the oracle's deformable convolution on doubles.  Products are multiples of 1/16."""
    from oracle import mvsgi_oracle as O
    N, Cin, Cout, Hh, W, k, st, pad, dil, res, slope = DEFORM_ROWS[i]
    rng = np.random.default_rng(1700 + i)
    x, w = wide(rng, (N, Cin, Hh, W), "f32", 1.0), narrow(rng, (Cout, Cin, k, k), 7)
    Ho = (Hh + 2 * pad - (dil * (k - 1) + 1)) // st + 1
    Wo = (W + 2 * pad - (dil * (k - 1) + 1)) // st + 1
    off = torch.from_numpy(np.round(rng.normal(0, 1.5, (N, 2 * k * k, Ho, Wo)) * 4) / 4)
    off[:, :, 0, :] = torch.round(off[:, :, 0, :])                       # whole numbers
    off[:, 0, 1 % Ho, :] = -50.0                                         # far outside
    off[:, 3, 2 % Ho, :] = 1e4
    # tap (0, 0) of output row 3 lands exactly on y = -1, tap (k-1, k-1) of the last row exactly on y = H
    off[:, 0, 3 % Ho, :] = -1.0 - (float(3 % Ho) * st - pad)
    off[:, 2 * (k * k - 1), Ho - 1, :] = Hh - (float(Ho - 1) * st - pad + (k - 1) * dil)
    offs = {"per_image": off, "shared": off[:1].clone()}
    out = types.SimpleNamespace(row=DEFORM_ROWS[i], x=x.float(), w=w.float(), slope=slope, off={}, ref={}, abs_sum_frac=0.0)
    scale = torch.tensor([2.0 ** (1 - ch % 3) for ch in range(Cout)], dtype=torch.float64)
    shift = narrow(rng, (Cout,), 15)
    r = narrow(rng, (N, Cout, Ho, Wo), 31) if res else None
    for kind, o in offs.items():
        acc = O.deform_conv2d(x, o, w, None, (st, st), (pad, pad), (dil, dil))
        a = float(O.deform_conv2d(x.abs(), o, w.abs(), None, (st, st), (pad, pad), (dil, dil)).max()) * 16
        assert a < TWO24, f"condition (a): {a / TWO24:.3f}"
        out.abs_sum_frac = max(out.abs_sum_frac, a / TWO24)
        assert torch.equal(torch.round(acc * 16), acc * 16)
        stages = [acc, acc * scale.view(1, -1, 1, 1)]
        stages.append(stages[-1] + shift.view(1, -1, 1, 1))
        if res:
            stages.append(stages[-1] + r)
        stages.append(torch.where(stages[-1] > 0, stages[-1], stages[-1] * slope))
        for j, v in enumerate(stages):
            assert representable(v), f"condition (b): stage {j}"
        assert torch.equal(O.deform_conv2d(x.float(), o.float(), w.float(), None, (st, st), (pad, pad), (dil, dil)).double(), acc), "fp32 oracle != float64"
        out.off[kind], out.ref[kind] = o.float(), stages[-1]
    out.scale, out.shift, out.r = scale.float(), shift.float(), (None if r is None else r.float())
    return out


RESIZE_CASES = [((2, 16, 3, 5, 7), 2), ((1, 5, 2, 3, 5), 2), ((2, 16, 3, 5, 7), 4), ((1, 5, 2, 3, 5), 4)]


@functools.lru_cache(maxsize=None)
def resize_case(i: int):
    """Trilinear x2 / x4 of an integer volume: coefficients k/4 and k/8 per axis, exact in fp32 (asserted against float64)."""
    shape, f = RESIZE_CASES[i]
    x = wide(np.random.default_rng(1800 + i), shape, "f32", 1.0)
    size = tuple(f * s for s in shape[2:])
    ref = F.interpolate(x, size=size, mode="trilinear", align_corners=False)
    assert representable(ref) and torch.equal(F.interpolate(x.float(), size=size, mode="trilinear", align_corners=False).double(), ref)
    return types.SimpleNamespace(x=x.float(), size=size, ref=ref, lsb=1.0 / (2 * f) ** 3)


# ================================================================================================ launch-size cases
# tests/test_gpu_exact_launches.py: the same operands and conditions at the sizes where the dispatcher takes its many-frame
# variants, where the launcher skips border planes and where a persistent workgroup walks a second and later unit.  Every case is
# built on FRAMES distinct frames presented B times (make_case(frames=...), frame_index).  Recorded for 256 CUs, like
# tests/golden/conv3d_dispatch_pin.json.
FRAMES = 4
LAUNCH_CUS = 256


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---- the streaming kernel and the exact-fp32 MFMA kernel: one shape per row of csrc/conv3d_variants.inc at which
# H.conv3d_variant / H.conv3d_up2_variant names the row (the cheapest of a search over frames of H in {6, 8, 10, 12, 15}, W in
# {24, 40} -- ragged against the 16-wide bricks, 8 mod 16 for the 10 x 8 ones -- three or five planes deep unless the row is a one-
# or two-plane form; up2: the low-resolution size).
# (row, entry point, B, Cin, Cout, D, H, W, stride, layout)
VARIANT_ROWS = [
    ("V_S1_N16_B256", "conv", 1, 16, 16, 3, 6, 24, 1, "mfma"),
    ("V_S1_N32_B256", "conv", 320, 16, 32, 3, 6, 24, 1, "mfma"),
    ("V_S1_N32_B64", "conv", 1, 16, 32, 3, 6, 24, 1, "mfma"),
    ("V_S1_N64_B128", "conv", 160, 16, 128, 3, 6, 24, 1, "mfma"),
    ("V_S1_N64_B64", "conv", 1, 16, 64, 3, 6, 24, 1, "mfma"),
    ("V_S2_N32_B64", "conv", 1, 16, 16, 3, 6, 24, 2, "mfma"),
    ("V_S2_N64_B64", "conv", 1, 16, 64, 3, 6, 24, 2, "mfma"),
    ("B3_N16", "conv", 1, 16, 16, 3, 6, 24, 1, "generic"),
    ("B3_N32", "conv", 48, 16, 32, 5, 6, 24, 1, "generic"),
    ("B3_N48", "conv", 1, 16, 48, 3, 6, 24, 1, "generic"),
    ("B3_N64", "conv", 24, 16, 64, 3, 6, 24, 1, "generic"),
    ("B3_N64_H5", "conv", 20, 16, 64, 3, 15, 24, 1, "generic"),
    ("B3_N96", "conv", 48, 16, 96, 3, 6, 24, 1, "generic"),
    ("B3_N96_H5", "conv", 32, 16, 96, 3, 15, 24, 1, "generic"),
    ("B3_N128_P", "conv", 96, 16, 128, 1, 6, 24, 1, "generic"),
    ("B3_N128_PH5", "conv", 24, 16, 128, 1, 15, 24, 1, "generic"),
    ("B3_N192_PH5", "conv", 64, 16, 192, 1, 15, 24, 1, "generic"),
    ("B3_N64_S", "conv", 12, 16, 64, 3, 6, 24, 1, "generic"),
    ("B3_N16_TW", "conv", 1, 16, 64, 3, 6, 24, 1, "generic"),
    ("B3_N32_TB", "conv", 1, 16, 32, 3, 6, 24, 1, "generic"),
    ("B3_S2_N32B", "conv", 1, 16, 16, 3, 6, 24, 2, "generic"),
    ("B3_S2_N64", "conv", 48, 16, 96, 3, 6, 24, 2, "generic"),
    ("B3_S2_N96", "conv", 64, 16, 192, 3, 10, 24, 2, "generic"),
    ("B3_S2_N128", "conv", 64, 16, 128, 5, 10, 24, 2, "generic"),
    ("B3_S2_N192", "conv", 64, 16, 192, 5, 10, 24, 2, "generic"),
    ("B3_N64_W8", "conv", 24, 16, 64, 3, 10, 24, 1, "generic"),
    ("B3_N96_W8", "conv", 48, 16, 96, 3, 10, 24, 1, "generic"),
    ("B3_N128_PW8", "conv", 32, 16, 128, 1, 10, 24, 1, "generic"),
    ("B3_N192_PW8", "conv", 96, 16, 192, 1, 10, 24, 1, "generic"),
    ("B3U_N16", "up2", 1, 16, 16, 2, 3, 12, 1, "generic"),
    ("B3U_N32", "up2", 40, 16, 32, 2, 3, 12, 1, "generic"),
    ("B3U_N32_M", "up2", 1, 16, 32, 2, 3, 12, 1, "generic"),
    ("B3U_N48", "up2", 1, 16, 48, 2, 3, 12, 1, "generic"),
    ("B3U_N64", "up2", 12, 16, 64, 2, 3, 12, 1, "generic"),
    ("B3U_N96", "up2", 48, 16, 96, 2, 3, 12, 1, "generic"),
    ("B3U_N32_TB", "up2", 1, 16, 64, 2, 3, 12, 1, "generic"),
    ("B3P_N16", "conv", 1, 16, 16, 3, 6, 24, 1, "c16"),
    ("B3PU_N16", "up2", 1, 16, 16, 2, 3, 12, 1, "c16"),
    ("B3V_N32", "conv", 48, 16, 32, 5, 6, 24, 1, "v32"),
    ("B3V_N64", "conv", 24, 16, 96, 3, 6, 24, 1, "v32"),
    ("B3VU_N32", "up2", 48, 16, 32, 3, 3, 12, 1, "v32"),
    ("B3VU_N64", "up2", 48, 16, 64, 2, 3, 12, 1, "v32"),
    ("B3D_N64", "conv", 24, 32, 64, 3, 6, 24, 1, "d32"),
    ("B3D_N64_H5", "conv", 20, 32, 64, 3, 15, 24, 1, "d32"),
    ("B3D_N64_W8", "conv", 24, 32, 64, 3, 10, 24, 1, "d32"),
    ("B3D_N96", "conv", 48, 32, 96, 3, 6, 24, 1, "d32"),
    ("B3D_N96_H5", "conv", 32, 32, 96, 3, 15, 24, 1, "d32"),
    ("B3D_N96_W8", "conv", 48, 32, 96, 3, 10, 24, 1, "d32"),
    ("B3D_N128_P", "conv", 96, 32, 128, 1, 6, 24, 1, "d32"),
    ("B3D_N128_PH5", "conv", 24, 32, 128, 1, 15, 24, 1, "d32"),
    ("B3D_N128_PW8", "conv", 32, 32, 128, 1, 10, 24, 1, "d32"),
    ("B3D_N192_PH5", "conv", 64, 32, 192, 1, 15, 24, 1, "d32"),
    ("B3D_N192_PW8", "conv", 96, 32, 192, 1, 10, 24, 1, "d32"),
    ("B3D_N32_TB", "conv", 1, 32, 32, 3, 6, 24, 1, "d32"),
    ("B3D_N64_S", "conv", 12, 32, 64, 3, 6, 24, 1, "d32"),
    ("B3D2_N64", "conv", 40, 32, 64, 2, 6, 24, 1, "d32"),
    ("B3D2_N64_H5", "conv", 40, 32, 64, 2, 15, 24, 1, "d32"),
    ("B3D2_N64_W8", "conv", 48, 32, 64, 2, 10, 24, 1, "d32"),
    ("B3D2_N96", "conv", 96, 32, 96, 2, 6, 24, 1, "d32"),
    ("B3D2_N96_H5", "conv", 64, 32, 96, 2, 15, 24, 1, "d32"),
    ("B3D2_N96_W8", "conv", 96, 32, 96, 2, 10, 24, 1, "d32"),
    ("B3D2_N32_TB", "conv", 1, 32, 32, 2, 6, 24, 1, "d32"),
    ("B3D2_N64_S", "conv", 20, 32, 64, 2, 6, 24, 1, "d32"),
    ("B3DU_N64", "up2", 12, 32, 64, 2, 3, 12, 1, "d32"),
    ("B3DU_N96", "up2", 48, 32, 96, 2, 3, 12, 1, "d32"),
    ("B3DU2_N64", "up2", 24, 32, 64, 1, 3, 12, 1, "d32"),
    ("B3DU2_N96", "up2", 96, 32, 96, 1, 3, 12, 1, "d32"),
]
# the unit walk of the streaming kernel (units >= 2 R + r, R = 512): the plain, the _d32 and the fused-upsample 2 x 4 x 16 bricks
VARIANT_ROWS += [
    ("B3_N64", "conv", 130, 16, 64, 3, 6, 24, 1, "generic"),
    ("B3D_N64", "conv", 130, 32, 64, 3, 6, 24, 1, "d32"),
    ("B3U_N64", "up2", 130, 16, 64, 2, 3, 12, 1, "generic"),
]
WALK_VARIANT_IDS = ("B3_N64-130", "B3D_N64-130", "B3U_N64-130")


def variant_row_id(row) -> str:
    return f"{row[0]}-{row[2]}"


def parse_variants_inc(path):
    """csrc/conv3d_variants.inc -> {row: (kind 'MFMA' | 'B3', kernel suffix, [template arguments])} in file order."""
    import re
    out = {}
    with open(path) as f:
        for line in f:
            m = re.match(r"MVSGI_(B3|MFMA)\((\w+), (.*)\)\s*$", line)
            if m:
                kind, row, rest = m.groups()
                suffix, args = rest.split(", ", 1) if kind == "B3" else ("", rest)
                out[row] = (kind, suffix, args)
    return out


def variant_kernel_name(variants, row: str, fmt: str) -> str:
    """The name csrc/conv3d.hip:variant_name reports for a row in a split ('bf16' | 'f16'; 'f32' for the MFMA rows)."""
    kind, suffix, args = variants[row]
    if kind == "MFMA":
        return f"conv3d_mfma_kernel<{args}>"
    return f"conv3d_{'f16x3' if fmt == 'f16' else 'bf16x3'}{suffix}<{args}>"


def streaming_units(variants, row: str, B, Do, Ho, Wo, Cout) -> int:
    """launch_bf16x3 (csrc/conv3d_bf16x3.hpp:1455-1477): B * tiles_d * tiles_h * tiles_w * cdiv(CT, WN * NW), CT = Cout / 16 (32 for
    the 32x32x16 schedule).  Template arguments: NW, MW, WM, WN, TD, TH, TW, ..."""
    a = variants[row][2].split(", ")
    NW, _, _, WN, TD, TH, TW = (int(v) for v in a[:7])
    v32 = len(a) > 11 and a[11] == "true"
    return B * cdiv(Do, TD) * cdiv(Ho, TH) * cdiv(Wo, TW) * cdiv(Cout // (32 if v32 else 16), WN * NW)


def variant_case(row, fmt: str, regime: str):
    name, fn, B, ci, co, D, Hh, W, s, lay = row
    i = [r for r in VARIANT_ROWS].index(row)
    return make_case(fmt, regime, B, ci, co, (D, Hh, W), stride=s, res=bool(i % 2), slope=_slope(i), up2=(fn == "up2"),
                     seed=2000 + i, frames=FRAMES)


# ---- the border-plane skip (launch_bf16x3, csrc/conv3d_bf16x3.hpp:1461-1475): the 2 x 4 x 16 bricks of the 32-channel-slice kernels
# in a volume FOUR planes deep whose layer of bricks, B * cdiv(H, 4) * cdiv(W, 16) * cdiv(Cout / 16, WN * NW), is at least 4 rounds of
# the chip (4 * CUs).  The variant's name does not say that the skip ran: the tests restate this condition.
# (row, entry point, B, Cin, Cout, D, H, W of the OUTPUT volume's input: low resolution for up2, skip expected)
BORDER_ROWS = [
    ("B3D_N64", "conv", 256, 32, 64, 4, 8, 32, True),
    ("B3D_N96", "conv", 256, 32, 96, 4, 8, 32, True),
    ("B3DU_N64", "up2", 256, 32, 64, 2, 4, 16, True),
    ("B3DU_N96", "up2", 256, 32, 96, 2, 4, 16, True),
    ("B3D_N64", "conv", 255, 32, 64, 4, 8, 32, False),      # the control: one frame below the condition, the same variant
]


def border_layer(variants, row: str, B, Ho, Wo, Cout) -> int:
    a = [int(v) for v in variants[row][2].split(", ")[:7]]
    NW, MW, WM, WN, TD, TH, TW = a
    assert (TD, WM, MW, TH, TW) == (2, 2, 4, 4, 16), "kBorderSplit (conv3d_bf16x3.hpp:1461)"
    return B * cdiv(Ho, TH) * cdiv(Wo, TW) * cdiv(Cout // 16, WN * NW)


def border_case(row, fmt: str, regime: str):
    name, fn, B, ci, co, D, Hh, W, _ = row
    i = BORDER_ROWS.index(row)
    return make_case(fmt, regime, B, ci, co, (D, Hh, W), res=bool(i % 2), slope=_slope(i + 1), up2=(fn == "up2"), seed=2200 + i, frames=FRAMES)


# ---- unit walks: every persistent family at units >= 2 R + r, R = CUs x (the launcher's max_wgs_per_cu argument to
# persistent_geometry), 0 < r < R: every workgroup walks a second unit behind its first (weights resident, the next unit's image
# staged during the current one's matrix work) and the last round is ragged.  units_of restates each launcher's tile counts.
# family -> (B, D, H, W) or (B, H, W); (units per frame, max_wgs_per_cu, source)
WALKS = {
    "conv3d_rs": ((65, 3, 5, 17), lambda d, h, w: cdiv(d, 2) * cdiv(h, 4) * cdiv(w, 16), 1, "conv3d_rs.hip:925-928, 955"),
    "conv3d_rs16": ((65, 5, 5, 17), lambda d, h, w: cdiv(d, 4) * cdiv(h, 4) * cdiv(w, 16), 1, "conv3d_rs.hip:1050-1053, 1069"),
    # (input size; the units are counted on the stride-2 output)
    "conv3d_s2rs": ((65, 3, 9, 33), lambda d, h, w: cdiv(d, 2) * cdiv(cdiv(h, 2), 4) * cdiv(cdiv(w, 2), 16), 1, "conv3d_s2rs.hip:278-282, 289"),
    "conv3d_wino": ((130, 8, 4, 64), lambda d, h, w: (h // 2) * (w // 32), 1, "conv3d_wino.hip:573-575, 474-475"),
    # per role: 4 (H, W) phases x tiles_d depth roles share the grid, 8 XCDs x walkers workgroups each, walkers = CUs / (8 * 4 * tiles_d)
    "conv3d_up2_poly": ((35, 2, 5, 17), lambda d, h, w: cdiv(h, 4) * cdiv(w, 16), 0.25, "conv3d_rs.hip:1003-1006, 1019-1025"),
    # per row phase: 8 XCDs x (CUs / 16) walkers
    "conv3d_up2_poly_wino": ((260, 8, 2, 32), lambda d, h, w: (h // 2) * (w // 32), 0.5, "conv3d_wino_up2.hip:515-517, 526-530"),
    "resblock2d": ((258, 15, 31), lambda h, w: cdiv(h, 14) * cdiv(w, 30), 2, "conv2d.hip:439-441, 447; resblock2d_rs.hip:713-715, 443"),
    # (input size; units on the stride-2 output)
    "conv2d_s2_split": ((258, 17, 33), lambda h, w: cdiv(cdiv(h, 2), 8) * cdiv(cdiv(w, 2), 16), 2, "resblock2d_rs.hip:645-647, 652"),
}


def walk_units(family: str):
    """-> (units, R): asserts units >= 2 R + r with 0 < r < R for R = CUs x max_wgs_per_cu AND for one workgroup per CU."""
    shape, per_frame, wgs, _ = WALKS[family]
    units, R = shape[0] * per_frame(*shape[1:]), int(LAUNCH_CUS * wgs)
    assert units >= 2 * R and units % R != 0 and units % max(1, int(LAUNCH_CUS * min(wgs, 1))) != 0, (family, units, R)
    return units, R


WALK_FMTS = {"conv3d_rs": ("bf16", "f16"), "conv3d_rs16": ("bf16", "f16"), "conv3d_s2rs": ("bf16", "f16"), "conv3d_wino": ("f16",),
             "conv3d_up2_poly": ("bf16", "f16"), "conv3d_up2_poly_wino": ("f16",), "conv2d_s2_split": ("bf16",)}
RESBLOCK_WALK_SEED = 2500


def walk_case(family: str, fmt: str, regime: str):
    shape = WALKS[family][0]
    i = list(WALKS).index(family)
    assert fmt in WALK_FMTS[family]
    cin, cout, kw = {"conv3d_rs": (32, 32, dict(res=True)), "conv3d_rs16": (16, 16, {}), "conv3d_s2rs": (16, 32, dict(stride=2, fold_scale=True)),
                     "conv3d_wino": (32, 32, dict(res=True, wino=True)), "conv3d_up2_poly": (32, 16, dict(up2=True, poly=True)),
                     "conv3d_up2_poly_wino": (32, 16, dict(up2=True, poly=True, polywino=True)),
                     "conv2d_s2_split": (16, 16, dict(stride=2, fold_scale=True))}[family]
    # the range of the delivered output, as in the small-shape table
    bound = {"conv3d_s2rs": F32P_MAX if fmt == "f16" else None, "conv3d_wino": F32P_MAX, "conv2d_s2_split": None}.get(
        family, F16_MAX if fmt == "f16" else None)
    return make_case(fmt, regime, shape[0], cin, cout, tuple(shape[1:]), slope=_slope(i), seed=2400 + i, frames=FRAMES, bound=bound, **kw)


def resblock_walk_case(regime: str):
    B, h, w = WALKS["resblock2d"][0]
    return make_resblock_case(B, h, w, regime, RESBLOCK_WALK_SEED, slope=0.0 if regime == "w2_wide" else 0.25, frames=FRAMES)


# ---- the split cost head's whole-depth march: nd = 1 once B * cdiv(H, 8) * cdiv(W, 32) >= 1024 windows
# (conv3d_headsplit.hip:283-290); D odd, ragged windows, one and two channel slices
HEAD_MARCH_SHAPES = [(256, 16, 3, 9, 33), (256, 32, 3, 9, 33)]


def head_march_case(shape, fmt: str, regime: str):
    B, ci, d, h, w = shape
    assert B * cdiv(h, 8) * cdiv(w, 32) >= 1024 and d % 2 == 1
    return make_case(fmt, regime, B, ci, 1, (d, h, w), slope=1.0, seed=2600 + HEAD_MARCH_SHAPES.index(shape), frames=FRAMES)


def launch_cases():
    """(id, builder) of every launch-size case built with make_case, in the order the GPU module runs them."""
    out = []
    for row in VARIANT_ROWS:
        for fmt in (("f32",) if row[9] == "mfma" else ("bf16", "f16")):
            for rg in REGIMES:
                out.append((f"variant-{variant_row_id(row)}-{fmt}-{rg}", functools.partial(variant_case, row, fmt, rg)))
    for row in BORDER_ROWS:
        for fmt in ("bf16", "f16"):
            for rg in REGIMES:
                out.append((f"border-{row[0]}-{row[2]}-{fmt}-{rg}", functools.partial(border_case, row, fmt, rg)))
    for family, fmts in WALK_FMTS.items():
        for fmt in fmts:
            for rg in REGIMES:
                out.append((f"walk-{family}-{fmt}-{rg}", functools.partial(walk_case, family, fmt, rg)))
    for shape in HEAD_MARCH_SHAPES:
        for fmt in ("bf16", "f16"):
            for rg in REGIMES:
                out.append((f"head-{shape}-{fmt}-{rg}", functools.partial(head_march_case, shape, fmt, rg)))
    return out


def direct_reference(c, frames):
    """act(conv(x [upsampled]) * scale + shift (+ r)) of the frames `frames` of the BATCH the kernel sees, in float64, from the
    case's delivered fp32 tensors alone: no frame index, no expansion."""
    sel = torch.as_tensor(list(frames))
    x = c.x[sel].double()
    acc = _conv(_up2(x) if c.up2 else x, c.w.double(), c.stride)
    bc = (1, -1) + (1,) * (x.dim() - 2)
    v = acc * c.scale.double().view(bc) + c.shift.double().view(bc)
    if c.r is not None:
        v = v + c.r[sel].double()
    return torch.where(v > 0, v, v * c.slope)
