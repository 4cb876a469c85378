"""Cases for the confidence maps of the soft-argmin's softmax (mvs_gi_amd/csrc/confidence.hip): the four maps in float64 from
tests/softargmin_cases.py's reference, per-element bounds from reference quantities only, a checker, and a step-by-step fp32
emulation of the kernel's expressions with the wrong implementations the checker has to reject.  NumPy only.  Used by
tests/test_confidence_host.py (CPU) and tests/test_gpu_confidence.py (MI355X).

Definitions, per output pixel, v_d the blended cost of candidate d (SC.ref64: fields v, gap, p, inv, M, y, x):
    m = max_d v_d, g_d = m - v_d, e_d = exp(-g_d), S = sum e_d, p_d = e_d / S, w_d = inv_idx[d], mu = sum p_d w_d
    max_prob = max_d p_d = 1 / S                    entropy = -sum p_d ln p_d = ln S + sum p_d g_d   (natural log; / ln D normalised)
    spread   = sqrt(V) / post_div, V = sum p_d (w_d - mu)^2                argmax = the lowest d with g_d == 0; -1 where NaN
(ln S + G and -sum p ln p agree to 1e-15 in float64: test_confidence_host.py asserts it.)

Bounds, first order in u = 2^-24, all from the reference.  dv is the blended cost's absolute error exactly as SC.bounds computes
it (5 u M, plus 4 u M (src_y + src_x + 1) at non-dyadic factors) and (x_p, x_inv) = SC.bounds(r) the relative bounds of p_d and
of the expectation.
    max_prob   relative: x_p at the winner = x_p.min(axis = 1), the term with g = 0 (max_prob IS the winner's probability).
    entropy    H = ln S + G, G = sum p_d g_d.  d(ln S) = dS / S: the relative error of the sum, which is that of the winner's
               probability: x_p|winner.  G = sum p_d g_d: each term errs relatively by x_p[d] (its p) plus the error of g_d
               itself, 2 dv absolute in total over a convex combination: sum p_d g_d x_p[d] + 2 dv.  D fmas, one division, the
               logarithm (a few ulps of ln S <= H), one addition: u (D + 4) H.
               absolute: x_p|winner + sum_d p_d g_d x_p[d] + 2 dv + u (D + 4) H; divided by ln D when normalised.
    spread     sigma = sqrt(V).  d sigma = dV / (2 sigma).  V's terms err relatively by x_p[d] (the probability) and through
               mu: d/dmu sum p (w - mu)^2 = 0 at the mean, so mu's error enters sigma only as a shift of the centre, bounded by
               |d mu| = mu x_inv.  Accumulation (D fmas), the square, the division, the root: u (D + 5) sigma.
               absolute: (sigma / 2) (sum_d p_d (w_d - mu)^2 x_p[d]) / V + mu x_inv + u (D + 5) sigma, all / post_div; the first
               term is 0 where V = 0.
    argmax     equal to the reference's wherever the best-to-second gap of v exceeds 4 dv (each of the two blended values moves
               by at most dv in the implementation and the reference's own fp64 value is exact: 2 dv would do; 4 dv leaves room
               for the fused / unfused coordinate); elsewhere the best or the second is accepted.  Such ambiguous pixels may be
               at most 1 % of a case (measured on the table below: <= 0.09 %).

Exact regime (SC.exact_case: one-hot costs with ties at dyadic factors 1, 2, 4; T the tie set): argmax = min T, max_prob =
fl32(1 / |T|), entropy = +0 and spread = +0 bit for bit on single-winner pixels, spread within 1 ulp of fl32(sqrt(V)) where |T| is a
power of two (mu, the deviations, their squares and the sums are then exact in fp32 and the root is correctly rounded), entropy
within LOGF_ULPS + 1 ulps of fl32(ln |T|) on tie pixels (S = |T| and G = 0 exactly, so the entropy is logf(|T|)).
LOGF_ULPS = 3: the OpenCL full-profile limit for log, which the ROCm device library's fp32 logf is built to meet -- the same
source tests/grid_exact_cases.py takes its sin / cos / atan2 figures from: a specification, not a measurement.  (The HIP math
API table of the ROCm documentation could not be consulted when this was written; if it gives a smaller figure, this one
is merely generous by the difference.)  One more ulp is the reference's own rounding of ln |T| to fp32.
"""
from __future__ import annotations

import functools
import math
import os
from types import SimpleNamespace

import numpy as np

import softargmin_cases as SC

f32 = np.float32
U = SC.U
LOGF_ULPS = 3
MAPS = ("max_prob", "entropy", "spread", "argmax")
FLOAT_MAPS = MAPS[:3]
AMBIGUOUS_MAX = 0.01

SHAPES = [(2, 16, 7, 13), (1, 33, 6, 10), (1, 16, 3, 130), (2, 5, 5, 9), (1, 48, 2, 132), (1, 1, 2, 3)]
FACTORS = (1, 2, 4, 3, 1.5, 0.75)
SIGMAS = (4.0, 10.0)
POST_DIV_SHAPE = (2, 16, 7, 13)              # post_div in {1, 96} on this shape, 1 elsewhere
EXACT_FACTORS = (1, 2, 4)
GOLDEN_ROWS = [((2, 16, 7, 13), 2), ((2, 16, 7, 13), 4), ((2, 16, 7, 13), 1.5), ((1, 33, 6, 10), 2)]      # Gaussian costs, sigma 4
BF = 96.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_name(shape, s) -> str:
    return f"confidence_{'x'.join(map(str, shape))}_x{s:g}.npz"


# ------------------------------------------------------------------------------------------------ the maps in float64, and their bounds
def blend_error(r):
    """dv [B, 1, OH, OW], exactly as SC.bounds computes it."""
    dv = 5.0 * U * r.M
    if not SC.is_dyadic(r.s):
        dv = dv + 4.0 * U * r.M * (r.y[4].astype(np.float64)[:, None] + r.x[4].astype(np.float64)[None, :] + 1.0)
    return dv


def maps64(r, finite=None, normalize=False):
    """r = SC.ref64(costs, inv_idx, s, post_div) -> namespace: the four maps in float64 ([B, 1, OH, OW]; argmax int64, -1 where the
    float maps are NaN), `second` (the runner-up's index), `sure` (best-to-second gap > 4 dv), and the bounds b_max_prob
    (relative), b_entropy, b_spread (absolute).  finite: mask of the candidates that count (SC.nonfinite_case's -inf kind)."""
    D = r.shape[1]
    w = r.inv_idx64.reshape(1, -1, 1, 1)
    nan = np.isnan(r.inv)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        gap = r.gap if finite is None else np.where(finite, r.gap, np.inf)
        e = np.exp(-gap)
        S = e.sum(axis=1, keepdims=True)
        p = e / S
        pg = np.where(p > 0, p * np.where(p > 0, gap, 0.0), np.where(np.isnan(p), np.nan, 0.0))
        G = pg.sum(axis=1, keepdims=True)
        H = np.log(S) + G
        mu = (p * w).sum(axis=1, keepdims=True)
        dev2 = (w - mu) ** 2
        V = (p * dev2).sum(axis=1, keepdims=True)
        sigma = np.sqrt(V)
        order = np.argsort(np.where(np.isnan(gap), np.inf, gap), axis=1, kind="stable")
        best = order[:, :1]
        second = order[:, 1:2] if D > 1 else best
        gap2 = np.take_along_axis(gap, second, axis=1) if D > 1 else np.full(r.m.shape, np.inf)
        dv = blend_error(r)
        x_p, x_inv = SC.bounds(r, finite)
        x_win = x_p.min(axis=1, keepdims=True)
        b_ent = x_win + (pg * x_p).sum(axis=1, keepdims=True) + 2.0 * dv + U * (D + 4) * H
        first = np.where(V > 0, 0.5 * sigma * (p * dev2 * x_p).sum(axis=1, keepdims=True) / np.where(V > 0, V, 1.0), 0.0)
        b_spread = (first + mu * x_inv + U * (D + 5) * sigma) / r.post_div
        sure = gap2 > 4.0 * dv
    ln_d = math.log(D) if (normalize and D > 1) else 1.0
    return SimpleNamespace(max_prob=1.0 / S, entropy=H / ln_d, spread=sigma / r.post_div, argmax=np.where(nan, -1, best),
                           second=second, sure=sure | nan, nan=nan, b_max_prob=x_win, b_entropy=b_ent / ln_d, b_spread=b_spread,
                           p=p, S=S, G=G, V=V, mu=mu, D=D)


def check_maps(tag, ref, got, want=MAPS):
    """got: {name: array [B, 1, OH, OW]} -> {name: largest error / bound} (argmax: the fraction of ambiguous pixels).  NaN set of
    every float map == ref.nan, argmax == -1 exactly there; everything else finite and inside its bound."""
    ok = ~ref.nan
    ratios = {}
    for n in want:
        g = np.asarray(got[n])
        assert g.shape == ref.nan.shape, f"{tag}: {n} has shape {g.shape}, expected {ref.nan.shape}"
        if n == "argmax":
            assert g.dtype == np.int32, f"{tag}: argmax is {g.dtype}"
            assert np.array_equal(g == -1, ref.nan), f"{tag}: argmax is -1 at {int((g == -1).sum())} pixels, expected {int(ref.nan.sum())}"
            good = (g == ref.argmax) | (~ref.sure & (g == ref.second))
            assert good.all(), f"{tag}: argmax wrong at {int((~good).sum())} of {good.size} pixels"
            ratios[n] = float((~ref.sure).mean())
            continue
        assert g.dtype == np.float32, f"{tag}: {n} is {g.dtype}"
        assert np.array_equal(np.isnan(g), ref.nan), f"{tag}: {n} is NaN at {int(np.isnan(g).sum())} pixels, expected {int(ref.nan.sum())}"
        assert np.isfinite(g[ok]).all(), f"{tag}: {n} holds an infinity"
        want64 = getattr(ref, n)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(g.astype(np.float64) - want64)
            if n == "max_prob":
                err = err / want64
            ratio = np.where(ok, err / getattr(ref, "b_" + n), 0.0)
            ratio = np.where(ok & (err == 0.0), 0.0, ratio)          # 0 / 0: an exact value under a zero bound
        ratios[n] = float(ratio.max())
        assert ratios[n] <= 1.0, f"{tag}: {n} error / bound {ratios[n]:.3f} (largest error {float(np.where(ok, err, 0).max()):.3e})"
    return ratios


# ------------------------------------------------------------------------------------------------ tolerance regime
def tol_rows():
    """-> [(shape, factor, sigma, post_div)]: every shape at every factor and sigma; post_div 96 on one shape."""
    rows = []
    for sh in SHAPES:
        for s in FACTORS:
            for sigma in SIGMAS:
                rows.append((sh, s, sigma, 1.0))
                if sh == POST_DIV_SHAPE:
                    rows.append((sh, s, sigma, 96.0))
    return rows


@functools.lru_cache(maxsize=None)
def tol_case(shape, s, sigma, post_div=1.0, normalize=False):
    """Gaussian costs, stock candidates -> namespace(costs, inv_idx, ref (maps64), post_div, normalize); conditions asserted."""
    c = SC.tol_case(shape, s, sigma, post_div)
    ref = maps64(c.r, normalize=normalize)
    amb = float((~ref.sure).mean())
    assert amb <= AMBIGUOUS_MAX, (shape, s, sigma, amb)
    return SimpleNamespace(costs=c.costs, inv_idx=c.inv_idx, ref=ref, r=c.r, s=s, shape=shape, sigma=sigma, post_div=post_div,
                           normalize=normalize, ambiguous=amb)


@functools.lru_cache(maxsize=None)
def nonfinite_case(shape, s, kind):
    c = SC.nonfinite_case(shape, s, kind)
    ref = maps64(c.r, c.finite if kind == "-inf" else None)
    assert np.array_equal(ref.nan, c.nan_px)
    return SimpleNamespace(costs=c.costs, inv_idx=c.inv_idx, ref=ref, r=c.r, s=s, shape=shape, kind=kind, post_div=1.0, normalize=False)


NONFINITE = [(s, sh, k) for s in (1, 2, 3) for sh in SC.NONFINITE_SHAPES[s] for k in SC.NONFINITE_KINDS]


# ------------------------------------------------------------------------------------------------ exact regime
def exact_rows():
    return [(sh, s) for sh in SHAPES for s in EXACT_FACTORS]


@functools.lru_cache(maxsize=None)
def exact_case(shape, s):
    """SC.exact_case's one-hot field -> namespace(costs, inv_idx, argmax, max_prob, single, pow2, spread_pow2, ln_n) (expectations
    from integers)."""
    e = SC.exact_case(shape, s)
    r = SC.ref64(e.costs, e.inv_idx, s)
    T = r.gap == 0.0
    n = T.sum(axis=1, keepdims=True)
    w = e.inv_idx.astype(np.float64).reshape(1, -1, 1, 1)
    mu = (T * w).sum(axis=1, keepdims=True) / n
    V = (T * (w - mu) ** 2).sum(axis=1, keepdims=True) / n
    return SimpleNamespace(costs=e.costs, inv_idx=e.inv_idx, s=s, shape=shape, argmax=T.argmax(axis=1)[:, None].astype(np.int32),
                           max_prob=(1.0 / n).astype(np.float32), single=n == 1, pow2=e.pow2,
                           spread=np.sqrt(V).astype(np.float32), ln_n=np.log(n).astype(np.float32), ties=e.ties)


def check_exact(tag, c, got):
    am, mp, en, sp = (np.asarray(got[n]) for n in ("argmax", "max_prob", "entropy", "spread"))
    assert am.dtype == np.int32 and np.array_equal(am, c.argmax), f"{tag}: argmax is not the lowest index of the tie set at {int((am != c.argmax).sum())} pixels"
    SC.assert_exact(f"{tag} max_prob", mp, c.max_prob)
    zero = np.zeros_like(c.max_prob)
    SC.assert_exact(f"{tag} entropy (single winner)", np.where(c.single, en, zero).astype(np.float32), zero)
    SC.assert_exact(f"{tag} spread (single winner)", np.where(c.single, sp, zero).astype(np.float32), zero)
    d = SC._ulp_diff(np.where(c.pow2, sp, zero), np.where(c.pow2, c.spread, zero))
    assert int(d.max()) <= 1, f"{tag}: spread is {int(d.max())} ulps from sqrt(V) where |T| is a power of two"
    tie = ~c.single
    d = SC._ulp_diff(np.where(tie, en, zero), np.where(tie, c.ln_n, zero))
    assert int(d.max()) <= LOGF_ULPS + 1, f"{tag}: entropy is {int(d.max())} ulps from ln |T| on tie pixels"


# ------------------------------------------------------------------------------------------------ goldens from the reference
# tests/golden/confidence_*.npz (tools/make_confidence_goldens.py): the reference regressor's fp32 norm_costs and the four maps
# derived from it in float64.  ATen's p is an fp32 result within x_p of ref64, so the golden's max_prob and spread carry the
# bounds above and its entropy -sum p ln p carries sum_d p_d x_p[d] (|ln p_d| + 1) (d(p ln p) = (ln p + 1) dp).
def golden_case(shape, s):
    """-> (costs [B, D, H, W], inv_idx, z, ref (maps64 of ref64), golden-side bounds {name: array})."""
    z = np.load(os.path.join(GOLDEN, golden_name(shape, s)))
    assert float(z["factor"]) == float(s) and float(z["bf"]) == BF
    costs = np.ascontiguousarray(z["costs"][:, 0])
    inv_idx = (np.float32(z["bf"]) / z["dist_cands"].astype(np.float32)).astype(np.float32)
    r = SC.ref64(costs, inv_idx, s)
    ref = maps64(r)
    x_p, _ = SC.bounds(r)
    p = ref.p
    with np.errstate(divide="ignore", invalid="ignore"):
        b_ent = (p * x_p * (np.abs(np.log(np.where(p > 0, p, 1.0))) + 1.0)).sum(axis=1, keepdims=True)
    return costs, inv_idx, z, ref, {"max_prob": ref.b_max_prob, "entropy": b_ent, "spread": ref.b_spread}


def check_against_golden(tag, z, ref, gb, got, own_bounds):
    """got: {name: array}; every float map within (its own bound + the golden's bound) of the golden; argmax equal where sure."""
    for n in FLOAT_MAPS:
        g = np.asarray(got[n], np.float64)
        bound = gb[n] + (getattr(ref, "b_" + n) if own_bounds else 0.0)
        err = np.abs(g - z[n])
        if n == "max_prob":
            err = err / ref.max_prob
        assert float((err / bound).max()) <= 1.0, f"{tag}: {n} off the golden by {float((err / bound).max()):.3f} of the summed bounds"
    a = np.asarray(got["argmax"])
    good = (a == z["argmax"]) | ~ref.sure
    assert good.all(), f"{tag}: argmax differs from the golden at {int((~good).sum())} sure pixels"



# ------------------------------------------------------------------------------------------------ fp32, step by step
MUTANTS = ("entropy without ln S", "entropy in log2", "variance as spread", "spread around w[argmax]", "spread from E[w^2] - mu^2",
           "m from candidate 0", "x and y weights swapped", "i1 not clamped", "argmax of the nearest pixel", "highest index on ties",
           "normalised by log2 D")


def _fma(a, b, c):
    """fl32(a * b + c): the product of two fp32 numbers is exact in float64; the sum is rounded there and then to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def emulate(costs, inv_idx, s, post_div=1.0, normalize=False, mutant=None):
    """The kernel's expressions one fp32 operation at a time (np.exp, np.log, np.sqrt on fp32) -> {name: [B, 1, OH, OW]}.
    mutant: one of MUTANTS, a wrong implementation built from the same steps."""
    assert mutant is None or mutant in MUTANTS, mutant
    c = np.asarray(costs, f32)
    B, D, H, W = c.shape
    w = np.asarray(inv_idx, f32)
    i0y, i1y, l0y, l1y, srcy = SC.axis(H, s)
    i0x, i1x, l0x, l1x, srcx = SC.axis(W, s)
    if mutant == "i1 not clamped":               # the tap behind the border, read from the other side of the image
        i1y, i1x = (i0y + 1) % H, (i0x + 1) % W
    ly0, ly1 = l0y[:, None], l1y[:, None]
    lx0, lx1 = l0x[None, :], l1x[None, :]
    if mutant == "x and y weights swapped":      # the row weights of column ox mod OH, the column weights of row oy mod OW
        OHn, OWn = len(i0y), len(i0x)
        ly0, ly1 = l0y[np.arange(OWn) % OHn][None, :], l1y[np.arange(OWn) % OHn][None, :]
        lx0, lx1 = l0x[np.arange(OHn) % OWn][:, None], l1x[np.arange(OHn) % OWn][:, None]
    ra, rb = c[:, :, i0y], c[:, :, i1y]
    zx, zy = lx1 == 0, ly1 == 0
    a0, a1 = ra[..., i0x], np.where(zx, f32(0), ra[..., i1x])
    b0, b1 = np.where(zy, f32(0), rb[..., i0x]), np.where(zx | zy, f32(0), rb[..., i1x])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = _fma(ly1, _fma(lx1, b1, lx0 * b0), ly0 * _fma(lx1, a1, lx0 * a0))          # sa_blend
        m = np.fmax.reduce(v, axis=1, keepdims=True)                                      # `v > m` skips a NaN
        m = np.where(np.isnan(m), f32(-np.inf), m).astype(f32)
        hit = v == m
        k = hit.argmax(axis=1)[:, None]
        if mutant == "highest index on ties":
            k = (D - 1 - hit[:, ::-1].argmax(axis=1))[:, None]
        if mutant == "argmax of the nearest pixel":
            ny = np.minimum(np.floor((np.arange(len(i0y)) + 0.5) / s).astype(np.int64), H - 1)
            nx = np.minimum(np.floor((np.arange(len(i0x)) + 0.5) / s).astype(np.int64), W - 1)
            k = c[:, :, ny][..., nx].argmax(axis=1)[:, None]
        if mutant == "m from candidate 0":
            m = v[:, :1]
        g = (m - v).astype(f32)
        e = np.exp(-g).astype(f32)
        S = np.zeros_like(m)
        T = np.zeros_like(m)
        G = np.zeros_like(m)
        for d in range(D):
            ed, gd = e[:, d:d + 1], g[:, d:d + 1]
            S = (S + ed).astype(f32)
            T = _fma(ed, w[d], T)
            G = np.where(ed != 0, _fma(ed, np.where(ed != 0, gd, f32(0)), G), G)
        mu = (T / S).astype(f32)
        if mutant == "spread from E[w^2] - mu^2":
            Q = np.zeros_like(m)
            for d in range(D):
                Q = _fma(e[:, d:d + 1], w[d] * w[d], Q)
            var = ((Q / S).astype(f32) - mu * mu).astype(f32)
            var = np.maximum(var, f32(0))
        else:
            centre = w[k] if mutant == "spread around w[argmax]" else mu
            V = np.zeros_like(m)
            for d in range(D):
                dw = (w[d] - centre).astype(f32)
                V = _fma(e[:, d:d + 1], dw * dw, V)
            var = (V / S).astype(f32)
        sd = var if mutant == "variance as spread" else np.sqrt(var).astype(f32)
        if post_div != 1.0:
            sd = (sd / f32(post_div)).astype(f32)
        h = ((f32(0) if mutant == "entropy without ln S" else np.log(S).astype(f32)) + (G / S).astype(f32)).astype(f32)
        if mutant == "entropy in log2":
            h = (h / f32(math.log(2.0))).astype(f32)
        if normalize and D > 1:
            h = (h / f32(math.log2(D) if mutant == "normalised by log2 D" else math.log(D))).astype(f32)
        mp = (f32(1) / S).astype(f32)
    return {"max_prob": mp, "entropy": h, "spread": sd, "argmax": np.where(np.isnan(S), -1, k).astype(np.int32)}


def round64(ref):
    """The float64 maps rounded to fp32: the best any fp32 implementation can return."""
    return {"max_prob": ref.max_prob.astype(f32), "entropy": ref.entropy.astype(f32), "spread": ref.spread.astype(f32),
            "argmax": ref.argmax.astype(np.int32)}


def table_failures(impl, first_only=False):
    """Run an implementation impl(costs, inv_idx, s, post_div, normalize) -> maps over every tolerance row (plain, and
    normalised on the post_div shape), every exact row and every non-finite row -> [failure messages]."""
    fails = []

    def attempt(fn):
        try:
            fn()
        except AssertionError as ex:
            fails.append(str(ex)[:300])
        return bool(fails) and first_only
    for sh, s, sigma, pd in tol_rows():
        for norm in ((False, True) if (sh == POST_DIV_SHAPE and pd == 1.0) else (False,)):
            t = tol_case(sh, s, sigma, pd, norm)
            if attempt(lambda: check_maps(f"{sh} x{s:g} sigma {sigma:g} / {pd:g}{' normalised' if norm else ''}", t.ref,
                                          impl(t.costs, t.inv_idx, s, pd, norm))):
                return fails
    for sh, s in exact_rows():
        x = exact_case(sh, s)
        if attempt(lambda: check_exact(f"exact {sh} x{s:g}", x, impl(x.costs, x.inv_idx, s, 1.0, False))):
            return fails
    for s, sh, kind in NONFINITE:
        n = nonfinite_case(sh, s, kind)
        if attempt(lambda: check_maps(f"{kind} {sh} x{s:g}", n.ref, impl(n.costs, n.inv_idx, s, 1.0, False))):
            return fails
    return fails
