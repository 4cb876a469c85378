"""CPU: the conditions of tests/softargmin_cases.py -- every case of the instance table builds with its conditions holding (blends
representable, gaps >= 104, ATen fp32 bit-equal to the integer expectation, at most 30 % of a classified case left out, at most
2 % of the probabilities below 2^-100), ATen fp32 on the CPU stays inside the derived per-element bound for every row, ref64
reproduces the reference's golden outputs inside it, the restated launch rule sends every row to the instance the table names,
and the expected NaN sets of the non-finite cases against ATen.  A fp32 NumPy soft-argmin with a weight off by 2^-19 must leave
the bound: it sees what the 1e-5 bar of tests/test_softargmin_scales_host.py cannot."""
import math
import os

import numpy as np
import pytest

import softargmin_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ROWS = C.table_rows()
RATIOS = {}                     # factor -> [inv_dist, norm_costs]: ATen's largest error / bound, printed by the last test


def impl32(costs, inv_idx, s, l1_scale=f32(1), post_div=1.0):
    """The kernels' arithmetic in NumPy fp32 (blend tree, max, exp, sums, t / s, v * (1 / s)); l1_scale != 1 is scratch defect (b)."""
    B, D, H, W = costs.shape
    y, x = C.axis(H, s), C.axis(W, s)
    ly1, lx1 = (y[3] * l1_scale).astype(f32)[:, None], (x[3] * l1_scale).astype(f32)
    ly0, lx0 = y[2][:, None], x[2]
    ra, rb = costs[:, :, y[0]], costs[:, :, y[1]]
    v = ly0 * (lx0 * ra[..., x[0]] + lx1 * ra[..., x[1]]) + ly1 * (lx0 * rb[..., x[0]] + lx1 * rb[..., x[1]])
    assert v.dtype == np.float32
    e = np.exp(v - v.max(axis=1, keepdims=True))
    ssum = e.sum(axis=1, keepdims=True, dtype=np.float32)
    t = (e * inv_idx.reshape(1, -1, 1, 1)).sum(axis=1, keepdims=True, dtype=np.float32)
    inv = t / ssum
    return (inv if post_div == 1.0 else inv / f32(post_div)), e * (f32(1) / ssum)


# ------------------------------------------------------------------------------------------------ the table
def test_every_row_reaches_the_instance_the_table_names():
    """The launch rule of csrc/softargmin.hip restated (256 CUs): register form by D, LDS of the chosen column tile against
    64 KiB (attribute branch) and 160 KiB (thread-per-pixel kernel / SA_BAND refusal)."""
    seen = set()
    for rid, inst, f, variant, shape in ROWS:
        seen.add(C.assert_row_instance(rid, inst, f, variant, shape))
    want = {"softargmin_kernel s=1", "softargmin_kernel s=2", "softargmin_scaled_kernel", "softargmin_rows_kernel<0> attr",
            "softargmin_band_kernel<0,true> attr", "softargmin_band_kernel<0,false> attr"}
    want |= {f"softargmin_rows_kernel<{d}>" for d in (16, 32, 0)}
    want |= {f"softargmin_band_kernel<{d},{x}>" for d in (16, 32, 0) for x in ("true", "false")}
    assert seen == want, seen ^ want
    # the sizes the table quotes
    assert C.launch_xt(1, 128, 2, 64) == (64, 69632) and C.launch_xt(1, 301, 2, 64) == (64, 163744)
    assert C.launch_xt(1, 304, 2, 64) == (64, 165376) and 163744 <= 160 * 1024 < 165376
    # tiles: W = 130 and 132 shrink to 36 columns (scalar / 16-byte staging, seams, a ragged last tile of 22 / 24 columns);
    # the narrowest ragged tile a small frame can have is at W = 542: fifteen tiles of 36 and one of two columns
    assert C.launch_xt(1, 16, 3, 130)[0] == 36 and C.launch_xt(1, 16, 2, 132)[0] == 36 and C.launch_xt(1, 17, 1, 542)[0] == 36
    assert 130 % 36 == 22 and 132 % 36 == 24 and 542 % 36 == 2
    assert all(W % C.launch_xt(1, 16, 1, W)[0] not in (1, 2, 3) for W in range(65, 541) if W % 4)


@pytest.mark.parametrize("rid,inst,f,variant,shape", ROWS, ids=[r[0] for r in ROWS])
def test_row_conditions_and_aten_inside_the_bound(rid, inst, f, variant, shape):
    if C.is_dyadic(f):
        c = C.exact_case(shape, f)                # asserts representability, gaps, ATen == expectation
        assert c.want_p.shape[2:] == (math.floor(shape[2] * f), math.floor(shape[3] * f))
    else:
        c = C.classified_case(shape, f)
        assert c.left_out <= 0.30
        for pd in C.POST_DIVS:
            inv, pr = C.aten32(c.costs, c.inv_idx, f, pd)
            C.check_classified(f"ATen {rid} /{pd:g}", c, inv, pr, pd)
    for sigma, pd in ((4.0, 1.0), (10.0, 96.0)):
        t = C.tol_case(shape, f, sigma, pd)
        assert t.below <= 0.02
        inv, pr = C.aten32(t.costs, t.inv_idx, f, pd)
        ri, rp = C.check_tolerance(f"ATen {rid} sigma {sigma:g}", t, inv, pr)
        w = RATIOS.setdefault(f, [0.0, 0.0])
        w[0], w[1] = max(w[0], ri), max(w[1], rp)


def test_aten_ratios_report():
    for f, (ri, rp) in sorted(RATIOS.items()):
        print(f"ATen fp32 x{f:g}: largest error / bound inv_dist {ri:.3f} norm_costs {rp:.3f}")
    assert all(max(v) <= 1.0 for v in RATIOS.values())


# ------------------------------------------------------------------------------------------------ ref64 itself
def test_ref64_reproduces_the_reference_goldens_inside_the_bound():
    """tests/golden/regress_scales.npz holds the outputs of the reference's own regressor (fp32): an implementation like any
    other to ref64."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "regress_scales.npz"))
    for i, s in enumerate(z["factors"]):
        costs = np.ascontiguousarray(z[f"costs_{i}"][:, 0])
        inv_idx = (float(z["bf"]) / z[f"dist_cands_{i}"]).astype(f32)
        r = C.ref64(costs, inv_idx, float(s))
        bp, bi = C.bounds(r)
        t = C.SimpleNamespace(r=r, bound_p=bp, bound_inv=bi, inv_idx=inv_idx, post_div=1.0)
        ri, rp = C.check_tolerance(f"golden row {i} x{float(s):g}", t, z[f"inv_{i}"], z[f"pr_{i}"] if f"pr_{i}" in z else None)
        print(f"golden row {i} x{float(s):g}: error / bound inv_dist {ri:.3f} norm_costs {rp:.3f}")


def test_expectation_is_not_the_weighted_sum_of_rounded_probabilities():
    """|T| = 3: fl32(t / 3) is what t / s gives; sum(fl32(1 / 3) * inv_idx) in fp32 is another number for some t."""
    inv_idx = C.int_candidates(48)
    third = f32(1) / f32(3)
    differ = 0
    for a in range(0, 46):
        T = inv_idx[[a, a + 1, a + 2]]
        want = f32(float(T.sum()) / 3.0)
        got = f32(0)
        for w in T:
            got = f32(got + third * w)
        differ += int(got != want)
    assert differ > 0


@pytest.mark.parametrize("s", [2, 3, 4])
def test_a_weight_off_by_a_few_ulps_of_bf16_leaves_the_bound(s):
    """Scratch defect (b) in NumPy: l1 * (1 + eps).  The correct fp32 arithmetic passes both regimes.  eps = 2^-12 fails the
    tolerance regime and the 1e-5 `_rel` bar of the older tests alike; eps = 2^-19 fails the tolerance regime and sits UNDER
    the older bar.  The exact regime cannot see a weight error: the gaps stay far above 104 and the tie sets (same winners,
    same taps) are unchanged -- it checks taps, staging, tie arithmetic and the divisions; the weights are the other regime's."""
    shape = (2, 16, 5, 9)
    t = C.tol_case(shape, s, 10.0, 1.0)
    C.check_tolerance("fp32 NumPy", t, *impl32(t.costs, t.inv_idx, s))
    a_inv, a_pr = C.aten32(t.costs, t.inv_idx, s)
    for k in (12, 19):
        bad_inv, bad_pr = impl32(t.costs, t.inv_idx, s, f32(1 + 2.0 ** -k))
        with pytest.raises(AssertionError):
            C.check_tolerance("defect (b)", t, bad_inv, bad_pr)
        rel = max(np.abs(bad_inv - a_inv).max() / a_inv.max(), np.abs(bad_pr - a_pr).max() / a_pr.max())
        print(f"x{s} defect (b) eps 2^-{k}: _rel {rel:.2e}")
        assert (rel <= 1e-5) == (k == 19)
    if C.is_dyadic(s):
        e = C.exact_case(shape, s)
        inv, pr = impl32(e.costs, e.inv_idx, s)
        C.assert_exact("fp32 NumPy inv_dist", inv, e.want_inv[1.0])
        C.assert_exact("fp32 NumPy norm_costs", pr, e.want_p)


# ------------------------------------------------------------------------------------------------ non-finite costs
NONFINITE = [(s, sh, k) for s, shapes in C.NONFINITE_SHAPES.items() for sh in shapes for k in C.NONFINITE_KINDS]


@pytest.mark.parametrize("s,shape,kind", NONFINITE, ids=[f"x{s}-{'x'.join(map(str, sh))}-{k}" for s, sh, k in NONFINITE])
def test_nonfinite_expectation_against_aten(s, shape, kind):
    """ref64's NaN set (outputs that blend the non-finite pixel under a NON-ZERO weight) against ATen.  They agree at factors 1
    (where the regressor does not interpolate), 2 and 4.  At factor 3 ATen returns NaN at more pixels: the centre-aligned
    output of the pixel to the left / above has the non-finite pixel as its right / lower tap under a weight of exactly 0, and
    0 * inf is NaN.  ref64's rule stands; the difference is exactly `zero_weight_neighbours`."""
    c = C.nonfinite_case(shape, s, kind)
    inv, pr = C.aten32(c.costs, c.inv_idx, s)
    extra = C.zero_weight_neighbours(c)[None, None]
    if s == 1:                                    # every pixel has such a tap at factor 1; the regressor reads none of them
        assert int(extra.sum()) == 3
        extra = np.zeros_like(extra)
    assert extra.any() == (s == 3)
    assert not (extra & c.touched).any()
    if kind == "-inf":
        a_nan = np.isnan(inv)
        assert np.array_equal(a_nan, extra & np.ones_like(a_nan)), "ATen is NaN only where a zero weight meets the -inf"
        keep = ~np.broadcast_to(extra, inv.shape)
        inv2, pr2 = np.where(keep, inv, c.r.inv.astype(f32)), np.where(keep, pr, c.r.p.astype(f32))
        if not extra.any():
            C.check_nonfinite(f"ATen x{s} {kind}", c, inv2, pr2)
        else:                                     # the sum-to-one property is ATen's own only off the patched pixels
            r = c.r
            e = np.where(keep, np.abs(inv.astype(np.float64) - r.inv) / r.inv / c.bound_inv, 0.0)
            assert float(e.max()) <= 1.0
            assert (pr[np.broadcast_to(keep, pr.shape) & ~c.finite] == 0).all()
    else:
        assert np.array_equal(np.isnan(inv), c.nan_px | extra)
        assert np.array_equal(np.isnan(pr), np.broadcast_to(c.nan_px | extra, pr.shape))
    # the set itself: a (2 s) x (2 s) block of outputs at an even factor, one pixel at factor 1
    n = int(c.touched.sum())
    assert n == {1: 1, 2: 16, 4: 64, 3: 25}[s], n
