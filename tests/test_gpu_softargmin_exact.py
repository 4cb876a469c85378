"""GPU (MI355X): every kernel instance of csrc/softargmin.hip against the float64 reference of tests/softargmin_cases.py, in two
regimes.  Exact: one-hot costs at dyadic factors, np.array_equal with an expectation computed from integers (no tolerance);
at other factors the pixels ref64 classifies as one-hot (best-to-second gap >= 200) bit for bit.  Tolerance: Gaussian costs
(sigma 4; sigma 10 with post_div 96), per-element relative error of inv_dist and of every probability >= 2^-100 against a
bound derived per element (softargmin_cases.bounds), plus the range of inv_dist and sum_d p_d = 1.  Every row runs both
regimes with and without norm_costs; the two inv_dist must be torch.equal.  The conditions of a case are asserted when it is
built, here as in tests/test_softargmin_cases_host.py.

instance                                  how reached                              shapes (B, D, H, W)
----------------------------------------  ---------------------------------------  -----------------------------------------------------
softargmin_kernel, s = 1                  s = 1                                    (2,16,5,9) (1,1,2,3) (1,17,1,4) (1,33,3,7)
softargmin_kernel, s = 2                  s = 2, LDS 165,376 B > 160 KiB           (1,304,2,64)
softargmin_rows_kernel<16 | 32 | 0>       s = 2                                    D in {1,5,16} / {17,32} / {33,48}: (2,D,5,9) (1,D,1,4)
                                                                                   (1,D,3,130) (1,D,2,132); D in {5,17,33}: (1,D,1,542)
same <0>, hipFuncSetAttribute branch      s = 2, LDS > 64 KiB                      (1,128,2,64) = 69,632 B, (1,301,2,64) = 163,744 B
softargmin_band_kernel<., true>           s = 4 (SA_BAND; SA_AUTO and SA_PIXEL     as the rows table, plus (1,128,2,64) and (1,301,2,64)
                                          must give the same exact expectation)
softargmin_band_kernel<., false>          s = 8 exact; 3, 5, 6, 7 classified       as the rows table, plus (1,128,2,64)
band -> pixel fall-through                s = 4 and 3 under SA_AUTO, 165,376 B     (1,304,2,64); SA_BAND: refused with "does not fit",
                                                                                   outputs pre-filled with a sentinel and untouched
softargmin_scaled_kernel                  1.5, 2.5, 0.75 classified, 0.5 exact     (2,16,7,13) (1,33,6,10) (1,16,3,130)
                                          (weights 1/2); SA_PIXEL at 3, 4, 8

Which branch a row takes is not observable from its output; it follows from the launch rule (restated as
softargmin_cases.launch_xt / expected_instance and asserted per row with the device's CU count) and is pinned at the one place
the library reports it: D = 304 is refused by SA_BAND with "does not fit the row-band kernel's LDS", D = 301 is not.
Sizes that changed against the issue's table: at these frame sizes the launchers shrink the column tile below 64 (to 36 for
W = 130 and 132), so W = 130 has four tiles 36 + 36 + 36 + 22 (scalar staging, three seams, a ragged last tile) and W = 132
36 + 36 + 36 + 24 (16-byte staging); no W below 541 with W % 4 != 0 has a last tile of fewer than four columns at H <= 3, so
(1,D,1,542) -- fifteen tiles of 36 and one of TWO columns -- is added for one D per register form.

Non-finite costs (test_nonfinite_costs): a NaN / +inf / -inf candidate, or all candidates -inf, at one interior pixel; the expected
NaN set is ref64's (outputs that blend the pixel under a non-zero weight).
"""
import numpy as np
import pytest
import torch

import guard_arena
import softargmin_cases as C
from mvs_gi_amd import _lib, hip_ops as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANT = {"auto": H.SA_AUTO, "pixel": H.SA_PIXEL, "band": H.SA_BAND}
ROWS = C.table_rows()
RATIOS = {}                     # (instance, factor) -> [inv_dist, norm_costs]: the largest error / bound, printed by the last test


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor the library allocates during a test of this module sits between NaN-sentinel guards, and unwritten
    fp32 outputs read as NaN (tests/guard_arena.py: what is guarded, guard sizes, exemptions)."""
    yield from guard_arena.fixture_body(request)


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(c, inv_idx, f, variant, post_div=1.0):
    """Both calls (with and without norm_costs) -> (inv_dist, norm_costs) as NumPy; the two inv_dist must be the same bits."""
    inv, pr = H.softargmin(c, inv_idx, f, True, post_div=post_div, variant=VARIANT[variant])
    only, none = H.softargmin(c, inv_idx, f, False, post_div=post_div, variant=VARIANT[variant])
    torch.cuda.synchronize()
    assert none is None and torch.equal(inv.view(torch.int32), only.view(torch.int32)), "inv_dist depends on whether norm_costs is stored"
    return inv.cpu().numpy(), pr.cpu().numpy()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("rid,inst,f,variant,shape", ROWS, ids=[r[0] for r in ROWS])
def test_instance_row(rid, inst, f, variant, shape):
    C.assert_row_instance(rid, inst, f, variant, shape, _cus())
    # where SA_BAND, SA_PIXEL and SA_AUTO all apply, all three must return the same exact expectation
    variants = ("band", "auto", "pixel") if variant == "band" else (variant,)
    # ---- exact regime
    if C.is_dyadic(f):
        e = C.exact_case(shape, f)
        c, w = _g(e.costs), _g(e.inv_idx)
        for var in variants:
            for pd in C.POST_DIVS:
                inv, pr = _run(c, w, f, var, pd)
                C.assert_exact(f"{rid} [{var}] inv_dist / {pd:g}", inv, e.want_inv[pd])
                C.assert_exact(f"{rid} [{var}] norm_costs", pr, e.want_p)
    else:
        e = C.classified_case(shape, f)
        c, w = _g(e.costs), _g(e.inv_idx)
        for var in variants:
            for pd in C.POST_DIVS:
                inv, pr = _run(c, w, f, var, pd)
                C.check_classified(f"{rid} [{var}] / {pd:g}", e, inv, pr, pd)
    # ---- tolerance regime
    for sigma, pd in ((4.0, 1.0), (10.0, 96.0)):
        t = C.tol_case(shape, f, sigma, pd)
        inv, pr = _run(_g(t.costs), _g(t.inv_idx), f, variant, pd)
        ri, rp = C.check_tolerance(f"{rid} sigma {sigma:g}", t, inv, pr)
        print(f"{rid} sigma {sigma:g}: error / bound inv_dist {ri:.3f} norm_costs {rp:.3f}")
        r = RATIOS.setdefault((inst, f), [0.0, 0.0])
        r[0], r[1] = max(r[0], ri), max(r[1], rp)


@pytest.mark.parametrize("f", [4, 3])
def test_row_band_kernel_refuses_what_its_lds_cannot_hold(f):
    """D = 304 at 64 columns needs 165,376 B: SA_BAND is refused before any launch and the outputs stay as they were (SA_AUTO
    takes the thread-per-pixel kernel: the fall-through rows of the table); D = 301 (163,744 B) is the largest that runs."""
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for D, fits in ((304, False), (301, True)):
        B, Hh, W = 1, 2, 64
        assert (C.launch_xt(B, D, Hh, W, 640, _cus())[1] <= 160 * 1024) == fits
        e = C.tol_case((B, D, Hh, W), f, 4.0, 1.0)
        c, w = _g(e.costs), _g(e.inv_idx)
        inv = torch.full((B, 1, f * Hh, f * W), -7.0, device=DEV)
        pr = torch.full((B, D, f * Hh, f * W), -7.0, device=DEV)
        rc = lib.mvsgi_softargmin_scaled_f32(c.data_ptr(), w.data_ptr(), inv.data_ptr(), pr.data_ptr(), B, D, Hh, W, float(f),
                                             f * Hh, f * W, 1.0, H.SA_BAND, st)
        msg = lib.mvsgi_last_error().decode()
        torch.cuda.synchronize()
        if fits:
            assert rc == 0, msg
            C.check_tolerance(f"D = {D} x{f} SA_BAND", e, inv.cpu().numpy(), pr.cpu().numpy())
        else:
            assert rc != 0 and "does not fit the row-band kernel's LDS" in msg and "304" in msg, msg
            assert bool((inv == -7.0).all()) and bool((pr == -7.0).all())


NONFINITE = [(s, sh, k) for s, shapes in C.NONFINITE_SHAPES.items() for sh in shapes for k in C.NONFINITE_KINDS]


@pytest.mark.parametrize("s,shape,kind", NONFINITE, ids=[f"x{s}-{'x'.join(map(str, sh))}-{k}" for s, sh, k in NONFINITE])
def test_nonfinite_costs(s, shape, kind):
    """One interior low-resolution pixel holds a NaN, a +inf or a -inf in one candidate, or -inf in all.  NaN / +inf / all -inf:
    inv_dist and every candidate of norm_costs are NaN exactly at the outputs that blend the pixel under a non-zero weight (ref64's
    set), finite and inside the bound elsewhere.  One -inf: that probability is 0 there, the rest renormalise inside the bound
    of the finite candidates.  D = 5 is the register form, D = 16 at factor 1 fills it; every variant that takes the factor runs
    (factor 3: the centre-aligned outputs next to the pixel have it as a tap under a weight of exactly 0 and must stay finite)."""
    e = C.nonfinite_case(shape, s, kind)
    c, w = _g(e.costs), _g(e.inv_idx)
    for var in (("auto", "pixel") if s in (1, 2) else ("band", "auto", "pixel")):
        inv, pr = _run(c, w, s, var)
        C.check_nonfinite(f"x{s} {shape} {kind} [{var}]", e, inv, pr)


def test_error_over_bound_report():
    for (inst, f), (ri, rp) in sorted(RATIOS.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print(f"x{f:g} {inst}: largest error / bound inv_dist {ri:.3f} norm_costs {rp:.3f}")
    assert all(max(v) <= 1.0 for v in RATIOS.values())
