"""CPU: the checker of the confidence maps (tests/confidence_cases.py) accepts an honest fp32 implementation and rejects wrong
ones; the exact regime; the committed goldens of the reference's norm_costs; the library's symbol; hip_ops.confidence's
argument errors.  The device runs the same table in tests/test_gpu_confidence.py."""
import os
import re

import numpy as np
import pytest
import torch

import confidence_cases as CC
import softargmin_cases as SC
from mvs_gi_amd import _lib, hip_ops as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = CC.GOLDEN


# ------------------------------------------------------------------------------ 1. the checker accepts an honest implementation
def test_checker_accepts_the_fp32_emulation_and_the_rounded_reference():
    fails = CC.table_failures(lambda c, w, s, pd, norm: CC.emulate(c, w, s, pd, norm))
    assert not fails, "\n".join(fails[:5])
    worst = dict.fromkeys(CC.MAPS, 0.0)
    for sh, s, sigma, pd in CC.tol_rows():
        t = CC.tol_case(sh, s, sigma, pd)
        CC.check_maps(f"float64 rounded {sh} x{s:g} sigma {sigma:g}", t.ref, CC.round64(t.ref))
        for n, v in CC.check_maps("emulation", t.ref, CC.emulate(t.costs, t.inv_idx, s, pd)).items():
            worst[n] = max(worst[n], v)
    print("fp32 emulation, largest error / bound (argmax: largest ambiguous fraction):", {n: round(v, 4) for n, v in worst.items()})
    assert worst["argmax"] <= CC.AMBIGUOUS_MAX


def test_the_two_entropy_expressions_agree_in_float64():
    for sh, s in (((2, 16, 7, 13), 2), ((1, 48, 2, 132), 1.5)):
        t = CC.tol_case(sh, s, 10.0)
        p = t.ref.p
        with np.errstate(divide="ignore", invalid="ignore"):
            direct = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(axis=1, keepdims=True)
        assert float(np.abs(direct - t.ref.entropy).max()) <= 1e-14
        assert np.allclose(t.ref.max_prob, p.max(axis=1, keepdims=True), rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------ 2. ... and rejects wrong ones
@pytest.mark.parametrize("mutant", CC.MUTANTS)
def test_checker_rejects(mutant):
    fails = CC.table_failures(lambda c, w, s, pd, norm: CC.emulate(c, w, s, pd, norm, mutant=mutant), first_only=True)
    assert fails, f"the table accepts '{mutant}'"
    print(f"{mutant}: {fails[0]}")


# ------------------------------------------------------------------------------ 3. exact regime
@pytest.mark.parametrize("shape,s", CC.exact_rows(), ids=[f"{'x'.join(map(str, sh))}-x{s}" for sh, s in CC.exact_rows()])
def test_exact_regime_emulation(shape, s):
    c = CC.exact_case(shape, s)
    CC.check_exact(f"{shape} x{s}", c, CC.emulate(c.costs, c.inv_idx, s))


def test_exact_regime_has_ties():
    assert sum(CC.exact_case(sh, s).ties for sh, s in CC.exact_rows()) > 100
    assert all(CC.exact_case(sh, s).single.any() for sh, s in CC.exact_rows())


# ------------------------------------------------------------------------------ goldens from the reference
@pytest.mark.parametrize("shape,s", CC.GOLDEN_ROWS, ids=[CC.golden_name(sh, s)[:-4] for sh, s in CC.GOLDEN_ROWS])
def test_float64_maps_agree_with_the_reference_goldens(shape, s):
    costs, inv_idx, z, ref, gb = CC.golden_case(shape, s)
    # ATen's norm_costs itself: an fp32 result within x_p of ref64
    x_p, _ = SC.bounds(SC.ref64(costs, inv_idx, s))
    big = ref.p >= SC.P_FLOOR
    assert float((np.abs(z["norm_costs"] - ref.p) / ref.p / x_p)[big].max()) <= 1.0
    ref_maps = {n: getattr(ref, n) for n in CC.MAPS}
    CC.check_against_golden(f"{shape} x{s}", z, ref, gb, ref_maps, own_bounds=False)
    # and the emulation, within the summed bounds
    CC.check_against_golden(f"{shape} x{s} emulation", z, ref, gb, CC.emulate(costs, inv_idx, s), own_bounds=True)


def test_goldens_are_small_data():
    for sh, s in CC.GOLDEN_ROWS:
        path = os.path.join(GOLDEN, CC.golden_name(sh, s))
        assert os.path.getsize(path) < 512 * 1024
        z = np.load(path)
        assert sorted(z.files) == sorted(["costs", "dist_cands", "bf", "factor", "norm_costs", *CC.MAPS])


# ------------------------------------------------------------------------------ 4. the library
def test_library_exports_and_header_declares_the_symbol():
    src = open(os.path.join(ROOT, "include", "mvsgi.h")).read()
    assert re.search(r"\bint\s+mvsgi_confidence_f32\s*\(", src)
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert hasattr(lib, "mvsgi_confidence_f32") and "mvsgi_confidence_f32" in _lib.SIGNATURES
    assert lib.mvsgi_abi_version() == 8
    import ctypes
    p = ctypes.c_void_p(16)
    for args, word in (((p, p, p, p, p, p, 1, 8, 4, 4, 0.0, 4, 4, 1.0, 0, None), b"scale"),
                       ((p, p, p, p, p, p, 1, 8, 4, 4, float("nan"), 4, 4, 1.0, 0, None), b"scale"),
                       ((p, p, p, p, p, p, 1, 8, 4, 4, -2.0, 4, 4, 1.0, 0, None), b"scale"),
                       ((p, p, p, p, p, p, 1, 8, 4, 4, 1.5, 6, 7, 1.0, 0, None), b"floor"),
                       ((p, p, None, None, None, None, 1, 8, 4, 4, 2.0, 8, 8, 1.0, 0, None), b"null")):
        assert lib.mvsgi_confidence_f32(*args) != 0 and word in lib.mvsgi_last_error(), (args, lib.mvsgi_last_error())


# ------------------------------------------------------------------------------ 5. argument errors before any device work
def test_hip_ops_confidence_argument_errors(monkeypatch):
    def no_device_work(*a, **k):
        raise AssertionError("a launch was attempted")
    monkeypatch.setattr(H, "_call", no_device_work)
    costs, w = torch.zeros((1, 4, 3, 5)), torch.ones(4)
    for want in ((), ("max_prob", "max_prob"), ("confidence",), ("entropy", "variance")):
        with pytest.raises(ValueError, match="want"):
            H.confidence(costs, w, 2, want=want)
    for scale in (0, -1.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            H.confidence(costs, w, scale)
    with pytest.raises(ValueError, match="empty"):
        H.confidence(costs, w, 0.1)
    good = {n: torch.zeros((1, 1, 6, 10), dtype=torch.int32 if n == "argmax" else torch.float32) for n in CC.MAPS}
    with pytest.raises(AssertionError, match="out"):
        H.confidence(costs, w, 2, out=dict(good, entropy=torch.zeros((1, 1, 6, 11))))
    with pytest.raises(TypeError, match="out"):
        H.confidence(costs, w, 2, out=dict(good, argmax=torch.zeros((1, 1, 6, 10), dtype=torch.int64)))
    with pytest.raises(TypeError, match="out"):
        H.confidence(costs, w, 2, out=dict(good, spread=torch.zeros((1, 1, 6, 10), dtype=torch.float64)))
    with pytest.raises(AssertionError, match="out"):
        H.confidence(costs, w, 2, out=dict(good, max_prob=torch.zeros((1, 1, 10, 6)).transpose(2, 3)))
    with pytest.raises(TypeError, match="out"):
        H.confidence(costs, w, 2, want=("spread",), out={})
    with pytest.raises(RuntimeError, match="GPU only"):          # everything above was checked before the tensors' device
        H.confidence(costs, w, 2, out=good)
