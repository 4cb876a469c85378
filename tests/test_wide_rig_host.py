"""CPU: the 5- to 8-camera masked-variance sweep -- the oracle against the reference's own outputs (tests/golden/wide_rig.npz),
the condition on the seeded inputs that makes the GPU tests mean something (every count of valid cameras occurs), the two
predicates of hip_ops, and the reciprocal-fma division of the kernel emulated exactly."""
import os

import numpy as np
import pytest
import torch

import wide_rig_cases as W
from grid_exact_cases import fma_f32
from mvs_gi_amd import hip_ops as H
from oracle import mvsgi_oracle as O


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "wide_rig.npz"))


@pytest.mark.parametrize("N", W.NS)
def test_oracle_reproduces_the_reference(z, N):
    """1e-6 of the tensor's maximum and the same zeros (the bar of test_sweep_std_nchw_five_and_six_cameras): another host's
    ATen may associate the camera sum differently from five addends on."""
    inp = W.small_case(N)
    assert W.digest(inp) == str(z[f"inputs_sha256_{N}"])
    want = z[f"vol_raw_{N}"]
    got = O.sweep_std_masked(*(torch.from_numpy(inp[k]) for k in ("feats", "grids", "grid_masks", "masks"))).numpy()
    assert got.shape == want.shape == (W.B, W.GOLDEN_C[N], W.D, W.HO, W.WO)
    print(f"N = {N}: rel {_rel(got, want):.3e}, {int((got != want).sum())} of {got.size} elements differ")
    assert _rel(got, want) <= 1e-6 and np.array_equal(got == 0, want == 0)


@pytest.mark.parametrize("N", W.NS)
def test_every_count_of_valid_cameras_occurs(N):
    inp = W.small_case(N)
    g = torch.from_numpy(inp["grids"]).flatten(0, 1)
    m = torch.from_numpy(inp["masks"]).flatten(0, 1)
    counts = np.zeros(N + 1, np.int64)
    for d in range(W.D):
        sm = (O.bilinear_sample_zeros(m, g[:, d]) > 0.0).reshape(W.B, N, W.HO, W.WO).numpy()
        n = (sm & inp["grid_masks"][:, :, d, :, :, 0]).sum(1)
        counts += np.bincount(n.ravel(), minlength=N + 1)
    print(f"N = {N}: voxels per count of valid cameras {counts.tolist()}")
    assert counts.sum() == W.B * W.D * W.HO * W.WO == 3360 and (counts > 0).all()


def test_predicates():
    f = lambda n, c: torch.empty((1, n, c, 2, 2))
    assert H.sweep_max_cams() == 8
    assert H.valid_sweep_ok(f(8, 16)) and H.valid_sweep_ok(f(8, 8)) and H.valid_sweep_ok(f(5, 4)) and H.valid_sweep_ok(f(3, 16))
    assert not H.valid_sweep_ok(f(9, 16)) and not H.valid_sweep_ok(f(8, 6)) and not H.valid_sweep_ok(torch.empty((8, 16, 2, 2)))
    assert H.nhwc_sweep_ok(f(4, 16)) and not H.nhwc_sweep_ok(f(5, 16))      # the mask-sampling channels-last kernel stays at N <= 4


# ------------------------------------------------------------------------------ the division sequence
def _markstein(x, d):
    inv = np.float32(1.0) / np.float32(d)
    dd = np.full_like(x, np.float32(d))
    q = (x.astype(np.float64) * np.float64(inv)).astype(np.float32)
    r = fma_f32(-dd, q, x)
    return fma_f32(r, np.full_like(x, inv), q)


@pytest.mark.parametrize("d", [5, 6, 7, 8])
def test_reciprocal_fma_division_is_the_rounded_quotient(d):
    """q = RN(x inv), r = x - d q, RN(q + r inv) with inv = RN(1 / d) equals IEEE x / d for |x| in [1e-30, 1e30] (the range the
    kernel uses it in), on 4e5 random floats per divisor with uniformly drawn exponent and mantissa bits."""
    rng = np.random.default_rng(d)
    n = 400_000
    lo, hi = np.float32(1e-30).view(np.uint32), np.float32(1e30).view(np.uint32)
    bits = rng.integers(int(lo), int(hi) + 1, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))
    x = bits.view(np.float32)
    assert np.isfinite(x).all() and (np.abs(x) >= np.float32(1e-30)).all() and (np.abs(x) <= np.float32(1e30)).all()
    want = x / np.float32(d)
    assert np.array_equal(_markstein(x, d).view(np.uint32), want.view(np.uint32))
    assert float.fromhex({5: "0x1.99999ap-3", 6: "0x1.555556p-3", 7: "0x1.24924ap-3", 8: "0x1p-3"}[d]) == float(np.float32(1.0) / np.float32(d))      # the kernel's table


def test_tiny_operands_need_the_hardware_division():
    """Why the kernel sends non-zero operands below 1e-30 to the hardware division: a subnormal x = (6 k + 3) ulp divided by 6 is
    an exact tie between two subnormals, which the sequence resolves by the sign of its residual instead of to even."""
    ulp = np.float32(2.0 ** -149)
    x = (np.arange(0, 200, dtype=np.float32) * 6 + 3) * ulp
    want = x / np.float32(6)
    assert (_markstein(x, 6).view(np.uint32) != want.view(np.uint32)).any()
