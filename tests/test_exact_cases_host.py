"""The exact-operand cases of tests/exact_cases.py, on the CPU: the reference alone keeps every case inside the conditions under
which a correct kernel must return the float64 bits.  For every case of the table make_case() asserts
  * hi + lo == operand bit for bit under the torch emulation of the split, and exactly one operand has lo != 0 (on the upsampled
    activation for the trilinear forms, on the transformed operands for Winograd);
  * condition (a) on |hi| + |lo|, (b) at every epilogue stage, (c) on the delivered output;
  * hi*hi + hi*lo + lo*hi in float64 equals the full convolution;
  * ATen's fp32 convolution (another summation order) equals float64.
The tests below build every case, check the figures make_case() reports, and pin the helpers themselves.  The launch-size cases
of tests/test_gpu_exact_launches.py (E.launch_cases) are built here too: the conditions on their distinct frames, the properties of
the frame sequence, and the expanded reference against a direct float64 evaluation of frames of the batch itself."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_cases as E

ALL = [(fam, name) for fam in E.TABLE for name in E.ids(fam)]


@pytest.mark.parametrize("family,name", ALL, ids=[f"{f}-{n}" for f, n in ALL])
def test_case_meets_the_conditions(family, name):
    c = E.case(family, name)                         # the conditions are asserted while the case is built
    assert 0.0 < c.abs_sum_frac < 1.0                # (a)
    assert E.representable(c.acc) and E.representable(c.ref)      # (b)
    assert c.bound is None or c.out_max < c.bound    # (c)
    assert 2.0 ** -8 <= c.density <= 1.0
    wide_op = c.x if c.regime == "x_wide" else c.w
    if c.polywino:      # 8- to 10-bit operands: the lo part appears in the kernel's own domain, where (a) holds in its lsb units too
        V, U = E.polywino_operands(c.x.double(), c.w.double())
        assert bool(E.split(V, "f16")[1].any()) != bool(E.split(U, "f16")[1].any())
        assert bool(E.split(V if c.regime == "x_wide" else U, "f16")[1].any())
        assert 0.0 < c.polywino_abs_sum < E.TWO24 and c.polywino_abs_sum <= c.abs_sum
    elif c.fmt != "f32":
        assert bool(E.split(wide_op, c.fmt)[1].any())      # the wide operand has a lo part before any transform, too
    s = c.scale.numpy()
    assert len(set(s.tolist())) == min(3, len(s)) and (np.log2(s) == np.round(np.log2(s))).all()      # powers of two that vary by channel
    assert torch.equal(torch.round(c.shift), c.shift) and (c.r is None or torch.equal(torch.round(c.r), c.r))
    if c.up2:
        assert float(((c.w if c.regime == "x_wide" else c.x) % 64).abs().max()) == 0.0
    if c.wino:
        assert float((c.w % 4).abs().max()) == 0.0


def test_table_covers_both_regimes_and_every_slope():
    for fam, rows in E.TABLE.items():
        kws = [kw for _, kw in rows]
        assert {kw["regime"] for kw in kws} == set(E.REGIMES), fam
    assert {kw["slope"] for rows in E.TABLE.values() for _, kw in rows} == set(E.SLOPES)


@pytest.mark.parametrize("name", E.RESBLOCK_IDS)
def test_resblock_case_meets_the_conditions(name):
    c = E.resblock_case(name)
    assert 0.0 < c.abs_sum_frac < 1.0 and E.representable(c.ref)
    assert (c.m_has_lo, c.w2_has_lo) == ((False, True) if c.regime == "w2_wide" else (True, False))      # conv2: each cross term in some regime


def test_polywino_domain_reproduces_interpolate_then_conv():
    """The domain the Winograd-form polyphase conditions are asserted in (V_up, U) gives interpolate -> conv off the H and W faces."""
    rng = np.random.default_rng(3)
    x, w = E.narrow(rng, (1, 2, 3, 6, 8), 7), E.narrow(rng, (2, 2, 3, 3, 3), 3) * 64
    V, U = E.polywino_operands(x, w)
    y = E.polywino_to_volume(E._polywino_y(V, U, E._AT))
    ref = F.conv3d(F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=False), w, padding=1)
    assert y.shape == ref.shape and torch.equal(y[:, :, :, 2:-2, 2:-2], ref[:, :, :, 2:-2, 2:-2])
    assert not torch.equal(y, ref)                      # the faces differ: they are the face kernels' corrections
    assert E.polywino_abs_sum(x, w) >= float(y.abs().max())


@pytest.mark.parametrize("i", range(len(E.DEFORM_ROWS)))
def test_deform_case_meets_the_conditions(i):
    c = E.deform_case(i)
    assert 0.0 < c.abs_sum_frac < 1.0
    off = c.off["per_image"]
    assert torch.equal(torch.round(off * 4), off * 4) and float(off.max()) == 1e4 and float(off.min()) == -50.0
    assert torch.equal(c.off["shared"][0], off[0]) and all(E.representable(r) for r in c.ref.values())


@pytest.mark.parametrize("i", range(len(E.RESIZE_CASES)))
def test_resize_case_is_exact_in_fp32(i):
    c = E.resize_case(i)
    assert E.representable(c.ref) and torch.equal(torch.round(c.ref / c.lsb), c.ref / c.lsb)


def test_split_emulation_known_values():
    x = torch.tensor([1023.0, 257.0, 4095.0, 1e5, -3e9, 0.0, 2049.0])
    hi, lo = E.split(x, "bf16")
    assert hi.tolist()[:3] == [1024.0, 256.0, 4096.0] and lo.tolist()[:3] == [-1.0, 1.0, -1.0]
    hi, lo = E.split(x, "f16")
    assert hi.tolist() == [1023.0, 257.0, 4096.0, 65504.0, -65504.0, 0.0, 2048.0] and lo.tolist() == [0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0]
    y = torch.tensor([12345.678, -0.3333])
    for fmt, bits in (("bf16", 15), ("f16", 21)):       # hi + lo keeps at least 8 + 7 / 11 + 10 bits
        assert float(((E.split_join(y, fmt) - y).abs() / y.abs()).max()) <= 2.0 ** -bits
    assert not np.array_equal(E.expected_split(torch.tensor([131329.0], dtype=torch.float64), "bf16"), [131329.0])     # 2^17 + 257: lo would need 9 bits


def test_winograd_transforms_reproduce_the_convolution():
    rng = np.random.default_rng(0)
    x, w = E.narrow(rng, (1, 3, 4, 4, 6), 7), E.narrow(rng, (2, 3, 3, 3, 3), 3) * 4
    V, U = E.wino_operands(x, w)
    M = sum(torch.einsum("bcdhwae,ocae->bodhwae", V[:, :, kd:kd + 4], U[:, :, kd]) for kd in range(3))
    y = torch.einsum("pa,bodhwae,qe->bodhwpq", E._AT, M, E._AT).permute(0, 1, 2, 3, 5, 4, 6).reshape(1, 2, 4, 4, 6)
    assert torch.equal(y, F.conv3d(x, w, padding=1))
    assert E.wino_abs_sum(x, w) >= float(F.conv3d(x.abs(), w.abs(), padding=1).max())


def test_mismatch_report_and_assert_exact():
    want = np.arange(12, dtype=np.float32).reshape(3, 4) * 0.25
    got = want.copy()
    E.assert_exact(got, want)
    got[1, 2] += 0.5
    got[2, 3] -= 0.25
    rep = E.mismatch_report(got, want, lsb=0.25)
    assert "2 of 12" in rep and "(1, 2)" in rep and "2 lsb" in rep
    with pytest.raises(AssertionError, match="2 of 12"):
        E.assert_exact(got, want, 0.25, "probe")
    got[0, 0] = np.nan
    assert "NaN" in E.mismatch_report(got, want)
    assert E.mismatch_report(want[:2], want).startswith("shape")


def test_a_dropped_cross_term_under_the_old_bar_is_not_exact():
    """One input channel of one tap missing from the lo(x) * hi(w) stream: under the 1e-4 of the tensor's maximum that the bf16
    split's tolerance tests allow (the figure they compute), and still a mismatch here."""
    c = E.case("conv3d_rs_bf16", "(2, 5, 7, 37)-x_wide-res0")
    xhi, xlo = (t.double() for t in E.split(c.x, "bf16"))
    w1 = c.w64.clone()
    w1[:, 0, 1, 1, 1] = 0                                   # centre tap, input channel 0, of the lo stream only
    broken = F.conv3d(xhi, c.w64, padding=1) + F.conv3d(xlo, w1, padding=1)
    assert not torch.equal(broken, c.acc)
    rel = float((broken - c.acc).abs().max() / c.acc.abs().max())       # _rel() of tests/test_gpu_parity.py
    assert 0.0 < rel < 1e-4, rel
    assert "differ" in E.mismatch_report(broken.numpy(), c.acc.numpy())


# ------------------------------------------------------------------------------------------------ launch-size cases
LAUNCH = E.launch_cases()
# the direct float64 evaluation runs on the FULL batch for these three, on two frames of the sequence for every other case
FULL_BATCH = ("variant-B3_N64_S-12-bf16-x_wide", "variant-B3DU2_N64-24-f16-w_wide", "walk-conv3d_rs16-bf16-x_wide")


def test_full_batch_rows_exist():
    assert set(FULL_BATCH) <= {i for i, _ in LAUNCH}


@pytest.mark.parametrize("cid,build", LAUNCH, ids=[i for i, _ in LAUNCH])
def test_launch_case_meets_the_conditions_and_expands_to_the_direct_reference(cid, build):
    c = build()                                      # (a)-(c), the split identities and ATen == float64 on the distinct frames
    B = c.x.shape[0]
    assert c.n_frames == min(E.FRAMES, B) and c.x_frames.shape[0] == c.n_frames and c.ref.shape[0] == B
    E.check_frame_index(c.idx, B, c.n_frames)
    assert torch.equal(c.x, c.x_frames[torch.from_numpy(c.idx)])
    assert 0.0 < c.abs_sum_frac < 1.0 and E.representable(c.ref) and (c.bound is None or c.out_max < c.bound)
    assert c.r is None or c.r.shape[0] == B
    if c.r is not None and B > c.n_frames:           # the residual is not periodic: two occurrences of a frame carry different ones
        b0, b1 = (int(b) for b in np.flatnonzero(c.idx == c.idx[0])[:2])
        assert not torch.equal(c.r[b0], c.r[b1])
    if cid in FULL_BATCH:
        frames = range(B)
    else:                                            # the last frame and the one before it (always two different frames)
        frames = sorted({B - 1, max(B - 2, 0)})
    assert torch.equal(E.direct_reference(c, frames), c.ref[list(frames)])


@pytest.mark.parametrize("regime", E.RESBLOCK_REGIMES)
def test_resblock_walk_case(regime):
    c = E.resblock_walk_case(regime)
    B = c.x.shape[0]
    E.check_frame_index(c.idx, B, c.n_frames)
    assert c.n_frames == E.FRAMES and c.ref.dtype == torch.float64
    assert torch.equal(c.x, c.x_frames[torch.from_numpy(c.idx)]) and 0.0 < c.abs_sum_frac < 1.0 and E.representable(c.ref)
    bc = (1, -1, 1, 1)
    for b in (B - 1, B - 2):                          # the block evaluated directly on a frame of the batch
        x = c.x[b:b + 1].double()
        m = F.conv2d(x, c.w1.double(), padding=1) * c.s1.double().view(bc) + c.b1.double().view(bc)
        m = torch.where(m > 0, m, m * c.slope)
        y = F.conv2d(m, c.w2.double(), padding=1) * c.s2.double().view(bc) + c.b2.double().view(bc) + x
        assert torch.equal(torch.where(y > 0, y, y * c.slope), c.ref[b:b + 1])


def test_frame_index_properties():
    for B, Fr in ((2, 2), (3, 3), (5, 4), (12, 4), (32, 4), (130, 4), (260, 4), (7, 7)):
        idx = E.frame_index(B, Fr, seed=B)
        E.check_frame_index(idx, B, Fr)
        assert np.array_equal(idx, E.frame_index(B, Fr, seed=B))            # drawn from the seed alone
    assert E.frame_index(1, 1, 0).tolist() == [0]
    with pytest.raises(AssertionError, match="neighbouring"):
        E.check_frame_index([0, 1, 1, 2, 3], 5, 4)
    with pytest.raises(AssertionError, match="does not occur"):
        E.check_frame_index([0, 1, 0, 1, 2], 5, 4)
    with pytest.raises(AssertionError, match="ordered pair"):
        E.check_frame_index(([0, 1, 2, 3] * 9)[:33] , 33, 4)


def test_launch_tables_name_every_variant_row_once_and_count_their_units():
    import os
    variants = E.parse_variants_inc(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mvs_gi_amd", "csrc", "conv3d_variants.inc"))
    assert len(variants) == 67 and {r[0] for r in E.VARIANT_ROWS} == set(variants)
    assert E.variant_kernel_name(variants, "B3D_N128_PW8", "f16") == "conv3d_f16x3_d32_dk_kernel<2, 5, 1, 4, 1, 10, 8>"
    assert E.variant_kernel_name(variants, "V_S2_N64_B64", "f32") == "conv3d_mfma_kernel<2, 2, 2, 2, 2, 4, 8, 2>"
    for family in E.WALKS:
        units, R = E.walk_units(family)
        assert units >= 2 * R + 1 and 0 < units % R < R
    for row in E.VARIANT_ROWS[-3:]:                    # the streaming kernel's walk rows: R = 2 workgroups x 256 CUs
        up = 2 if row[1] == "up2" else 1
        units = E.streaming_units(variants, row[0], row[2], up * row[5], up * row[6], up * row[7], row[4])
        assert E.variant_row_id(row) in E.WALK_VARIANT_IDS and units == 1040 and units >= 2 * 512 + 1 and units % 512 and units % 256
    for row in E.BORDER_ROWS:
        up = 2 if row[1] == "up2" else 1
        assert (E.border_layer(variants, row[0], row[2], up * row[6], up * row[7], row[4]) >= 4 * E.LAUNCH_CUS) == row[8] and up * row[5] == 4
