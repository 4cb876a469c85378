"""GPU (MI355X): the out_costs tail on FP32 RECORDS.  The Winograd-form polyphase layer (K3w, csrc/conv3d_wino_up2.hip, OF32) writes
the 16 activated fp32 values of a voxel into the padded buffer where it used to write their fp16 (hi | lo) pair, and the cost head
(csrc/conv3d_headsplit.hip, X32) splits what it loads.  The head's operands are the split of the same fp32 values, so inside
+-65504 the costs are those of the pair path BIT FOR BIT: every comparison below is an equality, none a tolerance.  Out of range the
writer no longer clamps and the head's clamp engages (MVSGI_SAT_SPLIT raised by the reader, costs finite).

Every buffer of this module sits between NaN guards and every unwritten fp32 output reads as NaN (tests/guard_arena.py): a store
outside the interior fails the teardown, a load outside the buffer poisons the costs.

K3w needs D == 8, H even, W a multiple of 32 (low resolution).  Shapes (B, D, H, W): one unit per role; several units, two frames,
every H and W face; the largest of the existing Winograd-form test (more units than workgroups: a workgroup prefetches a next unit).
The head alone also runs on a ragged window (H = 9, W = 33, D = 3), on one and on two channel slices."""
import numpy as np
import pytest
import torch

from golden_cases import SMALL_CASES
import guard_arena
from mvs_gi_amd import hip_ops as H, synth
from mvs_gi_amd.pipeline import HotPath
import test_gpu_parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_WINO_FORM_SHAPES = next(m for m in P.test_conv3d_up2_polyphase_winograd_form_vs_interpolate_then_conv.pytestmark
                         if m.name == "parametrize").args[1]
SMALLEST = [(1, 8, 2, 32), (2, 8, 4, 64)]
SHAPES = SMALLEST + [max(_WINO_FORM_SHAPES, key=lambda s: s[0] * s[2] * s[3])]


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    yield from guard_arena.fixture_body(request)


@pytest.fixture(autouse=True)
def _clean_report():
    mode, policy = H.get_conv_mode(), H.get_range_check()
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    H.set_conv_mode(mode)
    H.set_range_check(policy)
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)


def _flags() -> int:
    torch.cuda.synchronize()
    return H.saturation_flags(clear=True)


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _layer(shape, x=None, wt=None, scale=None):
    """Operands of the polyphase layer (the random ones of the existing Winograd-form test) and of a cost head behind it."""
    B, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 19)
    xr = rng.standard_normal((B, d, h, w, 32), dtype=np.float32)
    wr = (rng.standard_normal((16, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32)
    sc, sh = P._bn(rng, 16)
    wh = (rng.standard_normal((1, 16, 3, 3, 3)) / np.sqrt(27 * 16)).astype(np.float32)
    xs = H.act_to_split(_g(xr) if x is None else x, fmt="f16")
    plan, un = H.conv3d_up2_poly_plan(_g(wr if wt is None else wt), d, h, w, fmt="f16")
    hw, hun = H.pack_head_split_weights_f16(_g(wh))
    return xs, plan, (_g(sc) if scale is None else scale) * un, _g(sh), hw, hun


def _buf(shape, rec):
    B, d, h, w = shape
    s = H.SplitAct(B, 2 * d, 2 * h, 2 * w, 16, DEV)
    s.rec = rec
    return s


def _interior(s):
    """The records of a buffer of fp32 records as an fp32 tensor [B, D, H, W, C] (a view)."""
    assert s.rec == "f32"
    return s.buf.view(torch.float32)[:, 1:-1, 1:-1, 1:-1]


def _border_is_zero(s) -> bool:
    b = s.buf.clone()
    b[:, 1:-1, 1:-1, 1:-1] = 0
    return int(b.abs().max()) == 0


def _to_rec32(x):
    """fp32 [B, D, H, W, C] -> a padded buffer of fp32 records (zero border), as the Winograd-form layer writes it."""
    B, d, h, w, c = x.shape
    s = H.SplitAct(B, d, h, w, c, x.device)
    s.buf.view(torch.float32)[:, 1:-1, 1:-1, 1:-1] = x
    s.fmt, s.rec = "f16", "f32"
    return s


@pytest.mark.parametrize("shape", SHAPES)
def test_k3w_fp32_records_and_head_reproduce_the_pair_path_bit_for_bit(shape):
    """(K3w fp32 out -> head fp32 in) == (K3w split out -> head split in) on the same input buffer, in-range random operands: the
    records are the values whose split the pair path stores, the costs are equal, the border stays zero, no flag."""
    xs, plan, sc, sh, hw, hun = _layer(shape)
    pairs = H.conv3d_up2_poly_split(xs, plan, sc, sh, out=_buf(shape, "pairs"), neg_slope=0.01, wino=True)
    recs = H.conv3d_up2_poly_split(xs, plan, sc, sh, out=_buf(shape, "f32"), neg_slope=0.01, wino=True)
    assert recs.fmt == "f16" and recs.rec == "f32" and pairs.rec == "pairs"
    assert _border_is_zero(recs)
    y = _interior(recs)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) < 65504.0
    assert torch.equal(H.act_to_split(y.contiguous(), fmt="f16").buf, pairs.buf)
    want = H.conv3d_head_split(pairs, hw, hun, 0.37, f16=True)
    got = H.conv3d_head_split(recs, hw, hun, 0.37, f16=True)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert _flags() == 0
    # a second call over its own output (the face corrections overwrite the records first): the same bits
    again = H.conv3d_up2_poly_split(xs, plan, sc, sh, out=recs, neg_slope=0.01, wino=True)
    assert torch.equal(H.act_to_split(_interior(again).contiguous(), fmt="f16").buf, pairs.buf)


@pytest.mark.parametrize("shape", [(2, 16, 3, 9, 33), (1, 32, 4, 9, 33), (1, 16, 1, 1, 1), (3, 16, 16, 8, 64)])
def test_head_on_fp32_records_equals_head_on_their_split(shape):
    """The head alone: ragged windows (H = 9, W = 33), one and two channel slices, a single voxel, a chunked march -- costs from fp32
    records equal those from the fp16 pairs of the same tensor; values beyond +-65504 included (act_to_split clamps them to the
    same number the head's own clamp gives), and then the flag is the reader's."""
    B, cin, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + 5)
    x = _g(rng.standard_normal((B, d, h, w, cin), dtype=np.float32) * 40.0)
    hw, hun = H.pack_head_split_weights_f16(_g((rng.standard_normal((1, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32)))
    want = H.conv3d_head_split(H.act_to_split(x, fmt="f16"), hw, hun, -0.2, f16=True)
    assert _flags() == 0
    got = H.conv3d_head_split(_to_rec32(x), hw, hun, -0.2, f16=True)
    assert _flags() == 0
    assert tuple(got.shape) == (B, d, h, w, 1) and bool(torch.isfinite(got).all()) and torch.equal(got, want)
    x.view(-1)[::7] = 7.0e4
    x.view(-1)[3::11] = -3.0e38
    want = H.conv3d_head_split(H.act_to_split(x, fmt="f16"), hw, hun, -0.2, f16=True)
    assert _flags() == H.SAT_SPLIT
    got = H.conv3d_head_split(_to_rec32(x), hw, hun, -0.2, f16=True)
    assert _flags() == H.SAT_SPLIT
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    with pytest.raises(AssertionError, match="fp16 split only"):
        r = _to_rec32(x)
        r.fmt = "bf16"
        H.conv3d_head_split(r, hw, hun, -0.2)


def test_out_of_range_tail_saturates_in_the_head_and_reports():
    """An output beyond 65504: the fp32-record writer stores it unclamped and raises nothing for it, the head's input clamp engages
    (exactly +-65504, MVSGI_SAT_SPLIT) and the costs are finite.  First with in-range transformed planes (only the reader can raise
    the flag), then the constant 6e4 volume of tests/test_gpu_range.py (the writer's transformed sums leave the range as well)."""
    shape = (2, 8, 4, 32)
    centre = _g(P_centre(16, 32))
    ones_h = _g(np.full((1, 16, 3, 3, 3), 1.0 / 432, np.float32))
    hw, hun = H.pack_head_split_weights_f16(ones_h)
    plan, un = H.conv3d_up2_poly_plan(centre, 8, 4, 32, "f16")
    zeros = torch.zeros(16, device=DEV)
    xs = H.act_to_split(torch.full((2, 8, 4, 32, 32), 100.0, device=DEV), fmt="f16")
    for s, want in ((100.0, 0), (700.0, H.SAT_SPLIT), (-7.0e6, H.SAT_SPLIT)):
        recs = H.conv3d_up2_poly_split(xs, plan, un * s, zeros, _buf(shape, "f32"), neg_slope=1.0, wino=True)
        assert _flags() == 0, s                                    # the writer neither clamps nor reports its output
        y = _interior(recs)
        assert abs(float(y.abs().max()) - 100.0 * abs(s)) <= 1e-4 * 100.0 * abs(s)
        costs = H.conv3d_head_split(recs, hw, hun, 0.0, f16=True)
        assert _flags() == want, s
        assert bool(torch.isfinite(costs).all())
        # the mean of 27 x 16 equal inputs (zero padding: fewer at the faces), each clamped to exactly +-65504
        bound = min(100.0 * abs(s), 65504.0)
        assert abs(float(costs.abs().max()) - bound) <= 1e-4 * bound, (s, float(costs.abs().max()))
    xs = H.act_to_split(torch.full((2, 8, 4, 32, 32), 6.0e4, device=DEV), fmt="f16")
    assert _flags() == 0
    recs = H.conv3d_up2_poly_split(xs, plan, un * 8.0, zeros, _buf(shape, "f32"), neg_slope=1.0, wino=True)
    assert _flags() == H.SAT_SPLIT                                 # x1 + x2 = 1.2e5 saturates in the conversion of V
    assert float(_interior(recs).abs().max()) > 65504.0            # the output itself left the range, unclamped
    costs = H.conv3d_head_split(recs, hw, hun, 0.0, f16=True)
    assert _flags() == H.SAT_SPLIT
    assert bool(torch.isfinite(costs).all()) and float(costs.abs().max()) <= 65504.0 * (1 + 1e-4)


def P_centre(cout, cin, value=1.0):
    """[cout, cin, 3, 3, 3] weights whose centre tap copies channel co % cin (tests/test_gpu_range.py::_centre)."""
    w = np.zeros((cout, cin, 3, 3, 3), np.float32)
    for co in range(cout):
        w[co, co % cin, 1, 1, 1] = value
    return w


@pytest.mark.parametrize("shape", SMALLEST)
def test_new_entry_points_on_guarded_arenas(shape, _guarded_allocations):
    """Address safety of mvsgi_conv3d_up2_poly_rec32 and mvsgi_conv3d_head_rec32_f16: inputs, plan, weights, record buffer and costs
    in arenas of their own between NaN guards, the costs poisoned.  Every interior record is written, the border is not, nothing
    outside the buffers is (snapshots of the whole arenas of the inputs are unchanged; the guards are compared at teardown), and no
    poisoned byte reaches the costs."""
    ga = _guarded_allocations
    assert ga is not None and ga.n_guarded == 0
    B, d, h, w = shape
    xs, plan, sc, sh, hw, hun = _layer(shape)
    plan, hw, sc, sh = ga.guarded(plan), ga.guarded(hw), ga.guarded(sc), ga.guarded(sh)
    snaps = [(t, ga.snapshot(t)) for t in (xs.buf, plan, hw, sc, sh)]
    recs = _buf(shape, "f32")
    _interior(recs).fill_(float("nan"))                            # no corrections, no results yet: every record must be written
    H.conv3d_up2_poly_split(xs, plan, sc, sh, out=recs, neg_slope=0.01, wino=True)
    assert _border_is_zero(recs) and bool(torch.isfinite(_interior(recs)).all())
    rsnap = ga.snapshot(recs.buf)
    costs = H.conv3d_head_split(recs, hw, hun, 0.37, f16=True)
    assert tuple(costs.shape) == (B, 2 * d, 2 * h, 2 * w, 1) and bool(torch.isfinite(costs).all())
    assert ga.unchanged(recs.buf, rsnap) and all(ga.unchanged(t, s) for t, s in snaps)
    assert ga.n_guarded >= 8 and _flags() == 0


def test_fp32_records_are_asked_for_only_where_the_winograd_form_writes_them():
    """H.conv3d_up2_poly_split refuses fp32 records from the direct kernel and from the bf16 split (no quiet fall-back), the C entry
    point refuses a geometry the Winograd form does not take, and a reader of pairs refuses a buffer of records."""
    shape = (1, 8, 2, 32)
    xs, plan, sc, sh, hw, hun = _layer(shape)
    with pytest.raises(AssertionError, match="Winograd form"):
        H.conv3d_up2_poly_split(xs, plan, sc, sh, out=_buf(shape, "f32"), direct=True)
    with pytest.raises(AssertionError, match="Winograd form"):
        H.conv3d_up2_poly_split(H.act_to_split(H.act_from_split(xs)), plan, sc, sh, out=_buf(shape, "f32"))
    odd = (1, 3, 5, 7)
    xo = H.act_to_split(torch.zeros((1, 3, 5, 7, 32), device=DEV), fmt="f16")
    plan_o, _ = H.conv3d_up2_poly_plan(torch.zeros((16, 32, 3, 3, 3), device=DEV), 3, 5, 7, fmt="f16")
    with pytest.raises(RuntimeError, match="Winograd form needs"):
        H.conv3d_up2_poly_split(xo, plan_o, sc, sh, out=_buf(odd, "f32"))
    recs = H.conv3d_up2_poly_split(xs, plan, sc, sh, out=_buf(shape, "f32"))
    with pytest.raises(AssertionError, match="fp32 records"):
        H.act_from_split(recs)


def test_switch_keeps_the_pair_path_and_the_default_meets_the_golden(golden_dir):
    """MVSGI_TAIL_F32 (cost_volume_regulator._TAIL_F32).  On a volume whose tail runs the Winograd form (3 frames of [16, 8, 64]: six
    units per role) the regulator's costs with the switch off -- the pair path, as before fp32 records existed -- and with the
    default are equal bit for bit, and the hand-over buffer holds what the switch says.  On the small golden (std_d16_rand, whose tail
    is too small for the Winograd form: pairs either way) both settings meet the golden at the fp16 split's bar."""
    from mvs_gi_amd.dropin import cost_volume_regulator as cr
    name = "std_d16_rand"
    case = SMALL_CASES[name]
    cfg, z = case["cfg"], P._load(golden_dir, name)
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"], grid_mask_dtype=case["grid_mask_dtype"])
    H.set_conv_mode("f16x3")
    old_tail, old_min = cr._TAIL_F32, cr._POLY_MIN_UNITS
    try:
        cr._POLY_MIN_UNITS = 0
        gain = case["gains"][0]
        hp = HotPath(cfg, synth.make_weights(cfg, seed=case["seed"], gain=gain), inp, device=DEV)
        vol = _g(np.random.default_rng(7).standard_normal((3, 16, 16, 8, 64), dtype=np.float32))
        assert H.conv3d_up2_poly_wino_pays(3, 8, 4, 32)
        costs, inv = {}, {}
        for tail in (False, True):
            cr._TAIL_F32 = tail
            costs[tail] = hp.cv_regulator(vol).clone()
            bufs = hp.cv_regulator.__dict__["_mvsgi_poly_bufs"]
            hand = [b for k, b in bufs.items() if "hi" in k and b.shape == (3, 16, 8, 64, 16)]
            assert len(hand) == 1 and hand[0].rec == ("f32" if tail else "pairs") and hand[0].fmt == "f16"
            inv[tail] = hp(_g(inp["feats"]))[0].cpu().numpy()
            assert all(b.rec == "pairs" for b in hp.cv_regulator.__dict__["_mvsgi_poly_bufs"].values() if b is not hand[0])
        assert hp.check_range() == 0
        assert bool(torch.isfinite(costs[True]).all()) and torch.equal(costs[True], costs[False])
        ref = z[f"inv_dist_g{gain:g}"]
        assert np.array_equal(inv[True], inv[False])
        assert P._rel(inv[True], ref) <= 1e-4 and P._rel(inv[False], ref) <= 1e-4
    finally:
        cr._TAIL_F32, cr._POLY_MIN_UNITS = old_tail, old_min
