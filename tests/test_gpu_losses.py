"""GPU (MI355X): the loss functions (csrc/losses.hip through dropin.LossEvaluator and the loss modules) against the definition
restated in tests/losses_cases.py.  The bars and their derivations are in that module's text: smooth_l1, inbounds, n_vol and n_px
within 1 ulp of float64; vol on given probabilities within VOL_BAR = (U_LOG + 2) * 2^-23 relative; vol on the fused softmax within
fused_bar(), propagated per case from softargmin_cases.bounds."""
import numpy as np
import pytest
import torch

import guard_arena
import losses_cases as LC
import softargmin_cases as SC
from mvs_gi_amd import dropin, hip_ops as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOL, ULP_COLS = 0, [1, 2, 3, 4]


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor allocated during a test of this module (the evaluator's workspace and table, outputs) sits between
    NaN-sentinel guards and starts out as NaN (tests/guard_arena.py)."""
    yield from guard_arena.fixture_body(request)


_CASES = {}


def _case(name):
    """inputs, the reference's fp32 probabilities and both restatements of a case, computed once for the module"""
    if name not in _CASES:
        inp = LC.make_inputs(name)
        _, p32 = SC.aten32(inp["costs"], inp["inv_idx"], inp["scale"])
        given, t = LC.restate_case(inp, p32)
        fused, _ = LC.restate_case(inp, inp["r"].p)
        bar = LC.fused_bar(inp["r"], t.numpy(), inp["r"].p, inp["vol_mask"])
        _CASES[name] = dict(inp=inp, p32=p32, given=given, fused=fused, bar=bar, t=t.numpy())
    return _CASES[name]


def _evaluator(D, **kw):
    return dropin.LossEvaluator(bf=LC.BF, dist_list=LC.dist_list(D), near_dist_threshold=LC.NEAR_DIST, far_dist_threshold=LC.FAR_DIST, **kw)


def _poisoned(B):
    return torch.empty((B + 1, 5), dtype=torch.float64, device=DEV).fill_(float("nan"))


def _d(t):
    if t is None:
        return None
    return (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


def _run(inp, p=None, fused=False, ev=None, true_cost=None, **over):
    """One evaluation of a case's inputs: p given (an fp32 array), or fused on the case's costs, or neither."""
    D = len(inp["inv_list"])
    ev = ev or _evaluator(D)
    kw = dict(pred=_d(inp.get("pred")), vol_mask=_d(inp.get("vol_mask")), px_mask=_d(inp.get("px_mask")), label_max=inp.get("label_max"))
    kw.update(over)
    if p is not None:
        kw["norm_costs"] = _d(np.ascontiguousarray(p, np.float32))
    if fused:
        kw["costs"], kw["scale"] = _d(inp["costs"]), inp["scale"]
    out = ev.evaluate(_d(inp["labels"]), out=_poisoned(inp["labels"].shape[0]), true_cost=true_cost, **kw)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _within_ulps(got, ref, n=1):
    same_nan = np.isnan(got) == np.isnan(ref)
    with np.errstate(invalid="ignore"):
        close = np.abs(got - ref) <= n * np.spacing(np.abs(ref))
    return same_nan & (close | np.isnan(ref))


def _rel(got, ref):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isnan(ref), 0.0, np.abs(got - ref) / np.abs(ref))


def _check_given(tag, got, ref):
    rel = _rel(got[:, VOL], ref[:, VOL])
    with np.errstate(invalid="ignore"):
        ulps = np.abs(got[:, ULP_COLS] - ref[:, ULP_COLS]) / np.spacing(np.abs(ref[:, ULP_COLS]))
    print(f"{tag}: vol relative distance {rel.max():.3e} (bar {LC.VOL_BAR:.3e}); other columns {np.nanmax(ulps) if not np.isnan(ulps).all() else 0:.2f} ulp")
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    assert _within_ulps(got[:, ULP_COLS], ref[:, ULP_COLS]).all(), (got[:, ULP_COLS], ref[:, ULP_COLS])
    assert (rel <= LC.VOL_BAR).all(), (got[:, VOL], ref[:, VOL])


@pytest.mark.parametrize("name", list(LC.CASES))
def test_given_probabilities_against_the_restatement(name):
    c = _case(name)
    B, D, OH, OW = LC.out_shape(name)
    tc = torch.empty((B, D, OH, OW), dtype=torch.float32, device=DEV)
    got = _run(c["inp"], p=c["p32"], true_cost=tc)
    _check_given(name, got, c["given"])
    assert np.array_equal(tc.cpu().numpy().view(np.int32), c["t"].view(np.int32)), "true_cost"


@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("shape", [(2, 16, 7, 13), (1, 33, 6, 10)])
def test_exact_regime_fused_equals_given_bit_for_bit(shape, s):
    """One-hot costs at a dyadic factor: p is exactly fl32(1 / |T|) or +0, so the fused walk and the given walk see the same
    numbers; both -100 clamps engage (p = 0 under log, p = 1 under log1p)."""
    c, x = LC.exact_inputs(shape, s)
    assert (c.want_p == 0).any() and (c.want_p == 1).any()
    inp = dict(x, costs=c.costs, scale=s)
    given = _run(inp, p=c.want_p)
    fused = _run(inp, fused=True)
    assert np.array_equal(_bits(fused), _bits(given)), (fused, given)
    near, far = np.float32(1.0 / LC.NEAR_DIST), np.float32(1.0 / LC.FAR_DIST)
    ref, _ = LC.restate(x["labels"], x["inv_list"], p=c.want_p, pred=x["pred"], inbounds=(near, far))
    _check_given(f"exact {shape} x{s}", given, ref)
    assert ref[-1, VOL] > 1.0          # a -100 clamp weighs in


@pytest.mark.parametrize("name", list(LC.CASES))
def test_fused_softmax_against_the_float64_chain(name):
    c = _case(name)
    got = _run(c["inp"], fused=True)
    ref, bar = c["fused"], c["bar"]
    with np.errstate(invalid="ignore"):
        dist = np.abs(got[:, VOL] - ref[:, VOL])
    ok = ~np.isnan(ref[:, VOL])
    print(f"{name}: fused vol |table - float64 chain| {dist[ok].max():.3e}, bar {bar[ok].min():.3e} .. {bar[ok].max():.3e}, "
          f"distance / bar {np.max(dist[ok] / bar[ok]):.3f}")
    assert np.array_equal(np.isnan(got[:, VOL]), np.isnan(ref[:, VOL]))
    assert (dist[ok] <= bar[ok]).all(), (got[:, VOL], ref[:, VOL], bar)
    # the image columns and the counts do not depend on where p comes from
    assert _within_ulps(got[:, ULP_COLS], ref[:, ULP_COLS]).all()


@pytest.mark.parametrize("name", ["tiny", "d10_x2", "d33_x2", "frames"])
def test_volume_labels_bit_for_bit(name):
    c = _case(name)
    inp = c["inp"]
    got = H.volume_labels(_d(inp["labels"]), _d(inp["inv_list"])).cpu().numpy()
    assert np.array_equal(got.view(np.int32), c["t"].view(np.int32))
    ev = _evaluator(len(inp["inv_list"]))
    assert np.array_equal(ev.volume_labels(_d(inp["labels"])).cpu().numpy().view(np.int32), c["t"].view(np.int32))
    # every planted label, alone in a frame of its own
    lst = inp["inv_list"]
    pl = torch.tensor(LC.planted(lst.tolist()), dtype=torch.float32).reshape(-1, 1, 1, 1)
    got = H.volume_labels(pl.to(DEV), lst.to(DEV)).cpu().numpy()
    want = LC.true_cost(pl, lst).numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_selections_give_the_same_bits():
    c = _case("d16_x4")
    inp = c["inp"]
    D = len(inp["inv_list"])
    a = _run(inp, p=c["p32"])                                                        # a pixel mask for both
    b = _run(inp, p=c["p32"], vol_mask=_d(inp["vol_mask"].repeat(1, D, 1, 1)))      # the same mask as a volume mask
    u = _run(inp, p=c["p32"], vol_mask=_d(inp["vol_mask"].to(torch.uint8)), px_mask=_d(inp["px_mask"].to(torch.uint8)))
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(u))
    assert 0 < a[-1, 4] < inp["labels"].numel() and a[-1, 3] == D * a[-1, 4]
    c = _case("d10_x2")
    inp = c["inp"]
    a = _run(inp, fused=True)                                                        # label_max
    b = _run(inp, fused=True, label_max=None, px_mask=_d(inp["labels"] <= LC.LABEL_MAX))
    assert np.array_equal(_bits(a), _bits(b)) and 0 < a[-1, 4] < inp["labels"].numel()
    # the evaluator's own default label_max is the same evaluation
    e = _run(inp, fused=True, label_max=None, ev=_evaluator(10, label_max=LC.LABEL_MAX))
    assert np.array_equal(_bits(a), _bits(e))


@pytest.mark.parametrize("fused", [False, True])
def test_frame_of_a_batch_equals_the_one_frame_call(fused):
    c = _case("frames")
    inp = c["inp"]
    B = inp["labels"].shape[0]
    kw = dict(fused=True) if fused else dict(p=c["p32"])
    full = _run(inp, **kw)
    for b in range(B):
        one = {k: (v[b:b + 1].clone() if isinstance(v, torch.Tensor) and v.dim() == 4 else v) for k, v in inp.items()}
        one["costs"] = inp["costs"][b:b + 1]
        if not fused:
            kw = dict(p=c["p32"][b:b + 1])
        got = _run(one, **kw)
        assert np.array_equal(_bits(got[0]), _bits(full[b])), b
        assert np.array_equal(_bits(got[1]), _bits(got[0])), "B = 1: the pooled row is the frame's"
    # frame 1 selects nothing: NaN, counts 0; the pooled row skips it; frame 2 selects every pixel
    assert np.isnan(full[1, :3]).all() and full[1, 3] == 0 and full[1, 4] == 0
    assert not np.isnan(full[-1]).any() and full[-1, 4] == full[[0, 2, 3, 4], 4].sum()
    assert full[2, 4] == 9 * 17 and full[2, 3] == 8 * 9 * 17


def test_missing_inputs_are_nan_columns():
    c = _case("d10_x2")
    inp = c["inp"]
    no_pred = _run(inp, p=c["p32"], pred=None)
    assert np.isnan(no_pred[:, [1, 2]]).all() and not np.isnan(no_pred[:, [0, 3, 4]]).any()
    no_p = _run(inp)
    assert np.isnan(no_p[:, [0, 3]]).all() and not np.isnan(no_p[:, [1, 2, 4]]).any()
    no_inb = _run(inp, ev=dropin.LossEvaluator(bf=LC.BF, dist_list=LC.dist_list(10)))
    assert np.isnan(no_inb[:, 2]).all() and np.array_equal(_bits(no_inb[:, [1, 4]]), _bits(no_p[:, [1, 4]]))


def test_two_runs_give_the_same_bits():
    for name in ("operating", "frames"):
        c = _case(name)
        for kw in (dict(p=c["p32"]), dict(fused=True)):
            a, b = _run(c["inp"], **kw), _run(c["inp"], **kw)
            assert np.array_equal(_bits(a), _bits(b))
            ev = _evaluator(len(c["inp"]["inv_list"]))
            x, y = _run(c["inp"], ev=ev, **kw), _run(c["inp"], ev=ev, **kw)          # and with a workspace that has been used
            assert np.array_equal(_bits(a), _bits(x)) and np.array_equal(_bits(x), _bits(y))


def test_captured_evaluation_replays_to_the_eager_bits():
    """evaluate() on static inputs inside torch.cuda.graph: a synchronisation would end the capture with an error; the allocator's
    counters show that nothing was allocated inside."""
    c = _case("d16_x1.5")
    inp = c["inp"]
    B = inp["labels"].shape[0]
    sl, sp, sc, sm = _d(inp["labels"]), _d(inp["pred"]), _d(inp["costs"]), _d(inp["px_mask"])
    ev = _evaluator(16, scale=inp["scale"])
    table = _poisoned(B)
    ev.evaluate(sl, pred=sp, costs=sc, vol_mask=sm, px_mask=sm, out=table)      # first use: the evaluator's workspace and list
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]      # (beginning a capture allocates on its own)
        ev.evaluate(sl, pred=sp, costs=sc, vol_mask=sm, px_mask=sm, out=table)
        inside = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    assert inside == before, "evaluate() allocated device memory"
    g = torch.Generator().manual_seed(5)
    for k in range(2):
        costs = inp["costs"] * np.float32(1.0 + 0.25 * k) + np.float32(0.01 * (k + 1))
        pred = inp["pred"] + 0.05 * torch.randn(inp["pred"].shape, generator=g)
        m = torch.rand(inp["px_mask"].shape, generator=g) < 0.5
        sc.copy_(_d(costs)), sp.copy_(_d(pred)), sm.copy_(_d(m))
        table.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(dict(inp, costs=costs, pred=pred, px_mask=m, vol_mask=m), fused=True)
        assert np.array_equal(_bits(table.cpu().numpy()), _bits(eager)), k


def test_modules_return_the_table():
    c = _case("d10_x2")
    inp = c["inp"]
    lab, pred, p = _d(inp["labels"]), _d(inp["pred"]), _d(c["p32"])
    dl = LC.dist_list(10)
    reg = dropin.DistanceRegressorWithFixedCandidates(bf=LC.BF, dist_cands=dl)
    pm = _d(LC.px_selection(inp))
    vce = dropin.VolumeCrossEntropy(bf=LC.BF, dist_list=dl)
    sl1 = dropin.MaskedSmoothL1Loss(reg)
    inb = dropin.InBoundsBCEDistanceLoss(reg, far_dist_threshold=LC.FAR_DIST, near_dist_threshold=LC.NEAR_DIST)
    f32 = lambda v: np.float64(v).astype(np.float32)
    same = lambda t, v: t.dtype == torch.float32 and t.dim() == 0 and t.is_cuda and \
        np.array_equal(t.cpu().numpy().view(np.int32), f32(v).view(np.int32))
    for vm in (None, _d(inp["vol_mask"]), _d(inp["vol_mask"].repeat(1, 10, 1, 1))):
        table = _run(inp, p=c["p32"], vol_mask=vm, px_mask=None, label_max=None)
        assert same(vce(p, lab, vm), table[-1, 0])
    for mask in (None, pm, pm.repeat(1, 10, 1, 1)):                       # MaskedSmoothL1Loss reads channel 0 of its mask
        table = _run(inp, px_mask=None if mask is None else pm, label_max=None)
        assert same(sl1(pred, lab, mask), table[-1, 1])
    for mask in (None, pm):
        table = _run(inp, px_mask=mask, label_max=None)
        assert same(inb(pred, lab, mask), table[-1, 2]) and 0 < table[-1, 2] < 100
    for m in (sl1, inb):
        with pytest.raises(NotImplementedError):
            m(p, lab)
    # the golden of the reference's own classes, at the host test's bar
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz"))["d10_x2/pooled"]
    got = [float(vce(p, lab, _d(inp["vol_mask"].repeat(1, 10, 1, 1)))), float(sl1(pred, lab, pm)), float(inb(pred, lab, pm))]
    assert np.allclose(got, gold, rtol=1e-6, atol=0), (got, gold)


def test_near_focus_is_the_literal_composition():
    c = _case("d10_x2")
    inp = c["inp"]
    lab, p = _d(inp["labels"]), _d(c["p32"])
    dl = LC.dist_list(10)
    near_thresh, w = 0.02, (0.7, 0.3)                       # 1 / 0.02 = 50: labels on both sides
    far_mask = inp["labels"] < 1.0 / near_thresh
    assert 0.1 < float(far_mask.float().mean()) < 0.9
    nf = dropin.NearFocusDistanceLoss(dropin.VolumeCrossEntropy(LC.BF, dl), dropin.VolumeCrossEntropy(LC.BF, dl), near_thresh, w, dl)
    got = nf(p, lab)
    ev = _evaluator(10)
    far = ev.evaluate(lab, norm_costs=p, vol_mask=_d(far_mask))[-1, 0].to(torch.float32).clone()
    near = ev.evaluate(lab, norm_costs=p, vol_mask=_d(~far_mask))[-1, 0].to(torch.float32).clone()
    want = (w[0] * near) + (w[1] * far)
    assert got.dtype == torch.float32 and got.dim() == 0 and torch.equal(got, want) and float(near) != float(far)
    # a loss function of another kind gets the reference's repeated mask
    seen = []

    class Other(torch.nn.Module):
        def forward(self, pred_cost, inv_dist_true, mask=None):
            seen.append(tuple(mask.shape))
            return torch.zeros((), device=pred_cost.device)
    dropin.NearFocusDistanceLoss(Other(), Other(), near_thresh, w, dl)(p, lab)
    assert seen == [tuple(p.shape)] * 2


@pytest.mark.parametrize("name", ["d10_x2", "d16_x1.5"])
def test_evaluator_behind_a_regressor_that_stores_no_norm_costs(name):
    c = _case(name)
    inp = c["inp"]
    B, D, H, W, s, _ = LC.CASES[name]
    mk = lambda: dropin.DistanceRegressorWithFixedCandidates(bf=LC.BF, dist_cands=LC.dist_list(D), interp_scale_factor=s, pre_interp=True).to(DEV)
    lean, full = mk(), mk()
    lean.return_norm_costs = False
    costs5 = _d(inp["costs"]).unsqueeze(1)
    inv, none = lean(costs5)
    inv2, pr = full(costs5)
    assert none is None and pr is not None
    lab, vm = _d(inp["labels"]), _d(inp["vol_mask"])
    a = dropin.LossEvaluator.from_regressor(lean).evaluate(lab, pred=inv, costs=costs5, vol_mask=vm).cpu().numpy()
    b = dropin.LossEvaluator.from_regressor(full).evaluate(lab, pred=inv, norm_costs=pr, vol_mask=vm).cpu().numpy()
    dist = np.abs(a[:, VOL] - b[:, VOL])
    print(f"{name}: |fused - stored norm_costs| {dist.max():.3e}, bar {c['bar'].min():.3e}")
    assert (dist <= c["bar"]).all() and np.array_equal(_bits(a[:, [1, 3, 4]]), _bits(b[:, [1, 3, 4]]))
    assert (np.abs(a[:, VOL] - c["fused"][:, VOL]) <= c["bar"]).all()


@pytest.mark.parametrize("shape,s", [((2, 5, 4, 15), 1), ((1, 17, 3, 19), 1), ((2, 16, 5, 13), 2), ((1, 33, 3, 13), 4), ((1, 5, 6, 10), 1.5)])
def test_address_safety_at_odd_widths(shape, s, _guarded_allocations):
    """Every input and output in an arena of its own with NaN-sentinel guards (the fixture checks them at teardown): OW = 15, 19, 26,
    52 and 15 again at a non-integer factor, optional outputs null."""
    ga = _guarded_allocations
    B, D, Hh, W = shape
    costs = SC.gauss_costs(shape, LC.SIGMA, seed=sum(shape))
    inv_idx = SC.stock_candidates(D)
    r = SC.ref64(costs, inv_idx, s)
    _, _, OH, OW = r.shape
    assert OW in (15, 19, 26, 52)
    _, p32 = SC.aten32(costs, inv_idx, s)
    lst = LC.inv_list(D)
    g = torch.Generator().manual_seed(sum(shape))
    pred = (torch.from_numpy(r.inv) + 0.3 * torch.randn(B, 1, OH, OW, generator=g, dtype=torch.float64)).to(torch.float32)
    labels = LC.make_labels((B, 1, OH, OW), lst.tolist(), pred, sum(shape) + 1)
    vm = torch.rand(B, D, OH, OW, generator=g) < 0.7
    pm = torch.rand(B, 1, OH, OW, generator=g) < 0.7
    near, far = np.float32(1.0 / LC.NEAR_DIST), np.float32(1.0 / LC.FAR_DIST)
    G = lambda t: ga.guarded((torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV))
    d_lab, d_pred, d_p, d_costs, d_vm, d_pm = G(labels), G(pred), G(p32), G(costs), G(vm), G(pm)
    ev = _evaluator(D, scale=s)
    ev._lists[torch.device(DEV)] = G(lst)
    tc = ga.alloc((B, D, OH, OW), torch.float32, DEV)
    table = ga.alloc((B + 1, 5), torch.float64, DEV)
    given = ev.evaluate(d_lab, pred=d_pred, norm_costs=d_p, vol_mask=d_vm, px_mask=d_pm, out=table, true_cost=tc).cpu().numpy()
    ref, t = LC.restate(labels, lst, p=p32, pred=pred, vol_mask=vm, px_mask=pm, inbounds=(near, far))
    _check_given(f"{shape} x{s}", given, ref)
    assert np.array_equal(tc.cpu().numpy().view(np.int32), t.numpy().view(np.int32))
    # null optional outputs and inputs: the poisoned true_cost of a second buffer stays poisoned, guards included
    tc2 = ga.alloc((B, D, OH, OW), torch.float32, DEV)
    snap = ga.snapshot(tc2)
    fused = ev.evaluate(d_lab, costs=d_costs, vol_mask=d_pm, out=table).cpu().numpy()
    assert ga.unchanged(tc2, snap) and bool(torch.isnan(tc2).all())
    ref64, t64 = LC.restate(labels, lst, p=r.p, vol_mask=pm, px_mask=None)
    bar = LC.fused_bar(r, t64.numpy(), r.p, pm)
    assert (np.abs(fused[:, VOL] - ref64[:, VOL]) <= bar).all() and np.isnan(fused[:, [1, 2]]).all()
    assert np.array_equal(fused[:, [3, 4]], ref64[:, [3, 4]])
