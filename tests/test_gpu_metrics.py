"""GPU (MI355X): the validation metrics (csrc/metrics.hip through dropin.Evaluator and the metric modules) against the definition
restated in tests/metrics_cases.py and the values of the reference's own classes in tests/golden/metrics.npz.

Bars.  rmse, mae, bad and n: within 1 ulp of float64 of the restatement after the final division or root -- both sides hold the sums
of the same fp32 addends rounded once (the restatement exactly, by math.fsum; the kernel by compensated float64 accumulation, good to
~2^-100 before that rounding), so what is left is the last operation.  ssim: 1e-9 absolute -- 121-term float64 sums carry about 1.3e-14 relative error on moments of
up to (2 R)^2 (metrics_cases.SSIM_CONDITION), divided by c2 = 9e-4 R^2, over a few terms; an indexing error shows at 1e-4.
The pooled row against the golden (an fp32 evaluation): the host test's bar, 4 |restate(fp32) - restate(float64)| + 4 fp32 ulp."""
import os

import numpy as np
import pytest
import torch

import guard_arena
import metrics_cases as MC
from mvs_gi_amd import dropin, hip_ops as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RED = [0, 1, 2, 4, 5, 6, 8]          # the reduction columns and n
SSIM = [3, 7]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor allocated during a test of this module (inputs, the evaluator's workspace and table) sits between
    NaN-sentinel guards and starts out as NaN (tests/guard_arena.py)."""
    yield from guard_arena.fixture_body(request)


_RESTATED = {}


def _case(name):
    """inputs and restatements of a case, computed once for the module"""
    if name not in _RESTATED:
        inp = MC.make_inputs(name)
        args = (inp["preds"], inp["target"], inp["mask"], inp["label_range"])
        _RESTATED[name] = dict(inp=inp, frame=MC.restate(*args, scope="frame"), batch=MC.restate(*args, scope="batch"))
    return _RESTATED[name]


def _evaluator(**kw):
    return dropin.Evaluator(bf=MC.BF, dist_list=MC.DIST_LIST, delta_thresh=MC.THRESH, delta_thresh_dist=MC.THRESH_DIST, **kw)


def _poisoned(B):
    return torch.empty((B + 1, 9), dtype=torch.float64, device=DEV).fill_(float("nan"))


def _run(ev, inp, scope="frame", **kw):
    d = lambda t: None if t is None else t.to(DEV)
    B = inp["preds"].shape[0]
    out = ev.evaluate(d(inp["preds"]), d(inp["target"]), valid_mask=d(inp.get("mask")), label_range=inp.get("label_range"),
                      out=_poisoned(B), range_scope=scope, **kw)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _within_ulps(got, ref, n=1):
    same_nan = np.isnan(got) == np.isnan(ref)
    with np.errstate(invalid="ignore"):
        close = np.abs(got - ref) <= n * np.spacing(np.abs(ref))
    return same_nan & (close | np.isnan(ref))


@pytest.mark.parametrize("scope", ["frame", "batch"])
@pytest.mark.parametrize("name", list(MC.CASES))
def test_every_case_against_the_restatement(name, scope):
    c = _case(name)
    got, ref = _run(_evaluator(), c["inp"], scope), c[scope]
    with np.errstate(invalid="ignore"):
        ulps = np.abs(got[:, RED] - ref[:, RED]) / np.spacing(np.abs(ref[:, RED]))
        print(f"{name} [{scope}] reduction columns: largest distance {np.nanmax(ulps) if not np.isnan(ulps).all() else 0:.2f} ulp; "
              f"ssim: largest distance {np.nanmax(np.abs(got[:, SSIM] - ref[:, SSIM])) if not np.isnan(ref[:, SSIM]).all() else 0:.3e}")
    assert _within_ulps(got[:, RED], ref[:, RED]).all(), (got[:, RED], ref[:, RED])
    assert np.array_equal(np.isnan(got[:, SSIM]), np.isnan(ref[:, SSIM]))
    ok = np.isnan(ref[:, SSIM]) | (np.abs(got[:, SSIM] - ref[:, SSIM]) <= 1e-9)
    assert ok.all(), (got[:, SSIM], ref[:, SSIM])
    B, Hh, W, _ = MC.CASES[name]
    if Hh < 11 or W < 11:
        assert np.isnan(got[:, SSIM]).all() and not np.isnan(got[:, [0, 1, 4, 5]]).any()


def test_exact_operands_bit_for_bit():
    """bf = 64, clamp range [1, 64], every value a multiple of 1/8: the direct form's partial sums are exact in any order, so the
    table's reduction columns are the restatement's bits; the distance form's sums are rounded once on both sides."""
    x = MC.exact_inputs()
    ev = dropin.Evaluator(bf=x["bf"], dist_list=x["dist_list"], delta_thresh=0.25, delta_thresh_dist=0.002)
    assert (ev.clamp_min, ev.clamp_max) == (1.0, 64.0)
    for mask in (x["mask"], None):
        inp = dict(preds=x["preds"], target=x["target"], mask=mask)
        got = _run(ev, inp)
        ref = MC.restate(x["preds"], x["target"], mask, None, bf=x["bf"], cmin=1.0, cmax=64.0, thresh=0.25, thresh_dist=0.002)
        assert 0 < ref[0, 2] < 1 and 0 < ref[0, 6] < 1          # both thresholds bite
        assert np.array_equal(_bits(got[:, RED]), _bits(ref[:, RED])), (got[:, RED], ref[:, RED])


def test_mask_tensor_and_label_range_give_the_same_bits():
    inp = _case("odd")["inp"]
    ev = _evaluator()
    a = _run(ev, inp)
    b = _run(ev, dict(preds=inp["preds"], target=inp["target"], mask=MC.validity(inp)))
    c = _run(ev, dict(preds=inp["preds"], target=inp["target"], mask=MC.validity(inp).to(torch.uint8)))
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    assert 0 < a[-1, 8] < inp["preds"].numel()
    # the evaluator's own default range (Evaluator.from_regressor sets the regressor's) is the same evaluation
    reg = dropin.DistanceRegressorWithFixedCandidates(bf=MC.BF, dist_cands=MC.DIST_LIST)
    ev2 = dropin.Evaluator.from_regressor(reg, delta_thresh=MC.THRESH, delta_thresh_dist=MC.THRESH_DIST)
    assert ev2.label_range == (reg.inv_dist_idx_min, reg.inv_dist_idx_max) and (ev2.clamp_min, ev2.clamp_max) == (ev.clamp_min, ev.clamp_max)
    d = ev2.evaluate(inp["preds"].to(DEV), inp["target"].to(DEV)).cpu().numpy()
    e = _run(ev, dict(preds=inp["preds"], target=inp["target"], label_range=ev2.label_range))
    assert np.array_equal(_bits(d), _bits(e))


def test_nan_prediction_at_an_invalid_pixel_changes_no_reduction_column():
    inp = dict(_case("row_tail")["inp"])
    ev = _evaluator()
    clean = _run(ev, inp)
    preds = inp["preds"].clone()
    invalid = (~inp["mask"]).nonzero()
    assert len(invalid) > 20
    for i in invalid[::7]:
        preds[tuple(i)] = float("nan")
    dirty = _run(ev, dict(inp, preds=preds))
    assert np.array_equal(_bits(clean[:, RED]), _bits(dirty[:, RED]))
    assert np.isnan(dirty[:, SSIM]).all()          # the SSIM does not use the mask


def test_two_runs_give_the_same_bits():
    for name in ("operating", "masked_frames"):
        inp = _case(name)["inp"]
        a, b = _run(_evaluator(), inp), _run(_evaluator(), inp)
        assert np.array_equal(_bits(a), _bits(b))
        ev = _evaluator()
        c, d = _run(ev, inp), _run(ev, inp)                   # and with a workspace that has been used
        assert np.array_equal(_bits(a), _bits(c)) and np.array_equal(_bits(c), _bits(d))


def test_frame_of_a_batch_equals_the_one_frame_call():
    inp = _case("masked_frames")["inp"]
    ev = _evaluator()
    full = _run(ev, inp)
    for b in range(inp["preds"].shape[0]):
        one = _run(ev, {k: (v[b:b + 1].clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
        assert np.array_equal(_bits(one[0]), _bits(full[b])), b
        assert np.array_equal(_bits(one[1][[3, 7]]), _bits(full[b][[3, 7]]))        # one frame: the pooled SSIM is the frame's
    # frame 1 has no valid pixel: NaN, NaN, 1.0 in both forms; frame 2 counts every pixel
    assert np.isnan(full[1, [0, 1, 4, 5]]).all() and (full[1, [2, 6]] == 1.0).all() and full[1, 8] == 0
    assert full[2, 8] == 33 * 67


def test_no_valid_pixel_at_all():
    inp = dict(_case("row_tail")["inp"])
    inp["mask"] = torch.zeros_like(inp["mask"])
    got = _run(_evaluator(), inp)
    assert np.isnan(got[:, [0, 1, 4, 5]]).all() and (got[:, [2, 6]] == 1.0).all() and (got[:, 8] == 0).all()
    assert not np.isnan(got[:, SSIM]).any()


@pytest.mark.parametrize("name", list(MC.CASES))
def test_pooled_row_against_the_reference_golden(name):
    c = _case(name)
    inp = c["inp"]
    gold = np.load(GOLDEN)[f"{name}/pooled"]
    r32 = MC.restate(inp["preds"], inp["target"], inp["mask"], inp["label_range"], scope="batch", dtype=torch.float32)[-1, :8]
    bar = 4 * np.abs(r32 - c["batch"][-1, :8]) + 4 * np.spacing(np.abs(gold)).astype(np.float64)
    got = _run(_evaluator(), inp, "batch")[-1, :8]
    dist = np.abs(got - gold.astype(np.float64))
    print(f"{name}: |table - golden| / bar = {dist / bar}")
    assert np.array_equal(np.isnan(got), np.isnan(gold))
    assert (np.isnan(gold) | (dist <= bar)).all(), (got, gold, bar)


def test_captured_evaluation_replays_to_the_eager_bits():
    """evaluate() on static inputs inside torch.cuda.graph: a synchronisation would end the capture with an error; the allocator's
    counters show that nothing was allocated inside."""
    inp = _case("tile_plus_one")["inp"]
    B, _, Hh, W = inp["preds"].shape
    sp, st = inp["preds"].to(DEV), inp["target"].to(DEV)
    sm = inp["mask"].to(DEV)
    ev = _evaluator()
    ev.evaluate(sp, st, valid_mask=sm)                       # first use: the evaluator's workspace and table
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]      # (beginning a capture allocates on its own)
        table = ev.evaluate(sp, st, valid_mask=sm)
        inside = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    assert inside == before, "evaluate() allocated device memory"
    g = torch.Generator().manual_seed(3)
    for k in range(2):
        p = inp["preds"] * (1.0 + 0.1 * k) + 0.01 * torch.randn(inp["preds"].shape, generator=g)
        m = torch.rand(inp["mask"].shape, generator=g) < 0.5
        sp.copy_(p.to(DEV)), sm.copy_(m.to(DEV))
        table.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(_evaluator(), dict(preds=p, target=inp["target"], mask=m))
        assert np.array_equal(_bits(table.cpu().numpy()), _bits(eager)), k


def test_modules_return_the_table_and_share_one_evaluation():
    inp = _case("odd")["inp"]
    p, t, m = inp["preds"].to(DEV), inp["target"].to(DEV), MC.validity(inp).to(DEV)
    # the six metrics of configs/base_model.yaml, and the bad-pixel ratio in both forms: separately built, same parameters
    mk = lambda C, **kw: C(bf=96, dist_list=MC.DIST_LIST, **kw)
    mods = dict(ssim=mk(dropin.SSIMMetric), rmse=mk(dropin.RMSEMetric), mae=mk(dropin.MAEMetric),
                mae_dist=dropin.InverseMetricWrapper(mk(dropin.MAEMetric)), rmse_dist=dropin.InverseMetricWrapper(mk(dropin.RMSEMetric)),
                ssim_dist=dropin.InverseMetricWrapper(mk(dropin.SSIMMetric)))
    extra = dict(bad=mk(dropin.BadPixelRatioMetric), bad_dist=dropin.InverseMetricWrapper(mk(dropin.BadPixelRatioMetric)))
    for with_mask in (True, False):
        vm = m if with_mask else None
        ref = dropin.Evaluator(bf=96, dist_list=MC.DIST_LIST, range_scope="batch").evaluate(p, t, valid_mask=vm, label_range=None)
        ref = ref[-1].to(torch.float32).cpu()
        p = p.clone()                                            # new tensors: a new evaluation
        n0 = H.METRICS_EVALUATIONS
        got = {k: mod(p, t, vm) for k, mod in mods.items()}
        assert H.METRICS_EVALUATIONS == n0 + 1, "six modules on the same tensors: one evaluation"
        got.update({k: mod(p, t, vm) for k, mod in extra.items()})
        assert H.METRICS_EVALUATIONS == n0 + 1
        for k, v in got.items():
            assert v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda
            assert np.array_equal(v.cpu().numpy().view(np.int32), ref[H.METRICS_COLUMNS.index(k)].numpy().view(np.int32)), k
        p.mul_(1.01)                                             # written in place: _version moves, evaluated again
        mods["rmse"](p, t, vm)
        assert H.METRICS_EVALUATIONS == n0 + 2
    # an evaluator of one's own, shared explicitly: its thresholds hold
    ev = _evaluator()
    own = [mk(dropin.BadPixelRatioMetric).use_evaluator(ev), dropin.InverseMetricWrapper(mk(dropin.BadPixelRatioMetric).use_evaluator(ev)),
           mk(dropin.RMSEMetric).use_evaluator(ev)]
    n0 = H.METRICS_EVALUATIONS
    vals = [float(o(p, t, m)) for o in own]
    assert H.METRICS_EVALUATIONS == n0 + 1
    ref = _evaluator(range_scope="batch").evaluate(p, t, valid_mask=m)[-1].to(torch.float32).cpu()
    assert vals == [float(ref[2]), float(ref[6]), float(ref[0])] and 0 < vals[0] < 1


def test_freed_and_reallocated_inputs_are_evaluated_again():
    """One frame per step, as the reference validates: each step's tensors are freed before the next step's are made, so the
    allocator hands out the same blocks again (same address, same shape, _version 0).  Every step must be a new evaluation with
    that step's values."""
    inp = _case("odd")["inp"]
    mods = [dropin.RMSEMetric(bf=96, dist_list=MC.DIST_LIST), dropin.InverseMetricWrapper(dropin.MAEMetric(bf=96, dist_list=MC.DIST_LIST))]
    ev = dropin.Evaluator(bf=96, dist_list=MC.DIST_LIST, range_scope="batch")
    seen, ptrs = [], []
    for b in range(3):
        p, t = inp["preds"][b:b + 1].to(DEV), inp["target"][b:b + 1].to(DEV)
        assert p._version == 0 and t._version == 0
        ptrs.append((p.data_ptr(), t.data_ptr()))
        n0 = H.METRICS_EVALUATIONS
        got = [float(m(p, t)) for m in mods]
        assert H.METRICS_EVALUATIONS == n0 + 1, "two modules, one step: one evaluation"
        ref = ev.evaluate(p, t, label_range=None)[-1].to(torch.float32).cpu()
        assert got == [float(ref[0]), float(ref[5])], b
        seen.append(got)
        del p, t
    assert len({tuple(g) for g in seen}) == 3
    assert ptrs[1] != ptrs[0], "the remembered tensors are held: their blocks are not handed to the next step's"
