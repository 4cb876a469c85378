"""CPU: the validation metrics' definition (tests/metrics_cases.restate) against values of the reference's own classes
(tests/golden/metrics.npz, tools/make_metrics_goldens.py), the drop-in classes' constructors / buffers / pickling / aliases against
the reference's, and the C ABI's argument validation and workspace size.

Bars of test_restatement_matches_reference_goldens.  The golden is an fp32 evaluation (the reference's classes over an fp32
stand-in for torchmetrics), the restatement float64 with exactly rounded sums (math.fsum): the golden is the noisy side.  Its noise is
estimated by the restatement itself recomputed in fp32 (fp32 sums, fp32 final division / root, fp32 SSIM): per case, row and
metric
    bar = 4 * |restate(fp32) - restate(float64)| + 4 ulp_fp32(golden)
Measured (largest over the table): rmse / mae bars up to 8.3e-9 with |golden - restatement| at most 0.16 of the bar; ssim bars up
to 8.7e-7 (direct form) and 6.3e-5 (distance form, whose c2 is small against the moments) with the distance at most 0.83 of the
bar; the bad-pixel ratios differ by at most 1 fp32 ulp (a count divided in fp32)."""
import ctypes
import hashlib
import importlib
import inspect
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import metrics_cases as MC
from mvs_gi_amd import _lib, dropin, hip_ops as H
from mvs_gi_amd.dropin import metrics as DM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
CLASSES = ("MVSMetric", "SSIMMetric", "RMSEMetric", "MAEMetric", "BadPixelRatioMetric", "InverseMetricWrapper")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _digest(inp):
    h = hashlib.sha256()
    for k in ("preds", "target", "mask"):
        if inp[k] is not None:
            h.update(inp[k].numpy().tobytes())
    return h.hexdigest()


def _params(fn):
    return [[k, None if q.default is q.empty else repr(q.default)] for k, q in inspect.signature(fn).parameters.items()]


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_restatement_matches_reference_goldens(name, golden):
    B, Hh, W, _ = MC.CASES[name]
    inp = MC.make_inputs(name)
    assert _digest(inp) == str(golden[f"{name}/sha256"]), "the seeded inputs are not the ones the golden was made from"
    if name in MC.STORED_INPUTS:
        assert np.array_equal(inp["preds"].numpy(), golden[f"{name}/preds"])
        assert np.array_equal(inp["target"].numpy(), golden[f"{name}/target"])
        if inp["mask"] is not None:
            assert np.array_equal(np.packbits(inp["mask"].numpy()), golden[f"{name}/mask"])
    worst = MC.check_condition(inp["preds"], inp["target"])
    print(f"{name}: max(|P|, |T|) / R = {worst:.3f}")
    args = (inp["preds"], inp["target"], inp["mask"], inp["label_range"])
    for scope, rows, gold in (("frame", slice(0, B), golden[f"{name}/frames"]), ("batch", slice(B, B + 1), golden[f"{name}/pooled"][None])):
        r64 = MC.restate(*args, scope=scope)[rows, :8]
        r32 = MC.restate(*args, scope=scope, dtype=torch.float32)[rows, :8]
        gold = gold.astype(np.float64)
        bar = 4 * np.abs(r32 - r64) + 4 * _ulp32(gold)
        dist = np.abs(gold - r64)
        for c, col in enumerate(MC.COLUMNS[:8]):
            print(f"{name} [{scope}] {col:10s} |golden - restatement| {np.nanmax(dist[:, c]) if not np.isnan(dist[:, c]).all() else float('nan'):.3e}"
                  f"  bar {np.nanmax(bar[:, c]) if not np.isnan(bar[:, c]).all() else float('nan'):.3e}")
        both_nan = np.isnan(gold) & np.isnan(r64)
        assert np.array_equal(np.isnan(gold), np.isnan(r64)), (name, scope)
        assert np.all((dist <= bar) | both_nan), (name, scope, dist, bar)
    if Hh < 11 or W < 11:
        assert np.isnan(MC.restate(*args)[:, [3, 7]]).all()


def test_classes_match_the_reference(golden):
    facts = json.loads(str(golden["class_facts"]))
    assert DM.DEFAULT_BF == facts["DEFAULT_BF"] and DM.DEFAULT_DIST_LIST == facts["DEFAULT_DIST_LIST"]
    for cls in CLASSES:
        C = getattr(dropin, cls)
        obj = C(dropin.RMSEMetric()) if cls == "InverseMetricWrapper" else C()
        f = facts[cls]
        assert _params(C.__init__) == f["signature"], cls
        assert _params(C.forward) == f["forward"], cls
        assert sorted(k for k, _ in obj.named_buffers()) == f["buffers"], cls
        assert sorted(obj.state_dict()) == f["state_dict"], cls
        for k, b in obj.named_buffers():
            assert b.dtype == torch.float32 and b.dim() == 0 and float(b) == f["buffer_values"][k], (cls, k)
    m = dropin.BadPixelRatioMetric(bf=64, dist_list=[1, 2, 4], delta_thresh=0.25)
    assert (m.bf, m.delta_thresh, float(m.clamp_min), float(m.clamp_max)) == (64, 0.25, 16.0, 64.0)
    with pytest.raises(NotImplementedError):
        dropin.MVSMetric()(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2))


def test_pickle_round_trip_drops_the_evaluator():
    ev = dropin.Evaluator(bf=64, dist_list=[1, 2, 4])
    w = dropin.InverseMetricWrapper(dropin.BadPixelRatioMetric(bf=64, dist_list=[1, 2, 4], delta_thresh=0.2).use_evaluator(ev))
    w2 = pickle.loads(pickle.dumps(w))
    assert type(w2) is dropin.InverseMetricWrapper and type(w2.metric) is dropin.BadPixelRatioMetric
    assert (w2.metric.bf, w2.metric.delta_thresh) == (64, 0.2)
    assert float(w2.metric.clamp_min) == 16.0 and float(w2.metric.clamp_max) == 64.0
    assert "_mvsgi_evaluator" not in w2.metric.__dict__ and w.metric.__dict__["_mvsgi_evaluator"] is ev
    assert list(w2.state_dict()) == []


def test_install_aliases_resolve_the_metric_classes():
    names = ("dsta_mvs.support", "dsta_mvs.support.loss_function", "dsta_mvs.support.loss_function.metrics")
    ref_path = "dsta_mvs.support.loss_function.metrics"
    assert not any(n in sys.modules for n in names)
    assert dropin.install("alias") == "alias"
    try:
        lf = importlib.import_module("dsta_mvs.support.loss_function")
        assert lf.RMSEMetric is dropin.RMSEMetric
        for cls in CLASSES:
            assert getattr(lf, cls) is getattr(dropin, cls)
            assert getattr(importlib.import_module(ref_path), cls) is getattr(dropin, cls)
        # an object pickled under the reference's import path, as its checkpoints hold them
        old = dropin.MAEMetric.__module__
        dropin.MAEMetric.__module__ = ref_path
        try:
            blob = pickle.dumps(dropin.MAEMetric(bf=48))
        finally:
            dropin.MAEMetric.__module__ = old
        assert ref_path.encode() in blob and b"mvs_gi_amd" not in blob
        back = pickle.loads(blob)
        assert type(back) is dropin.MAEMetric and back.bf == 48 and float(back.clamp_max) == 96.0
    finally:
        dropin.uninstall()
    for n in names:
        assert n not in sys.modules
    with pytest.raises(ModuleNotFoundError):
        pickle.loads(blob)


def test_cpu_tensors_raise():
    p, t = torch.ones(1, 1, 12, 12), torch.ones(1, 1, 12, 12)
    for m in (dropin.RMSEMetric(), dropin.SSIMMetric(), dropin.InverseMetricWrapper(dropin.MAEMetric())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(p, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dropin.Evaluator().evaluate(p, t)


def test_argument_validation_rejects_before_any_launch(lib):
    P = ctypes.c_void_p
    good = dict(preds=P(64), target=P(128), mask=None, kind=0, lo=0.0, hi=0.0, bf=96.0, cmin=0.96, cmax=192.0, th=0.1, thd=0.1, scope=0,
                ws=P(256), ws_bytes=1 << 20, out=P(512), B=1, H=16, W=16)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mvsgi_metrics_f32(a["preds"], a["target"], a["mask"], a["kind"], a["lo"], a["hi"], a["bf"], a["cmin"], a["cmax"],
                                     a["th"], a["thd"], a["scope"], a["ws"], a["ws_bytes"], a["out"], a["B"], a["H"], a["W"], None)
    for kw, msg in ((dict(preds=None), b"null pointer"), (dict(target=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(out=None), b"null pointer"), (dict(kind=1), b"null pointer"), (dict(B=0), b"non-positive"),
                    (dict(H=0), b"non-positive"), (dict(kind=3), b"mask_kind"), (dict(kind=-1), b"mask_kind"),
                    (dict(kind=2, lo=2.0, hi=1.0), b"lo = "), (dict(kind=2, lo=float("nan"), hi=1.0), b"lo = "),
                    (dict(scope=2), b"range_scope"), (dict(bf=0.0), b"bf"), (dict(B=70000), b"launch geometry"),
                    (dict(ws_bytes=lib.mvsgi_metrics_ws_bytes(1, 16, 16) - 8), b"too small"),
                    (dict(preds=P(68)), b"16-byte aligned"), (dict(kind=1, mask=P(6)), b"4-byte aligned")):
        assert call(**kw) != 0, kw
        assert msg in lib.mvsgi_last_error(), (kw, lib.mvsgi_last_error())


@pytest.mark.parametrize("B,Hh,W", [(1, 11, 11), (1, 10, 40), (2, 27, 43), (3, 37, 130), (128, 160, 640), (1, 264, 1000), (1, 64, 64)])
def test_workspace_bytes_match_the_slab_layout(lib, B, Hh, W):
    lay = H.metrics_ws_layout(B, Hh, W)
    assert lib.mvsgi_metrics_ws_bytes(B, Hh, W) == 8 * lay["total"]
    G = min(max(-(-Hh * W // 4096), 1), 64)
    T = -(-(Hh - 10) // MC.SSIM_TILE[0]) * -(-(W - 10) // MC.SSIM_TILE[1]) if min(Hh, W) >= 11 else 0
    assert (lay["G"], lay["T"]) == (G, T)
    assert lay["total"] == B * G * 20 + B * 20 + B * 4 + 2 * B * T
    assert lay["records"] < lay["frame_sums"] < lay["consts"] < lay["tiles"] <= lay["total"]
    assert lib.mvsgi_metrics_ws_bytes(0, Hh, W) == 0 and lib.mvsgi_metrics_ws_bytes(B, 0, W) == 0


def test_patch_mode_rebinds_the_reference_metric_classes(tmp_path):
    """With a user's checkout importable, install() rebinds forward of its metric classes (and leaves the rest patched where the
    metrics module does not import: test_dropin_host's stand-in has none)."""
    from test_dropin_host import _run, _write_reference_stand_in
    _write_reference_stand_in(tmp_path)
    pkg = tmp_path / "dsta_mvs" / "support" / "loss_function"
    pkg.mkdir(parents=True)
    (tmp_path / "dsta_mvs" / "support" / "__init__.py").touch()
    (pkg / "__init__.py").write_text("from .metrics import *\n")
    (pkg / "metrics.py").write_text(
        "import torch\n"
        "class MVSMetric(torch.nn.Module):\n"
        "    def __init__(self, bf=96, dist_list=(1, 2)):\n"
        "        super().__init__()\n"
        "        self.bf = bf\n"
        "        self.register_buffer('clamp_min', torch.tensor(48.0), persistent=False)\n"
        "        self.register_buffer('clamp_max', torch.tensor(96.0), persistent=False)\n"
        "    def forward(self, preds, target, valid_mask=None):\n"
        "        return 'reference'\n"
        + "".join(f"class {n}(MVSMetric):\n    pass\n" for n in ("SSIMMetric", "RMSEMetric", "MAEMetric", "BadPixelRatioMetric"))
        + "class InverseMetricWrapper(torch.nn.Module):\n"
          "    def __init__(self, metric):\n"
          "        super().__init__()\n"
          "        self.metric = metric\n"
          "    def forward(self, preds, target, valid_mask=None):\n"
          "        return 'reference'\n")
    out = _run("""
        import torch, mvs_gi_amd
        from dsta_mvs.support.loss_function import RMSEMetric, SSIMMetric, InverseMetricWrapper
        x = torch.ones(1, 1, 12, 12)
        mods = [RMSEMetric(), InverseMetricWrapper(SSIMMetric())]
        assert [m(x, x) for m in mods] == ["reference"] * 2
        assert mvs_gi_amd.install() == "patch"
        for m in mods:
            try:
                m(x, x)
            except RuntimeError as e:
                assert "no CPU fallback" in str(e)
            else:
                raise SystemExit("the reference's forward still runs")
        from mvs_gi_amd.dropin.install import uninstall
        uninstall()
        assert [m(x, x) for m in mods] == ["reference"] * 2
        print("OK")
    """, [str(tmp_path)])
    assert "OK" in out


def test_evaluator_construction_and_shared_registry():
    import gc
    reg = dropin.DistanceRegressorWithFixedCandidates(bf=96, dist_cands=MC.DIST_LIST)
    ev = dropin.Evaluator.from_regressor(reg, delta_thresh=0.2)
    plain = dropin.Evaluator(bf=96, dist_list=MC.DIST_LIST)
    assert (ev.clamp_min, ev.clamp_max) == (plain.clamp_min, plain.clamp_max) == MC.clamp_range()
    assert ev.label_range == (reg.inv_dist_idx_min, reg.inv_dist_idx_max) and plain.label_range is None
    assert (ev.delta_thresh, ev.delta_thresh_dist, ev.range_scope) == (0.2, 0.2, "frame")
    assert dropin.Evaluator(bf=64, clamp_min=1.0, clamp_max=64.0).clamp_max == 64.0
    with pytest.raises(ValueError, match="both or neither"):
        dropin.Evaluator(clamp_min=1.0)
    with pytest.raises(ValueError, match="range_scope"):
        dropin.Evaluator(range_scope="image")
    # separately built modules with the same parameters resolve to one evaluator; it goes when they go
    a, b, c = dropin.RMSEMetric(), dropin.InverseMetricWrapper(dropin.SSIMMetric()), dropin.BadPixelRatioMetric(delta_thresh=0.3)
    ea, eb, ec = DM._resolve_evaluator(a, "rmse", False), DM._resolve_evaluator(b.metric, "ssim", True), DM._resolve_evaluator(c, "bad", False)
    assert ea is eb and ec is not ea and (ec.delta_thresh, ec.delta_thresh_dist) == (0.3, 0.1) and ea.range_scope == "batch"
    assert DM._resolve_evaluator(a, "rmse", False) is ea
    n = len(DM._EVALUATORS)
    del a, b, c, ea, eb, ec
    gc.collect()
    assert len(DM._EVALUATORS) == n - 2
    ev.release()
    assert ev._bufs == {} and ev._last is None
