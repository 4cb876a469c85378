"""CPU: the loss functions' definition (tests/losses_cases.restate) against values of the reference's own classes
(tests/golden/losses.npz, tools/make_losses_goldens.py), the conditions under which the GPU test's bars are derived, the drop-in
classes' constructors / buffers / pickling / aliases, and the C ABI's argument validation and workspace size.

Bar of test_restatement_matches_reference_goldens: 1e-6 relative.  The golden is the reference's fp32 scalar (fp32 addends, an fp32
sum and mean), the restatement float64 on the same fp32 probabilities (ATen's softmax of the regressor, recomputed here); measured
over the committed cases the two lie within 1.2e-7 of each other (tools/make_losses_goldens.py prints the distances; an fp32 scalar
alone carries 6e-8), a margin of about 8."""
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

import losses_cases as LC
import softargmin_cases as SC
from mvs_gi_amd import _lib, dropin, hip_ops as H
from mvs_gi_amd.dropin import losses as DL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz")
CLASSES = ("VolumeCrossEntropy", "MaskedSmoothL1Loss", "InBoundsBCEDistanceLoss", "NearFocusDistanceLoss")
REF_PKG = "dsta_mvs.support.loss_function"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _digest(inp):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(inp["costs"]).tobytes())
    for k in ("labels", "pred", "vol_mask", "px_mask"):
        if inp[k] is not None:
            h.update(inp[k].numpy().tobytes())
    return h.hexdigest()


def _params(fn):
    return [[k, None if q.default is q.empty else repr(q.default)] for k, q in inspect.signature(fn).parameters.items()]


@pytest.mark.parametrize("name", list(LC.CASES))
def test_restatement_matches_reference_goldens(name, golden):
    inp = LC.make_inputs(name)
    assert _digest(inp) == str(golden[f"{name}/sha256"]), "the seeded inputs are not the ones the golden was made from"
    if name in LC.STORED_INPUTS:
        assert np.array_equal(inp["costs"], golden[f"{name}/costs"])
        assert np.array_equal(inp["labels"].numpy(), golden[f"{name}/labels"]) and np.array_equal(inp["pred"].numpy(), golden[f"{name}/pred"])
        for k in ("vol_mask", "px_mask"):
            if inp[k] is not None:
                assert np.array_equal(np.packbits(inp[k].numpy()), golden[f"{name}/{k}"])
    _, p32 = SC.aten32(inp["costs"], inp["inv_idx"], inp["scale"])
    table, _ = LC.restate_case(inp, p32)
    gold = golden[f"{name}/pooled"].astype(np.float64)
    dist = np.abs(gold - table[-1, :3])
    print(f"{name}: reference {gold}, restatement {table[-1, :3]}, relative distance {dist / np.abs(table[-1, :3]).clip(min=1e-300)}")
    assert np.isfinite(gold).all() and (dist <= 1e-6 * np.abs(table[-1, :3])).all(), (gold, table[-1])


@pytest.mark.parametrize("name", LC.STORED_INPUTS)
def test_true_cost_of_the_restatement_is_the_references(name, golden):
    inp = LC.make_inputs(name)
    t = LC.true_cost(inp["labels"], inp["inv_list"]).numpy()
    want = golden[f"{name}/true_cost"]
    assert t.dtype == want.dtype == np.float32 and np.array_equal(t.view(np.int32), want.view(np.int32))
    # two-hot: at most two non-zeros per pixel, adjacent, in [0, 1], summing to 1 within an ulp
    assert ((t != 0).sum(1) <= 2).all() and (t >= 0).all() and (t <= 1).all() and np.abs(t.sum(1) - 1).max() <= 2.0 ** -23
    # the planted labels: a candidate exactly is a one-hot at that candidate (the last candidate: weight 1 on the upper end of the last bin)
    D = t.shape[1]
    if t.shape[2] * t.shape[3] >= D:
        flat = t.reshape(t.shape[0], D, -1)
        for d in range(D):
            assert flat[0, d, d] == 1.0 and flat[0, :, d].sum() == 1.0, d


@pytest.mark.parametrize("name", list(LC.CASES))
def test_conditions_of_the_bars(name):
    inp = LC.make_inputs(name)
    r = inp["r"]
    _, p32 = SC.aten32(inp["costs"], inp["inv_idx"], inp["scale"])
    lo32, hi32 = LC.check_conditions(p32)
    lo64, hi64 = LC.check_conditions(r.p)
    table, t = LC.restate_case(inp, r.p)
    bar = LC.fused_bar(r, t.numpy(), r.p, inp["vol_mask"])
    ok = ~np.isnan(table[:, 0])
    print(f"{name}: p in [{min(lo32, lo64):.3e}, {max(hi32, hi64):.4f}], fused bar / loss {np.max(bar[ok] / table[ok, 0]):.3e}")
    assert np.array_equal(np.isnan(bar), np.isnan(table[:, 0])) and (bar[ok] <= 1e-4 * table[ok, 0]).all(), (bar, table[:, 0])
    quad, lin = LC.branches(inp)
    if name != "tiny":                     # one pixel has one branch
        assert quad > 0 and lin > 0, (quad, lin)
    # the selections select: neither everything nor nothing
    if inp["vol_mask"] is not None:
        assert 0 < table[-1, 3] < t.numel()
    if LC.px_selection(inp) is not None:
        assert 0 < table[-1, 4] < inp["labels"].numel()
    if name == "frames":
        assert np.isnan(table[1, :3]).all() and table[1, 3] == 0 and table[1, 4] == 0 and table[2, 4] == 9 * 17
        assert not np.isnan(table[[0, 2, 3, 4, 5], :3]).any()


def test_exact_regime_has_both_clamps():
    for shape in ((2, 16, 7, 13), (1, 33, 6, 10)):
        for s in (1, 2, 4):
            c, _ = LC.exact_inputs(shape, s)
            assert (c.want_p == 0).any() and (c.want_p == 1).any()


def test_classes_match_the_reference(golden):
    facts = json.loads(str(golden["class_facts"]))
    reg = dropin.DistanceRegressorWithFixedCandidates()
    objs = dict(VolumeCrossEntropy=dropin.VolumeCrossEntropy(), MaskedSmoothL1Loss=dropin.MaskedSmoothL1Loss(reg),
                InBoundsBCEDistanceLoss=dropin.InBoundsBCEDistanceLoss(reg, 100.0, 0.5))
    objs["NearFocusDistanceLoss"] = dropin.NearFocusDistanceLoss(dropin.VolumeCrossEntropy(), dropin.VolumeCrossEntropy(), 2.0, (0.7, 0.3),
                                                                 [1, 2, 3])
    for cls in CLASSES:
        C, obj, f = getattr(dropin, cls), objs[cls], facts[cls]
        assert _params(C.__init__) == f["signature"], cls
        assert _params(C.forward) == f["forward"], cls
        assert sorted(k for k, _ in obj.named_buffers()) == f["buffers"], cls
        assert sorted(obj.state_dict()) == f["state_dict"], cls
        for k, v in f["attrs"].items():
            assert getattr(obj, k) == v, (cls, k)
    v = dropin.VolumeCrossEntropy(bf=64, dist_list=[1, 2, 4])
    assert v.inv_dist_list.tolist() == [64.0, 32.0, 16.0] and v.inv_dist_list_flipped.tolist() == [16.0, 32.0, 64.0]
    assert v.bin_widths.tolist() == [-32.0, -16.0] and list(v.state_dict()) == []


def test_pickle_round_trip_drops_the_evaluator():
    v = dropin.VolumeCrossEntropy(bf=64, dist_list=[1, 2, 4])
    s = dropin.MaskedSmoothL1Loss(dropin.DistanceRegressorWithFixedCandidates())
    DL._own_evaluator(v, lambda: dropin.LossEvaluator(inv_dist_idx=v.inv_dist_list))
    DL._own_evaluator(s, DL._image_evaluator)
    assert "_mvsgi_evaluator" in v.__dict__ and "_mvsgi_evaluator" in s.__dict__
    v2, s2 = pickle.loads(pickle.dumps(v)), pickle.loads(pickle.dumps(s))
    assert type(v2) is dropin.VolumeCrossEntropy and type(s2) is dropin.MaskedSmoothL1Loss
    assert not any(k.startswith("_mvsgi_") for k in v2.__dict__) and not any(k.startswith("_mvsgi_") for k in s2.__dict__)
    assert v2.inv_dist_list.tolist() == [64.0, 32.0, 16.0] and type(s2.dist_regressor) is dropin.DistanceRegressorWithFixedCandidates


def test_install_aliases_resolve_the_loss_classes():
    leaf = REF_PKG + ".distance_loss"
    assert REF_PKG not in sys.modules and leaf not in sys.modules
    assert dropin.install("alias") == "alias"
    try:
        lf = importlib.import_module(REF_PKG)
        dl = importlib.import_module(leaf)
        for cls in CLASSES:
            assert getattr(lf, cls) is getattr(dropin, cls) and getattr(dl, cls) is getattr(dropin, cls)
            # the class paths of configs/base_model.yaml and configs/loss/*.yaml, as hydra / jsonargparse resolve them
            mod, _, attr = f"{REF_PKG}.{cls}".rpartition(".")
            assert getattr(importlib.import_module(mod), attr) is getattr(dropin, cls)
        assert lf.RMSEMetric is dropin.RMSEMetric            # the metrics stay
        blobs = []
        for C, args in ((dropin.VolumeCrossEntropy, dict(bf=48)), (dropin.MaskedSmoothL1Loss, dict(dist_regressor=None))):
            old = C.__module__
            C.__module__ = leaf
            try:
                obj = C(**args)
                obj.__dict__["_mvsgi_evaluator"] = "derived"
                blobs.append(pickle.dumps(obj))
            finally:
                C.__module__ = old
            assert leaf.encode() in blobs[-1] and b"_mvsgi_" not in blobs[-1]
            back = pickle.loads(blobs[-1])
            assert type(back) is C and "_mvsgi_evaluator" not in back.__dict__
        assert float(pickle.loads(blobs[0]).inv_dist_list[0]) == 96.0
    finally:
        dropin.uninstall()
    assert REF_PKG not in sys.modules and leaf not in sys.modules
    with pytest.raises(ModuleNotFoundError):
        pickle.loads(blobs[0])


def test_patch_mode_rebinds_the_reference_loss_classes(tmp_path):
    from test_dropin_host import _run, _write_reference_stand_in
    _write_reference_stand_in(tmp_path)
    pkg = tmp_path / "dsta_mvs" / "support" / "loss_function"
    pkg.mkdir(parents=True)
    (tmp_path / "dsta_mvs" / "support" / "__init__.py").touch()
    (pkg / "__init__.py").write_text("from .distance_loss import *\n")
    (pkg / "distance_loss.py").write_text(
        "import torch\n"
        + "".join(f"class {n}(torch.nn.Module):\n"
                  "    def __init__(self, *a, **k):\n"
                  "        super().__init__()\n"
                  "        self.register_buffer('inv_dist_list', 96 / torch.Tensor([1, 2, 4]), persistent=False)\n"
                  "        self.near_inv_dist_thresh, self.far_inv_dist_thresh = 2.0, 0.01\n"
                  "    def forward(self, *a, **k):\n"
                  "        return 'reference'\n" for n in CLASSES))
    out = _run("""
        import torch, mvs_gi_amd
        from dsta_mvs.support.loss_function import VolumeCrossEntropy, MaskedSmoothL1Loss, InBoundsBCEDistanceLoss
        x = torch.ones(1, 1, 4, 4)
        mods = [VolumeCrossEntropy(), MaskedSmoothL1Loss(), InBoundsBCEDistanceLoss()]
        assert [m(x, x) for m in mods] == ["reference"] * 3
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
        assert [m(x, x) for m in mods] == ["reference"] * 3
        print("OK")
    """, [str(tmp_path)])
    assert "OK" in out


def test_cpu_tensors_raise():
    x, v = torch.ones(1, 1, 4, 4), torch.full((1, 10, 4, 4), 0.1)
    reg = dropin.DistanceRegressorWithFixedCandidates()
    for call in (lambda: dropin.VolumeCrossEntropy()(v, x), lambda: dropin.MaskedSmoothL1Loss(reg)(x, x),
                 lambda: dropin.InBoundsBCEDistanceLoss(reg, 100.0, 0.5)(x, x), lambda: dropin.LossEvaluator().evaluate(x, pred=x),
                 lambda: dropin.NearFocusDistanceLoss(dropin.VolumeCrossEntropy(), dropin.VolumeCrossEntropy(), 2.0, (0.5, 0.5), list(range(10)))(v, x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_volume_inputs_of_the_distance_losses_raise():
    reg = dropin.DistanceRegressorWithFixedCandidates()
    v, x = torch.full((1, 10, 4, 4), 0.1), torch.ones(1, 1, 4, 4)
    for m in (dropin.MaskedSmoothL1Loss(reg), dropin.InBoundsBCEDistanceLoss(reg, 100.0, 0.5)):
        with pytest.raises(NotImplementedError, match="TypeError"):
            m(v, x)


@pytest.mark.parametrize("dl", [[1, 3, 2], [1, 1, 2], [0, 1, 2], [-1, 1, 2], [2], [2, 1], [1, float("inf")], [1, float("nan"), 3]])
def test_a_dist_list_without_bins_raises(dl):
    with pytest.raises(ValueError, match="dist_list"):
        dropin.LossEvaluator(dist_list=dl)
    v = dropin.VolumeCrossEntropy(dist_list=dl)          # the constructor accepts it, as the reference's does; forward refuses
    with pytest.raises(ValueError, match="dist_list"):
        v(torch.full((1, len(dl), 2, 2), 0.5), torch.ones(1, 1, 2, 2))


def test_evaluator_construction():
    reg = dropin.DistanceRegressorWithFixedCandidates(bf=96, dist_cands=LC.DEFAULT_DIST_LIST, interp_scale_factor=2, pre_interp=True)
    ev = dropin.LossEvaluator.from_regressor(reg, near_dist_threshold=0.5, far_dist_threshold=100.0, label_max=191)
    assert torch.equal(ev.inv_list, LC.inv_list(10)) and ev.scale == 2.0 and ev.bf == 96.0 and ev.label_max == 191.0
    assert ev.inbounds == (2.0, 0.01)
    assert dropin.LossEvaluator.from_regressor(dropin.DistanceRegressorWithFixedCandidates(interp_scale_factor=2)).scale == 1.0
    plain = dropin.LossEvaluator()
    assert torch.equal(plain.inv_list, ev.inv_list) and plain.inbounds is None and plain.label_max is None and plain.scale == 1.0
    with pytest.raises(ValueError, match="both or neither"):
        dropin.LossEvaluator(near_dist_threshold=1.0)
    assert H.LOSSES_COLUMNS == LC.COLUMNS


@pytest.mark.parametrize("B,OH,OW", [(1, 1, 1), (2, 14, 26), (1, 12, 20), (5, 9, 17), (64, 160, 640), (1, 264, 1000), (3, 256, 256), (1, 257, 256)])
def test_workspace_bytes_match_the_slab_layout(lib, B, OH, OW):
    lay = H.losses_ws_layout(B, OH, OW)
    assert lay == H.losses_ws_layout(B, OH, OW) and lib.mvsgi_losses_ws_bytes(B, OH, OW) == 8 * lay["total"]
    G = min(max(-(-OH * OW // 256), 1), 256)
    assert lay["G"] == G and lay["total"] == B * G * 8 + B * 8 and lay["records"] == 0 and lay["frame_sums"] == B * G * 8
    assert (OH * OW > LC.REDUCE_CAP_PIXELS) == (-(-OH * OW // 256) > 256)
    assert lib.mvsgi_losses_ws_bytes(0, OH, OW) == 0 and lib.mvsgi_losses_ws_bytes(B, 0, OW) == 0 and lib.mvsgi_losses_ws_bytes(70000, OH, OW) == 0


def test_argument_validation_rejects_before_any_launch(lib):
    P = ctypes.c_void_p
    good = dict(labels=P(64), pred=P(128), probs=P(256), p_kind=1, inv=P(512), vm=None, vk=0, pm=None, pk=0, hi=0.0, inb=0, near=0.0,
                far=0.0, tc=None, ws=P(1024), ws_bytes=1 << 20, out=P(2048), B=1, D=4, H=8, W=8, scale=2.0, OH=16, OW=16)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mvsgi_losses_f32(a["labels"], a["pred"], a["probs"], a["p_kind"], a["inv"], a["vm"], a["vk"], a["pm"], a["pk"], a["hi"],
                                    a["inb"], a["near"], a["far"], a["tc"], a["ws"], a["ws_bytes"], a["out"], a["B"], a["D"], a["H"], a["W"],
                                    a["scale"], a["OH"], a["OW"], None)
    for kw, msg in ((dict(labels=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(probs=None), b"null pointer"), (dict(inv=None), b"null pointer"), (dict(p_kind=0, tc=P(4096), inv=None), b"null pointer"),
                    (dict(vk=1), b"null pointer"), (dict(vk=2), b"null pointer"), (dict(pk=1), b"null pointer"),
                    (dict(D=1), b"at least two"), (dict(p_kind=2, D=1), b"at least two"), (dict(p_kind=0, tc=P(4096), D=0), b"at least two"),
                    (dict(p_kind=3), b"p_kind"), (dict(p_kind=-1), b"p_kind"), (dict(vk=3, vm=P(64)), b"vol_kind"), (dict(pk=3), b"px_kind"),
                    (dict(pk=2, hi=float("nan")), b"label_max"), (dict(B=0), b"non-positive"), (dict(OH=0), b"non-positive"),
                    (dict(B=70000), b"launch geometry"),
                    (dict(p_kind=2, OH=17), b"is not floor"), (dict(p_kind=2, OW=15), b"is not floor"), (dict(p_kind=2, scale=1.5), b"is not floor"),
                    (dict(p_kind=2, scale=0.0), b"scale"), (dict(p_kind=2, scale=float("nan")), b"scale"), (dict(p_kind=2, H=0), b"non-positive"),
                    (dict(ws_bytes=lib.mvsgi_losses_ws_bytes(1, 16, 16) - 8), b"too small"),
                    (dict(ws=P(1028)), b"8-byte aligned"), (dict(labels=P(66)), b"4-byte aligned")):
        assert call(**kw) != 0, kw
        assert msg in lib.mvsgi_last_error(), (kw, lib.mvsgi_last_error())
