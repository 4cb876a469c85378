#!/usr/bin/env python3
"""Golden values for the loss functions, produced by the REFERENCE's own classes (dsta_mvs/support/loss_function/distance_loss.py on
the norm_costs and inv_dist of dsta_mvs/model/distance_regressor/distance_regressor.py) on the CPU, for every case of
tests/losses_cases.py.

  python tools/make_losses_goldens.py [REFERENCE_CHECKOUT]      ->  tests/golden/losses.npz

Both files are imported by path (they import torch alone; the package __init__ of loss_function pulls in torchmetrics).  Per case:
the reference's VolumeCrossEntropy on its own regressor's norm_costs (mask as the case selects; a pixel mask repeated over D, as
NearFocusDistanceLoss does), MaskedSmoothL1Loss and InBoundsBCEDistanceLoss on the case's pred -- three fp32 scalars -- a digest of
the inputs, and for the small cases the inputs themselves and the reference's two-hot true_cost (recomputed from its buffers by its own
lines, forward does not return it).  Also stored: the constructors' signatures and buffers of the reference's classes.
Prints, per case, the relative distance of the reference's scalars from tests/losses_cases.restate on the same probabilities."""
import hashlib
import importlib.util
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_by_path(ref, name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digest(inp):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(inp["costs"]).tobytes())
    for k in ("labels", "pred", "vol_mask", "px_mask"):
        if inp[k] is not None:
            h.update(inp[k].numpy().tobytes())
    return h.hexdigest()


def params(fn):          # [name, repr(default) or None]: annotations print differently under postponed evaluation
    return [[k, None if q.default is q.empty else repr(q.default)] for k, q in inspect.signature(fn).parameters.items()]


def main():
    import losses_cases as LC
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MVSGI_REFERENCE", os.path.join(ROOT, "..", "reference"))
    L = load_by_path(ref, "dsta_mvs_ref_distance_loss", "dsta_mvs", "support", "loss_function", "distance_loss.py")
    R = load_by_path(ref, "dsta_mvs_ref_distance_regressor", "dsta_mvs", "model", "distance_regressor", "distance_regressor.py")
    out = {}
    for name, (B, D, H, W, s, kind) in LC.CASES.items():
        inp = LC.make_inputs(name)
        dl = LC.dist_list(D)
        reg = R.DistanceRegressorWithFixedCandidates(bf=LC.BF, dist_cands=dl, interp_scale_factor=s if s != 1 else 0, pre_interp=s != 1)
        _, norm_costs = reg(torch.from_numpy(inp["costs"]).unsqueeze(1))
        vce = L.VolumeCrossEntropy(bf=LC.BF, dist_list=dl)
        assert torch.equal(vce.inv_dist_list, inp["inv_list"])
        vm = inp["vol_mask"]
        if vm is not None and vm.shape[1] == 1:
            vm = vm.repeat(1, D, 1, 1)
        vol = vce(norm_costs, inp["labels"], vm)
        pm = LC.px_selection(inp)
        sl1 = L.MaskedSmoothL1Loss(reg)(inp["pred"], inp["labels"], pm)
        inb = L.InBoundsBCEDistanceLoss(reg, far_dist_threshold=LC.FAR_DIST, near_dist_threshold=LC.NEAR_DIST)(inp["pred"], inp["labels"], pm)
        got = np.array([float(vol), float(sl1), float(inb)], np.float32)
        out[f"{name}/pooled"] = got
        out[f"{name}/sha256"] = np.array(digest(inp))
        table, t = LC.restate_case(inp, norm_costs.numpy())
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(got.astype(np.float64) - table[-1, :3]) / np.abs(table[-1, :3])
        print(f"{name:16s} reference {got}  |reference - restatement| / restatement = {rel}")
        if name in LC.STORED_INPUTS:
            out[f"{name}/costs"] = inp["costs"]
            out[f"{name}/labels"], out[f"{name}/pred"] = inp["labels"].numpy(), inp["pred"].numpy()
            for k in ("vol_mask", "px_mask"):
                if inp[k] is not None:
                    out[f"{name}/{k}"] = np.packbits(inp[k].numpy())
            # the reference's label stage, its own lines on its own buffers (distance_loss.py:22-41)
            x = torch.clamp(inp["labels"], vce.inv_dist_list[-1], vce.inv_dist_list[0])
            bin_idx = len(vce.inv_dist_list) - torch.bucketize(x, vce.inv_dist_list_flipped)
            bin_idx = torch.clamp(bin_idx - 1, min=0, max=len(vce.inv_dist_list) - 2).to(torch.long)
            flat = bin_idx.flatten()
            d = (x - vce.inv_dist_list[flat].view_as(bin_idx)) / vce.bin_widths[flat].view_as(bin_idx)
            tc = torch.zeros_like(norm_costs)
            tc.scatter_(1, bin_idx, 1 - d)
            tc.scatter_(1, bin_idx + 1, d)
            out[f"{name}/true_cost"] = tc.numpy()
            assert np.array_equal(tc.numpy(), t.numpy())
    facts = {}
    reg = R.DistanceRegressorWithFixedCandidates()
    objs = dict(VolumeCrossEntropy=L.VolumeCrossEntropy(), MaskedSmoothL1Loss=L.MaskedSmoothL1Loss(reg),
                InBoundsBCEDistanceLoss=L.InBoundsBCEDistanceLoss(reg, 100.0, 0.5))
    objs["NearFocusDistanceLoss"] = L.NearFocusDistanceLoss(L.VolumeCrossEntropy(), L.VolumeCrossEntropy(), 2.0, (0.7, 0.3), [1, 2, 3])
    for cls, obj in objs.items():
        C = getattr(L, cls)
        facts[cls] = dict(signature=params(C.__init__), forward=params(C.forward), buffers=sorted(k for k, _ in obj.named_buffers()),
                          state_dict=sorted(obj.state_dict()),
                          attrs={k: v for k, v in vars(obj).items() if isinstance(v, (int, float)) and not k.startswith("_") and k != "training"})
    out["class_facts"] = np.array(json.dumps(facts, sort_keys=True))
    path = os.path.join(ROOT, "tests", "golden", "losses.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
