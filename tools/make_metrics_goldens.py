#!/usr/bin/env python3
"""Golden values for the validation metrics, produced by the REFERENCE's own classes
(dsta_mvs/support/loss_function/metrics.py) on the CPU, for every case of tests/metrics_cases.py: one frame per call (what
validation_step does) and once on the whole batch.

  python tools/make_metrics_goldens.py [REFERENCE_CHECKOUT]      ->  tests/golden/metrics.npz

The reference's file imports three functions of torchmetrics.functional; torchmetrics is not installed where this tool runs and
the reference pins no version of it.  The three functions below are OURS, a stand-in written from the package's published
definitions, in fp32 as the package computes:
  mean_squared_error(p, t, squared)   sum((p - t)^2) / numel, its root when squared=False
  mean_absolute_error(p, t)           sum(|p - t|) / numel
  structural_similarity_index_measure(p, t)   Gaussian 11 x 11, sigma 1.5, data_range = max(p.max() - p.min(), t.max() - t.min()),
                                      k1 0.01, k2 0.03, reflect padding of 5 that is cropped off again, mean over the batch of the
                                      per-image means
What the file pins is therefore the reference's own part -- clamp, scale, masking, the bad-pixel ratio, the inverse wrapper --
and not torchmetrics itself.  Also stored: the constructors' signatures, buffers and state_dict keys of the reference's classes,
the inputs of the small cases and a digest of the inputs of all of them.
"""
import hashlib
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("rmse", "mae", "bad", "ssim", "rmse_dist", "mae_dist", "bad_dist", "ssim_dist")


def mean_squared_error(preds, target, squared=True):
    d = preds - target
    mse = torch.sum(d * d) / target.numel()
    return mse if squared else torch.sqrt(mse)


def mean_absolute_error(preds, target):
    return torch.sum(torch.abs(preds - target)) / target.numel()


def structural_similarity_index_measure(preds, target):
    k = torch.arange(-5, 6, dtype=preds.dtype)
    g = torch.exp(-((k / 1.5) ** 2) / 2)
    g = (g / g.sum()).unsqueeze(0)
    kernel = (g.t() @ g).expand(preds.shape[1], 1, 11, 11)
    R = max(preds.max() - preds.min(), target.max() - target.min())
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    p, t = F.pad(preds, (5, 5, 5, 5), mode="reflect"), F.pad(target, (5, 5, 5, 5), mode="reflect")
    out = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel, groups=preds.shape[1])
    mu_p, mu_t, pp, tt, pt = out.split(preds.shape[0])
    s_p, s_t, s_pt = pp - mu_p * mu_p, tt - mu_t * mu_t, pt - mu_p * mu_t
    m = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_p + s_t + c2))
    m = m[..., 5:-5, 5:-5]
    return m.reshape(m.shape[0], -1).mean(-1).mean()


def load_reference(ref):
    tm = types.ModuleType("torchmetrics")
    tm.__path__ = []
    fn = types.ModuleType("torchmetrics.functional")
    fn.mean_squared_error, fn.mean_absolute_error = mean_squared_error, mean_absolute_error
    fn.structural_similarity_index_measure = structural_similarity_index_measure
    tm.functional = fn
    sys.modules["torchmetrics"], sys.modules["torchmetrics.functional"] = tm, fn
    spec = importlib.util.spec_from_file_location("dsta_mvs_ref_metrics", os.path.join(ref, "dsta_mvs", "support", "loss_function",
                                                                                       "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digest(inp):
    h = hashlib.sha256()
    for k in ("preds", "target", "mask"):
        if inp[k] is not None:
            h.update(inp[k].numpy().tobytes())
    return h.hexdigest()


def main():
    import metrics_cases as MC
    R = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MVSGI_REFERENCE", os.path.join(ROOT, "..", "reference")))
    base = dict(ssim=R.SSIMMetric, rmse=R.RMSEMetric, mae=R.MAEMetric, bad=R.BadPixelRatioMetric)
    metrics = {}
    for n in NAMES:
        kw = dict(delta_thresh=MC.THRESH_DIST if n.endswith("_dist") else MC.THRESH) if n.startswith("bad") else {}
        m = base[n.replace("_dist", "")](bf=MC.BF, dist_list=MC.DIST_LIST, **kw)
        metrics[n] = R.InverseMetricWrapper(m) if n.endswith("_dist") else m
    out = {}
    for name, (B, H, W, _) in MC.CASES.items():
        inp = MC.make_inputs(name)
        MC.check_condition(inp["preds"], inp["target"])
        v = MC.validity(inp)
        ssim_ok = H >= 11 and W >= 11      # below 11 the definition here is NaN, whatever the padded stand-in returns

        def call(n, sl):
            if n.startswith("ssim") and not ssim_ok:
                return float("nan")
            return float(metrics[n](inp["preds"][sl], inp["target"][sl], None if v is None else v[sl]))
        out[f"{name}/frames"] = np.array([[call(n, slice(b, b + 1)) for n in NAMES] for b in range(B)], np.float32)
        out[f"{name}/pooled"] = np.array([call(n, slice(None)) for n in NAMES], np.float32)
        out[f"{name}/sha256"] = np.array(digest(inp))
        if name in MC.STORED_INPUTS:
            out[f"{name}/preds"], out[f"{name}/target"] = inp["preds"].numpy(), inp["target"].numpy()
            if inp["mask"] is not None:
                out[f"{name}/mask"] = np.packbits(inp["mask"].numpy())
    facts = {}
    for cls in ("MVSMetric", "SSIMMetric", "RMSEMetric", "MAEMetric", "BadPixelRatioMetric", "InverseMetricWrapper"):
        C = getattr(R, cls)
        obj = C(R.RMSEMetric()) if cls == "InverseMetricWrapper" else C()
        def params(fn):          # [name, repr(default) or None]: annotations print differently under postponed evaluation
            return [[k, None if q.default is q.empty else repr(q.default)] for k, q in inspect.signature(fn).parameters.items()]
        facts[cls] = dict(signature=params(C.__init__), buffers=sorted(k for k, _ in obj.named_buffers()),
                          state_dict=sorted(obj.state_dict()),
                          buffer_values={k: float(b) for k, b in obj.named_buffers()},
                          forward=params(C.forward))
    facts["DEFAULT_BF"], facts["DEFAULT_DIST_LIST"] = R.DEFAULT_BF, R.DEFAULT_DIST_LIST
    out["class_facts"] = np.array(json.dumps(facts, sort_keys=True))
    path = os.path.join(ROOT, "tests", "golden", "metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
