#!/usr/bin/env python3
"""Generate tests/golden/extractor_args.npz and tests/golden/extractor_args_routes.npz by running the REFERENCE's own feature
extractors (imported from the reference checkout, as tools/make_topology_goldens.py does) built with the constructor arguments of
tests/extractor_cases.py, on that table's seeded images and weights.

The sphere classes call torchvision.ops.deform_conv2d, and torchvision is not installed: the project's restated operator
(oracle.mvsgi_oracle.deform_conv2d, which runs in float64 unchanged) stands under the stubbed name.  Parity of that ONE operator
therefore stays unpinned, as tests/test_gpu_parity.py::test_sphere_feature_extractor_vs_oracle already says; the offset field, the
chain in front of it and the norm / activation behind it are the reference's.

Only data leaves this script, per case and size `<case>/<size>/...`:
  feats       the reference's float64 result (a .double() copy of the module) rounded to float32
  err32       max |fp32 result - float64 result| / max |float64 result|: the reference's own fp32 error
  err32_ch    the same per output channel, relative to that channel's maximum (0 for an all-zero channel)
  x_sha256    digest of the regenerated uint8 images       w_sha256    digest of the drawn weights
  offset_sha256 (sphere cases)  digest of the reference's `offset` buffer
and per case `<case>/signature`, the state dict at S1 as "key:shape" strings.

The script asserts what keeps the comparison sharp: every result finite, 0.1 <= max |feats| <= 100, err32 <= 5e-6, at most 60 % of
the elements exactly zero."""
import copy
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("MVSGI_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from oracle import mvsgi_oracle as O  # noqa: E402

tv, ops = types.ModuleType("torchvision"), types.ModuleType("torchvision.ops")
def _deform(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    assert mask is None
    return O.deform_conv2d(input, offset, weight, bias, stride, padding, dilation)
ops.deform_conv2d = _deform
tv.ops = ops
sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, ops

from dsta_mvs.model.feature_extractor.simple_feature_extractor import SimpleFeatExtraction  # noqa: E402
from dsta_mvs.model.feature_extractor.sphere_feature_extractor import SphereEquirectFeatExtraction  # noqa: E402

from mvs_gi_amd import synth  # noqa: E402
import extractor_cases as X  # noqa: E402

REFERENCE = types.SimpleNamespace(SimpleFeatExtraction=SimpleFeatExtraction, SphereEquirectFeatExtraction=SphereEquirectFeatExtraction)
OUT = os.path.join(ROOT, "tests", "golden")
FAILED = []           # (case, size, condition) of every result outside the conditions above: nothing is written then
torch.manual_seed(0)
torch.set_num_threads(min(16, os.cpu_count() or 1))


def extractor_file(entries):
    out = {}
    for cname, sname in entries:
        case = X.CASES[cname]
        ext = X.make_module(REFERENCE, case, sname).eval()
        w = X.load_drawn(ext, case["seed"], case["gain"])
        if sname == "S1":
            out[f"{cname}/signature"] = np.asarray(X.signature(ext))
        u8 = X.make_images(case, sname)
        x32 = X.to_float(torch.from_numpy(u8))
        ext64 = copy.deepcopy(ext).double()
        with torch.no_grad():
            y32, y64 = ext(x32).numpy().astype(np.float64), ext64(x32.double()).numpy()
        assert y64.dtype == np.float64 and y64.shape == X.out_shape(case, sname), (cname, sname, y64.shape)
        top = np.abs(y64).max()
        top_ch = np.abs(y64).max(axis=(0, 2, 3))
        err = np.float64(np.abs(y32 - y64).max() / top)
        err_ch = np.abs(y32 - y64).max(axis=(0, 2, 3)) / np.where(top_ch > 0, top_ch, 1.0)
        err_ch = np.where(top_ch > 0, err_ch, 0.0)
        feats = y64.astype(np.float32)
        zeros = float((feats == 0).mean())
        print(f"  {cname:16s} {sname} {tuple(u8.shape)} -> {tuple(feats.shape)} max {top:.3f} err32 {err:.2e} "
              f"err32_ch max {err_ch.max():.2e} zeros {zeros:.2f}", flush=True)
        for ok, what in ((np.isfinite(y64).all(), "finite"), (0.1 <= top <= 100, f"max {top}"), (err <= 5e-6, f"err32 {err}"),
                         (zeros <= 0.60, f"zeros {zeros}")):
            if not ok:
                FAILED.append((cname, sname, what))
        p = f"{cname}/{sname}/"
        out[p + "feats"], out[p + "err32"], out[p + "err32_ch"] = feats, err, err_ch.astype(np.float64)
        out[p + "x_sha256"], out[p + "w_sha256"] = np.asarray(synth.digest({"x": u8})), np.asarray(synth.digest(w))
        if case["cls"] == "Sphere":
            out[p + "offset_sha256"] = np.asarray(synth.digest({"offset": ext.final_layer.blk[0].offset.numpy()}))
    return out


if __name__ == "__main__":
    files = {fname: extractor_file(entries) for fname, entries in X.FILES.items()}
    assert not FAILED, FAILED
    for fname, out in files.items():
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(f"{path}: {size} bytes", flush=True)
        assert size < 1_000_000, size
