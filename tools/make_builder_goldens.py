#!/usr/bin/env python3
"""Generate tests/golden/builder_args_*.npz by running the REFERENCE's own cost-volume builders (imported from the reference
checkout, as tools/make_topology_goldens.py does) built with the constructor arguments of tests/builder_cases.py, on that table's
seeded inputs and weights.

Only data leaves this script, per case and shape `<case>/<shape>/...`:
  vol_raw_sha256  digest of the reference's fp32 `sweep` output, the sign of its zeros dropped (the array is not stored: the oracle
                  regenerates it, and this script asserts that it does, bit for bit, for every SphericalSweepStdMasked entry; a
                  sampled feature that is zero has the sign its sampler's arithmetic leaves, and np.array_equal ignores it too)
  vol             post_vol of a .double() copy of the module applied to that fp32 vol_raw cast to double, rounded to float32.  The
                  double chain starts BEHIND the sweep on purpose: in double the sampler's `> 0` mask test can flip a voxel's
                  validity against fp32, which is a discontinuity, not an error -- the sweep is pinned bit for bit instead
  err32           max |fp32 post_vol - vol| / max |vol|: the reference's own fp32 error          err32_ch  the same per output
                  channel, relative to that channel's maximum (0 for an all-zero channel)
  x_sha256        digest of the regenerated inputs          w_sha256    digest of the drawn weights
and per case `<case>/signature`, the state dict as "key:shape" strings, and `<case>/attrs`, what the constructor set
(num_cams, feat_chs, norm_type, relu_type, grid_sample_mode; the two types by class name).

The script asserts what keeps the comparison sharp, for the reference alone: every output finite, 0.1 <= max |vol| <= 100, at most
80 % of a vol_raw exactly zero (N = 1 exempt: there all of it is) and at most 75 % of a vol, each file within 1 000 000 bytes."""
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

tv, ops = types.ModuleType("torchvision"), types.ModuleType("torchvision.ops")
def _absent(*a, **k):
    raise NotImplementedError("torchvision not installed")
ops.deform_conv2d = _absent
tv.ops = ops
sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, ops

from dsta_mvs.model.cost_volume_builder import SphericalSweep, SphericalSweepStdMasked  # noqa: E402

from mvs_gi_amd import synth  # noqa: E402
from oracle import mvsgi_oracle as O  # noqa: E402
import builder_cases as X  # noqa: E402

REFERENCE = types.SimpleNamespace(SphericalSweep=SphericalSweep, SphericalSweepStdMasked=SphericalSweepStdMasked)
OUT = os.path.join(ROOT, "tests", "golden")
FAILED = []           # (case, shape, condition) of every result outside the conditions above: nothing is written then
torch.manual_seed(0)
torch.set_num_threads(min(16, os.cpu_count() or 1))


def attrs_of(m):
    return [str(m.num_cams), str(m.feat_chs), m.norm_type.__name__, m.relu_type.__name__, str(m.grid_sample_mode)]


def builder_file(entries, done):
    out = {}
    for cname, sname in entries:
        case = X.CASES[cname]
        cvb = X.make_module(REFERENCE, case).eval()
        w = X.load_drawn(cvb, case)
        if cname not in done:
            done.add(cname)
            out[f"{cname}/signature"], out[f"{cname}/attrs"] = np.asarray(X.signature(cvb)), np.asarray(attrs_of(cvb))
        inp = X.make_inputs(case, sname)
        t = {k: torch.from_numpy(v) for k, v in inp.items()}
        cvb64 = copy.deepcopy(cvb).double()
        with torch.no_grad():
            raw = cvb.sweep(*[t[k] for k in X.ARGS]) if case["cls"] == "Std" else cvb.sweep(t["feats"], t["grids"], t["masks"])
            y32, y64 = cvb.post_vol(raw).numpy().astype(np.float64), cvb64.post_vol(raw.double()).numpy()
            whole = cvb(*[t[k] for k in X.ARGS])
        raw = np.ascontiguousarray(raw.numpy())
        assert raw.dtype == np.float32 and y64.dtype == np.float64 and y64.shape == raw.shape == X.vol_shape(case, sname)
        assert np.array_equal(whole.numpy().astype(np.float64), y32)                    # forward is post_vol(sweep)
        ours = (O.sweep_std_masked(*[t[k] for k in X.ARGS]) if case["cls"] == "Std" else O.sweep_concat(t["feats"], t["grids"])).numpy()
        top, top_ch = np.abs(y64).max(), np.abs(y64).max(axis=(0, 2, 3, 4))
        d = np.abs(y32 - y64)
        err = np.float64(d.max() / top)
        err_ch = np.where(top_ch > 0, d.max(axis=(0, 2, 3, 4)) / np.where(top_ch > 0, top_ch, 1.0), 0.0)
        vol = y64.astype(np.float32)
        z_raw, z_vol = float((raw == 0).mean()), float((vol == 0).mean())
        print(f"  {cname:14s} {sname} -> {tuple(vol.shape)} max {top:.3f} err32 {err:.2e} err32_ch max {err_ch.max():.2e} "
              f"zeros raw {z_raw:.2f} vol {z_vol:.2f} oracle {'==' if np.array_equal(ours, raw) else '!='} reference", flush=True)
        for ok, what in ((np.isfinite(y64).all() and np.isfinite(raw).all(), "finite"), (0.1 <= top <= 100, f"max {top}"),
                         (case["cls"] != "Std" or np.array_equal(ours, raw), "the oracle's sweep differs from the reference's"),
                         (z_raw <= 0.80 or (case["cls"] == "Std" and case["n"] == 1), f"vol_raw zeros {z_raw}"),
                         (case["cls"] != "Std" or case["n"] != 1 or z_raw == 1.0, "N = 1: vol_raw is not all zero"),
                         (z_vol <= 0.75, f"vol zeros {z_vol}")):
            if not ok:
                FAILED.append((cname, sname, what))
        p = f"{cname}/{sname}/"
        out[p + "vol_raw_sha256"] = np.asarray(X.raw_digest(raw))
        out[p + "vol"], out[p + "err32"], out[p + "err32_ch"] = vol, err, err_ch.astype(np.float64)
        out[p + "x_sha256"], out[p + "w_sha256"] = np.asarray(synth.digest(inp)), np.asarray(synth.digest(w))
    return out


if __name__ == "__main__":
    done = set()
    files = {fname: builder_file(entries, done) for fname, entries in X.FILES.items()}
    assert not FAILED, FAILED
    for fname, out in files.items():
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(f"{path}: {size} bytes", flush=True)
        assert size <= X.MAX_FILE_BYTES, size
