#!/usr/bin/env python3
"""Generate tests/golden/topology.npz and tests/golden/topology_routes.npz by running the REFERENCE's own regulators (imported
from the reference checkout, as tools/make_instnorm_goldens.py does) built with the constructor arguments of
tests/topology_cases.py, on that table's seeded inputs and weights.

Only data leaves this script, per case and shape `<case>/<shape>/...`:
  costs       the reference's float64 result (a .double() copy of the module) rounded to float32
  err32       max |fp32 result - float64 result| / max |float64 result|: the reference's own fp32 error
  x_sha256    digest of the regenerated input          w_sha256    digest of the drawn weights
and per case `<case>/signature`, the state dict as "key:shape" strings.  The composed cases (`composed/<case>/...`) store
reg(cvb(...)) of the reference's SphericalSweepStdMasked + regulator in the same way.
"""
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

from dsta_mvs.model.cost_volume_builder import SphericalSweepStdMasked  # noqa: E402
from dsta_mvs.model.cost_volume_regulator import unet_regulator  # noqa: E402

from mvs_gi_amd import synth  # noqa: E402
import topology_cases as T  # noqa: E402
from golden_cases import SMALL_CASES  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.manual_seed(0)
torch.set_num_threads(min(16, os.cpu_count() or 1))


def _both(run32, run64):
    """-> (float64 result rounded to float32, err32)."""
    with torch.no_grad():
        y32, y64 = run32().numpy().astype(np.float64), run64().numpy()
    assert y64.dtype == np.float64 and np.isfinite(y64).all() and np.abs(y64).max() > 0
    return y64.astype(np.float32), np.float64(np.abs(y32 - y64).max() / np.abs(y64).max())


def regulator_file(name, entries):
    out = {}
    for cname, sname in entries:
        case = T.CASES[cname]
        reg = T.make_module(unet_regulator, case).eval()
        w = T.load_drawn(reg, case["seed"])
        out[f"{cname}/signature"] = np.asarray(T.signature(reg))
        x = T.make_input(case, sname, reg.in_chs)
        reg64, x32, x64 = copy.deepcopy(reg).double(), torch.from_numpy(x), torch.from_numpy(x).double()
        costs, err = _both(lambda: reg(x32), lambda: reg64(x64))
        p = f"{cname}/{sname}/"
        out[p + "costs"], out[p + "err32"] = costs, err
        out[p + "x_sha256"], out[p + "w_sha256"] = np.asarray(synth.digest({"x": x})), np.asarray(synth.digest(w))
        print(f"  {cname:16s} {sname} {tuple(x.shape)} -> {tuple(costs.shape)} max {np.abs(costs).max():.3f} err32 {err:.2e}", flush=True)
    return out


def composed_cases():
    base = SMALL_CASES["std_d8"]
    cfg = base["cfg"]
    inp = synth.make_inputs(cfg, seed=base["seed"], batch=T.COMPOSED_BATCH, grid_kind=base["grid_kind"],
                            grid_mask_dtype=base["grid_mask_dtype"])
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    t64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in t.items()}
    out = {"composed/inputs_sha256": np.asarray(synth.digest(inp))}
    for cname, case in T.COMPOSED.items():
        cvb = SphericalSweepStdMasked(**T.builder_kwargs(case, cfg)).eval()
        reg = unet_regulator.UNetCostVolumeRegulatorBase(**case["kwargs"]).eval()
        wb, wr = T.load_drawn(cvb, case["seed"] + T.BUILDER_SEED_OFFSET), T.load_drawn(reg, case["seed"])
        cvb64, reg64 = copy.deepcopy(cvb).double(), copy.deepcopy(reg).double()
        args = ("feats", "grids", "grid_masks", "masks")
        costs, err = _both(lambda: reg(cvb(*[t[k] for k in args])), lambda: reg64(cvb64(*[t64[k] for k in args])))
        p = f"composed/{cname}/"
        out[p + "costs"], out[p + "err32"] = costs, err
        out[p + "w_sha256"] = np.asarray(synth.digest({**{"b." + k: v for k, v in wb.items()}, **{"r." + k: v for k, v in wr.items()}}))
        out[p + "signature"] = np.asarray(T.signature(cvb) + T.signature(reg))
        print(f"  composed {cname:8s} -> {tuple(costs.shape)} max {np.abs(costs).max():.3f} err32 {err:.2e}", flush=True)
    return out


if __name__ == "__main__":
    for fname, entries in T.FILES.items():
        out = regulator_file(fname, entries)
        if fname == "topology":
            out.update(composed_cases())
        path = os.path.join(OUT, fname + ".npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes", flush=True)
