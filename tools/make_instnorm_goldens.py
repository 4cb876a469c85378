#!/usr/bin/env python3
"""Generate tests/golden/instnorm_*.npz by running the REFERENCE's own modules built with norm_type='instance'
(imported from the reference checkout, as tools/make_goldens.py does) on the seeded cases of tests/instnorm_cases.py.

Only data leaves this script: input / weight sha256 digests and the reference's outputs.  The affine variant swaps
nn.InstanceNorm3d(c, affine=True) into the reference's modules (mvs_gi_amd.pipeline.affine_instance_norms) before the
seeded gamma / beta are loaded.  Usage: tools/make_instnorm_goldens.py [small] [full] [extractor]
"""
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

from dsta_mvs.model.cost_volume_builder import SphericalSweepStdMasked, SphericalSweep  # noqa: E402
from dsta_mvs.model.cost_volume_regulator.unet_regulator import UNetCostVolumeRegulatorBase  # noqa: E402
from dsta_mvs.model.distance_regressor.distance_regressor import DistanceRegressorWithFixedCandidates  # noqa: E402

from mvs_gi_amd import synth  # noqa: E402
from mvs_gi_amd.pipeline import affine_instance_norms  # noqa: E402
from instnorm_cases import SMALL_CASES, FULL_CASES, EXTRACTOR_CASE  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.manual_seed(0)
torch.set_num_threads(min(16, os.cpu_count() or 1))


def build_reference(cfg, weights):
    Builder = SphericalSweepStdMasked if cfg.builder == "std" else SphericalSweep
    cvb = Builder(num_cams=cfg.num_cams, feat_chs=cfg.vol_chs, post_k_sz=3, norm_type=cfg.norm_type)
    reg = UNetCostVolumeRegulatorBase(in_chs=cfg.reg_in_chs, f_int_chs=cfg.reg_f_int_chs, norm_type=cfg.norm_type)
    if cfg.norm_affine:
        affine_instance_norms(cvb)
        affine_instance_norms(reg)
    dr = DistanceRegressorWithFixedCandidates(bf=cfg.bf, dist_cands=list(cfg.dist_cands),
                                              interp_scale_factor=cfg.interp_scale_factor, pre_interp=cfg.pre_interp)
    cvb.load_state_dict({k: torch.from_numpy(v) for k, v in weights["cv_builder"].items()}, strict=True)
    reg.load_state_dict({k: torch.from_numpy(v) for k, v in weights["cv_regulator"].items()}, strict=True)
    return cvb.eval(), reg.eval(), dr.eval()


def weights_digest(w):
    return np.asarray(synth.digest({**w["cv_builder"], **{"r." + k: v for k, v in w["cv_regulator"].items()}}))


def run_case(name, case):
    cfg = case["cfg"]
    inp = synth.make_inputs(cfg, seed=case["seed"], batch=case["batch"], grid_kind=case["grid_kind"],
                            grid_mask_dtype=case["grid_mask_dtype"])
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    out = {"inputs_sha256": np.asarray(synth.digest(inp))}
    for gain in case["gains"]:
        w = synth.make_weights(cfg, seed=case["seed"], gain=gain)
        cvb, reg, dr = build_reference(cfg, w)
        with torch.no_grad():
            inv, pr = dr(reg(cvb(t["feats"], t["grids"], t["grid_masks"], t["masks"])))
        tag = f"g{gain:g}"
        out[f"inv_dist_{tag}"] = inv.numpy()
        out[f"weights_sha256_{tag}"] = weights_digest(w)
        print(f"  {name} gain={gain}: inv_dist {tuple(inv.shape)} range [{inv.min():.4f}, {inv.max():.4f}] "
              f"maxprob {pr.max(1)[0].mean():.3f}", flush=True)
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **out)


def extractor_case():
    import importlib.util
    from dsta_mvs.model.feature_extractor import SimpleFeatExtraction
    spec = importlib.util.spec_from_file_location("torch_only", os.path.join(REF, "dsta_mvs/model/mvs_model/torch_only.py"))
    torch_only = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(torch_only)
    cfg, seed, batch = EXTRACTOR_CASE["cfg"], EXTRACTOR_CASE["seed"], EXTRACTOR_CASE["batch"]
    fw = synth.make_extractor_weights(seed, norm_type="instance")
    fe = SimpleFeatExtraction(in_size=(64, 256), in_chs=3, chs=16, k_sz=3, layers=[5, 10], norm_type="instance").eval()
    fe.load_state_dict({k: torch.from_numpy(v) for k, v in fw.items()}, strict=True)
    imgs = synth.make_images(cfg, seed=seed, batch=batch)
    inp = synth.make_inputs(cfg, seed=seed, batch=batch)
    w = synth.make_weights(cfg, seed=seed)
    cvb, reg, dr = build_reference(cfg, w)
    model = torch_only.SphericalSweepStereoBase(fe, cvb, reg, dr).eval()
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    with torch.no_grad():
        feats = model.extract_features(torch.from_numpy(imgs))
        inv, _ = model(torch.from_numpy(imgs), t["grids"], t["grid_masks"], t["masks"])
    np.savez_compressed(os.path.join(OUT, "instnorm_extractor.npz"), feats=feats.numpy(), inv_dist=inv.numpy(),
                        imgs_sha256=np.asarray(synth.digest({"imgs": imgs})), inputs_sha256=np.asarray(synth.digest(inp)),
                        weights_sha256=weights_digest(w), extractor_sha256=np.asarray(synth.digest(fw)))
    print("  instnorm_extractor: feats", tuple(feats.shape), "std", float(feats.std()), "inv", tuple(inv.shape), flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["small", "full", "extractor"]
    if "small" in which:
        for name, case in SMALL_CASES.items():
            run_case(name, case)
    if "extractor" in which:
        extractor_case()
    if "full" in which:
        for name, case in FULL_CASES.items():
            run_case(name, case)
