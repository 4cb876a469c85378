"""CPU: the instance-norm C entry points validate their arguments on the host, and norm_type='instance' configurations give
state dicts that load strict=True into the drop-in modules, while the default weights stay what they were."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mvs_gi_amd import _lib, dropin, synth
from mvs_gi_amd.configs import CONFIGS, DIST_8L, PathConfig
from mvs_gi_amd.pipeline import build_modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = ctypes.c_void_p(16)          # a non-null, 16-byte aligned address that no call below may dereference


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("args, msg", [
    ((None, None, None, None, _P, _P, 1, 64, 16), b"null pointer"),
    ((_P, None, None, None, None, _P, 1, 64, 16), b"null pointer"),
    ((_P, None, None, None, _P, None, 1, 64, 16), b"null pointer"),
    ((_P, None, None, None, _P, _P, 1, 64, 18), b"multiple of 4"),
    ((_P, None, None, None, _P, _P, 1, 1, 16), b"more than one spatial element"),
    ((_P, None, None, None, _P, _P, 0, 64, 16), b"non-positive"),
    ((ctypes.c_void_p(20), None, None, None, _P, _P, 1, 64, 16), b"16-byte aligned"),
])
def test_instance_norm_rejects_bad_arguments(lib, args, msg):
    rc = lib.mvsgi_instance_norm_f32(*args, 1e-5, 0.01, None)
    assert rc != 0 and msg in lib.mvsgi_last_error(), lib.mvsgi_last_error()


def test_instance_norm_workspace_size(lib):
    assert lib.mvsgi_instance_norm_ws_bytes(1, 1, 16) == 0
    assert lib.mvsgi_instance_norm_ws_bytes(1, 64, 6) == 0
    one = lib.mvsgi_instance_norm_ws_bytes(1, 16 * 80 * 320, 16)
    assert 0 < one <= (2 * 64 + 1) * 16 * 4                      # at most 64 partials per frame and channel, plus the pivot
    assert lib.mvsgi_instance_norm_ws_bytes(5, 16 * 80 * 320, 16) == 5 * one      # per frame: the chunking ignores B


def _load_strict(mod, sd):
    mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("tag", ["G16V", "E8-light", "G16VV"])
def test_instance_state_dicts_load_strict(tag, affine):
    cfg0 = CONFIGS[tag].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32), dist_cands=DIST_8L)
    cfg = PathConfig(**{**cfg0.__dict__, "norm_type": "instance", "norm_affine": affine})
    w = synth.make_weights(cfg, seed=3)
    assert not any(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for d in w.values() for k in d)
    assert any(k.endswith("norm_layer.weight") for k in w["cv_regulator"]) == affine
    cvb, reg, _ = build_modules(cfg, w, device="cpu")
    norms = [m for m in list(cvb.modules()) + list(reg.modules()) if isinstance(m, torch.nn.InstanceNorm3d)]
    assert norms and all(m.affine == affine and not m.track_running_stats for m in norms)
    if not affine:
        # the reference-named drop-ins built straight from the NORM3D_TYPE table
        B = dropin.SphericalSweepStdMasked if cfg.builder == "std" else dropin.SphericalSweep
        _load_strict(B(num_cams=cfg.num_cams, feat_chs=cfg.vol_chs, post_k_sz=3, norm_type="instance"), w["cv_builder"])
        _load_strict(dropin.UNetCostVolumeRegulatorBase(in_chs=cfg.reg_in_chs, f_int_chs=cfg.reg_f_int_chs, norm_type="instance"),
                     w["cv_regulator"])
    # the same generator stream as the batch-norm twin: the conv weights are identical
    wb = synth.make_weights(cfg0, seed=3)
    for part in ("cv_builder", "cv_regulator"):
        for k, v in w[part].items():
            if "conv_layer" in k:
                assert np.array_equal(v, wb[part][k]), k
            else:
                assert np.array_equal(v, wb[part][k]), k          # affine gamma / beta: the batch norm's weight / bias draws


def test_instance_extractor_state_dict_loads_strict():
    sd = synth.make_extractor_weights(4, norm_type="instance")
    assert not any("norm_layer" in k for k in sd)
    fe = dropin.SimpleFeatExtraction(in_size=(64, 256), in_chs=3, chs=16, k_sz=3, layers=[5, 10], norm_type="instance")
    _load_strict(fe, sd)
    sdb = synth.make_extractor_weights(4)
    assert all(np.array_equal(v, sdb[k]) for k, v in sd.items())


def test_default_weights_unchanged():
    """The default configuration (norm_type 'batch') draws exactly the weights the committed reference goldens were made from."""
    from golden_cases import SMALL_CASES
    for name in ("std_d8", "cat_d8"):
        case = SMALL_CASES[name]
        assert case["cfg"].norm_type == "batch"
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        w = synth.make_weights(case["cfg"], seed=case["seed"], gain=case["gains"][0])
        got = synth.digest({**w["cv_builder"], **{"r." + k: v for k, v in w["cv_regulator"].items()}})
        assert got == str(z[f"weights_sha256_g{case['gains'][0]:g}"])


def test_instance_norm_goldens_match_regenerated_weights():
    """Every instnorm_* golden was made from the weights make_weights draws today (and the inputs make_inputs draws)."""
    from instnorm_cases import FULL_CASES, SMALL_CASES
    for name, case in {**SMALL_CASES, **FULL_CASES}.items():
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        for gain in case["gains"]:
            w = synth.make_weights(case["cfg"], seed=case["seed"], gain=gain)
            got = synth.digest({**w["cv_builder"], **{"r." + k: v for k, v in w["cv_regulator"].items()}})
            assert got == str(z[f"weights_sha256_g{gain:g}"]), (name, gain)
