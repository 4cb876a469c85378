"""CPU: the drop-in regulators across the reference's constructor arguments (tests/topology_cases.py) -- state-dict signatures,
conv specs and the seeded weight / input draws against what tools/make_topology_goldens.py recorded from the reference's own
modules.  No GPU, no reference checkout."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import topology_cases as T
from golden_cases import SMALL_CASES
from mvs_gi_amd import dropin, synth
from mvs_gi_amd.configs import regulator_conv_specs


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {f: np.load(os.path.join(golden_dir, f + ".npz")) for f in T.FILES}


def test_tables_are_consistent(goldens):
    assert len(T.CASES) == 24 and set(T.ROUTE_CASES) <= set(T.CASES) and len(T.ROUTE_CASES) == 12
    assert len({c["seed"] for c in T.CASES.values()}) == len(T.CASES)
    for f, entries in T.FILES.items():
        for cname, sname in entries:
            assert f"{cname}/{sname}/costs" in goldens[f], (f, cname, sname)
    for f in goldens:
        assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", f + ".npz")) <= 1 << 20


@pytest.mark.parametrize("name", list(T.CASES))
def test_signature_matches_the_reference(goldens, name):
    """Keys, shapes and order of the drop-in's state dict are the reference's."""
    reg = T.make_module(dropin, T.CASES[name])
    assert T.signature(reg) == [str(s) for s in goldens["topology"][f"{name}/signature"]]
    if name in T.ROUTE_CASES:
        assert T.signature(reg) == [str(s) for s in goldens["topology_routes"][f"{name}/signature"]]


@pytest.mark.parametrize("name", [n for n, c in T.CASES.items() if c["cls"] == "Base"])
def test_conv_specs_match_the_module(name):
    """configs.regulator_conv_specs with the case's arguments names the module's conv layers, in order, with their channels."""
    kw = {k: v for k, v in T.CASES[name]["kwargs"].items() if k not in ("norm_type", "relu_type")}
    reg = T.make_module(dropin, T.CASES[name])
    specs = regulator_conv_specs(kw.pop("in_chs", 16), kw.pop("f_int_chs", 32), **kw)
    convs = [(n[:-len(".conv_layer")], m.in_channels, m.out_channels, m.bias is not None)
             for n, m in reg.named_modules() if isinstance(m, nn.Conv3d)]
    assert [(p, ci, co, b) for p, ci, co, _, b in specs] == convs


@pytest.mark.parametrize("name", list(T.CASES))
def test_weight_and_input_digests(goldens, name):
    """draw_state_dict on the drop-in module and the regenerated inputs are the arrays the reference ran on."""
    case = T.CASES[name]
    reg = T.make_module(dropin, case)
    w = T.load_drawn(reg, case["seed"])
    assert all(torch.equal(reg.state_dict()[k], torch.from_numpy(np.asarray(v))) for k, v in w.items())
    for f, entries in T.FILES.items():
        for cname, sname in entries:
            if cname != name:
                continue
            z = goldens[f]
            assert synth.digest(w) == str(z[f"{name}/{sname}/w_sha256"])
            x = T.make_input(case, sname, reg.in_chs)
            assert x.shape == (2, reg.in_chs) + T.SHAPES[sname] and not np.array_equal(x[0], x[1])
            assert synth.digest({"x": x}) == str(z[f"{name}/{sname}/x_sha256"])
            err32 = float(z[f"{name}/{sname}/err32"])
            assert 1e-7 < err32 < 5e-6, err32               # the reference's own fp32 error: what the f32-mode figures are read against


@pytest.mark.parametrize("name", list(T.COMPOSED))
def test_composed_case_digests(goldens, name):
    z = goldens["topology"]
    base = SMALL_CASES["std_d8"]
    cfg = base["cfg"]
    inp = synth.make_inputs(cfg, seed=base["seed"], batch=T.COMPOSED_BATCH, grid_kind=base["grid_kind"],
                            grid_mask_dtype=base["grid_mask_dtype"])
    assert synth.digest(inp) == str(z["composed/inputs_sha256"])
    case = T.COMPOSED[name]
    cvb = dropin.SphericalSweepStdMasked(**T.builder_kwargs(case, cfg))
    reg = dropin.UNetCostVolumeRegulatorBase(**case["kwargs"])
    assert T.signature(cvb) + T.signature(reg) == [str(s) for s in z[f"composed/{name}/signature"]]
    wb, wr = T.load_drawn(cvb, case["seed"] + T.BUILDER_SEED_OFFSET), T.load_drawn(reg, case["seed"])
    both = {**{"b." + k: v for k, v in wb.items()}, **{"r." + k: v for k, v in wr.items()}}
    assert synth.digest(both) == str(z[f"composed/{name}/w_sha256"])
    assert tuple(z[f"composed/{name}/costs"].shape) == (T.COMPOSED_BATCH, 1, cfg.num_cands, *cfg.cv_hw)


def test_draw_state_dict_refuses_an_unknown_key():
    with pytest.raises(KeyError, match="no rule"):
        T.draw_state_dict(nn.Linear(2, 2), 0)


@pytest.mark.parametrize("keep, consistent", [([1], False), ([2], False), ([0], False), ([1, 2], True)])
def test_older_class_constructs_with_keep_last_chs_like_the_reference(keep, consistent):
    """The reference constructs UNetCostVolumeRegulator with a non-empty keep_last_chs and then, for every such list but the one
    that keeps ALL deeper levels, fails in its own forward (a layer's output does not have the channels of the skip or of the
    next layer's weight: INTEGRATION.md).  The drop-in constructs the same module -- checkpoints of such a model load -- and the
    channel plan shows the mismatch; no forward behaviour is promised for it."""
    kw = dict(T.CASES["old_one_cam"]["kwargs"], keep_last_chs=keep)
    reg = dropin.UNetCostVolumeRegulator(**kw)
    downs = [b.first.conv_layer.out_channels for b in reg.down_blks]
    ups = [u.conv.conv_layer.out_channels for u in reg.upBlks]
    chain_in = [u.conv.conv_layer.in_channels for u in reg.upBlks] + [reg.out_costs[0].conv.conv_layer.in_channels]
    plan_ok = ups == downs[:-1][::-1] and chain_in == [downs[-1]] + ups
    assert plan_ok == consistent
