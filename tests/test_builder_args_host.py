"""CPU: the drop-in cost-volume builders across the reference's constructor arguments (tests/builder_cases.py) -- state-dict
signatures and constructor attributes, the seeded input / weight draws and the oracle's sweeps against what
tools/make_builder_goldens.py recorded from the reference's own modules, the conditions that keep the goldens sharp, and the route
table against the predicates it restates.  No GPU, no reference checkout."""
import os

import numpy as np
import pytest
import torch

import builder_cases as X
from mvs_gi_amd import dropin, hip_ops as H, synth
from mvs_gi_amd.dropin import common_modules as cm, cost_volume_builder as cb
from oracle import mvsgi_oracle as O


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {f: np.load(os.path.join(golden_dir, f + ".npz")) for f in X.FILES}


def _z(goldens, name, sname):
    return goldens[X.FILE_OF[(name, sname)]], f"{name}/{sname}/"


def test_tables_are_consistent(goldens, golden_dir):
    assert len(X.CASES) == 37 and sum(c["cls"] == "Std" for c in X.CASES.values()) == 26
    assert [c["seed"] for c in X.CASES.values()] == list(range(len(X.CASES)))
    assert len(X.RUNS) == 85 and sorted(X.FILE_OF) == sorted(X.RUNS)
    assert {c for c in X.CASES if "S2" not in X.shapes_of(X.CASES[c])} == {"instance", "instance_c8", "cat_instance"}
    assert [c for c in X.CASES if "S3" in X.shapes_of(X.CASES[c])] == [
        "n1", "n2", "default", "n4", "n5", "n8", "relu", "linear", "nonorm", "nonorm_relu", "instance", "gm_u8", "gm_f32", "gm_f32_values"]
    assert X.WIDE_CASES == [c for c, v in X.CASES.items() if v["cls"] == "Std" and v["n"] > 4]
    assert X.FRONT_CHUNK == 16 and X.S3[0] > 2                     # the walked module's chunk of 2 (test_gpu_builder_args.py)
    assert max(X.feat_chs(c) for c in X.CASES.values()) == 128
    for f, entries in X.FILES.items():
        assert os.path.getsize(os.path.join(golden_dir, f + ".npz")) <= X.MAX_FILE_BYTES == 1_000_000, f
        for cname, sname in entries:
            assert f"{cname}/{sname}/vol" in goldens[f], (f, cname, sname)
    stored = sorted(os.path.basename(p)[:-4] for p in os.listdir(golden_dir) if p.startswith("builder_args"))
    assert stored == sorted(X.FILES)


@pytest.mark.parametrize("name", list(X.CASES))
def test_signature_and_attributes_match_the_reference(goldens, name):
    """Keys, shapes and order of the drop-in's state dict are the reference's, and so is what the constructor sets."""
    case = X.CASES[name]
    cvb = X.make_module(dropin, case)
    z = goldens[X.FILE_OF[(name, "S1")]]
    assert X.signature(cvb) == [str(s) for s in z[f"{name}/signature"]]
    attrs = [str(cvb.num_cams), str(cvb.feat_chs), cvb.norm_type.__name__, cvb.relu_type.__name__, str(cvb.grid_sample_mode)]
    assert attrs == [str(s) for s in z[f"{name}/attrs"]]
    assert cvb.num_cams == case["n"] and cvb.feat_chs == X.feat_chs(case) and cvb.grid_sample_mode == "bilinear"
    res = cvb.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in X.T.draw_state_dict(cvb, 0).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


@pytest.mark.parametrize("name", list(X.CASES))
def test_inputs_weights_and_the_oracles_sweep(goldens, name):
    """The regenerated inputs and weights are the arrays the reference ran on; the oracle's sweep is the reference's, bit for bit
    (what the GPU tests compare the kernels with); the stored volumes keep the conditions the maker asserted."""
    case = X.CASES[name]
    for sname in X.shapes_of(case):
        z, p = _z(goldens, name, sname)
        cvb = X.make_module(dropin, case)
        w = X.load_drawn(cvb, case)
        assert all(torch.equal(cvb.state_dict()[k], torch.from_numpy(np.asarray(v))) for k, v in w.items())
        assert synth.digest(w) == str(z[p + "w_sha256"])
        inp = X.make_inputs(case, sname)
        b, hi, wi, d, ho, wo, hm, wm = X.SHAPES[sname]
        assert inp["feats"].shape == (b, case["n"], case["c"], hi, wi) and inp["grids"].shape == (b, case["n"], d, ho, wo, 2)
        assert inp["grid_masks"].shape == (b, case["n"], d, ho, wo, 1) and inp["masks"].shape == (b, case["n"], 1, hm, wm)
        assert inp["grid_masks"].dtype == {"bool": np.bool_, "u8": np.uint8, "f32": np.float32, "f32_values": np.float32}[case["gm"]]
        if case["gm"] == "f32_values" and sname != "S2":
            assert set(np.unique(inp["grid_masks"]).tolist()) == {-2.0, 0.0, 0.5, 1.0}
        assert synth.digest(inp) == str(z[p + "x_sha256"])
        t = {k: torch.from_numpy(v) for k, v in inp.items()}
        raw = (O.sweep_std_masked(*[t[k] for k in X.ARGS]) if case["cls"] == "Std" else O.sweep_concat(t["feats"], t["grids"])).numpy()
        assert raw.dtype == np.float32 and raw.shape == X.vol_shape(case, sname)
        assert X.raw_digest(raw) == str(z[p + "vol_raw_sha256"]), (name, sname)
        if case["cls"] == "Std":          # the cameras added one by one: the same bits up to four cameras, a last-bit difference above
            in_order = O.sweep_std_masked(*[t[k] for k in X.ARGS], camera_order=True).numpy()
            if name in X.WIDE_CASES:
                rel = float(np.abs(in_order.astype(np.float64) - raw).max() / np.abs(raw).max())
                print(f"{name}/{sname}: {int((in_order != raw).sum())} of {raw.size} elements differ in camera order, max-rel {rel:.2e}")
                assert rel <= X.WIDE_BAR and np.array_equal(in_order == 0, raw == 0)
            else:
                assert np.array_equal(in_order, raw)
        vol = z[p + "vol"]
        assert vol.dtype == np.float32 and vol.shape == raw.shape and np.isfinite(vol).all()
        assert 0.1 <= float(np.abs(vol).max()) <= 100
        zeros_raw, zeros_vol = float((raw == 0).mean()), float((vol == 0).mean())
        print(f"{name}/{sname}: zeros vol_raw {zeros_raw:.2f} vol {zeros_vol:.2f} err32 {float(z[p + 'err32']):.2e}")
        if case["cls"] == "Std" and case["n"] == 1:
            assert zeros_raw == 1.0
        else:
            assert zeros_raw <= 0.80
        assert zeros_vol <= 0.75
        err32, err_ch = float(z[p + "err32"]), z[p + "err32_ch"]
        assert 1e-8 < err32 <= 2e-6, err32          # the reference's own fp32 error: what the f32-mode figures are read against
        assert err_ch.shape == (X.feat_chs(case),) and (err_ch >= 0).all() and float(err_ch.max()) < 2e-5


def test_one_camera_gives_the_activation_of_the_shift(goldens):
    """N = 1: `summed_mask > 1` never holds, vol_raw is zero and every voxel of channel c is act(beta - mean * gamma / sqrt(var + eps))."""
    case = X.CASES["n1"]
    w = {k: np.asarray(v, np.float64) for k, v in X.T.draw_state_dict(X.make_module(dropin, case), X.WEIGHT_SEED_OFFSET + case["seed"]).items()}
    alpha = w["post_vol.norm_layer.weight"] / np.sqrt(w["post_vol.norm_layer.running_var"] + 1e-5)
    shift = w["post_vol.norm_layer.bias"] - w["post_vol.norm_layer.running_mean"] * alpha
    want = np.where(shift > 0, shift, 0.01 * shift)
    assert (shift > 0).any() and (shift < 0).any()
    for sname in X.shapes_of(case):
        z, p = _z(goldens, "n1", sname)
        vol = z[p + "vol"]
        assert np.allclose(vol, np.broadcast_to(want[None, :, None, None, None], vol.shape), rtol=1e-6, atol=0)
        assert (vol == vol[:1, :, :1, :1, :1]).all()


def _feats(case, sname):
    b, hi, wi = X.SHAPES[sname][:3]
    return torch.empty((b, case["n"], case["c"], hi, wi))


def test_expected_route_is_total_and_agrees_with_the_predicates():
    """expected_route for every case x mode x shape x (cache on | off) x (first | later forward), against hip_ops' predicates and
    the condition of _std_front evaluated on shapes and module attributes alone."""
    assert cb._FRONT_CHUNK == X.FRONT_CHUNK and cb._USE_RS and cb._RIG_CACHE_ENV
    known = {"sweep_validity", "sweep_std_valid_split", "conv3d_rs16", "sweep_std_valid", "sweep_std", "sweep_cat", "conv3d split",
             "conv3d f32", "instance_norm"}
    n = 0
    for name, sname in X.RUNS:
        case = X.CASES[name]
        cvb = X.make_module(dropin, case).eval()
        conv, norm = cvb.post_vol.conv_layer, cvb.post_vol.norm_layer
        f = _feats(case, sname)
        slope = cm.act_slope(cvb.post_vol.activation)
        assert slope == {"leaky": 0.01, "original": 0.0, "none": 1.0}[X.kwargs_of(case)["relu_type"]]
        inorm = isinstance(norm, torch.nn.InstanceNorm3d)
        assert inorm == X.is_instance(case) and not (inorm and norm.track_running_stats)
        for mode in X.MODES:
            split = mode != "f32"
            for cache in (True, False):
                usable = cache and H.valid_sweep_ok(f)                                  # _rig_cache_usable on a device tensor
                front = case["cls"] == "Std" and cb._USE_RS and split and conv.in_channels == 16 and conv.out_channels == 16 \
                    and not inorm and 0.0 <= slope <= 1.0 and f.shape[2] == 16 and usable
                assert front == X.front_ok(case, mode, cache), (name, mode, cache)
                for first in (True, False):
                    r = X.expected_route(case, mode, sname, cache=cache, first=first)
                    n += 1
                    assert r and set(r) <= known, r
                    assert X.expected_route(case, mode, "S1", cache=cache, first=first) == r        # no shape decides a route here
                    conv_split = split and conv.in_channels % 16 == 0 and conv.out_channels % 16 == 0      # ConvLaunch._run_conv
                    if case["cls"] == "Cat":
                        assert r[0] == "sweep_cat" and len(r) == 2 + inorm
                    else:
                        assert ("sweep_validity" in r) == ((usable and first) or (not cache and not H.nhwc_sweep_ok(f) and H.valid_sweep_ok(f)))
                        assert (r[-2:] == ["sweep_std_valid_split", "conv3d_rs16"]) == front
                        assert ("sweep_std" in r) == (not usable)
                        assert ("sweep_std_valid" in r) == (not front and H.valid_sweep_ok(f) and (usable or not H.nhwc_sweep_ok(f)))
                    if not front:
                        assert r[-1 - inorm] == ("conv3d split" if conv_split else "conv3d f32")
                        assert (r[-1] == "instance_norm") == inorm
                    assert X.sweep_route(case, cache, first) == [t for t in X.expected_route(case, "f32", sname, cache, first) if t.startswith("sweep")]
    assert n == 85 * 3 * 2 * 2
    # the chunked front end: B = 5 in chunks of 2 on a stride-0 rig, and only there
    d = X.CASES["default"]
    assert X.expected_route(d, "f16x3", "S3", chunk=2, shared_rig=True) == ["sweep_validity"] + ["sweep_std_valid_split", "conv3d_rs16"] * 3
    assert X.expected_route(d, "f16x3", "S3", chunk=2, shared_rig=True, first=False, batch=2) == ["sweep_std_valid_split", "conv3d_rs16"]
    assert X.expected_route(d, "f16x3", "S3", chunk=2, shared_rig=False) == ["sweep_validity", "sweep_std_valid_split", "conv3d_rs16"]
    assert X.expected_route(d, "f32", "S3", chunk=2, shared_rig=True) == ["sweep_validity", "sweep_std_valid", "conv3d f32"]


def test_literal_routes():
    """What was read from the code, written out."""
    R = lambda name, mode, **k: X.expected_route(X.CASES[name], mode, "S1", **k)
    assert R("default", "f16x3") == ["sweep_validity", "sweep_std_valid_split", "conv3d_rs16"]
    assert R("default", "bf16x3", first=False) == ["sweep_std_valid_split", "conv3d_rs16"]
    assert R("default", "f32") == ["sweep_validity", "sweep_std_valid", "conv3d f32"]
    assert R("default", "f16x3", cache=False) == ["sweep_std", "conv3d split"]
    assert R("n8", "f16x3", cache=False) == ["sweep_std", "sweep_validity", "sweep_std_valid", "conv3d split"]
    assert R("n6_c8", "f16x3", cache=False) == ["sweep_std", "sweep_validity", "sweep_std_valid", "conv3d f32"]
    assert R("n6_c5", "f16x3") == R("c5", "f32") == R("c6", "bf16x3", cache=False) == ["sweep_std", "conv3d f32"]
    assert R("c8", "f16x3") == R("c24", "bf16x3") == ["sweep_validity", "sweep_std_valid", "conv3d f32"]
    assert R("c32", "f16x3") == R("c64", "bf16x3") == ["sweep_validity", "sweep_std_valid", "conv3d split"]
    assert R("c32", "f32") == ["sweep_validity", "sweep_std_valid", "conv3d f32"]
    assert R("instance", "f16x3") == ["sweep_validity", "sweep_std_valid", "conv3d split", "instance_norm"]
    assert R("instance_c8", "f16x3") == R("instance", "f32") == ["sweep_validity", "sweep_std_valid", "conv3d f32", "instance_norm"]
    assert R("relu", "f16x3") == R("linear", "f16x3") == R("nonorm_relu", "bf16x3") == R("gm_f32_values", "f16x3") == R("default", "f16x3")
    assert R("cat_3x5", "f16x3") == R("cat_3x4", "f16x3") == R("cat_3x16", "f32") == ["sweep_cat", "conv3d f32"]
    assert R("cat_3x16", "f16x3") == R("cat_2x8", "bf16x3") == R("cat_8x16", "f16x3") == ["sweep_cat", "conv3d split"]
    assert R("cat_instance", "bf16x3") == ["sweep_cat", "conv3d split", "instance_norm"]


@pytest.mark.parametrize("k", [1, 5])
def test_other_post_vol_kernels_construct_with_the_reference_signature(k):
    """post_k_sz of 1 and 5 constructs (the reference's does) and a checkpoint loads; forward refuses it (test_gpu_builder_args.py)."""
    cvb = dropin.SphericalSweepStdMasked(num_cams=3, feat_chs=16, post_k_sz=k)
    assert tuple(cvb.post_vol.conv_layer.weight.shape) == (16, 16, k, k, k) and tuple(cvb.post_vol.conv_layer.padding) == (k // 2,) * 3
    assert [s.split(":")[0] for s in X.signature(cvb)] == [s.split(":")[0] for s in X.signature(X.make_module(dropin, X.CASES["default"]))]
