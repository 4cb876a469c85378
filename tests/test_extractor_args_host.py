"""CPU: the drop-in feature extractors across the reference's constructor arguments (tests/extractor_cases.py) -- state-dict
signatures, the sphere conv's offset field, output shapes and the seeded weight / image draws against what
tools/make_extractor_goldens.py recorded from the reference's own modules.  No GPU, no reference checkout."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import extractor_cases as X
from mvs_gi_amd import dropin, synth


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {f: np.load(os.path.join(golden_dir, f + ".npz")) for f in X.FILES}


def test_tables_are_consistent(goldens):
    assert len(X.CASES) == 32 and set(X.S2_CASES) <= set(X.CASES) and len(X.S2_CASES) == 8
    assert [c["seed"] for c in X.CASES.values()] == list(range(len(X.CASES)))
    assert all("S1" in X.SIZES_OF[c] for c in X.CASES)
    no_s3 = {c for c in X.CASES if "S3" not in X.SIZES_OF[c]}
    assert no_s3 == {"layers_2_0_2", "layers_2_2_2", "instance", "instance_c8", "sphere_instance"}
    for f, entries in X.FILES.items():
        for cname, sname in entries:
            assert f"{cname}/{sname}/feats" in goldens[f], (f, cname, sname)
    for f in goldens:
        assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", f + ".npz")) <= 1_000_000


@pytest.mark.parametrize("name", list(X.CASES))
def test_signature_matches_the_reference(goldens, name):
    """Keys, shapes and order of the drop-in's state dict are the reference's."""
    ext = X.make_module(dropin, X.CASES[name], "S1")
    assert X.signature(ext) == [str(s) for s in goldens["extractor_args"][f"{name}/signature"]]


@pytest.mark.parametrize("name", list(X.CASES))
def test_weights_images_shapes_and_offsets(goldens, name):
    """draw_state_dict on the drop-in module and the regenerated images are the arrays the reference ran on; infer_size
    predicts the golden's shape; the sphere conv's offset buffer is the reference's, bit for bit."""
    case = X.CASES[name]
    for sname in X.SIZES_OF[name]:
        z, p = goldens[X.FILE_OF[sname]], f"{name}/{sname}/"
        ext = X.make_module(dropin, case, sname)
        w = X.load_drawn(ext, case["seed"], case["gain"])
        assert all(torch.equal(ext.state_dict()[k], torch.from_numpy(np.asarray(v))) for k, v in w.items())
        assert synth.digest(w) == str(z[p + "w_sha256"])
        u8 = X.make_images(case, sname)
        assert u8.dtype == np.uint8 and u8.shape == (X.M,) + X.SHAPES[sname] + (X.kwargs_of(case)["in_chs"],)
        assert not np.array_equal(u8[0], u8[1])
        assert synth.digest({"x": u8}) == str(z[p + "x_sha256"])
        size = ext.first.infer_size(X.SHAPES[sname])
        for layer in ext.blks:
            size = layer.infer_size(size)
        feats = z[p + "feats"]
        assert feats.dtype == np.float32 and feats.shape == (X.M, ext.chs) + tuple(size) == X.out_shape(case, sname)
        top = float(np.abs(feats).max())
        assert np.isfinite(feats).all() and 0.1 <= top <= 100 and float((feats == 0).mean()) <= 0.60
        err32, err_ch = float(z[p + "err32"]), z[p + "err32_ch"]
        assert 1e-8 < err32 <= 5e-6, err32          # the reference's own fp32 error: what the f32-mode figures are read against
        assert err_ch.shape == (ext.chs,) and (err_ch >= 0).all() and float(err_ch.max()) < 1e-4
        if case["cls"] == "Sphere":
            assert synth.digest({"offset": ext.final_layer.blk[0].offset.numpy()}) == str(z[p + "offset_sha256"])
        else:
            assert p + "offset_sha256" not in z


@pytest.mark.parametrize("name", list(X.CASES))
def test_state_dict_loads(name):
    """strict=True with every key; for a sphere case a checkpoint without the `offset` buffer loads with strict=False and
    misses nothing else."""
    case = X.CASES[name]
    ext = X.make_module(dropin, case, "S1")
    drawn = {k: torch.from_numpy(np.asarray(v)) for k, v in X.draw_state_dict(ext, case["seed"], case["gain"]).items()}
    full = dict(ext.state_dict())
    full.update(drawn)
    res = ext.load_state_dict(full, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    res = ext.load_state_dict(drawn, strict=False)
    assert res.unexpected_keys == []
    assert res.missing_keys == (["final_layer.blk.0.offset"] if case["cls"] == "Sphere" else [])


def test_draw_state_dict_refuses_an_unknown_key():
    with pytest.raises(KeyError, match="no rule"):
        X.draw_state_dict(nn.Linear(2, 2), 0)


def test_the_restated_walk_says_what_was_read_from_the_code():
    """extractor_cases.expected_route (what the GPU tests compare the recorded launches with) against the literal sequences, and the
    properties stated for whole groups of cases."""
    for name, want in X.LITERAL_ROUTES.items():
        for mode in ("bf16x3", "f16x3"):
            assert X.expected_route(name, mode) == want, (name, mode)
    for name in X.CASES:
        kw = X.kwargs_of(X.CASES[name])
        f32 = X.expected_route(name, "f32")
        assert not any(t in ("rb", "s2s") or t.startswith("rbs") or "->split" in t or " b3" in t for t in f32), name
        for t in f32:
            if t.startswith("conv"):
                k, io = int(t.split()[1][1:]), t.split()[3].split("->")
                assert (" mfma packed" in t) == (k == 3 and int(io[0]) % 16 == 0 and int(io[1]) in (16, 32)), (name, t)
        b3 = X.expected_route(name, "bf16x3")
        sphere = X.CASES[name]["cls"] == "Sphere"
        # stem, two per block, the stride-2 layers, final
        n_layers = 1 + 2 * sum(kw["layers"]) + max(len(kw["layers"]) - 1, 0) + 1
        assert (b3[-1] == "deform" or b3[-2:] == ["deform", "inorm"]) == sphere
        if kw["norm_type"] == "instance":
            assert b3 == f32 and b3.count("inorm") == n_layers and not any(" b3" in t for t in b3), name
        if name in ("k1", "k5", "k7"):
            assert not any(t.startswith("rb") for t in b3) and [t for t in b3 if " b3" in t] == ["conv k3 s2 16->16 b3 packed"]
            assert b3.count(f"conv k{kw['k_sz']} s1 16->16 auto") == 2 * sum(kw["layers"]) + 1
        if name in ("default", "chs6"):
            assert len(b3) == n_layers and all(t.startswith("conv") and " auto" in t for t in b3)
        if kw["chs"] >= 32:
            assert all(t.startswith("conv") or t == "deform" for t in b3)
            assert all(" b3 packed" in t for t in b3 if t.startswith("conv k3")) and b3[0].endswith("auto nchw")
            assert (kw["chs"] // 16, 1) in X.B3_TEMPLATE and (kw["chs"] // 16, 2) in X.B3_TEMPLATE
        u8 = X.expected_route(name, "bf16x3", u8=True)
        assert u8[1:] == b3[1:]
        if (kw["in_chs"], kw["chs"]) == (3, 16):
            assert u8[0] == b3[0].replace("auto nchw", "auto u8 packed")
        else:
            assert u8[0] == b3[0]
