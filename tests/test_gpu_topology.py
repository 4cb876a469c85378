"""GPU (MI355X): the drop-in regulators across the reference's constructor arguments (tests/topology_cases.py) against the
topology goldens made by the reference's own modules in float64 (tools/make_topology_goldens.py).  The lowering in
dropin/cost_volume_regulator.py and dropin/common_modules.py is a decision tree over channels, stride, slope, norm and level
geometry: these cases reach its branches away from the default topology -- as shipped, with the fast routes forced on at the
smallest volume they accept, across the builder -> regulator hand-over, and with one module walked over two shapes.

Bars: the project's own for the `costs` stage (test_gpu_parity.py::test_small_cases_vs_reference_goldens): 1e-4 of the maximum in
'f32' mode, 1e-3 in the two 16-bit splits; 5e-4 between two 16-bit approximations of one path.

Measured on an MI355X, worst over the shapes a case runs at (max |got - ref| / max |ref| against the float64 golden):
  case             f32      bf16x3   f16x3   | case             f32      bf16x3   f16x3
  default          2.0e-6   2.9e-5   1.8e-6  | linear           2.3e-6   2.2e-5   1.3e-6
  depth1           1.0e-6   1.0e-5   5.2e-7  | nonorm           2.2e-6   2.0e-5   1.1e-6
  depth2           1.8e-6   1.9e-5   1.2e-6  | nonorm_relu      1.2e-6   1.7e-5   7.4e-7
  depth4           1.5e-6   1.5e-5   9.3e-7  | in8_f24          1.4e-6   5.4e-6   1.5e-6
  width1           1.5e-6   1.8e-5   9.8e-7  | in16_f16         9.3e-7   1.2e-5   5.6e-7
  width2           1.6e-6   1.8e-5   1.0e-6  | in32_f32         1.7e-6   1.9e-5   1.0e-6
  width3           1.6e-6   2.7e-5   1.5e-6  | in48_f32_w2      1.7e-6   1.8e-5   1.1e-6
  factor1          2.6e-6   3.1e-5   1.7e-6  | old_3cam         1.5e-6   9.8e-6   1.7e-6
  factor3          2.4e-6   3.2e-5   1.4e-6  | old_one_cam      2.7e-6   3.3e-5   1.7e-6
  keep1            1.6e-6   2.8e-5   1.5e-6  | old_4cam_d2_w2   2.3e-6   2.0e-5   1.3e-6
  keep2            2.6e-6   1.9e-5   1.3e-6  | composed width2  2.8e-6   1.8e-5   2.2e-6
  keep12           1.1e-6   1.6e-5   7.5e-7  | composed width1  2.6e-6   1.8e-5   2.1e-6
  final2           1.5e-6   2.2e-5   1.2e-6  | composed relu    1.6e-6   1.3e-5   1.3e-6
  relu             1.1e-6   1.9e-5   1.3e-6  |
In 'f32' mode the largest ratio of the measured error to the reference's own fp32 error (`err32`) is 1.73 (keep2 at S2)."""
import os

import numpy as np
import pytest
import torch

import guard_arena
import parity_log
import topology_cases as T
from golden_cases import SMALL_CASES
from mvs_gi_amd import dropin, hip_ops as H, synth
from mvs_gi_amd.dropin import cost_volume_regulator as cr
from mvs_gi_amd.dropin.torch_only import build_and_regulate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["f32", "bf16x3", "f16x3"]
SPLIT_MODES = ["bf16x3", "f16x3"]
BAR = {"f32": 1e-4, "bf16x3": 1e-3, "f16x3": 1e-3}
TWO_SPLITS_BAR = 5e-4


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor the library allocates during a test of this module sits between NaN-sentinel guards, and unwritten
    fp32 outputs read as NaN (tests/guard_arena.py: what is guarded, guard sizes, exemptions)."""
    yield from guard_arena.fixture_body(request)


@pytest.fixture(autouse=True)
def _restore_mode():
    old = H.get_conv_mode()
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)
    yield
    H.set_conv_mode(old)
    torch.cuda.synchronize()
    H.saturation_flags(clear=True)


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {f: np.load(os.path.join(golden_dir, f + ".npz")) for f in T.FILES}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _module(name):
    case = T.CASES[name]
    reg = T.make_module(dropin, case)
    T.load_drawn(reg, case["seed"])
    return reg.eval().to(DEV)


def _input(name, sname, reg):
    return torch.from_numpy(T.make_input(T.CASES[name], sname, reg.in_chs)).to(DEV)


def _run(reg, x):
    """module(x) -> numpy [B, final_chs, D, H, W], with the checks every run gets: dtype, no NaN (the arena pre-fills outputs, so
    an element no kernel stored reads as NaN), range flags 0."""
    with torch.no_grad():
        y = reg(x)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.shape[:2] == (x.shape[0], reg.final_chs)
    got = y.contiguous().cpu().numpy()
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} of {got.size} output elements are NaN (unwritten?)"
    assert H.saturation_flags() == 0
    return got


def _check(tag, mode, got, z, prefix):
    ref, err32 = z[prefix + "costs"], float(z[prefix + "err32"])
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = _rel(got, ref)
    print(f"topology {tag} [{mode}]: costs max-rel {err:.3e}  reference fp32 err32 {err32:.3e}  ratio {err / err32:.2f}")
    parity_log.record(f"topology:{tag}", mode, 1.0, err, float(np.abs(got - ref).mean() / np.abs(ref).mean()), "golden")
    assert err <= BAR[mode], (tag, mode, err)
    return err


def _rs_levels(reg):
    return [i for i, b in enumerate(reg.down_blks) if "_mvsgi_rs_bufs" in b.__dict__]


# ---- a. as shipped ------------------------------------------------------------------------------------------------------
# The register-stationary chain serves a level whose first conv is (multiple of 16) -> 32 channels with 32 -> 32 residual convs
# behind it (cost_volume_regulator._rs_chain), in the split modes only
def _rs_expected(name, mode):
    if mode == "f32":
        return []
    reg = T.make_module(dropin, T.CASES[name])
    out = []
    for i, b in enumerate(reg.down_blks):
        c = b.first.conv_layer
        if c.in_channels % 16 == 0 and c.out_channels == 32 and len(b.blks) > 0:
            out.append(i)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sname", ["S1", "S2"])
@pytest.mark.parametrize("name", list(T.CASES))
def test_as_shipped_vs_reference_golden(goldens, name, sname, mode):
    H.set_conv_mode(mode)
    reg = _module(name)
    got = _run(reg, _input(name, sname, reg))
    _check(f"{name}/{sname}", mode, got, goldens["topology"], f"{name}/{sname}/")
    assert _rs_levels(reg) == _rs_expected(name, mode)
    assert "_mvsgi_poly_bufs" not in reg.__dict__            # the polyphase tail waits for _POLY_MIN_UNITS bricks


# ---- b. fast routes forced ----------------------------------------------------------------------------------------------
RS_LEVELS = {"default": [0], "width2": [0], "width3": [0], "relu": [0], "linear": [0], "final2": [0], "depth2": [0], "depth4": [0],
             "old_one_cam": [0], "keep1": [0, 1], "factor1": [0, 1, 2], "keep12": [0, 1, 2]}


@pytest.mark.parametrize("mode", SPLIT_MODES)
@pytest.mark.parametrize("name", T.ROUTE_CASES)
def test_fast_routes_forced_vs_golden_and_streaming(goldens, monkeypatch, name, mode):
    """S3: level 0 is (8, 4, 32).  With the polyphase tail's and the Winograd form's pay-off thresholds out of the way every fast
    route the predicates allow runs; then the same module with every layer on the streaming kernels."""
    H.set_conv_mode(mode)
    monkeypatch.setattr(cr, "_POLY_MIN_UNITS", 0)
    monkeypatch.setattr(cr, "_wino_pays", lambda *a, **k: True)
    for switch in ("_USE_POLY", "_USE_RS", "_USE_WINO"):
        monkeypatch.setattr(cr, switch, True)
    wino_calls = []
    real_wino = H.conv3d_wino

    def spy(x, *a, **k):
        wino_calls.append(tuple(x.shape))
        return real_wino(x, *a, **k)
    monkeypatch.setattr(H, "conv3d_wino", spy)

    reg = _module(name)
    x = _input(name, "S3", reg)
    fast = _run(reg, x)
    _check(f"{name}/S3(fast)", mode, fast, goldens["topology_routes"], f"{name}/S3/")
    B, (D, Hh, W) = T.BATCH, T.S3
    assert _rs_levels(reg) == RS_LEVELS[name]
    poly = reg.__dict__.get("_mvsgi_poly_bufs", {})
    assert (B, D // 2, Hh // 2, W // 2, x.device) in poly            # the last up block wrote the polyphase layer's split-padded input
    has_head = any(len(k) > 4 and k[4] == "hi" for k in poly)
    assert has_head == (name != "final2")          # final_chs = 2: out_costs.0 writes fp32 and the exact head reads it
    width = len(reg.down_blks[0].blks) + 1
    if mode == "f16x3":
        assert len(wino_calls) == 2 * (width - 1) and all(s == (B, D // 2, Hh // 2, W // 2, 32) for s in wino_calls)
    else:
        assert not wino_calls
    print(f"topology routes {name} [{mode}]: rs levels {_rs_levels(reg)} poly tail {bool(poly)} split head {has_head} "
          f"winograd launches {len(wino_calls)}")

    monkeypatch.setattr(cr, "_USE_RS", False)
    monkeypatch.setattr(cr, "_USE_POLY", False)
    n_wino = len(wino_calls)
    slow = _run(reg, x)
    assert len(wino_calls) == n_wino
    _check(f"{name}/S3(streaming)", mode, slow, goldens["topology_routes"], f"{name}/S3/")
    two = _rel(fast, slow)
    print(f"topology routes {name} [{mode}]: fast vs streaming {two:.3e}")
    assert two <= TWO_SPLITS_BAR, two


# ---- c. hand-over -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def composed_inputs():
    base = SMALL_CASES["std_d8"]
    inp = synth.make_inputs(base["cfg"], seed=base["seed"], batch=T.COMPOSED_BATCH, grid_kind=base["grid_kind"],
                            grid_mask_dtype=base["grid_mask_dtype"])
    return base["cfg"], inp


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(T.COMPOSED))
def test_builder_to_regulator_hand_over(goldens, composed_inputs, name, mode):
    H.set_conv_mode(mode)
    cfg, inp = composed_inputs
    z = goldens["topology"]
    assert synth.digest(inp) == str(z["composed/inputs_sha256"])
    case = T.COMPOSED[name]
    cvb = dropin.SphericalSweepStdMasked(**T.builder_kwargs(case, cfg))
    reg = dropin.UNetCostVolumeRegulatorBase(**case["kwargs"])
    T.load_drawn(cvb, case["seed"] + T.BUILDER_SEED_OFFSET)
    T.load_drawn(reg, case["seed"])
    cvb, reg = cvb.eval().to(DEV), reg.eval().to(DEV)
    args = [torch.from_numpy(inp[k]).to(DEV) for k in ("feats", "grids", "grid_masks", "masks")]
    B, D, (Ho, Wo) = T.COMPOSED_BATCH, cfg.num_cands, cfg.cv_hw

    takes = reg.takes_split((B, D, Ho, Wo, 16))
    assert takes == (mode != "f32" and name != "width1")
    with torch.no_grad():
        vol = cvb(*args)
    assert isinstance(vol, torch.Tensor) and vol.dtype == torch.float32 and tuple(vol.shape) == (B, 16, D, Ho, Wo)
    apart = _run(reg, vol)
    _check(f"composed {name}: reg(cvb())", mode, apart, z, f"composed/{name}/")
    assert "_mvsgi_rs_x0" not in cvb.__dict__            # the tensor interface makes no hand-over buffer
    with torch.no_grad():
        y = build_and_regulate(cvb, reg, *args)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and H.saturation_flags() == 0
    joined = y.contiguous().cpu().numpy()
    assert not np.isnan(joined).any()
    _check(f"composed {name}: build_and_regulate", mode, joined, z, f"composed/{name}/")
    # the split-padded hand-over buffer (post_vol's output, module-owned by the builder) exists exactly where the regulator takes it
    assert ("_mvsgi_rs_x0" in cvb.__dict__) == takes
    if mode == "f32":
        assert "_mvsgi_rs_vol" not in cvb.__dict__ and _rs_levels(reg) == []
    if not takes:
        assert np.array_equal(joined, apart)             # the same launches both ways


# ---- d. one module, two shapes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["keep12", "depth4"])
def test_one_module_two_shapes(goldens, name):
    """The module-owned buffers and launch caches are keyed by shape: S1, S2, S1 again through one module object -- at levels
    that never own buffers in the default topology -- and the third result is the first, bit for bit."""
    mode = "bf16x3"
    H.set_conv_mode(mode)
    reg = _module(name)
    x1, x2 = _input(name, "S1", reg), _input(name, "S2", reg)
    first = _run(reg, x1).copy()
    second = _run(reg, x2).copy()
    third = _run(reg, x1)
    _check(f"{name}/S1(1st)", mode, first, goldens["topology"], f"{name}/S1/")
    _check(f"{name}/S2(2nd)", mode, second, goldens["topology"], f"{name}/S2/")
    assert np.array_equal(third, first)
    for i in _rs_levels(reg):
        assert len(reg.down_blks[i].__dict__["_mvsgi_rs_bufs"]) == 2          # one entry per shape
