"""GPU (MI355X): the confidence maps of the soft-argmin's softmax (csrc/confidence.hip, hip_ops.confidence) against the float64
reference and the per-element bounds of tests/confidence_cases.py, and through every module that exposes them.  Every tensor
the library allocates sits between guard bands and is pre-filled with a NaN sentinel (tests/guard_arena.py); inputs are copied
into guarded arenas of their own.

Shapes (B, D, H, W): (2,16,7,13) (1,33,6,10) (1,16,3,130) (2,5,5,9) (1,48,2,132) (1,1,2,3), and (1,24,3,9): D = 1, 5 and 16 take
the register form for D <= 16, D = 24 the one for D <= 32 (none of the other shapes reaches it), D = 33 and 48 the multi-pass form;
W = 130 / 132 at x4 gives more than one block in x; H = 2 / 3 exercises the border clamps.  Factors 1, 2, 4, 3, 1.5, 0.75;
post_div 1 and 96, and the normalised entropy, on (2,16,7,13).
"""
import gc
import os

import numpy as np
import pytest
import torch

import confidence_cases as CC
import guard_arena
import softargmin_cases as SC
from mvs_gi_amd import hip_ops as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}                     # factor -> {map: largest error / bound}, printed by the last test
SECOND_REGISTER_FORM = (1, 24, 3, 9)      # 16 < D <= 32


@pytest.fixture(autouse=True)
def arena(request):
    yield from guard_arena.fixture_body(request)


def _g(arena, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return arena.guarded(t)


def _np(out):
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in out.items()}


def _run(arena, c, s, post_div=1.0, normalize=False, want=CC.MAPS):
    return _np(H.confidence(_g(arena, c.costs), _g(arena, c.inv_idx), s, want, post_div=post_div, normalize_entropy=normalize))


def _bits(a, b):
    return all(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)) for n in a)


# ------------------------------------------------------------------------------ 1. tolerance regime
TOL = [(sh, s) for sh in CC.SHAPES + [SECOND_REGISTER_FORM] for s in CC.FACTORS]


@pytest.mark.parametrize("shape,s", TOL, ids=[f"{'x'.join(map(str, sh))}-x{s:g}" for sh, s in TOL])
def test_tolerance_regime(arena, shape, s):
    for sigma in CC.SIGMAS:
        for pd in ((1.0, 96.0) if shape == CC.POST_DIV_SHAPE else (1.0,)):
            for norm in ((False, True) if (shape == CC.POST_DIV_SHAPE and pd == 1.0) else (False,)):
                t = CC.tol_case(shape, s, sigma, pd, norm)
                got = _run(arena, t, s, pd, norm)
                r = CC.check_maps(f"{shape} x{s:g} sigma {sigma:g} / {pd:g}{' normalised' if norm else ''}", t.ref, got)
                print(f"{shape} x{s:g} sigma {sigma:g} / {pd:g} norm {norm}: error / bound " +
                      " ".join(f"{n} {r[n]:.3f}" for n in CC.FLOAT_MAPS) + f", ambiguous argmax {r['argmax']:.4f}")
                w = RATIOS.setdefault(s, dict.fromkeys(CC.MAPS, 0.0))
                for n in CC.MAPS:
                    w[n] = max(w[n], r[n])


# ------------------------------------------------------------------------------ 2. exact regime
@pytest.mark.parametrize("shape,s", CC.exact_rows(), ids=[f"{'x'.join(map(str, sh))}-x{s}" for sh, s in CC.exact_rows()])
def test_exact_regime(arena, shape, s):
    c = CC.exact_case(shape, s)
    CC.check_exact(f"{shape} x{s}", c, _run(arena, c, s))


# ------------------------------------------------------------------------------ 3. goldens from the reference
@pytest.mark.parametrize("shape,s", CC.GOLDEN_ROWS, ids=[CC.golden_name(sh, s)[:-4] for sh, s in CC.GOLDEN_ROWS])
def test_reference_goldens(arena, shape, s):
    costs, inv_idx, z, ref, gb = CC.golden_case(shape, s)
    got = _np(H.confidence(_g(arena, costs), _g(arena, inv_idx), s))
    CC.check_maps(f"golden {shape} x{s}", ref, got)
    CC.check_against_golden(f"golden {shape} x{s}", z, ref, gb, got, own_bounds=True)


# ------------------------------------------------------------------------------ 4. non-finite costs
@pytest.mark.parametrize("s,shape,kind", CC.NONFINITE, ids=[f"x{s}-{'x'.join(map(str, sh))}-{k}" for s, sh, k in CC.NONFINITE])
def test_nonfinite_costs(arena, s, shape, kind):
    """NaN / +inf in one candidate or every candidate -inf at one interior pixel: the three float maps are NaN and argmax is -1
    exactly at the outputs that blend it under a non-zero weight, everything else is finite and inside the bounds.  One -inf
    candidate: p = 0 exactly, bounds over the finite candidates."""
    c = CC.nonfinite_case(shape, s, kind)
    got = _run(arena, c, s)
    CC.check_maps(f"{kind} {shape} x{s}", c.ref, got)
    if kind == "-inf":
        assert not np.isnan(got["max_prob"]).any() and (got["argmax"] >= 0).all()


# ------------------------------------------------------------------------------ 5. selection
@pytest.mark.parametrize("shape,s", [((2, 16, 7, 13), 2), ((1, 33, 6, 10), 1.5)])
def test_selection_gives_the_same_bits_and_leaves_the_rest_alone(arena, shape, s):
    t = CC.tol_case(shape, s, 4.0)
    c, w = _g(arena, t.costs), _g(arena, t.inv_idx)
    full = H.confidence(c, w, s)
    oshape = tuple(full["max_prob"].shape)
    for want in [(n,) for n in CC.MAPS] + [("spread", "argmax")]:
        out = {n: arena.alloc(oshape, torch.int32 if n == "argmax" else torch.float32, DEV) for n in CC.MAPS}
        ptrs = {n: out[n].data_ptr() for n in out}
        got = H.confidence(c, w, s, want=want, out=out)
        torch.cuda.synchronize()
        assert tuple(got) == want and all(got[n].data_ptr() == ptrs[n] for n in want)
        for n in CC.MAPS:
            if n in want:
                assert torch.equal(got[n].view(torch.int32), full[n].view(torch.int32)), (want, n)
            else:
                assert bool((out[n].view(torch.int32) == guard_arena.SENTINEL).all()), f"want {want}: {n} was written"
    # without `out` only the wanted maps exist
    assert tuple(H.confidence(c, w, s, want=("entropy",))) == ("entropy",)


# ------------------------------------------------------------------------------ 6. batch independence and determinism
@pytest.mark.parametrize("shape,s", [((2, 16, 7, 13), 4), ((2, 5, 5, 9), 0.75), ((2, 24, 3, 9), 3)])
def test_batch_independence_and_determinism(arena, shape, s):
    costs = SC.gauss_costs(shape, 4.0)
    w = _g(arena, SC.stock_candidates(shape[1]))
    c = _g(arena, costs)
    both = H.confidence(c, w, s)
    again = H.confidence(c, w, s)
    assert _bits(both, again)
    for b in range(shape[0]):
        one = H.confidence(_g(arena, costs[b:b + 1]), w, s)
        assert _bits({n: t[b:b + 1].contiguous() for n, t in both.items()}, one), b


# ------------------------------------------------------------------------------ 7. consistency with the path
@pytest.mark.parametrize("shape,s", [((2, 16, 7, 13), 2), ((1, 48, 2, 132), 4), ((1, 33, 6, 10), 1.5)])
def test_consistent_with_the_soft_argmin(arena, shape, s):
    """inv_idx[argmax] lies among the candidates, and |inv_dist - inv_idx[argmax]| <= spread sqrt(1 / max_prob): by Chebyshev on
    the winner's mass, P(|w - mu| >= |w_k - mu|) >= p_k = max_prob, so |w_k - mu| sqrt(max_prob) <= sigma.  Allowance: the
    spread's absolute bound (which holds the expectation's own error, mu x_inv)."""
    for sigma in CC.SIGMAS:
        t = CC.tol_case(shape, s, sigma)
        c, w = _g(arena, t.costs), _g(arena, t.inv_idx)
        got = _np(H.confidence(c, w, s))
        inv, _ = H.softargmin(c, w, s, False)
        inv = inv.cpu().numpy().astype(np.float64)
        wk = t.inv_idx.astype(np.float64)[got["argmax"]]
        assert (got["argmax"] >= 0).all() and (got["argmax"] < shape[1]).all()
        assert wk.min() >= float(t.inv_idx.min()) and wk.max() <= float(t.inv_idx.max())
        lhs = np.abs(inv - wk)
        rhs = got["spread"].astype(np.float64) * np.sqrt(1.0 / got["max_prob"].astype(np.float64)) * (1 + 2.0 ** -10) + t.ref.b_spread
        assert (lhs <= rhs).all(), f"{shape} x{s} sigma {sigma}: exceeded by {float((lhs - rhs).max()):.3e}"


# ------------------------------------------------------------------------------ 8. frame bases beyond 2^31 elements
@pytest.fixture
def big():
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def test_large_offsets(arena, big):
    """costs [B, 16, 64, 256] whose last frames start beyond 2^31 elements: the first, second to last and last frame equal
    one-frame launches."""
    D, Hh, W = 16, 64, 256
    B = (1 << 31) // (D * Hh * W) + 3
    g = torch.Generator(device=DEV).manual_seed(31)
    costs = torch.randn((B, D, Hh, W), device=DEV, generator=g)
    costs.mul_(4.0)
    assert (B - 1) * D * Hh * W > (1 << 31)
    w = _g(arena, SC.stock_candidates(D))
    out = H.confidence(costs, w, 1)
    for b in (0, B - 2, B - 1):
        one = H.confidence(costs[b:b + 1].clone(), w, 1)
        assert not bool(torch.isnan(one["entropy"]).any())
        assert _bits({n: t[b:b + 1].contiguous() for n, t in out.items()}, one), b
    print(f"[large-offset] confidence B={B}: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ------------------------------------------------------------------------------ 9. through the modules
def _tiny_cfg():
    from mvs_gi_amd.configs import CONFIGS, DIST_8L
    return CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32), dist_cands=DIST_8L)


def test_regressor_confidence_dropin(arena):
    from mvs_gi_amd import dropin
    shape, s = (2, 16, 7, 13), 4
    costs = _g(arena, SC.gauss_costs(shape, 4.0)[:, None])               # [B, 1, D, H, W]
    cands = [float(v) for v in np.geomspace(0.5, 100.0, shape[1])]
    dr = dropin.DistanceRegressorWithFixedCandidates(bf=96.0, dist_cands=cands, interp_scale_factor=s, pre_interp=True).to(DEV)
    dr.post_div = 96.0
    direct = H.confidence(costs[:, 0], dr.inv_dist_idx, s, post_div=96.0)
    assert _bits(dr.confidence(costs), direct)
    assert tuple(dr.confidence(costs, want=("spread",))) == ("spread",)
    dr.pre_interp = False                                                # forward does not interpolate then, nor does this
    assert _bits(dr.confidence(costs), H.confidence(costs[:, 0], dr.inv_dist_idx, 1, post_div=96.0))
    inv, _ = dr(costs)
    assert tuple(inv.shape) == tuple(dr.confidence(costs)["argmax"].shape)


def test_regressor_confidence_on_an_unpickled_reference_regressor(arena, golden_dir, request):
    import mvs_gi_amd
    assert mvs_gi_amd.install() in ("alias", "patch")
    request.addfinalizer(mvs_gi_amd.dropin.uninstall)       # the host tests of install() start from a process without the aliases
    hp = torch.load(os.path.join(golden_dir, "pickled_modules_tiny.pt"), weights_only=False)["hyper_parameters"]
    z = np.load(os.path.join(golden_dir, "pickled_modules_tiny_io.npz"))
    dr = hp["dist_regressor"].eval().to(DEV)
    costs = _g(arena, z["costs"])
    scale = dr.interp_scale_factor if (dr.pre_interp and dr.interp_scale_factor > 0) else 1
    got = dr.confidence(costs)
    assert _bits(got, H.confidence(costs[:, 0], dr.inv_dist_idx, scale))
    inv, _ = dr(costs)
    assert tuple(got["max_prob"].shape) == tuple(inv.shape) and bool(torch.isfinite(got["spread"]).all())


def test_hot_path_confidence_eager(arena):
    from mvs_gi_amd import synth
    from mvs_gi_amd.dropin.torch_only import build_and_regulate
    from mvs_gi_amd.pipeline import HotPath
    cfg = _tiny_cfg()
    inp, w = synth.make_inputs(cfg, seed=11, batch=1), synth.make_weights(cfg, seed=11)
    feats = torch.from_numpy(inp["feats"]).to(DEV)
    plain = HotPath(cfg, w, inp, device=DEV)
    assert plain.confidence is None
    inv0, _ = plain(feats)
    assert plain.confidence is None
    hp = HotPath(cfg, w, inp, device=DEV, confidence=("max_prob", "entropy", "spread", "argmax"))
    inv, _ = hp(feats)
    assert torch.equal(inv.view(torch.int32), inv0.view(torch.int32)), "inv_dist changed with confidence maps switched on"
    with torch.no_grad():
        costs = build_and_regulate(hp.cv_builder, hp.cv_regulator, feats, hp.grids, hp.grid_masks, hp.masks)
        direct = hp.dist_regressor.confidence(costs)
    assert tuple(hp.confidence) == CC.MAPS and _bits(hp.confidence, direct)
    first = {n: t.data_ptr() for n, t in hp.confidence.items()}
    hp(feats)
    assert {n: t.data_ptr() for n, t in hp.confidence.items()} == first, "the maps are allocated once per batch shape"
    with pytest.raises(ValueError):
        HotPath(cfg, w, inp, device=DEV, confidence=("max_prob", "nope"))


def test_inference_pipeline_confidence_captured_and_replayed(arena):
    from mvs_gi_amd import synth
    from mvs_gi_amd.dropin.torch_only import build_and_regulate
    from mvs_gi_amd.pipeline import InferencePipeline
    cfg = _tiny_cfg()
    seed = 8
    w = synth.make_weights(cfg, seed=seed)
    w["feature_extractor"] = synth.make_extractor_weights(seed)
    inp = synth.make_inputs(cfg, seed=seed, batch=1)
    rng = np.random.default_rng(seed)
    imgs = [torch.from_numpy(rng.integers(0, 256, (cfg.num_cams, 64, 256, 3), dtype=np.uint8)).to(DEV) for _ in range(2)]
    plain = InferencePipeline(cfg, w, inp, device=DEV)
    pipe = InferencePipeline(cfg, w, inp, device=DEV, confidence=CC.MAPS)

    def direct(im):
        with torch.no_grad():
            f = pipe.feature_extractor(im)
            hot = pipe.hot
            costs = build_and_regulate(hot.cv_builder, hot.cv_regulator, f.unsqueeze(0), hot.grids, hot.grid_masks, hot.masks)
            return {n: t.clone() for n, t in hot.dist_regressor.confidence(costs).items()}
    want = [direct(im) for im in imgs]
    inv_plain = [plain.forward_device(im).clone() for im in imgs]
    eager = pipe.forward_device(imgs[0])
    assert torch.equal(eager.view(torch.int32), inv_plain[0].view(torch.int32)) and _bits(pipe.confidence, want[0])
    pipe.capture(imgs[0])
    static = {n: t.data_ptr() for n, t in pipe.confidence.items()}
    for i in (1, 0):
        inv = pipe.replay(imgs[i])
        torch.cuda.synchronize()
        assert torch.equal(inv.view(torch.int32), inv_plain[i].view(torch.int32)), "inv_dist differs from the pipeline without confidence"
        assert _bits(pipe.confidence, want[i]), f"replay of image set {i}"
        assert {n: t.data_ptr() for n, t in pipe.confidence.items()} == static
    # spread is in the unit of the returned map: inv_dist / bf
    assert float(pipe.confidence["spread"].max()) <= (max(1.0 / d for d in cfg.dist_cands) - min(1.0 / d for d in cfg.dist_cands))


def test_error_over_bound_report():
    for s, r in sorted(RATIOS.items()):
        print(f"x{s:g}: largest error / bound " + " ".join(f"{n} {r[n]:.3f}" for n in CC.FLOAT_MAPS) + f", ambiguous argmax {r['argmax']:.4f}")
    assert all(r[n] <= 1.0 for r in RATIOS.values() for n in CC.FLOAT_MAPS)
