"""GPU (MI355X): the packed point cloud (csrc/cloud.hip, hip_ops.pack_cloud, dropin.CloudPacker) -- bit for bit against the
composition it is defined by (Reprojector.point_cloud for xyz, torch comparisons for the predicate, a torch first-valid gather
for the colour, nonzero for the compaction), on values nobody should pass, under a capacity, with every tensor between guard
bands, beyond 2^31 output elements, run twice, captured and replayed, and as the last stage of InferencePipeline.  Every test runs
with guarded allocations (tests/guard_arena.py): outputs start as the NaN sentinel, so a row that must not be written is seen."""
import gc
import math

import numpy as np
import pytest
import torch

import cloud_cases as CC
import guard_arena
import reproject_cases as RC
from mvs_gi_amd import dropin, hip_ops as H, synth
from mvs_gi_amd.configs import CONFIGS
from mvs_gi_amd.dropin import sweep_grids as SG
from mvs_gi_amd.pipeline import InferencePipeline
from oracle import grid_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = guard_arena.SENTINEL


@pytest.fixture(autouse=True)
def arena(request):
    """The guarded allocator of tests/guard_arena.py, as in every GPU module; the tests here also carve their inputs from it."""
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


# ------------------------------------------------------------------------------ helpers
def _on_device(arena, case) -> dict:
    """The numpy case with every array in a guarded device allocation (bodies 16-byte aligned and not more)."""
    def g(a):
        return arena.guarded(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    t = dict(case)
    t["inv"], t["rays"] = g(case["inv"]), g(case["rays"])
    t["mask"] = None if case["mask"] is None else g(case["mask"])
    t["gates"] = [(g(p), lo, hi) for p, lo, hi in case["gates"]]
    t["attrs"] = [g(a) for a in case["attrs"]]
    t["warped"] = None if case["warped"] is None else g(case["warped"])
    t["valid"] = None if case["valid"] is None else g(case["valid"])
    return t


def _inputs(t) -> list:
    return [x for x in [t["inv"], t["rays"], t["mask"], t["warped"], t["valid"]] + [p for p, _, _ in t["gates"]] + t["attrs"] if x is not None]


def _reprojector(t) -> dropin.Reprojector:
    """One equirectangular camera at the origin: only its ray table (the case's) and bf matter to point_cloud()."""
    return dropin.Reprojector([SG.EquirectangularSampleGridMaker()], [np.eye(4)], (t["H"], t["W"]), bf=t["bf"], rays=t["rays"], device=DEV)


def _composition(t):
    """The definition, executed with what the project already has -> (points per frame, index per frame, counts [B, 2]).
    Synchronises (nonzero), allocates, cannot be captured: what pack_cloud() replaces."""
    inv = t["inv"]
    B, Hh, W = inv.shape
    xyz = _reprojector(t).point_cloud(inv)                                                 # the existing kernel's bits
    d = torch.full_like(inv, t["bf"]) / inv                                                # the IEEE division of reproject_chain
    i, j = torch.arange(Hh, device=DEV)[:, None], torch.arange(W, device=DEV)[None]
    keep = ((i % t["step"][0] == 0) & (j % t["step"][1] == 0)).expand(B, Hh, W).clone()
    if t["mask"] is not None:
        keep &= (t["mask"] != 0).expand(B, Hh, W)
    keep &= torch.isfinite(d) & (d >= t["d_range"][0]) & (d <= t["d_range"][1])
    for plane, lo, hi in t["gates"]:
        keep &= (plane >= lo) & (plane <= hi)
    parts = [xyz]
    if t["warped"] is not None:
        valid, warped = t["valid"], t["warped"]
        N, C = warped.shape[1], warped.shape[2]
        first = (valid.to(torch.int32).cumsum(dim=1) == 0).sum(dim=1).clamp(max=N - 1)     # cameras before the first valid one
        col = warped.gather(1, first[:, None, None].expand(B, 1, C, Hh, W))[:, 0]
        parts.append(torch.where(valid.any(dim=1)[:, None], col, torch.full_like(col, t["no_colour"])))
        if t["require_colour"]:
            keep &= valid.any(dim=1)
    parts += [a[:, None] for a in t["attrs"]]
    rec = torch.cat(parts, dim=1).permute(0, 2, 3, 1).reshape(B, Hh * W, -1)
    points, index, counts = [], [], torch.zeros((B, 2), dtype=torch.int32)
    for b in range(B):
        idx = keep[b].reshape(-1).nonzero()[:, 0]
        counts[b, 0], counts[b, 1] = min(idx.numel(), t["capacity"]), idx.numel()
        idx = idx[:t["capacity"]]
        points.append(rec[b][idx].contiguous())
        index.append(idx.to(torch.int32))
    return points, index, counts


def _kwargs(t) -> dict:
    return dict(d_range=t["d_range"], gates=t["gates"], mask=t["mask"], step=t["step"], warped=t["warped"], valid=t["valid"],
                require_colour=t["require_colour"], no_colour=t["no_colour"], attrs=t["attrs"], capacity=t["capacity"], want_index=True)


def _width(t) -> int:
    return 3 + (0 if t["warped"] is None else t["warped"].shape[2]) + len(t["attrs"])


def _outputs(arena, t) -> dict:
    """Caller-owned outputs, pre-filled with the sentinel."""
    B, cap = t["B"], t["capacity"]
    return dict(points=arena.alloc((B, cap, _width(t)), torch.float32, DEV), counts=arena.alloc((B, 2), torch.int32, DEV),
                index=arena.alloc((B, cap), torch.int32, DEV))


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def _assert_equals(got, want, what=""):
    """counts, and per frame points[:written] and index[:written], as int32 bit patterns; every row behind written still holds
    the sentinel the outputs were allocated with."""
    points, index, counts = want
    got_counts = got["counts"].cpu()
    assert got_counts.dtype == torch.int32 and torch.equal(got_counts, counts), (what, got_counts.tolist(), counts.tolist())
    for b in range(counts.shape[0]):
        n = int(counts[b, 0])
        assert torch.equal(_bits(got["points"][b, :n]), _bits(points[b])), (what, b, "points")
        assert bool((_bits(got["points"][b, n:]) == SENTINEL).all()), (what, b, "a row behind `written` was written")
        if "index" in got:
            assert got["index"].dtype == torch.int32 and torch.equal(got["index"][b, :n], index[b]), (what, b, "index")
            assert bool((got["index"][b, n:] == SENTINEL).all()), (what, b, "an index behind `written` was written")


def _run_and_check(arena, case, check_numpy=True):
    t = _on_device(arena, case)
    snaps = [(x, arena.snapshot(x)) for x in _inputs(t)]
    with arena.paused():
        want = _composition(t)
    if check_numpy:                                                      # the torch composition is the numpy definition
        assert np.array_equal(want[2].numpy(), CC.pack_reference(case)[2])
    out = _outputs(arena, t)
    ws = H.cloud_ws(t["B"], t["H"], t["W"], DEV)                         # guarded as well: its bands are checked at teardown
    got = H.pack_cloud(t["inv"], t["rays"], t["bf"], ws=ws, out=out, **_kwargs(t))
    torch.cuda.synchronize()                                             # no HIP error
    assert all(got[k] is out[k] for k in out)
    _assert_equals(got, want)
    for x, snap in snaps:
        assert arena.unchanged(x, snap), "an input or its guard band was written"
    return t, got, want


def _pattern_case(shape, pattern, via, bf=96.0):
    """A keep pattern realised through one clause of the predicate: the mask, a gate, or the distance."""
    B, Hh, W = shape
    keep = CC.keep_pattern(pattern, B, Hh, W)
    case = CC.make_case(B, Hh, W, seed=5, bf=bf, A=1)
    if via == "mask":
        case["mask"] = keep
    elif via == "gate":
        case["gates"] = [(np.where(keep, 1.0, np.where(np.arange(Hh * W).reshape(Hh, W) % 2 == 0, np.nan, 2.0)).astype(np.float32), 0.5, 1.5)]
    else:
        case["inv"] = np.where(keep, case["inv"], 0.0).astype(np.float32)
    return case, keep


# ------------------------------------------------------------------------------ 1. the bits of the composition
def _pattern_params():
    k = 0
    for shape in CC.SHAPES:
        for pattern in CC.PATTERNS:
            if CC.pattern_exists(pattern, *shape):
                yield pytest.param(shape, pattern, ("mask", "gate", "inv")[k % 3], id=f"{shape[0]}x{shape[1]}x{shape[2]}-{pattern}")
                k += 1


@pytest.mark.parametrize("shape,pattern,via", list(_pattern_params()))
def test_keep_patterns_are_the_bits_of_the_composition(arena, shape, pattern, via):
    case, keep = _pattern_case(shape, pattern, via)
    t, got, want = _run_and_check(arena, case)
    kept = want[2][:, 1]
    assert kept.tolist() == keep.reshape(shape[0], -1).sum(axis=1).tolist()
    HW = shape[1] * shape[2]
    if pattern in CC.BERNOULLI:
        assert bool(((kept > 0) & (kept < HW)).all())
    for b in range(shape[0]):
        assert got["index"][b, :int(kept[b])].cpu().tolist() == np.flatnonzero(keep[b]).tolist()


@pytest.mark.parametrize("shape", CC.VARIANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", list(CC.VARIANTS))
def test_variants_are_the_bits_of_the_composition(arena, name, shape):
    """0 / 1 / 4 gates, mask [H, W] / [B, H, W] / none, step (1, 1) / (2, 3), C in {0, 3} with three cameras, A in {0, 2}, a record
    of 16 floats, bf 96 / 1, a distance range.  The result read out by to_host is the numpy definition's, bit for bit."""
    case = CC.make_case(*shape, **CC.VARIANTS[name])
    t, got, want = _run_and_check(arena, case)
    ref_points, _, ref_counts = CC.pack_reference(case)
    host = dropin.CloudPacker.to_host(got)
    assert name != "record16" or host[0].shape[1] == H.CLOUD_MAX_RECORD
    for b in range(shape[0]):
        assert 0 < ref_counts[b, 1] and CC.same_bits(host[b], ref_points[b])
    # without index, and with the library's own (guarded, sentinel-filled) outputs and workspace
    kw = dict(_kwargs(t), want_index=False)
    lib_made = H.pack_cloud(t["inv"], t["rays"], t["bf"], **kw)
    assert set(lib_made) == {"points", "counts"}
    _assert_equals(lib_made, want)


def test_variants_on_the_many_tile_shape(arena):
    case = CC.make_case(1, 129, 2049, **CC.VARIANTS["colour_required"])
    _run_and_check(arena, case)


# ------------------------------------------------------------------------------ 2. values nobody should pass
@pytest.mark.parametrize("require_colour", [False, True])
@pytest.mark.parametrize("bf", [96.0, 1.0])
def test_values_nobody_should_pass(arena, bf, require_colour):
    B, Hh, W = 2, 33, 65
    case = CC.make_case(B, Hh, W, seed=7, bf=bf, n_gates=1, C=3, A=1, require_colour=require_colour, no_colour=-7.5)
    clean_keep = CC.keep_reference(case).reshape(B, -1)
    bad = np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan], np.float32)
    pos = np.random.default_rng(7).permutation(Hh * W)[:5 * len(bad)]
    poked, nan_gate = pos[:4 * len(bad)], pos[4 * len(bad):]
    for b in range(B):
        case["inv"][b].reshape(-1)[poked] = np.tile(bad, 4)
        case["gates"][0][0][b].reshape(-1)[nan_gate] = np.nan
    t, got, want = _run_and_check(arena, case)
    counts = got["counts"].cpu().numpy()
    none_valid = ~case["valid"].any(axis=1).reshape(B, -1)
    for b in range(B):
        idx = got["index"][b, :counts[b, 0]].cpu().numpy()
        assert not np.isin(pos, idx).any()                               # every poked pixel is dropped
        expect = clean_keep[b].copy()
        expect[pos] = False
        assert np.array_equal(idx, np.flatnonzero(expect))               # and nothing else changed: the neighbours are unaffected
        pts = got["points"][b, :counts[b, 0]].cpu().numpy()
        assert np.isfinite(pts).all()
        if require_colour:
            assert not none_valid[b][idx].any()
        else:
            assert none_valid[b][idx].any() and (pts[none_valid[b][idx], 3:6] == np.float32(-7.5)).all()
            assert (pts[~none_valid[b][idx], 3:6] != np.float32(-7.5)).all()


# ------------------------------------------------------------------------------ 3. capacity
@pytest.mark.parametrize("order", ["overflow_last", "overflow_first"])
def test_capacity(arena, order):
    """One frame keeps fewer points than the capacity, the other more: the first `capacity` are written, counts = (capacity, kept),
    the short frame's tail keeps the sentinel, and the bands behind the last row are clean (teardown)."""
    B, Hh, W = 2, 33, 65
    case = CC.make_case(B, Hh, W, seed=9, C=3, A=2)
    rng = np.random.default_rng(9)
    p = (0.3, 0.7) if order == "overflow_last" else (0.7, 0.3)
    case["mask"] = np.stack([rng.random((Hh, W)) < p[0], rng.random((Hh, W)) < p[1]])
    kept = CC.keep_reference(case).reshape(B, -1).sum(axis=1)
    for cap in (int(kept.min() + kept.max()) // 2, int(kept.min()), int(kept.min()) // 2, 1):
        case["capacity"] = cap
        t, got, want = _run_and_check(arena, case)
        assert got["counts"].cpu().tolist() == [[min(int(k), cap), int(k)] for k in kept]
    assert kept.min() < (kept.min() + kept.max()) // 2 < kept.max()


# ------------------------------------------------------------------------------ 4. address safety
@pytest.mark.parametrize("shape", CC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_address_safety(arena, shape):
    """Every input, output and the workspace between guard bands, bodies aligned to 16 bytes and not more, everything kept (the most
    stores) and nothing kept (no store at all): inputs and bands intact, the outputs' and the workspace's bands checked at teardown."""
    for pattern in ("all", "none"):
        case = CC.make_case(*shape, seed=5, C=3, A=1)
        case["mask"] = CC.keep_pattern(pattern, *shape)
        t, got, _ = _run_and_check(arena, case)
        for x in _inputs(t) + list(got.values()):
            assert x.data_ptr() % 16 == 0 and x.data_ptr() % 32 != 0
        n = int(got["counts"][0, 0])
        assert n == (shape[1] * shape[2] if pattern == "all" else 0)
        assert not bool((_bits(got["points"][:, :n]) == SENTINEL).any())


# ------------------------------------------------------------------------------ 5. beyond 2^31 output elements
@pytest.fixture
def big():
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def test_large_offsets_cloud(arena, big):
    """points [B][64 * 256][8] beyond 2^31 elements: the first and the last two frames equal the composition."""
    Hh, W, C, A, N = 64, 256, 3, 2, 1
    R = 3 + C + A
    B = (1 << 31) // (Hh * W * R) + 3
    g = torch.Generator(device=DEV).manual_seed(9)
    inv = RC.BF / torch.exp(torch.rand((B, Hh, W), device=DEV, generator=g) * float(np.log(200.0)) + float(np.log(0.5)))
    gate = torch.rand((B, Hh, W), device=DEV, generator=g)
    attrs = [torch.rand((B, Hh, W), device=DEV, generator=g) for _ in range(A)]
    warped = torch.rand((B, N, C, Hh, W), device=DEV, generator=g)
    valid = torch.rand((B, N, Hh, W), device=DEV, generator=g) < 0.7
    rays = torch.from_numpy(CC.unit_rays(Hh, W)).to(DEV)
    t = dict(B=B, H=Hh, W=W, bf=RC.BF, inv=inv, rays=rays, mask=None, gates=[(gate, 0.0, 0.5)], attrs=attrs, warped=warped, valid=valid,
             require_colour=False, no_colour=-2.0, step=(1, 1), d_range=H.CLOUD_D_RANGE, capacity=Hh * W)
    got = H.pack_cloud(inv, rays, RC.BF, **_kwargs(t))                    # outputs and workspace from the guarded allocator
    assert got["points"].numel() >= (1 << 31) + 2 * Hh * W * R
    counts = got["counts"].cpu()
    for b in (0, B - 2, B - 1):
        one = dict(t, B=1, inv=inv[b:b + 1].clone(), gates=[(gate[b:b + 1].clone(), 0.0, 0.5)], attrs=[a[b:b + 1].clone() for a in attrs],
                   warped=warped[b:b + 1].clone(), valid=valid[b:b + 1].clone())
        with arena.paused():
            want = _composition(one)
        _assert_equals({k: v[b:b + 1] for k, v in got.items()}, want, what=f"frame {b}")
        assert 0.4 < int(counts[b, 1]) / (Hh * W) < 0.6
    print(f"[large-offset] cloud B={B}: peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ------------------------------------------------------------------------------ 6. determinism and capture
def test_two_runs_give_the_same_bits_and_a_captured_call_replays(arena, monkeypatch):
    shape = (2, 33, 65)
    case = CC.make_case(*shape, **CC.VARIANTS["colour_attrs"])
    t = _on_device(arena, case)
    ws = H.cloud_ws(*shape, DEV)
    outs = [_outputs(arena, t) for _ in range(3)]
    first = H.pack_cloud(t["inv"], t["rays"], t["bf"], ws=ws, out=outs[0], **_kwargs(t))
    with monkeypatch.context() as m:                                     # the second call at a shape allocates nothing
        made = []
        real = torch.empty
        m.setattr(torch, "empty", lambda *a, **k: made.append(a) or real(*a, **k))
        second = H.pack_cloud(t["inv"], t["rays"], t["bf"], ws=ws, out=outs[1], **_kwargs(t))
        assert not made
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(second[k])), k          # sentinel tails included
    with arena.paused():
        want_a = _composition(t)
        other = dict(t, inv=torch.from_numpy(CC.positive_inv(*shape, t["bf"], seed=77)).to(DEV))
        other["inv"][:, 5] = 0.0                                         # and another keep pattern
        want_b = _composition(other)
    assert want_a[2].tolist() != want_b[2].tolist()
    static_inv = t["inv"].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        H.pack_cloud(static_inv, t["rays"], t["bf"], ws=ws, out=outs[2], **_kwargs(t))
    for inv, want in ((other["inv"], want_b), (t["inv"], want_a)):
        for o in outs[2].values():
            o.view(torch.int32).fill_(SENTINEL)
        static_inv.copy_(inv)
        graph.replay()
        torch.cuda.synchronize()
        _assert_equals(outs[2], want)


def test_packer_owns_its_buffers_and_allocates_once(arena, monkeypatch):
    shape = (2, 33, 65)
    case = CC.make_case(*shape, **CC.VARIANTS["colour_attrs"])
    t = _on_device(arena, case)
    conf = dict(max_prob=t["gates"][0][0], entropy=t["gates"][1][0], spread=t["attrs"][0].unsqueeze(1))
    packer = dropin.CloudPacker(_reprojector(t), gates={"max_prob": (0.1, 0.9), "entropy": (0.1, 0.9)}, attrs=("spread",), want_index=True)
    one = dict(t, gates=t["gates"][:2], attrs=t["attrs"][:1])
    with arena.paused():
        want = _composition(one)
    a = packer.pack(t["inv"].unsqueeze(1), confidence=conf, warped=t["warped"], valid=t["valid"])
    _assert_equals(a, want)
    with monkeypatch.context() as m:
        made = []
        real = torch.empty
        m.setattr(torch, "empty", lambda *x, **k: made.append(x) or real(*x, **k))
        b = packer.pack(t["inv"], confidence=conf, warped=t["warped"], valid=t["valid"])
        assert not made
    assert all(a[k] is b[k] for k in a) and packer.channels == 3 and packer.record_width() == 7
    _assert_equals(b, want)
    host = packer.to_host(b)
    assert [h.shape for h in host] == [(int(n), 7) for n in want[2][:, 0]]
    with pytest.raises(ValueError, match="channels"):
        packer.pack(t["inv"], confidence=conf, warped=t["warped"][:, :, :2].contiguous(), valid=t["valid"])


# ------------------------------------------------------------------------------ 7. the pipeline
def _makers(n):
    return [SG.EquirectangularSampleGridMaker() if k % 2 else SG.DoubleSphereSampleGridMaker(RC.DS_PARAMS, RC.DS_CALIB) for k in range(n)]


def _tiny_rig():
    """extractor_small's geometry (the rig of tests/test_gpu_reproject.py): 64 x 256 views, 16 x 64 output, three cameras."""
    cfg = CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32))
    w = synth.make_weights(cfg, seed=21)
    w["feature_extractor"] = synth.make_extractor_weights(21)
    inp = synth.make_inputs(cfg, seed=21, batch=1)
    rng = np.random.default_rng(22)
    imgs = [torch.from_numpy(rng.integers(0, 256, (3, 64, 256, 3), dtype=np.uint8)).to(DEV) for _ in range(2)]
    rp = dropin.Reprojector(_makers(3), G.ring_poses(3), (16, 64), RC.LON, RC.LAT, bf=1.0, device=DEV)
    return cfg, w, inp, imgs, rp


def test_pipeline_with_cloud(arena):
    H.set_conv_mode("f32")
    cfg, w, inp, (img_a, img_b), rp = _tiny_rig()
    maps = ("max_prob", "spread")
    plain = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=maps)
    want_inv = plain.forward_device(img_a).clone()
    # thresholds from the frame itself, so that the gates keep some pixels and drop some
    lo = float(plain.confidence["max_prob"].median())
    hi = float(plain.confidence["spread"].quantile(0.9))
    settings = dict(gates={"max_prob": (lo, math.inf), "spread": (-math.inf, hi)}, attrs=("max_prob",), want_index=True)
    packer, twin = dropin.CloudPacker(rp, **settings), dropin.CloudPacker(rp, **settings)
    pipe = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=maps, cloud=packer)
    assert pipe.cloud is None and plain.cloud is None

    def check(inv, expect_inv):
        assert torch.equal(inv, expect_inv)                              # inv_dist: the bits of a pipeline without the stage
        xyz, warped, valid = pipe.reprojection
        want = twin.pack(inv, confidence=pipe.confidence, warped=warped, valid=valid)
        counts = want["counts"].cpu()
        assert torch.equal(pipe.cloud["counts"].cpu(), counts) and 0 < int(counts[0, 1]) < 16 * 64 and int(counts[0, 0]) == int(counts[0, 1])
        n = int(counts[0, 0])
        assert tuple(pipe.cloud["points"].shape) == (1, 16 * 64, 7)
        assert torch.equal(_bits(pipe.cloud["points"][0, :n]), _bits(want["points"][0, :n]))
        assert torch.equal(pipe.cloud["index"][0, :n], want["index"][0, :n])
        # the records are the pipeline's own maps at the kept pixels
        idx = pipe.cloud["index"][0, :n].long()
        assert torch.equal(pipe.cloud["points"][0, :n, :3], xyz[0].reshape(3, -1)[:, idx].t())
        assert torch.equal(pipe.cloud["points"][0, :n, 6], pipe.confidence["max_prob"].reshape(-1)[idx])
        return n
    n_a = check(pipe.forward_device(img_a), want_inv)
    static = {k: v.data_ptr() for k, v in pipe.cloud.items()}
    pipe.capture(img_a)
    assert check(pipe.replay(img_a), want_inv) == n_a
    assert {k: v.data_ptr() for k, v in pipe.cloud.items()} == static     # the packer's buffers were never replaced
    other_inv = plain.forward_device(img_b).clone()
    assert not torch.equal(other_inv, want_inv)
    check(pipe.replay(img_b), other_inv)
    assert check(pipe.replay(img_a), want_inv) == n_a


def test_pipeline_without_cloud_launches_no_cloud_kernel(arena, monkeypatch):
    """cloud=None is the path as it was: the new symbol is not called; with a packer it is the last call of a frame."""
    H.set_conv_mode("f32")
    cfg, w, inp, (img_a, _), rp = _tiny_rig()
    called = []
    real = H._call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(H, "_call", spy)
    InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=("max_prob",)).forward_device(img_a)
    assert called and "mvsgi_cloud_pack_f32" not in called
    called.clear()
    packer = dropin.CloudPacker(rp, attrs=("max_prob",), colour=False)
    InferencePipeline(cfg, w, inp, device=DEV, confidence=("max_prob",), cloud=packer).forward_device(img_a)
    assert called.count("mvsgi_cloud_pack_f32") == 1 and called[-1] == "mvsgi_cloud_pack_f32" and "mvsgi_reproject_f32" not in called
