"""GPU (MI355X): the volumetric fusion (csrc/tsdf.hip, dropin.TsdfVolume) -- the integrated volume bit for bit against the composition
it is defined by (TsdfVolume.integrate_chain: the voxel centres through the transform and equirectangular grid kernels, then torch)
AND against the numpy restatement of tests/tsdf_cases.py; the ray-cast bit for bit against raycast_chain and the restatement, on
volumes the device itself integrated and on hand-made ones whose crossing is exact; every subset of the outputs between guard
bands; independence of the batch and of the run; a captured step replayed with staged poses; reset; the pipeline stage; the
semantic case against the bar derived in tests/tsdf_cases.py.  Every test runs with guarded allocations (tests/guard_arena.py).

What is compared how, and why:
  the cell of a voxel   numpy's atan2 is not the device's.  Every test prints how far the two grids are apart and asserts that the
                        restatement's cell (numpy) is the chain's (the device's grid kernel) for every voxel that reaches step 3: no
                        voxel of a case sits within their difference of a cell's edge.
  r                     the device's root against RN_fp32(sqrt(float64(r2))) of the restatement's r2 bits: bar 1 ulp.
  everything behind r   bit for bit against the chain and the restatement FED THE DEVICE'S r (torch's root stands in for the
                        correctly rounded one in the chain); the differences with torch's own root are printed, not asserted.
Every figure is printed by the tests."""
import itertools

import numpy as np
import pytest
import torch

import grid_exact_cases as GE
import guard_arena
import tsdf_cases as TC
from mvs_gi_amd import dropin, hip_ops as H
from mvs_gi_amd.dropin import sweep_grids as SG
from mvs_gi_amd.pipeline import InferencePipeline
from oracle import grid_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# which optional inputs go with which scroll: every combination of std and mask is run on every (case, pose, bf)
OPTIONAL = {"same": (True, True), "one": (True, False), "three": (False, False), "all": (False, True)}


@pytest.fixture(autouse=True)
def arena(request):
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


def _reprojector(hw, ranges, bf):
    return dropin.Reprojector([SG.EquirectangularSampleGridMaker()], [torch.eye(4, dtype=torch.float64)], hw, ranges[0], ranges[1], bf=bf,
                              device=DEV)


def _volume(name, bf=96.0, **kw):
    c = TC.CASES[name]
    kw.setdefault("trunc", TC.PARAMS["trunc"])
    kw.setdefault("w_max", TC.PARAMS["w_max"])
    kw.setdefault("r_range", TC.PARAMS["r_range"])
    kw.setdefault("w_min", TC.PARAMS["w_min"])
    return dropin.TsdfVolume(_reprojector(c["hw"], c["ranges"], bf), c["dims"], TC.VOXEL, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want) -> bool:
    got = _np(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = _np(want) if isinstance(want, torch.Tensor) else np.asarray(want)
    return GE.same_bits(got, want)


def _ulps(got, want, where):
    if not where.any():
        return 0
    return int(np.abs(got[where].view(np.int32).astype(np.int64) - want[where].view(np.int32).astype(np.int64)).max())


def _differ(a, b) -> int:
    a, b = _np(a), _np(b)
    return int((~(np.isnan(a) & np.isnan(b)) & (a != b)).sum())


def _raycast_all_ways(v, label, B):
    """The ray-cast of the volume v holds, from the staged pose: the device, the chain and the restatement -> the device's dict"""
    bufs = v.buffers(B)
    got = {k: t.clone() for k, t in v.raycast(B=B).items()}
    assert tuple(got) == H.TSDF_OUTPUTS and got["steps"].dtype == torch.int32
    chain = v.raycast_chain(bufs["vol"])
    rest = TC.raycast(_np(bufs["vol"]), _np(v.reprojector.rays), _np(bufs["P"]), _np(bufs["origin_prev"]), v.voxel, v.t0, v.step, v.K, v.w_min,
                      v.reprojector.bf)
    for k in H.TSDF_OUTPUTS:
        assert _same(got[k], chain[k]), f"{label}: raycast {k} differs from the chain in {_differ(got[k], chain[k])} pixels"
        assert _same(got[k], rest[k]), f"{label}: raycast {k} differs from the restatement in {_differ(got[k], rest[k])} pixels"
    return got


# ------------------------------------------------------------------------------ 1. the bits of the definition
@pytest.mark.parametrize("bf", TC.BFS)
@pytest.mark.parametrize("kind", TC.POSES)
@pytest.mark.parametrize("name", list(TC.CASES))
def test_volume_and_raycast_are_the_bits_of_the_chains_and_the_restatement(arena, name, kind, bf):
    c = TC.CASES[name]
    B = c["B"]
    v = _volume(name, bf)
    inp = TC.make_inputs(name, bf)
    d = {k: arena.guarded(torch.from_numpy(a).to(DEV)) for k, a in inp.items()}
    P = TC.poses(kind, name)
    v.set_pose(torch.from_numpy(P))
    bufs = v.buffers(B)
    T, origin = _np(bufs["T"]), _np(bufs["origin"])
    assert np.array_equal(origin, TC.origin_of(P, c["dims"])) and np.allclose(T, TC.rigid_inverse(P), atol=1e-6)
    aff = TC.affine(c["ranges"], c["hw"])
    par = TC.params(bf)
    r_out = arena.alloc(tuple(bufs["vol"].shape[:4]), torch.float32, DEV)
    crossings = 0
    for shift, (with_std, with_mask) in OPTIONAL.items():
        label = f"{name} {kind} bf {bf:g} scroll {shift}"
        prev = TC.shifted(origin, shift, c["dims"])
        bufs["origin_prev"].copy_(torch.from_numpy(prev))
        bufs["vol"].copy_(d["vol"])
        std, mask = (d["std"] if with_std else None), (d["mask"] if with_mask else None)
        ins = [(t, arena.snapshot(t)) for t in (d["inv"], d["std"], d["mask"])]
        got = v.integrate(d["inv"], std=std, mask=mask, r_out=r_out).clone()
        assert torch.equal(bufs["origin_prev"], bufs["origin"])
        rest = TC.integrate(inp["vol"], inp["inv"], inp["std"] if with_std else None, inp["mask"] if with_mask else None, T, origin, prev, par,
                            aff, r=_np(r_out))
        # r: 1 ulp from the correctly rounded root of the restatement's own r2 bits; 0 where r2 is rejected
        r_dev = _np(r_out)
        worst = _ulps(r_dev, TC.exact_root(rest["r2"]), rest["near"])
        assert worst <= 1 and (r_dev[~rest["near"]] == 0).all(), (label, worst)
        with arena.paused():
            fed = v.integrate_chain(d["vol"], d["inv"], std, mask, origin_prev=torch.from_numpy(prev), r=r_out)
            own = v.integrate_chain(d["vol"], d["inv"], std, mask, origin_prev=torch.from_numpy(prev))
        # the cell: numpy's atan2 against the device's; no voxel sits within their difference of a cell's edge
        reach = rest["near"] & (r_dev >= np.float32(par["r_range"][0])) & (r_dev <= np.float32(par["r_range"][1]))
        assert np.array_equal(_np(fed["cx"])[reach], rest["cx"][reach]) and np.array_equal(_np(fed["cy"])[reach], rest["cy"][reach]), label
        assert np.array_equal(_np(fed["hit"]), rest["hit"]), label
        assert _same(got, fed["vol"]), f"{label}: vol differs from the chain in {_differ(got, fed['vol'])} values"
        assert _same(got, rest["vol"]), f"{label}: vol differs from the restatement in {_differ(got, rest['vol'])} values"
        print(f"[tsdf] {label}: {int(rest['hit'].sum())} of {rest['hit'].size} voxels updated, {int(rest['fresh'].sum())} fresh; r at most {worst} ulp "
              f"from the correctly rounded root (bar 1); with torch's own root {_differ(got, own['vol'])} values of vol and "
              f"{_differ(r_out, own['r'].where(torch.from_numpy(rest['near']).to(DEV), torch.zeros_like(own['r'])))} of r differ")
        for t, snap in ins:
            assert arena.unchanged(t, snap)
        with arena.paused():
            cast = _raycast_all_ways(v, label, B)
        crossings += int((cast["steps"] < v.K).sum())
    if name != "line":
        assert crossings > 0, name


def test_hand_made_planes_cross_exactly(arena):
    """f = (3.5 - ix) / 4 along x, w = 2: the crossing between voxel 3 and voxel 4 is at a dyadic place, so t* is exact -- on a map
    whose rows are a multiple of four pixels and on one with a row tail, for two sequences with different poses."""
    dims, voxel, bf = (8, 4, 4), 0.25, 96.0
    for hw in ((1, 4), (3, 5)):
        rays = np.zeros((3,) + hw, np.float32)
        rays[0] = 1
        P = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
        P[0, :3, 3], P[1, :3, 3] = [0.125, 0.5, 0.5], [0.375, 0.25, 0.75]
        vol = TC.plane_volume(dims, B=2)
        org = np.zeros((2, 3), np.int32)
        dv = {k: arena.guarded(torch.from_numpy(a).to(DEV)) for k, a in dict(vol=vol, rays=rays, P=P, org=org).items()}
        got = H.tsdf_raycast(dv["vol"], dv["rays"], dv["P"], dv["org"], bf, voxel, 0.25, 0.125, 12)
        rest = TC.raycast(vol, rays, P, org, voxel, 0.25, 0.125, 12, 1.0, bf)
        for k in H.TSDF_OUTPUTS:
            assert _same(got[k], rest[k]), (hw, k)
        assert (_np(got["steps"])[0] == 5).all() and (_np(got["steps"])[1] == 3).all() and (_np(got["weight"]) == 2).all()
        assert np.array_equal(_np(got["inv"])[0], np.full(hw, np.float32(bf) / np.float32(0.8125)))
        assert np.array_equal(_np(got["inv"])[1], np.full(hw, np.float32(bf) / np.float32(0.5625)))


def test_hand_made_planes_on_two_frames_of_two_blocks(arena):
    """The same planes on maps of 270 and 300 quads (two blocks per frame, the second partly empty; the 16-byte form and a row tail)
    for two sequences: the thread's frame and quad come from csrc/panorama_map.hpp's frame_quad.  Every third ray is half as long,
    so neighbours in a quad stop at different steps; every pixel of both frames crosses."""
    dims, voxel, bf, K = (8, 4, 4), 0.25, 96.0, 24
    for hw in ((30, 36), (30, 38)):
        i, j = np.meshgrid(np.arange(hw[0]), np.arange(hw[1]), indexing="ij")
        half = (i * hw[1] + j) % 3 == 0
        rays = np.zeros((3,) + hw, np.float32)
        rays[0] = np.where(half, np.float32(0.5), np.float32(1))
        P = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
        P[0, :3, 3], P[1, :3, 3] = [0.125, 0.5, 0.5], [0.375, 0.25, 0.75]
        vol = TC.plane_volume(dims, B=2)
        org = np.zeros((2, 3), np.int32)
        dv = {k: arena.guarded(torch.from_numpy(a).to(DEV)) for k, a in dict(vol=vol, rays=rays, P=P, org=org).items()}
        got = H.tsdf_raycast(dv["vol"], dv["rays"], dv["P"], dv["org"], bf, voxel, 0.25, 0.125, K, w_min=1.0)
        rest = TC.raycast(vol, rays, P, org, voxel, 0.25, 0.125, K, 1.0, bf)
        for k in H.TSDF_OUTPUTS:
            assert _same(got[k], rest[k]), (hw, k)
        steps = _np(got["steps"])
        assert np.array_equal(steps[0], np.where(half, 12, 5)) and np.array_equal(steps[1], np.where(half, 8, 3)), hw
        assert (_np(got["weight"]) == 2).all(), hw


# ------------------------------------------------------------------------------ 2. structure
def test_every_subset_of_the_outputs_and_poisoned_tensors(arena):
    name = "b2"
    v = _volume(name)
    inp = TC.make_inputs(name)
    P = torch.from_numpy(TC.poses("rigid", name))
    v.integrate(torch.from_numpy(inp["inv"]).to(DEV), P=P)
    v.integrate(torch.from_numpy(inp["inv"]).to(DEV))
    bufs = v.buffers(2)
    rays = arena.guarded(v.reprojector.rays)
    vol, pose, org = arena.guarded(bufs["vol"]), arena.guarded(bufs["P"]), arena.guarded(bufs["origin_prev"])
    snaps = [(t, arena.snapshot(t)) for t in (vol, rays, pose, org)]
    args = (vol, rays, pose, org, v.reprojector.bf, v.voxel, v.t0, v.step, v.K)
    full = H.tsdf_raycast(*args)
    assert tuple(full) == H.TSDF_OUTPUTS and int((full["steps"] < v.K).sum()) > 0
    shape = tuple(full["inv"].shape)
    sentinel8 = torch.tensor(guard_arena.SENTINEL_BYTES, dtype=torch.uint8, device=DEV)
    for n in range(1, 4):
        for sub in itertools.combinations(H.TSDF_OUTPUTS, n):
            spare = {k: arena.alloc(shape, full[k].dtype, DEV) for k in H.TSDF_OUTPUTS}
            res = H.tsdf_raycast(*args, want=sub, out=spare)
            assert tuple(res) == sub
            for k in H.TSDF_OUTPUTS:
                raw = spare[k].view(-1).view(torch.uint8)
                if k in sub:
                    assert res[k] is spare[k] and torch.equal(raw, full[k].view(-1).view(torch.uint8)), (sub, k)
                else:
                    assert torch.equal(raw, sentinel8.repeat(-(-raw.numel() // 4))[:raw.numel()]), f"{k} was written although it is not wanted ({sub})"
    torch.cuda.synchronize()
    for t, snap in snaps:
        assert arena.unchanged(t, snap)
    # the optional range output changes nothing in the volume
    a, b = vol.clone(), vol.clone()
    inv = torch.from_numpy(inp["inv"]).to(DEV)
    r_out = arena.alloc(tuple(vol.shape[:4]), torch.float32, DEV)
    aff = v.affine
    H.tsdf_integrate(a, inv, bufs["T"], bufs["origin"], bufs["origin_prev"], 96.0, aff, v.voxel, v.trunc, v.w_max, v.r_range)
    H.tsdf_integrate(b, inv, bufs["T"], bufs["origin"], bufs["origin_prev"], 96.0, aff, v.voxel, v.trunc, v.w_max, v.r_range, r_out=r_out)
    assert _same(a, b) and not bool(torch.isnan(r_out).any())


def test_sequences_do_not_depend_on_the_batch_and_runs_repeat(arena):
    name = "b3"
    inp = TC.make_inputs(name)
    d = {k: torch.from_numpy(a).to(DEV) for k, a in inp.items()}
    P = torch.from_numpy(TC.poses("rigid", name))
    runs = []
    for _ in range(2):
        v = _volume(name)
        v.buffers(3)["vol"].copy_(d["vol"])
        vol = v.integrate(d["inv"], d["std"], d["mask"], P=P).clone()
        runs.append(dict({k: t.clone() for k, t in v.raycast(B=3).items()}, vol=vol))
    for k in runs[0]:
        assert _same(runs[0][k], runs[1][k]), k
    for b in range(3):
        v = _volume(name)
        v.buffers(1)["vol"].copy_(d["vol"][b:b + 1])
        vol = v.integrate(d["inv"][b:b + 1], d["std"][b:b + 1], d["mask"][b:b + 1], P=P[b:b + 1])
        assert _same(vol[0], runs[0]["vol"][b]), b
        for k, t in v.raycast(B=1).items():
            assert _same(t[0], runs[0][k][b]), (k, b)


@pytest.mark.parametrize("name", ["odd", "b2"])
def test_a_captured_step_replays_three_poses(arena, name):
    """Integrate and ray-cast captured once (poses and origins are read from device memory), replayed three times with set_pose and a
    fresh measurement: the bits of three eager steps, the volume scrolling along."""
    c = TC.CASES[name]
    B = c["B"]
    inp = TC.make_inputs(name)
    inv, std = torch.from_numpy(inp["inv"]).to(DEV), torch.from_numpy(inp["std"]).to(DEV)
    v, twin = _volume(name), _volume(name)
    static_inv = inv.clone()

    def step():
        v.integrate(static_inv, std)
        return v.raycast(B=B)
    step()                                                                 # makes the buffers (eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out = step()
    v.reset(), twin.buffers(B)
    v.buffers(B)["origin_prev"].copy_(twin.buffers(B)["origin_prev"])
    at = {k: t.data_ptr() for k, t in v.buffers(B).items() if isinstance(t, torch.Tensor)}
    scrolled = 0
    for n, kind in enumerate(("shift", "rigid", "yaw")):
        P = torch.from_numpy(TC.poses(kind, name))
        cur = inv * (1.0 + 0.01 * n)
        with arena.paused():
            before = twin.buffers(B)["origin_prev"].clone()
            twin.integrate(cur, std, P=P)
            want = {k: t.clone() for k, t in twin.raycast(B=B).items()}
            scrolled += int((before != twin.buffers(B)["origin_prev"]).any())
        v.set_pose(P)
        static_inv.copy_(cur)
        g.replay()
        torch.cuda.synchronize()
        assert _same(v.buffers(B)["vol"], twin.buffers(B)["vol"]), (n, kind)
        for k in H.TSDF_OUTPUTS:
            assert _same(out[k], want[k]), (n, kind, k)
    assert scrolled >= 2 and int((v.buffers(B)["vol"][..., 1] > 1).sum()) > 0
    assert {k: t.data_ptr() for k, t in v.buffers(B).items() if isinstance(t, torch.Tensor)} == at


def test_reset_empties_the_volume(arena):
    name = "odd"
    v = _volume(name)
    inp = TC.make_inputs(name)
    inv = torch.from_numpy(inp["inv"]).to(DEV)
    fresh = v.raycast(B=1)
    assert bool((fresh["steps"] == v.K).all()) and bool((fresh["inv"] == 0).all()) and bool((fresh["weight"] == 0).all())
    v.integrate(inv, P=torch.from_numpy(TC.poses("shift", name)))
    first = v.buffers(1)["vol"].clone()
    assert int((first[..., 1] > 0).sum()) > 0
    v.reset()
    vol = v.buffers(1)["vol"]
    assert bool((vol[..., 0] == 1).all()) and bool((vol[..., 1] == 0).all())
    assert _same(v.integrate(inv), first)                                 # the same first step again


# ------------------------------------------------------------------------------ 3. the pipeline stage
def test_pipeline_with_and_without_the_tsdf_stage(arena, monkeypatch):
    from test_gpu_reproject import _tiny_rig
    H.set_conv_mode("f32")
    cfg, w, inp, samplers, (img_a, img_b), rig = _tiny_rig(False)
    rp = dropin.Reprojector(rig.grid_makers, G.ring_poses(3), rig.out_shape, TC.FULL[0], TC.FULL[1], bf=1.0, device=DEV)
    called = []
    real = H._call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(H, "_call", spy)
    new = ["mvsgi_tsdf_integrate_f32", "mvsgi_tsdf_raycast_f32"]
    plain = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=("spread",))
    want_a = plain.forward_device(img_a).clone()
    spread_a = plain.confidence["spread"].clone()
    calls_plain = list(called)
    called.clear()
    none = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=("spread",), tsdf=None)
    assert torch.equal(none.forward_device(img_a), want_a) and torch.equal(none.confidence["spread"], spread_a)
    assert called == calls_plain and not set(new) & set(called) and none.tsdf is None and plain.tsdf is None and none.tsdf_stage is None
    want_b = plain.forward_device(img_b).clone()
    spread_b = plain.confidence["spread"].clone()
    called.clear()
    # the surfaces of this rig's prediction are bf / inv ~ metres away: a volume of 24^3 voxels of 0.5 m around the rig
    kw = dict(dims=(24, 20, 24), voxel=0.5, march=(0.5, 6.0, None))
    stage, twin = dropin.TsdfVolume(rp, **kw), dropin.TsdfVolume(rp, **kw)
    pipe = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=("spread",), tsdf=stage)
    assert pipe.tsdf is None and pipe.tsdf_stage is stage
    P = torch.from_numpy(TC.pose("shift", "odd"))

    def check(inv, expect_inv, spread):
        assert torch.equal(inv, expect_inv)                               # inv_dist: the bits of a pipeline without the stage
        with arena.paused():
            twin.integrate(expect_inv, std=spread)
            want = twin.raycast(B=1)
        assert tuple(pipe.tsdf) == H.TSDF_OUTPUTS
        for k in H.TSDF_OUTPUTS:
            assert _same(pipe.tsdf[k], want[k]), k
        assert _same(stage.buffers(1)["vol"], twin.buffers(1)["vol"])
        return int((want["steps"] < twin.K).sum())
    inv = pipe.forward_device(img_a)
    assert called[-2:] == new and called[:-2] == calls_plain              # the stage is the last one; everything before it is what it was
    check(inv, want_a, spread_a)
    stage.set_pose(P), twin.set_pose(P)
    check(pipe.forward_device(img_b), want_b, spread_b)
    static = {k: t.data_ptr() for k, t in pipe.tsdf.items()}
    pipe.capture(img_a)                                                   # runs the stage on its warm-up frames, then resets it
    twin.reset()
    eye = torch.eye(4)
    stage.set_pose(eye), twin.set_pose(eye)
    check(pipe.replay(img_a), want_a, spread_a)
    assert {k: t.data_ptr() for k, t in pipe.tsdf.items()} == static      # made by the first call, never replaced
    stage.set_pose(P), twin.set_pose(P)
    check(pipe.replay(img_b), want_b, spread_b)
    n = check(pipe.replay(img_b), want_b, spread_b)
    print(f"[tsdf] pipeline: {n} of {want_b.numel()} pixels of the ray-cast hit a surface after three frames")
    with pytest.raises(ValueError):
        InferencePipeline(cfg, w, inp, device=DEV, tsdf=stage)
    with pytest.raises(ValueError):
        InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, tsdf=dropin.TsdfVolume(_reprojector(rig.out_shape, TC.FULL, 1.0), **kw))


# ------------------------------------------------------------------------------ 4. the semantic case
def test_the_sphere_on_the_device_meets_the_derived_bar(arena):
    s = TC.SPHERE
    rp = _reprojector(s["hw"], TC.FULL, s["bf"])
    v = dropin.TsdfVolume(rp, s["dims"], s["voxel"], trunc=s["trunc"], march=(s["t0"], s["t_max"], s["step"]))
    assert v.K == TC.sphere_K()
    rays = _np(rp.rays)
    for a in s["views"]:
        d = TC.sphere_distance(a, rays).astype(np.float32)
        v.integrate(torch.from_numpy((np.float32(s["bf"]) / d)[None]).to(DEV), P=torch.from_numpy(TC.sphere_pose(a)))
    got = v.raycast(P=torch.from_numpy(TC.sphere_pose(s["cast"])))
    inv, steps = _np(got["inv"]).astype(np.float64), _np(got["steps"])
    miss = steps >= v.K
    true = TC.sphere_distance(s["cast"], rays)[None]
    err = np.abs(s["bf"] / inv[~miss] - true[~miss])
    bar, vx = TC.sphere_bar(), s["voxel"]
    print(f"[tsdf] sphere on the device: {int(miss.sum())} of {miss.size} pixels miss; |t* - t_true| worst {err.max() / vx:.3f} voxel, median "
          f"{np.median(err) / vx:.3f} voxel; bar {bar / vx:.3f} voxel")
    assert not miss.any()
    assert err.max() <= bar
