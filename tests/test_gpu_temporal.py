"""GPU (MI355X): the temporal fusion (csrc/temporal.hip, dropin.TemporalFusion) -- the keyed z-buffer bit for bit against the
composition it is defined by (TemporalFusion.splat_chain: Reprojector.reproject()'s xyz, the transform and equirectangular grid
kernels, torch's scatter_reduce(amin) on int64 keys) AND against the numpy restatement of tests/temporal_cases.py; the prior's
inverse distance against the correctly rounded value of the device's own r2; everything behind it bit for bit against the fuse of
the chain fed the device's own prior; independence of the batch and of the run; a captured step replayed with staged poses; reset;
every output between guard bands; the pipeline stage.  Every test runs with guarded allocations (tests/guard_arena.py).

Measured on one MI355X (every figure is printed by the tests):
  zkey                  the chain's and the restatement's bits on all 40 (case, pose, bf) and on the collapse at 48 x 100
  warped_inv            at most 1 ulp from RN_fp32(bf / sqrt(float64(r2))) (bar 2: a root within 1 ulp, then one division)
  warped_var, fused, var, age    the bits of the chain's fuse and of the restatement's, fed the device's warped_inv and src
  end to end (torch's own root in the chain)   0 elements differ in any output; the gate's decision agrees on every pixel outside
                        the margin, which leaves out 0 pixels of every case (bar 1 %)"""
import itertools

import numpy as np
import pytest
import torch

import grid_exact_cases as GE
import guard_arena
import temporal_cases as TC
from mvs_gi_amd import dropin, hip_ops as H
from mvs_gi_amd.dropin import sweep_grids as SG
from mvs_gi_amd.pipeline import InferencePipeline
from oracle import grid_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BEHIND = ("warped_var", "fused", "var", "age")


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


def _fusion(name, bf=96.0, **kw):
    c = TC.CASES[name]
    rp = dropin.Reprojector([SG.EquirectangularSampleGridMaker()], [torch.eye(4, dtype=torch.float64)], c["hw"], c["ranges"][0], c["ranges"][1],
                            bf=bf, device=DEV)
    kw.setdefault("gate", TC.GATE)
    kw.setdefault("q_var", TC.Q_VAR)
    return dropin.TemporalFusion(rp, **kw)


def _dev(arena, inp):
    return {k: arena.guarded(torch.from_numpy(v).to(DEV)) for k, v in inp.items()}


def _load(tf, d):
    """The evaluator's own state := the case's"""
    bufs = tf.buffers(d["prev_inv"].shape[0], DEV)
    bufs["inv"].copy_(d["prev_inv"]), bufs["var"].copy_(d["prev_var"]), bufs["age"].copy_(d["prev_age"])
    return bufs


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want) -> bool:
    """bit for bit; any NaN equals any NaN (grid_exact_cases.same_bits)"""
    got = _np(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = _np(want) if isinstance(want, torch.Tensor) else np.asarray(want)
    return GE.same_bits(got, want)


def _ulps(got, want, where):
    if not where.any():
        return 0
    return int(np.abs(got[where].view(np.int32).astype(np.int64) - want[where].view(np.int32).astype(np.int64)).max())


def _check_step(arena, tf, name, bf, T, label):
    """One step of a seeded case with the poses T, every output against the chain and the restatement."""
    inp = TC.make_inputs(name, bf)
    d = _dev(arena, inp)
    state = (d["prev_inv"], d["prev_var"], d["prev_age"])
    _load(tf, d)
    with arena.paused():
        z_chain = tf.splat_chain(d["prev_inv"], d["prev_age"], torch.from_numpy(T))
    got = {k: v.clone() for k, v in tf.step(d["cur_inv"], d["cur_std"], T=torch.from_numpy(T), want=tf.OUTPUTS).items()}
    assert tuple(got) == tf.OUTPUTS and got["age"].dtype == torch.uint8 and got["src"].dtype == torch.int32 and got["zkey"].dtype == torch.int64
    # 1. the keyed z-buffer: the chain's bits and the restatement's (hence src and the r2 bits)
    assert torch.equal(got["zkey"], z_chain), f"{label}: zkey differs from the chain in {int((got['zkey'] != z_chain).sum())} cells"
    A = TC.splat(inp["prev_inv"], inp["prev_age"], _np(tf.reprojector.rays), T, bf, TC.affine(TC.CASES[name]["ranges"], TC.CASES[name]["hw"]))
    zk = _np(got["zkey"]).view(np.uint64)
    assert np.array_equal(zk, A["zkey"]), f"{label}: zkey differs from the numpy restatement in {int((zk != A['zkey']).sum())} cells"
    assert np.array_equal(_np(got["src"]), TC.src_of(zk).astype(np.int32))
    filled = zk != TC.EMPTY
    # 2. warped_inv: 2 ulp from the correctly rounded value of the device's own r2 bits
    exact = TC.exact_warped_inv(zk, bf)
    w_inv = _np(got["warped_inv"])
    worst = _ulps(w_inv, exact, filled)
    print(f"[temporal] {label}: {int(filled.sum())} of {filled.size} cells filled; warped_inv at most {worst} ulp from RN_fp32(bf / sqrt(float64(r2))) (bar 2)")
    assert worst <= 2 and (w_inv[~filled] == 0).all() and not np.signbit(w_inv[~filled]).any()
    # 3. everything behind it: the chain's fuse and the restatement's, fed the device's own warped_inv and src
    with arena.paused():
        chain = tf.fuse_chain(None, state, d["cur_inv"], d["cur_std"], warped=(got["warped_inv"], got["src"]))
    rest = TC.fuse(None, (inp["prev_inv"], inp["prev_var"], inp["prev_age"]), inp["cur_inv"], inp["cur_std"], bf, warped=(w_inv, _np(got["src"])))
    for k in BEHIND:
        assert _same(got[k], chain[k]), f"{label}: {k} differs from the chain's fuse"
        assert _same(got[k], rest[k]), f"{label}: {k} differs from the restatement's fuse"
    # the state was advanced
    bufs = tf.buffers(d["prev_inv"].shape[0], DEV)
    assert _same(bufs["inv"], got["fused"]) and _same(bufs["var"], got["var"]) and _same(bufs["age"], got["age"])
    # 4. the whole chain end to end, torch's own root in it: counts are printed, the gate's decision is asserted outside the margin
    with arena.paused():
        whole = tf.fuse_chain(z_chain, state, d["cur_inv"], d["cur_std"])
    diff = {k: int((~(np.isnan(_np(got[k]).astype(np.float64)) & np.isnan(_np(whole[k]).astype(np.float64))) & (_np(got[k]) != _np(whole[k]))).sum())
            for k in ("warped_inv",) + BEHIND}
    print(f"[temporal] {label}: elements that differ from the whole chain (torch's root): " + ", ".join(f"{k} {v}" for k, v in diff.items()))
    r64 = TC.fuse(zk, (inp["prev_inv"], inp["prev_var"], inp["prev_age"]), inp["cur_inv"], inp["cur_std"], bf)
    decided = np.isin(r64["row"], (3, 4)) & (r64["margin"] > TC.GATE_MARGIN)
    left_out = int((np.isin(r64["row"], (3, 4)) & ~decided).sum())
    assert left_out <= 0.01 * decided.size, (label, left_out)
    age = _np(got["age"])
    assert np.array_equal(age[decided], r64["age"][decided]), f"{label}: the gate decided otherwise on {int((age[decided] != r64['age'][decided]).sum())} pixels"
    print(f"[temporal] {label}: {int(decided.sum())} gate decisions agree with the float64 restatement; {left_out} pixels within the margin left out")
    return got, inp


# ------------------------------------------------------------------------------ 1. the bits of the definition
@pytest.mark.parametrize("bf", TC.BFS)
@pytest.mark.parametrize("kind", TC.POSES)
@pytest.mark.parametrize("name", list(TC.CASES))
def test_outputs_are_the_bits_of_the_chain_and_the_restatement(arena, name, kind, bf):
    tf = _fusion(name, bf)
    got, inp = _check_step(arena, tf, name, bf, TC.poses(kind, name), f"{name} {kind} bf {bf:g}")
    if kind == "identity":
        live = TC.splat(inp["prev_inv"], inp["prev_age"], _np(tf.reprojector.rays), TC.poses(kind, name), bf,
                        TC.affine(TC.CASES[name]["ranges"], TC.CASES[name]["hw"]))["live"]
        own = np.broadcast_to(np.arange(live[0].size).reshape((1,) + live.shape[1:]), live.shape)
        assert np.array_equal(_np(got["src"])[live], own[live])
    if TC.CASES[name]["bad"]:
        assert int((~np.isfinite(inp["cur_inv"])).sum()) >= 2


def test_collapse_at_launch_size(arena):
    """Every pixel of a frame contends for one word: the minimum is still exact, and the lowest live index wins among equal r2."""
    name = "waves"
    tf = _fusion(name)
    T = np.stack([TC.collapse()] * TC.CASES[name]["B"])
    got, inp = _check_step(arena, tf, name, 96.0, T, "waves collapse")
    src = _np(got["src"])
    for b in range(src.shape[0]):
        assert int((src[b] >= 0).sum()) == 1
        live = (inp["prev_age"][b] != 0) & (inp["prev_inv"][b] > 0) & np.isfinite(inp["prev_inv"][b])
        assert src[b].max() == int(np.flatnonzero(live.reshape(-1))[0])


# ------------------------------------------------------------------------------ 2. structure
@pytest.mark.parametrize("name", ["tail", "part"])
def test_every_subset_of_the_outputs_and_poisoned_tensors(arena, name):
    """Every non-empty subset of want gives the bits of the full call into the caller's own tensors, pre-filled with the sentinel:
    a wanted output is overwritten everywhere, one that is not wanted is never touched; the inputs are intact."""
    tf = _fusion(name)
    rp = tf.reprojector
    inp = TC.make_inputs(name)
    d = _dev(arena, inp)
    rp.rays = arena.guarded(rp.rays)
    T = arena.guarded(torch.from_numpy(TC.poses("rigid", name)).to(DEV))
    ins = list(d.values()) + [rp.rays, T]
    snaps = [(t, arena.snapshot(t)) for t in ins]
    shape = tuple(d["prev_inv"].shape)
    zkey = H.temporal_splat(d["prev_inv"], d["prev_age"], rp.rays, T, rp.bf, tf.affine, out=arena.alloc(shape, torch.int64, DEV))
    assert not bool((zkey.view(torch.int32) == guard_arena.SENTINEL).any())            # the fill writes every cell
    args = (zkey, d["prev_inv"], d["prev_var"], d["prev_age"], d["cur_inv"], rp.bf)
    kw = dict(gate=tf.gate, q_var=tf.q_var, cur_std=d["cur_std"])
    full = H.temporal_fuse(*args, **kw)
    assert tuple(full) == H.TEMPORAL_OUTPUTS
    kinds = {k: v.dtype for k, v in full.items()}
    sentinel8 = torch.tensor(guard_arena.SENTINEL_BYTES, dtype=torch.uint8, device=DEV)
    for r in range(1, len(H.TEMPORAL_OUTPUTS) + 1):
        for sub in itertools.combinations(H.TEMPORAL_OUTPUTS, r):
            spare = {k: arena.alloc(shape, kinds[k], DEV) for k in H.TEMPORAL_OUTPUTS}
            res = H.temporal_fuse(*args, want=sub, out=spare, **kw)
            assert tuple(res) == sub
            for k in H.TEMPORAL_OUTPUTS:
                raw = spare[k].view(-1).view(torch.uint8)
                if k in sub:
                    assert res[k] is spare[k] and torch.equal(raw, full[k].view(-1).view(torch.uint8)), (sub, k)
                else:
                    assert torch.equal(raw, sentinel8.repeat(-(-raw.numel() // 4))[:raw.numel()]), f"{k} was written although it is not wanted ({sub})"
    # the scalar standard deviation is the map filled with it; [B, 1, H, W] is the same call
    flat = H.temporal_fuse(*args, gate=tf.gate, q_var=tf.q_var, meas_std=0.25)
    as_map = H.temporal_fuse(args[0], args[1], args[2], args[3], d["cur_inv"].unsqueeze(1), rp.bf, gate=tf.gate, q_var=tf.q_var,
                             cur_std=torch.full_like(d["cur_inv"], 0.25).unsqueeze(1))
    assert all(_same(flat[k], as_map[k]) for k in H.TEMPORAL_OUTPUTS)
    torch.cuda.synchronize()
    for t, snap in snaps:
        assert arena.unchanged(t, snap)


def test_frames_do_not_depend_on_the_batch_and_runs_repeat(arena):
    name = "waves"
    inp = TC.make_inputs(name)
    d = _dev(arena, inp)
    T = torch.from_numpy(TC.poses("rigid", name))
    tf = _fusion(name)
    runs = []
    for _ in range(2):
        _load(tf, d)
        runs.append({k: v.clone() for k, v in tf.step(d["cur_inv"], d["cur_std"], T=T, want=tf.OUTPUTS).items()})
    for k in tf.OUTPUTS:
        assert _same(runs[0][k], runs[1][k]), k
    for b in range(TC.CASES[name]["B"]):
        one = {k: v[b:b + 1].clone() for k, v in d.items()}
        _load(tf, one)
        got = tf.step(one["cur_inv"], one["cur_std"], T=T[b:b + 1], want=tf.OUTPUTS)
        for k in tf.OUTPUTS:
            assert _same(got[k][0], runs[0][k][b]), (k, b)


@pytest.mark.parametrize("name", ["tail", "waves"])
def test_a_captured_step_replays_three_poses(arena, name):
    """One step captured once (the pose is read from device memory), then replayed three times with set_pose and a fresh measurement:
    the bits of three eager steps."""
    inp = TC.make_inputs(name)
    d = _dev(arena, inp)
    B = d["prev_inv"].shape[0]
    tf, twin = _fusion(name), _fusion(name)
    static_inv, static_std = d["cur_inv"].clone(), d["cur_std"].clone()
    tf.step(static_inv, static_std)                                        # makes the buffers (eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tf.step(static_inv, static_std, want=tf.OUTPUTS)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out = tf.step(static_inv, static_std, want=tf.OUTPUTS)
    _load(tf, d), _load(twin, d)
    pose_at, moved = tf.buffers(B)["T"].data_ptr(), 0
    for n, kind in enumerate(("rigid", "yaw", "shift")):
        T = torch.from_numpy(TC.poses(kind, name))
        cur = d["cur_inv"] * (1.0 + 0.01 * n)
        with arena.paused():
            want = {k: v.clone() for k, v in twin.step(cur, d["cur_std"], T=T, want=twin.OUTPUTS).items()}
        tf.set_pose(T)
        static_inv.copy_(cur)
        g.replay()
        torch.cuda.synchronize()
        for k in tf.OUTPUTS:
            assert _same(out[k], want[k]), (n, kind, k)
        moved += int((out["src"] >= 0).sum())
        assert int(out["age"].max()) >= 2 or n == 0
    assert moved > 0 and tf.buffers(B)["T"].data_ptr() == pose_at


def test_reset_makes_the_next_step_measurement_only(arena):
    name = "b2"
    inp = TC.make_inputs(name)
    d = _dev(arena, inp)
    tf = _fusion(name, meas_std=0.3)
    first = {k: v.clone() for k, v in tf.step(d["cur_inv"], want=tf.OUTPUTS).items()}              # a fresh evaluator: no prior either
    tf.step(d["cur_inv"], d["cur_std"], T=torch.from_numpy(TC.poses("shift", name)))
    assert int(tf.buffers(2)["age"].max()) >= 2
    tf.reset()
    again = tf.step(d["cur_inv"], want=tf.OUTPUTS)
    m = inp["cur_inv"]
    ok = (m > 0) & np.isfinite(m)
    for res in (first, again):
        assert bool((res["src"] == -1).all()) and bool((res["zkey"] == H.TEMPORAL_EMPTY).all())
        assert _same(res["fused"], m) and np.array_equal(_np(res["age"]), ok.astype(np.uint8))
        assert np.array_equal(_np(res["var"])[ok], np.full(int(ok.sum()), np.float32(0.3) * np.float32(0.3))) and np.isposinf(_np(res["var"])[~ok]).all()


# ------------------------------------------------------------------------------ 3. the pipeline stage
def test_pipeline_with_and_without_the_temporal_stage(arena, monkeypatch):
    from test_gpu_reproject import _tiny_rig
    H.set_conv_mode("f32")
    cfg, w, inp, samplers, (img_a, img_b), rig = _tiny_rig(False)
    # that rig's cameras under a rig panorama whose ray table the stage can invert (the full sphere)
    rp = dropin.Reprojector(rig.grid_makers, G.ring_poses(3), rig.out_shape, TC.FULL[0], TC.FULL[1], bf=1.0, device=DEV)
    called = []
    real = H._call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(H, "_call", spy)
    new = {"mvsgi_temporal_splat_f32", "mvsgi_temporal_fuse_f32"}
    # temporal=None: every launch and return value as without the argument
    plain = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=("spread",))
    want_a = plain.forward_device(img_a).clone()
    spread_a = plain.confidence["spread"].clone()
    calls_plain = list(called)
    called.clear()
    none = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=("spread",), temporal=None)
    assert torch.equal(none.forward_device(img_a), want_a) and torch.equal(none.confidence["spread"], spread_a)
    assert called == calls_plain and not new & set(called) and none.temporal is None and plain.temporal is None
    want_b = plain.forward_device(img_b).clone()
    spread_b = plain.confidence["spread"].clone()
    assert not torch.equal(want_a, want_b)
    called.clear()
    # the stage behind the soft-argmin: std is the confidence map "spread"
    tf, twin = dropin.TemporalFusion(rp, q_var=1e-8), dropin.TemporalFusion(rp, q_var=1e-8)
    pipe = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, confidence=("spread",), temporal=tf)
    assert pipe.temporal is None and pipe.temporal_stage is tf
    T = torch.from_numpy(TC.pose("rigid", "tail"))

    def check(inv, expect_inv, spread):
        assert torch.equal(inv, expect_inv)                              # inv_dist: the bits of a pipeline without the stage
        with arena.paused():
            want = twin.step(expect_inv, spread, want=H.TEMPORAL_OUTPUTS)
        assert tuple(pipe.temporal) == H.TEMPORAL_OUTPUTS
        for k in H.TEMPORAL_OUTPUTS:
            assert _same(pipe.temporal[k], want[k]), k
        return int((want["src"] >= 0).sum()), int(want["age"].max())
    inv = pipe.forward_device(img_a)
    assert called[-2:] == ["mvsgi_temporal_splat_f32", "mvsgi_temporal_fuse_f32"] and called.count("mvsgi_temporal_fuse_f32") == 1
    assert called[:-2] == calls_plain                                    # the stage is the last one; everything before it is what it was
    assert check(inv, want_a, spread_a) == (0, 1)                        # the first frame: measurement only
    tf.set_pose(T), twin.set_pose(T)
    n, a = check(pipe.forward_device(img_b), want_b, spread_b)
    assert n > 0 and a >= 1
    static = {k: v.data_ptr() for k, v in pipe.temporal.items()}
    pipe.capture(img_a)                                                  # runs the stage on its warm-up frames, then resets it
    twin.reset()
    tf.set_pose(torch.eye(4)), twin.set_pose(torch.eye(4))
    assert check(pipe.replay(img_a), want_a, spread_a) == (0, 1)
    assert {k: v.data_ptr() for k, v in pipe.temporal.items()} == static     # made by the first call, never replaced
    tf.set_pose(T), twin.set_pose(T)
    n, _ = check(pipe.replay(img_b), want_b, spread_b)
    assert n > 0
    tf.set_pose(torch.eye(4)), twin.set_pose(torch.eye(4))
    _, a = check(pipe.replay(img_b), want_b, spread_b)                   # the same frame again, at rest: confirmed
    assert a >= 2
    with pytest.raises(ValueError):
        InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, temporal=dropin.TemporalFusion(rp))          # neither spread nor meas_std
    with pytest.raises(ValueError):
        InferencePipeline(cfg, w, inp, device=DEV, temporal=tf)
