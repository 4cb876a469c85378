"""GPU (MI355X): the camera range images and the visibility test (csrc/visibility.hip, dropin.Visibility) -- z2, visible and n_visible
bit for bit against the composition they are defined by (Visibility.evaluate_chain: Reprojector.reproject()'s outputs, the transform
kernel, torch's scatter_reduce(amin) and a comparison), the range image against the correctly rounded root, independence of the batch
and of the run, graph capture, every output between guard bands, and the consumers: photo_consistency(cam_seen=), pack_cloud(valid=
visible) and the pipeline stage.  Every test runs with guarded allocations (tests/guard_arena.py).

The cases are tests/visibility_cases.py's: a row tail (6 x 10 into 12 x 20), an odd buffer (8 x 16 into 5 x 7), eight cameras on one
row, a 1 x 1 buffer (every pixel of a camera contends for one word: the minimum must still be exact), B = 2 and 3, and one map sized
for the launch's geometry (48 x 100 x 3 frames).  Bad inverse distances (0, -1, NaN, inf) are seeded into all but one.

64-bit indexing over B is by construction only (every plane offset is formed from a long long frame index), as for the other
geometry kernels."""
import itertools

import numpy as np
import pytest
import torch

import guard_arena
import photo_cases as PC
import reproject_cases as RC
import visibility_cases as VC
from mvs_gi_amd import dropin, hip_ops as H
from mvs_gi_amd.dropin import sweep_grids as SG
from mvs_gi_amd.pipeline import InferencePipeline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT = ("z2", "visible", "n_visible")            # bit for bit; range to 1 ulp of the correctly rounded root
MASKS = (None, "mask_hw", "mask_frames")


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


def _makers(n, all_eq=False):
    return [SG.EquirectangularSampleGridMaker() if all_eq or k % 2 else SG.DoubleSphereSampleGridMaker(RC.DS_PARAMS, RC.DS_CALIB)
            for k in range(n)]


def _case(arena, name, bf=RC.BF, footprint=1, mask=None, tol=VC.TOL):
    """-> (Visibility, inv): the device inputs in guarded allocations; bf = 1 runs on inv / 96, the pipeline's metric map."""
    s = VC.spec(name)
    inp = VC.make_inputs(name)
    rp = dropin.Reprojector(_makers(s["N"], s["all_eq"]), RC.poses(s["base"]), s["hw"], RC.LON, RC.LAT, bf=bf, device=DEV)
    m = None if mask is None else arena.guarded(inp[mask].to(DEV))
    vis = dropin.Visibility(rp, zshape=s["zshape"], tol=tol, footprint=footprint, mask=m)
    return vis, arena.guarded((inp["inv"] / (RC.BF / bf)).to(DEV))


def _same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    got, want = got.cpu(), want.cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not got.is_floating_point():
        return bool(torch.equal(got, want))
    return bool(torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)))


def _check_range(label, rng: torch.Tensor, z2: torch.Tensor) -> int:
    """range against RN_fp32(sqrt(float64(z2))): +inf where z2 is, at most 1 ulp elsewhere"""
    got, want, z = rng.cpu().numpy(), VC.exact_root(z2).numpy(), z2.cpu().numpy()
    empty = np.isinf(z)
    assert np.array_equal(np.isinf(got), empty) and (got[empty] > 0).all()
    d = 0
    if (~empty).any():
        d = int(np.abs(got[~empty].view(np.int32).astype(np.int64) - want[~empty].view(np.int32).astype(np.int64)).max())
    print(f"[visibility] {label}: range at most {d} ulp from RN_fp32(sqrt(float64(z2))) (bar 1); {int((~empty).sum())} of {z.size} cells filled")
    assert d <= 1
    return d


# ------------------------------------------------------------------------------ 1. the bits of the composition
@pytest.mark.parametrize("bf", [96.0, 1.0])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("footprint", [1, 2])
@pytest.mark.parametrize("name", list(VC.ALL))
def test_outputs_are_the_bits_of_the_chain(arena, name, footprint, mask, bf):
    vis, inv = _case(arena, name, bf, footprint, mask)
    with arena.paused():
        want = vis.evaluate_chain(inv)
    full = {k: v.clone() for k, v in vis.evaluate(inv).items()}            # z2 is the evaluator's own: the next call overwrites it
    assert tuple(full) == vis.OUTPUTS and full["visible"].dtype == torch.bool and full["n_visible"].dtype == torch.uint8
    for k in EXACT:
        assert _same_bits(full[k], want[k]), k
    label = f"{name} footprint {footprint} mask {mask} bf {bf:g}"
    _check_range(label, full["range"], full["z2"])
    seen = int(full["visible"].sum())
    assert seen > 0
    if VC.spec(name)["bad"]:                                              # bad inverse distances: never visible
        dead = ~((inv > 0) & torch.isfinite(inv))
        assert int(dead.sum()) >= 4 and not bool(full["visible"].movedim(1, -1)[dead].any()) and bool((full["n_visible"][dead] == 0).all())
    if bf == RC.BF and mask is None:                                      # beside the CPU restatement: the same picture
        cpu = VC.build(name, footprint)["restated"]
        flips = int((full["visible"].cpu() != cpu["visible"]).sum())
        print(f"[visibility] {label}: {seen} visible (pixel, camera) pairs; {flips} differ from the CPU restatement (device sqrt / atan2 at a cell's edge)")


@pytest.mark.parametrize("name", list(VC.ALL))
def test_every_subset_of_the_outputs_and_caller_owned_tensors(arena, name):
    """Every non-empty subset of the outputs, on every case: the exact ones are the chain's bits, range the full call's."""
    vis, inv = _case(arena, name, mask="mask_hw")
    with arena.paused():
        want = vis.evaluate_chain(inv)
    full = {k: v.clone() for k, v in vis.evaluate(inv).items()}
    for r in range(1, len(vis.OUTPUTS) + 1):
        for sub in itertools.combinations(vis.OUTPUTS, r):
            got = vis.evaluate(inv, want=sub)
            assert tuple(got) == sub
            for k in sub:
                assert _same_bits(got[k], want[k] if k in EXACT else full[k]), (sub, k)
    # a caller's own tensors are written in place; [B, 1, H, W] is the same call
    out = {k: arena.alloc(full[k].shape, full[k].dtype, DEV) for k in vis.OUTPUTS}
    res = vis.evaluate(inv.unsqueeze(1), out=out)
    for k in vis.OUTPUTS:
        assert res[k] is out[k] and _same_bits(out[k], full[k]), k
    # the tolerance on the same buffer: a smaller one never sees more, and sees fewer where cells hold several points (the 5 x 7 buffer)
    rp = vis.reprojector
    strict, loose = (H.visibility(inv, rp.rays, rp.T, rp.cams, rp.bf, full["z2"], tol=t, want=("visible",))["visible"] for t in (0.0, 0.5))
    assert bool((strict <= full["visible"]).all()) and bool((full["visible"] <= loose).all())
    if name == "odd_buffer":
        assert int(strict.sum()) < int(loose.sum())


# ------------------------------------------------------------------------------ 2. no dependence on the batch or the run
@pytest.mark.parametrize("footprint", [1, 2])
@pytest.mark.parametrize("name", ["b3", "waves", "one_cell"])
def test_frames_do_not_depend_on_the_batch_and_runs_repeat(arena, name, footprint):
    vis, inv = _case(arena, name, footprint=footprint)
    first = {k: v.clone() for k, v in vis.evaluate(inv).items()}
    again = vis.evaluate(inv)
    for k in vis.OUTPUTS:
        assert _same_bits(first[k], again[k]), k
    for b in range(inv.shape[0]):
        one = vis.evaluate(inv[b:b + 1].clone())
        for k in vis.OUTPUTS:
            assert _same_bits(one[k][0], first[k][b]), (k, b)


# ------------------------------------------------------------------------------ 3. graph capture
@pytest.mark.parametrize("name,footprint,mask", [("tail", 1, "mask_frames"), ("eight", 2, None), ("waves", 1, None)])
def test_capture_and_replay_equal_the_eager_result(arena, name, footprint, mask):
    vis, inv = _case(arena, name, footprint=footprint, mask=mask)
    eager = {k: v.clone() for k, v in vis.evaluate(inv).items()}
    out = {k: torch.full_like(v, 7) for k, v in eager.items()}
    static_inv = inv.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vis.evaluate(static_inv, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for v in out.values():
        v.fill_(7)
    filled = {k: v.clone() for k, v in out.items()}                        # (a bool plane holds True, not 7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        vis.evaluate(static_inv, out=out)
    assert all(_same_bits(out[k], filled[k]) for k in out)                 # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    for k in vis.OUTPUTS:
        assert _same_bits(out[k], eager[k]), k
    # another input: the replay follows (the fill is part of the graph: nothing of the first frame is left in the buffer)
    static_inv.copy_(inv.flip(0).flip(-1))
    with arena.paused():
        other = {k: v.clone() for k, v in vis.evaluate(static_inv).items()}
    g.replay()
    torch.cuda.synchronize()
    assert not _same_bits(other["z2"], eager["z2"])
    for k in vis.OUTPUTS:
        assert _same_bits(out[k], other[k]), k


# ------------------------------------------------------------------------------ 4. address safety
@pytest.mark.parametrize("footprint", [1, 2])
@pytest.mark.parametrize("name", list(VC.ALL))
def test_address_safety(arena, name, footprint):
    """Inputs and outputs in guarded allocations, outputs pre-filled with the NaN sentinel: every output element is overwritten (the
    fill writes every cell of z2), the inputs are intact (the guard bands are checked at teardown); an output that is not wanted is
    never touched."""
    vis, inv = _case(arena, name, footprint=footprint, mask="mask_frames")
    rp = vis.reprojector
    rp.rays = arena.guarded(rp.rays)
    ins = [inv, rp.rays, vis.mask]
    snaps = [(t, arena.snapshot(t)) for t in ins]
    B, (Ho, Wo), N, (Hz, Wz) = inv.shape[0], rp.out_shape, rp.num_cams, vis.zshape
    shapes = {"visible": ((B, N, Ho, Wo), torch.bool), "n_visible": ((B, Ho, Wo), torch.uint8), "range": ((B, N, Hz, Wz), torch.float32),
              "z2": ((B, N, Hz, Wz), torch.float32)}
    out = {k: arena.alloc(s, d, DEV) for k, (s, d) in shapes.items()}
    vis.evaluate(inv, out=out)
    lib_made = vis.evaluate(inv)                                          # the evaluator's own allocations are guarded and pre-filled too
    torch.cuda.synchronize()
    for res in (out, lib_made):
        for k in ("z2", "range"):
            assert not bool((res[k].view(torch.int32) == guard_arena.SENTINEL).any()), f"{k}: an element was never stored"
        assert bool((res["visible"].view(torch.uint8) <= 1).all()), "visible: a byte was never stored"
        assert bool((res["n_visible"] <= N).all()), "n_visible: a byte was never stored"
    for k in vis.OUTPUTS:
        assert _same_bits(out[k], lib_made[k]), k
    sentinel8 = torch.tensor(guard_arena.SENTINEL_BYTES, dtype=torch.uint8, device=DEV)
    for sub in (("visible",), ("n_visible",), ("range",), ("n_visible", "range")):
        spare = {k: arena.alloc(s, d, DEV) for k, (s, d) in shapes.items() if k != "z2"}
        H.visibility(inv, rp.rays, rp.T, rp.cams, rp.bf, out["z2"], tol=vis.tol, want=sub, out=spare)
        torch.cuda.synchronize()
        for k in H.VISIBILITY_OUTPUTS:
            if k in sub:
                assert _same_bits(spare[k], out[k]), (sub, k)
            else:
                raw = spare[k].view(-1).view(torch.uint8)
                assert torch.equal(raw, sentinel8.repeat(-(-raw.numel() // 4))[:raw.numel()]), f"{k} was written although it is not wanted ({sub})"
    for t, snap in snaps:
        assert arena.unchanged(t, snap)


# ------------------------------------------------------------------------------ 5. the consumers
def _photo_case(arena, name, visibility=True):
    """A photo case (tests/photo_cases.py) with a Visibility on its reprojector."""
    s = PC.spec(name)
    inp = PC.make_inputs(name)
    rp = dropin.Reprojector(_makers(s["N"], s["all_eq"]), RC.poses(s["base"]), s["hw"], RC.LON, RC.LAT, bf=RC.BF, device=DEV)
    vis = dropin.Visibility(rp)
    kw = dict(cam_masks=None if inp["cam_masks"] is None else arena.guarded(inp["cam_masks"].to(DEV)),
              mask=None if inp["mask"] is None else arena.guarded(inp["mask"].to(DEV)), thresh=PC.THRESH)
    return (dropin.PhotoConsistency(rp, visibility=vis if visibility else None, **kw), dropin.PhotoConsistency(rp, **kw), vis,
            arena.guarded(inp["inv"].to(DEV)), arena.guarded(inp["imgs"].to(DEV)))


PHOTO_PLANES = ("n_views", "photo_var", "mean_colour")


@pytest.mark.parametrize("name", PC.GPU_CASES)
def test_photo_with_cam_seen_is_the_chain_with_seen_and_visible(arena, name):
    pc, plain, vis, inv, imgs = _photo_case(arena, name)
    visible = vis.evaluate(inv, want=("visible",))["visible"].clone()
    with arena.paused():
        want = plain.evaluate_chain(inv, imgs, cam_seen=visible)           # seen &= visible, then the fusion rule in torch
        want_own = pc.evaluate_chain(inv, imgs)                            # the same through the stage's own chain
    got = {k: v.clone() for k, v in pc.evaluate(inv, imgs).items()}       # evaluates its Visibility first
    by_hand = plain.evaluate(inv, imgs, cam_seen=visible)
    for k in PHOTO_PLANES:
        assert _same_bits(got[k], want[k]) and _same_bits(want_own[k], want[k]) and _same_bits(by_hand[k], want[k]), k
    for k in H.PHOTO_OUTPUTS:                                             # the stage's own route and cam_seen= by hand: one kernel, every output
        assert _same_bits(got[k], by_hand[k]), k
    # photo_std: 1 ulp from the correctly rounded root of the kernel's own photo_var, as tests/test_gpu_photo.py asks of the plain entry point
    std, root = got["photo_std"].cpu().numpy(), PC.exact_std(got["photo_var"])
    d = int(np.abs(std.view(np.int32).astype(np.int64) - root.view(np.int32).astype(np.int64)).max())
    print(f"[visibility] photo {name}: photo_std with cam_seen at most {d} ulp from RN_fp32(sqrt(float64(photo_var))) (bar 1)")
    assert d <= 1
    # the table: counts exact; mean_std, rms, bad, coverage within 1 ulp of float64 of the math.fsum restatement on the kernel's own maps
    t = got["table"].cpu().numpy()
    t_want = PC.table(std, got["photo_var"].cpu().numpy(), got["n_views"].cpu().numpy(), None if pc.mask is None else pc.mask.cpu().numpy(), PC.THRESH)
    assert np.array_equal(t[:, 0], t_want[:, 0]) and np.array_equal(t[:, 5:], t_want[:, 5:])
    for a, b in zip(t[:, 1:5].reshape(-1), t_want[:, 1:5].reshape(-1)):
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= np.spacing(abs(b)), (name, a, b)
    assert np.array_equal(got["table"].cpu().numpy()[:, 0], want["table"].cpu().numpy()[:, 0])
    assert np.array_equal(got["table"].cpu().numpy()[:, 5:], want["table"].cpu().numpy()[:, 5:])
    dropped = int(plain.evaluate(inv, imgs, want=("n_views",))["n_views"].sum()) - int(got["n_views"].sum())
    print(f"[visibility] photo {name}: visibility takes {dropped} (pixel, camera) views out of the fusion")
    assert dropped >= 0


@pytest.mark.parametrize("name", PC.GPU_CASES)
def test_photo_without_cam_seen_and_with_all_ones_is_the_existing_entry_point(arena, name, monkeypatch):
    _, plain, _, inv, imgs = _photo_case(arena, name, visibility=False)
    called = []
    real = H._call
    monkeypatch.setattr(H, "_call", lambda n, *a: (called.append(n), real(n, *a))[1])
    base = {k: v.clone() for k, v in plain.evaluate(inv, imgs).items()}
    none = {k: v.clone() for k, v in plain.evaluate(inv, imgs, cam_seen=None).items()}
    assert called == ["mvsgi_photo_consistency_f32"] * 2
    B, N = inv.shape[0], plain.num_cams
    ones = arena.guarded(torch.ones((B, N) + plain.out_shape, dtype=torch.uint8, device=DEV))
    seen = plain.evaluate(inv, imgs, cam_seen=ones)
    assert called[-1] == "mvsgi_photo_consistency_seen_f32"
    as_bool = plain.evaluate(inv, imgs, cam_seen=ones.bool(), want=PHOTO_PLANES)
    for k in H.PHOTO_OUTPUTS:
        assert _same_bits(none[k], base[k]) and _same_bits(seen[k], base[k]), k
    for k in PHOTO_PLANES:
        assert _same_bits(as_bool[k], base[k]), k
    zeros = plain.evaluate(inv, imgs, cam_seen=torch.zeros_like(ones), want=("n_views", "photo_var"))
    assert not bool(zeros["n_views"].any()) and not bool(zeros["photo_var"].any())


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_pack_cloud_with_visible_is_the_torch_composition(arena):
    """`visible` where `valid` goes: the colour of the lowest camera that sees the point, require_colour as "some camera sees it"."""
    _, _, vis, inv, imgs = _photo_case(arena, "b3")
    rp = vis.reprojector
    r = rp.reproject(inv, imgs, want=("xyz", "warped", "valid"))
    visible = vis.evaluate(inv, want=("visible",))["visible"]
    assert bool((visible <= r["valid"]).all()) and int(visible.sum()) < int(r["valid"].sum())
    got = H.pack_cloud(inv, rp.rays, rp.bf, d_range=H.CLOUD_D_RANGE, warped=r["warped"], valid=visible, require_colour=True, want_index=True)
    d = torch.full_like(inv, rp.bf) / inv
    lo, hi = H.CLOUD_D_RANGE
    keep = torch.isfinite(d) & (d >= lo) & (d <= hi) & visible.any(dim=1)
    first = torch.argmax(visible.to(torch.uint8), dim=1)                  # the lowest camera that sees the point
    counts = got["counts"].cpu()
    changed = 0
    for b in range(inv.shape[0]):
        idx = torch.nonzero(keep[b].reshape(-1)).flatten()
        n = int(counts[b, 0])
        assert n == idx.numel() == int(counts[b, 1]) and 0 < n < keep[b].numel()
        assert torch.equal(got["index"][b, :n].long(), idx)
        xyz = r["xyz"][b].reshape(3, -1)[:, idx].t()
        cam = first[b].reshape(-1)[idx]
        colour = r["warped"][b].reshape(rp.num_cams, 3, -1)[cam, :, idx]
        assert torch.equal(_bits(got["points"][b, :n, :3]), _bits(xyz)) and torch.equal(_bits(got["points"][b, :n, 3:6]), _bits(colour))
        changed += int((cam != torch.argmax(r["valid"][b].to(torch.uint8), dim=0).reshape(-1)[idx]).sum())
    print(f"[visibility] cloud b3: {changed} points take their colour from another camera than the lowest valid one")


def test_pipeline_with_and_without_the_visibility_stage(arena, monkeypatch):
    from test_gpu_reproject import _tiny_rig
    H.set_conv_mode("f32")
    cfg, w, inp, samplers, (img_a, img_b), rp = _tiny_rig(False)
    called = []
    real = H._call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(H, "_call", spy)
    new = {"mvsgi_camera_range_f32", "mvsgi_visibility_f32", "mvsgi_photo_consistency_seen_f32"}
    # visibility=None: every launch and return value as without the argument
    plain = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, photo=dropin.PhotoConsistency(rp))
    want_inv = plain.forward_device(img_a).clone()
    want_photo = {k: v.clone() for k, v in plain.photo.items()}
    calls_plain = list(called)
    called.clear()
    none = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, photo=dropin.PhotoConsistency(rp), visibility=None)
    assert torch.equal(none.forward_device(img_a), want_inv) and all(_same_bits(none.photo[k], want_photo[k]) for k in want_photo)
    assert called == calls_plain and not new & set(called) and none.visibility is None and plain.visibility is None
    called.clear()
    # the stage, a photo stage that fuses the seeing cameras only, and a packer coloured by them
    vis, twin = dropin.Visibility(rp), dropin.Visibility(rp)
    packer = dropin.CloudPacker(rp, want_index=True)
    pipe = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, visibility=vis, photo=dropin.PhotoConsistency(rp, visibility=vis),
                             cloud=packer)
    assert pipe.visibility is None
    called.clear()

    def check(inv, expect_inv, img):
        assert torch.equal(inv, expect_inv)                              # inv_dist: the bits of a pipeline without the stage
        want = {k: v.clone() for k, v in twin.evaluate(expect_inv).items()}
        assert tuple(pipe.visibility) == vis.OUTPUTS
        for k in vis.OUTPUTS:
            assert _same_bits(pipe.visibility[k], want[k]), k
        photo = dropin.PhotoConsistency(rp).evaluate(expect_inv, img, cam_seen=want["visible"])
        for k in H.PHOTO_OUTPUTS:
            assert _same_bits(pipe.photo[k], photo[k]), k
        by_hand = H.pack_cloud(inv, rp.rays, rp.bf, d_range=H.CLOUD_D_RANGE, warped=pipe.reprojection[1], valid=want["visible"], want_index=True)
        n = int(by_hand["counts"][0, 0])
        assert torch.equal(pipe.cloud["counts"].cpu(), by_hand["counts"].cpu()) and n > 0
        assert torch.equal(_bits(pipe.cloud["points"][0, :n]), _bits(by_hand["points"][0, :n]))
        return int(want["visible"].sum())
    n_a = check(pipe.forward_device(img_a), want_inv, img_a)
    tail = called[called.index("mvsgi_reproject_f32"):]
    assert tail[:4] == ["mvsgi_reproject_f32", "mvsgi_camera_range_f32", "mvsgi_visibility_f32", "mvsgi_photo_consistency_seen_f32"]
    static = {k: v.data_ptr() for k, v in pipe.visibility.items()}
    pipe.capture(img_a)
    assert check(pipe.replay(img_a), want_inv, img_a) == n_a
    assert {k: v.data_ptr() for k, v in pipe.visibility.items()} == static     # made by the first call, never replaced
    other_inv = plain.forward_device(img_b).clone()
    assert not torch.equal(other_inv, want_inv)
    check(pipe.replay(img_b), other_inv, img_b)
    assert check(pipe.replay(img_a), want_inv, img_a) == n_a
