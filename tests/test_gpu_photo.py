"""GPU (MI355X): the photometric consistency (csrc/photo.hip, dropin.PhotoConsistency) -- its per-pixel planes bit for bit against
the composition it is defined by (PhotoConsistency.evaluate_chain on Reprojector.reproject()'s outputs), the root against the correctly
rounded one, the table against the math.fsum restatement of tests/photo_cases.py, independence of the batch, graph capture, the
pipeline stage, the photometric cloud gate, and every output and the workspace between guard bands.  Every test runs with guarded
allocations (tests/guard_arena.py).

Measured on the MI355X (printed by the tests): photo_std is at most 0 ulp from the correctly rounded root in every case (bar 1); the
table's means are at most 0 ulp of float64 from the restatement (bar 1).

64-bit indexing over B is by construction only (every plane offset is formed from a long long frame index): a case beyond 2^31
elements needs more device memory than the existing large-offset tests allocate, so there is none here."""
import itertools
import math

import numpy as np
import pytest
import torch

import guard_arena
import photo_cases as PC
import reproject_cases as RC
from mvs_gi_amd import dropin, hip_ops as H
from mvs_gi_amd.dropin import sweep_grids as SG
from mvs_gi_amd.pipeline import InferencePipeline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANES = ("n_views", "photo_var", "mean_colour")          # bit for bit; photo_std to 1 ulp of the correctly rounded root


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


def _makers(n, all_eq=False):
    return [SG.EquirectangularSampleGridMaker() if all_eq or k % 2 else SG.DoubleSphereSampleGridMaker(RC.DS_PARAMS, RC.DS_CALIB)
            for k in range(n)]


def _reprojector(name, bf):
    s = PC.spec(name)
    return dropin.Reprojector(_makers(s["N"], s["all_eq"]), RC.poses(s["base"]), s["hw"], RC.LON, RC.LAT, bf=bf, device=DEV)


def _case(arena, name, bf=RC.BF, f32_images=False):
    """-> (PhotoConsistency, inv, imgs, the CPU inputs): the device inputs in guarded allocations; bf = 1 runs on inv / 96, the pipeline's
    metric map."""
    inp = PC.make_inputs(name)
    imgs = RC.as_f32_chw(inp["imgs"]).contiguous() if f32_images else inp["imgs"]
    pc = dropin.PhotoConsistency(_reprojector(name, bf), cam_masks=None if inp["cam_masks"] is None else arena.guarded(inp["cam_masks"].to(DEV)),
                                 mask=None if inp["mask"] is None else arena.guarded(inp["mask"].to(DEV)), thresh=PC.THRESH)
    return pc, arena.guarded((inp["inv"] / (RC.BF / bf)).to(DEV)), arena.guarded(imgs.to(DEV)), inp


def _same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    got, want = got.cpu(), want.cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not got.is_floating_point():
        return bool(torch.equal(got, want))
    view = torch.int32 if got.dtype == torch.float32 else torch.int64
    return bool(torch.equal(got.contiguous().view(view), want.contiguous().view(view)))


def _ulps32(a: np.ndarray, b: np.ndarray) -> int:
    """Largest distance in fp32 ulps between two arrays of non-negative finite fp32 numbers."""
    assert a.dtype == np.float32 and b.dtype == np.float32 and (a >= 0).all() and (b >= 0).all()
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _ulps64(a: float, b: float) -> float:
    if math.isnan(a) or math.isnan(b):
        return 0.0 if math.isnan(a) and math.isnan(b) else math.inf
    return abs(a - b) / np.spacing(abs(b)) if a != b else 0.0


def _check_std(name, std: torch.Tensor, var: torch.Tensor) -> int:
    d = _ulps32(std.cpu().numpy(), PC.exact_std(var))
    print(f"[photo] {name}: photo_std at most {d} ulp from RN_fp32(sqrt(float64(photo_var))) (bar 1)")
    assert d <= 1
    return d


def _check_table(name, res: dict, mask) -> None:
    """Counts exact; mean_std, rms, bad, coverage within 1 ulp of float64 of the math.fsum restatement on the kernel's own fp32 maps."""
    got = res["table"].cpu().numpy()
    want = PC.table(res["photo_std"].cpu().numpy(), res["photo_var"].cpu().numpy(), res["n_views"].cpu().numpy(),
                    None if mask is None else mask.cpu().numpy(), PC.THRESH)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 5:], want[:, 5:])
    worst = max(_ulps64(float(got[r, c]), float(want[r, c])) for r in range(got.shape[0]) for c in range(1, 5))
    print(f"[photo] {name}: table means at most {worst:g} ulp of float64 from the math.fsum restatement (bar 1); pooled row {got[-1, :5]}")
    assert worst <= 1


# ------------------------------------------------------------------------------ 1. the planes: the bits of the composition
@pytest.mark.parametrize("bf", [96.0, 1.0])
@pytest.mark.parametrize("name", PC.GPU_CASES)
def test_planes_are_the_bits_of_the_chain(arena, name, bf):
    pc, inv, imgs, inp = _case(arena, name, bf)
    with arena.paused():
        want = pc.evaluate_chain(inv, imgs)
        # evaluate_chain is product code: its planes are the CPU restatement (the text the reference golden pins) on the device's own
        # samples -- Reprojector's warped and valid, and the camera masks through the same sampler -- bit for bit
        rp, B, N = pc.reprojector, inv.shape[0], pc.num_cams
        r = rp.reproject(inv, imgs, 0.0, want=("warped", "valid", "grid"))
        seen = r["valid"]
        if pc.cam_masks is not None:
            m = H.resample_bilinear(pc.cam_masks.repeat(B, 1, 1, 1), r["grid"].view(B * N, *rp.out_shape, 2), r["valid"].view(B * N, *rp.out_shape))
            seen = seen & (m.view(B, N, *rp.out_shape) > 0)
        restated = PC.restate(r["warped"].cpu(), seen.cpu())
    for k in PLANES:
        assert _same_bits(want[k], restated[k]), f"evaluate_chain's {k} is not the restatement's"
    full = {k: v.clone() for k, v in pc.evaluate(inv, imgs).items()}          # the table is the evaluator's own: the next call overwrites it
    assert tuple(full) == H.PHOTO_OUTPUTS
    for k in PLANES:
        assert _same_bits(full[k], want[k]), k
    _check_std(f"{name} bf {bf:g}", full["photo_std"], full["photo_var"])
    _check_table(f"{name} bf {bf:g}", full, pc.mask)
    # the chain's own table is a plain float64 sum of the same n addends: within (n + 2) * 2^-52 relative of the kernel's, counts equal
    got_t, chain_t = full["table"].cpu().numpy(), want["table"].cpu().numpy()
    assert np.array_equal(got_t[:, 0], chain_t[:, 0]) and np.array_equal(got_t[:, 3:], chain_t[:, 3:], equal_nan=True)
    rel = np.abs(got_t[:, 1:3] - chain_t[:, 1:3]) / np.abs(got_t[:, 1:3])
    assert np.array_equal(np.isnan(got_t[:, 1:3]), np.isnan(chain_t[:, 1:3])) and (np.nan_to_num(rel) <= (got_t[:, :1] + 2) * 2.0 ** -52).all()
    if bf == RC.BF:                                       # the device's planes beside the CPU restatement: the same histogram of views
        cpu = PC.build(name)
        flips = int((full["n_views"].cpu() != cpu["restated"]["n_views"]).sum())
        print(f"[photo] {name}: {flips} of {full['n_views'].numel()} pixels count other views than the CPU chain (device sqrt / atan2 at an edge)")
    # every subset of the outputs: the others keep their bits, nothing else is made
    for r in range(1, len(H.PHOTO_OUTPUTS)):
        for sub in itertools.combinations(H.PHOTO_OUTPUTS, r):
            got = pc.evaluate(inv, imgs, want=sub)
            assert tuple(got) == sub
            for k in sub:
                assert _same_bits(got[k], full[k]), (sub, k)
    # a caller's own tensors are written in place; [B, 1, H, W] and [B, N, ...] are the same call
    out = {k: arena.alloc(full[k].shape, full[k].dtype, DEV) for k in H.PHOTO_OUTPUTS}
    res = pc.evaluate(inv.unsqueeze(1), imgs.view(inv.shape[0], pc.num_cams, *imgs.shape[1:]), out=out)
    for k in H.PHOTO_OUTPUTS:
        assert res[k] is out[k] and _same_bits(out[k], full[k]), k


@pytest.mark.parametrize("name", [n for n in PC.GPU_CASES if PC.spec(n)["u8"]])
def test_uint8_and_fp32_images_give_the_same_bits(arena, name):
    """A uint8 image is byte / 255 in fp32 (the facade's conversion): the fp32 kernel on the converted images returns the uint8 kernel's bits."""
    pc, inv, imgs, _ = _case(arena, name)
    _, _, imgs_f, _ = _case(arena, name, f32_images=True)
    a = {k: v.clone() for k, v in pc.evaluate(inv, imgs).items()}
    b = pc.evaluate(inv, imgs_f)
    assert imgs.dtype == torch.uint8 and imgs_f.dtype == torch.float32
    for k in H.PHOTO_OUTPUTS:
        assert _same_bits(a[k], b[k]), k


# ------------------------------------------------------------------------------ 2. the table does not depend on the batch or the run
@pytest.mark.parametrize("name", ["b3", "waves_f32"])          # one record per frame, and five (G > 1) with every wave of a block busy
def test_rows_do_not_depend_on_the_batch_and_runs_repeat(arena, name):
    pc, inv, imgs, _ = _case(arena, name)
    assert (H.photo_ws_layout(3, *pc.out_shape)["G"] > 1) == (name == "waves_f32")
    N = pc.num_cams
    first = {k: v.clone() for k, v in pc.evaluate(inv, imgs).items()}
    again = pc.evaluate(inv, imgs)
    for k in H.PHOTO_OUTPUTS:
        assert _same_bits(first[k], again[k]), k
    assert int(first["table"][-1, 0]) == int(first["table"][:3, 0].sum()) > 0
    for b in range(3):
        one = pc.evaluate(inv[b:b + 1].clone(), imgs[b * N:(b + 1) * N].clone())
        assert _same_bits(one["table"][0], first["table"][b]), b
        assert _same_bits(one["table"][1], first["table"][b]), b            # one frame: the pooled row is the frame's
        for k in H.PHOTO_MAPS:
            assert _same_bits(one[k][0], first[k][b]), (k, b)


def test_per_frame_pixel_mask_and_no_table_without_workspace(arena, monkeypatch):
    pc, inv, imgs, inp = _case(arena, "pixel_mask")
    assert pc.mask.dim() == 3
    full = pc.evaluate(inv, imgs)
    assert 0 < int(full["table"][-1, 0]) < int((full["n_views"] > 1).sum())          # the mask drops pixels two cameras see
    # without the table there is no workspace and no second launch: the library is called with ws = NULL
    seen = []
    real = H._call
    monkeypatch.setattr(H, "_call", lambda name, *a: (seen.append((name, a[14], a[15], a[16])), real(name, *a))[1])
    pc.evaluate(inv, imgs, want=H.PHOTO_MAPS)
    assert seen == [("mvsgi_photo_consistency_f32", None, 0, None)]


# ------------------------------------------------------------------------------ 3. graph capture
@pytest.mark.parametrize("name", ["cam_masks", "eight_u8", "waves_f32"])
def test_capture_and_replay_equal_the_eager_result(arena, name):
    pc, inv, imgs, _ = _case(arena, name)
    eager = {k: v.clone() for k, v in pc.evaluate(inv, imgs).items()}
    out = {k: torch.full_like(v, 7) for k, v in eager.items()}
    static_inv = inv.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pc.evaluate(static_inv, imgs, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for v in out.values():
        v.fill_(7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        pc.evaluate(static_inv, imgs, out=out)
    assert all(bool((v == 7).all()) for v in out.values())                 # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    for k in H.PHOTO_OUTPUTS:
        assert _same_bits(out[k], eager[k]), k
    # another input: the replay follows
    static_inv.copy_(inv.flip(0).flip(-1))
    with arena.paused():
        other = {k: v.clone() for k, v in pc.evaluate(static_inv, imgs).items()}
    g.replay()
    torch.cuda.synchronize()
    assert not _same_bits(other["photo_var"], eager["photo_var"])
    for k in H.PHOTO_OUTPUTS:
        assert _same_bits(out[k], other[k]), k


# ------------------------------------------------------------------------------ 4. the pipeline stage and the photometric cloud gate
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_cloud_gate_on_photo_std_is_pack_cloud_with_the_plane(arena):
    pc, inv, imgs, _ = _case(arena, "b3")
    rp = pc.reprojector
    photo = pc.evaluate(inv, imgs, want=("photo_std", "n_views"))
    r = rp.reproject(inv, imgs, want=("warped", "valid"))
    hi = float(photo["photo_std"][photo["n_views"] > 1].median())
    packer = dropin.CloudPacker(rp, gates={"photo_std": (0.0, hi)}, attrs=("photo_std",), want_index=True)
    with pytest.raises(ValueError, match="photo="):
        packer.pack(inv, warped=r["warped"], valid=r["valid"])
    got = packer.pack(inv, warped=r["warped"], valid=r["valid"], photo=photo)
    with arena.paused():
        want = H.pack_cloud(inv, rp.rays, rp.bf, d_range=H.CLOUD_D_RANGE, gates=[(photo["photo_std"], 0.0, hi)], warped=r["warped"],
                            valid=r["valid"], attrs=[photo["photo_std"]], want_index=True)
    counts = want["counts"].cpu()
    assert torch.equal(got["counts"].cpu(), counts)
    for b in range(3):
        n = int(counts[b, 0])
        assert 0 < n < inv[b].numel()
        assert torch.equal(_bits(got["points"][b, :n]), _bits(want["points"][b, :n])) and torch.equal(got["index"][b, :n], want["index"][b, :n])
        idx = got["index"][b, :n].long()
        assert torch.equal(got["points"][b, :n, 6], photo["photo_std"][b].reshape(-1)[idx]) and bool((got["points"][b, :n, 6] <= hi).all())


@pytest.mark.parametrize("with_samplers", [False, True], ids=["views", "raw"])
def test_pipeline_with_and_without_the_photo_stage(arena, monkeypatch, with_samplers):
    """With samplers the stage is handed the cameras' raw frames (and a Reprojector.from_samplers), the surrogate views otherwise."""
    from test_gpu_reproject import _tiny_rig
    H.set_conv_mode("f32")
    cfg, w, inp, samplers, (img_a, img_b), rp = _tiny_rig(with_samplers)
    called = []
    real = H._call

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    monkeypatch.setattr(H, "_call", spy)
    # photo=None: every launch and return value as without the argument
    plain = InferencePipeline(cfg, w, inp, device=DEV, samplers=samplers, reprojector=rp)
    want_inv = plain.forward_device(img_a).clone()
    want_rep = [t.clone() for t in plain.reprojection]
    calls_plain = list(called)
    called.clear()
    none = InferencePipeline(cfg, w, inp, device=DEV, samplers=samplers, reprojector=rp, photo=None)
    assert torch.equal(none.forward_device(img_a), want_inv) and all(torch.equal(a, b) for a, b in zip(none.reprojection, want_rep))
    assert called == calls_plain and "mvsgi_photo_consistency_f32" not in called and none.photo is None and plain.photo is None
    called.clear()
    # the stage, and a packer gated on its plane
    pc, twin = dropin.PhotoConsistency(rp, thresh=0.05), dropin.PhotoConsistency(rp, thresh=0.05)
    hi = float(twin.evaluate(want_inv, img_a, want=("photo_std",))["photo_std"].median())
    packer = dropin.CloudPacker(rp, gates={"photo_std": (0.0, hi)}, attrs=("photo_std",), want_index=True)
    pipe = InferencePipeline(cfg, w, inp, device=DEV, samplers=samplers, reprojector=rp, photo=pc, cloud=packer)
    assert pipe.photo is None
    called.clear()

    def check(inv, expect_inv, img):
        assert torch.equal(inv, expect_inv)                              # inv_dist: the bits of a pipeline without the stage
        want = twin.evaluate(expect_inv, img)
        assert tuple(pipe.photo) == H.PHOTO_OUTPUTS
        for k in H.PHOTO_OUTPUTS:
            assert _same_bits(pipe.photo[k], want[k]), k
        by_hand = H.pack_cloud(inv, rp.rays, rp.bf, d_range=H.CLOUD_D_RANGE, gates=[(want["photo_std"], 0.0, hi)], warped=pipe.reprojection[1],
                               valid=pipe.reprojection[2], attrs=[want["photo_std"]], want_index=True)
        counts = by_hand["counts"].cpu()
        n = int(counts[0, 0])
        assert torch.equal(pipe.cloud["counts"].cpu(), counts) and 0 < n < 16 * 64
        assert torch.equal(_bits(pipe.cloud["points"][0, :n]), _bits(by_hand["points"][0, :n]))
        return n
    n_a = check(pipe.forward_device(img_a), want_inv, img_a)
    tail = called[called.index("mvsgi_reproject_f32"):]
    assert tail[:2] == ["mvsgi_reproject_f32", "mvsgi_photo_consistency_f32"] and tail.count("mvsgi_photo_consistency_f32") == 2      # the stage, and check()'s twin
    static = {k: v.data_ptr() for k, v in pipe.photo.items()}
    pipe.capture(img_a)
    assert check(pipe.replay(img_a), want_inv, img_a) == n_a
    assert {k: v.data_ptr() for k, v in pipe.photo.items()} == static     # made by the first call, never replaced
    other_inv = plain.forward_device(img_b).clone()
    assert not torch.equal(other_inv, want_inv)
    check(pipe.replay(img_b), other_inv, img_b)
    assert check(pipe.replay(img_a), want_inv, img_a) == n_a


# ------------------------------------------------------------------------------ 5. address safety
@pytest.mark.parametrize("name", PC.GPU_CASES)
def test_address_safety(arena, name):
    """Inputs, outputs and the workspace in guarded allocations, outputs and workspace pre-filled with the NaN sentinel: every output
    element is overwritten, the inputs and their guard bands are intact (the outputs' bands are checked at teardown); an output that is
    not wanted is never touched."""
    pc, inv, imgs, _ = _case(arena, name)
    rp = pc.reprojector
    rp.rays = arena.guarded(rp.rays)
    ins = [t for t in (inv, imgs, rp.rays, pc.cam_masks, pc.mask) if t is not None]
    snaps = [(t, arena.snapshot(t)) for t in ins]
    B, (Ho, Wo), C = inv.shape[0], rp.out_shape, PC.spec(name)["C"]
    shapes = {"n_views": ((B, Ho, Wo), torch.uint8), "photo_var": ((B, Ho, Wo), torch.float32), "photo_std": ((B, Ho, Wo), torch.float32),
              "mean_colour": ((B, C, Ho, Wo), torch.float32), "table": ((B + 1, 14), torch.float64)}
    out = {k: arena.alloc(s, d, DEV) for k, (s, d) in shapes.items()}
    ws = arena.alloc((H.photo_ws_layout(B, Ho, Wo)["total"],), torch.float64, DEV)
    H.photo_consistency(inv, rp.rays, rp.T, rp.cams, rp.bf, imgs, cam_masks=pc.cam_masks, mask=pc.mask, thresh=PC.THRESH, out=out, ws=ws)
    lib_made = pc.evaluate(inv, imgs)                                   # the library's own allocations are guarded and pre-filled too
    torch.cuda.synchronize()
    sentinel8 = torch.tensor(guard_arena.SENTINEL_BYTES, dtype=torch.uint8, device=DEV)
    for res in (out, lib_made):
        for k in ("photo_var", "photo_std", "mean_colour"):
            assert not bool((res[k].view(torch.int32) == guard_arena.SENTINEL).any()), f"{k}: an element was never stored"
        assert bool((res["n_views"] <= 8).all()), "n_views: a byte was never stored"
        assert not bool((res["table"].view(torch.int32) == guard_arena.SENTINEL).any()), "table: an element was never stored"
    for k in H.PHOTO_OUTPUTS:
        assert _same_bits(out[k], lib_made[k]), k
    assert not bool((ws.view(torch.int32) == guard_arena.SENTINEL).any()), "the workspace has a part no launch wrote"
    # outputs that are not wanted: their tensors, offered in `out` all the same, keep the sentinel
    for sub in (("photo_var",), ("n_views", "table"), ("mean_colour", "photo_std")):
        spare = {k: arena.alloc(s, d, DEV) for k, (s, d) in shapes.items()}
        H.photo_consistency(inv, rp.rays, rp.T, rp.cams, rp.bf, imgs, cam_masks=pc.cam_masks, mask=pc.mask, thresh=PC.THRESH, want=sub,
                            out=spare, ws=ws)
        torch.cuda.synchronize()
        for k in H.PHOTO_OUTPUTS:
            if k in sub:
                assert _same_bits(spare[k], out[k]), (sub, k)
            else:
                raw = spare[k].view(-1).view(torch.uint8)                # the body starts on a word of the arena: the pattern starts at byte 0
                assert torch.equal(raw, sentinel8.repeat(-(-raw.numel() // 4))[:raw.numel()]), f"{k} was written although it is not wanted ({sub})"
    for t, snap in snaps:
        assert arena.unchanged(t, snap)
