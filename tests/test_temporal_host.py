"""CPU: the definition of the temporal fusion as tests/temporal_cases.py restates it -- the geometry of the splat (the affine map is
the inverse of the rig panorama's ray table, longitude wraps, the nearest source wins a cell and the lower index among equals), the
rows of the fuse's table, a sequence of steps, and the conditions the GPU tests' cases are chosen for."""
import numpy as np
import pytest

import temporal_cases as TC

F32 = np.float32


def _own_index(B, Hh, W):
    return np.broadcast_to(np.arange(Hh * W).reshape(1, Hh, W), (B, Hh, W))


@pytest.mark.parametrize("bf", TC.BFS)
@pytest.mark.parametrize("name", list(TC.CASES))
def test_identity_lands_every_live_pixel_in_its_own_cell(name, bf):
    """The coefficients of the affine map and their signs: lon is the ray maker's theta, lat its phi - pi / 2."""
    r = TC.step(name, "identity", bf)
    live, src = r["A"]["live"], TC.src_of(r["A"]["zkey"])
    assert live.any() and (~live).any() or name == "row"
    own = _own_index(*live.shape)
    assert np.array_equal(src[live], own[live]), name
    assert (src[~live] == -1).all()                                     # and nothing else lands anywhere
    assert np.array_equal(r["A"]["splat"], live)


@pytest.mark.parametrize("name", [n for n, c in TC.CASES.items() if c["ranges"] is TC.FULL])
def test_yaw_by_whole_columns_shifts_the_map_and_wraps(name):
    r = TC.step(name, "yaw")
    live, src = r["A"]["live"], TC.src_of(r["A"]["zkey"])
    B, Hh, W = live.shape
    wrapped = 0
    for b in range(B):
        k = TC.YAW_COLUMNS + b
        i, j = np.nonzero(live[b])
        jt = (j + k) % W                                                # the target column of source column j
        assert np.array_equal(src[b][i, jt], i * W + j), (name, b)
        assert int((src[b] >= 0).sum()) == i.size
        wrapped += int((j + k >= W).sum())
    assert wrapped > 0                                                  # some sources crossed the seam


@pytest.mark.parametrize("name", ["tail", "waves"])
def test_collapse_every_pixel_contends_for_one_word(name):
    inp = TC.make_inputs(name)
    c = TC.CASES[name]
    B = c["B"]
    T = np.stack([TC.collapse()] * B)
    A = TC.splat(inp["prev_inv"], inp["prev_age"], TC.rays(name), T, 96.0, TC.affine(c["ranges"], c["hw"]))
    src = TC.src_of(A["zkey"])
    for b in range(B):
        filled = np.argwhere(src[b] >= 0)
        assert len(filled) == 1                                          # the one cell that holds t
        lowest = int(np.flatnonzero(A["live"][b].reshape(-1))[0])
        assert src[b][tuple(filled[0])] == lowest                        # equal r2: the lower source index wins
        assert (A["cx"][b][A["splat"][b]] == filled[0][1]).all() and (A["cy"][b][A["splat"][b]] == filled[0][0]).all()
        t = TC.collapse()[:3, 3]
        assert (A["zkey"][b][tuple(filled[0])] >> np.uint64(32)) == np.uint64(F32((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]).view(np.uint32))


@pytest.mark.parametrize("name", ["tail", "b2", "waves"])
def test_two_surfaces_into_one_cell_the_nearer_wins(name):
    inp = TC.make_inputs(name)
    c = TC.CASES[name]
    B, (Hh, W) = c["B"], c["hw"]
    ray_table = TC.rays(name)
    A = TC.splat(inp["prev_inv"], inp["prev_age"], ray_table, np.stack([TC.onto_x()] * B), 96.0, TC.affine(c["ranges"], c["hw"]))
    src = TC.src_of(A["zkey"])
    with np.errstate(all="ignore"):
        px = (ray_table[0][None] * (F32(96.0) / inp["prev_inv"])).astype(F32)
    for b in range(B):
        front = A["live"][b] & (px[b] > 0)
        assert front.sum() > 4
        cell = (A["cy"][b][front][0], A["cx"][b][front][0])
        assert (A["cy"][b][front] == cell[0]).all() and (A["cx"][b][front] == cell[1]).all()       # the cell of the +x axis
        r2 = np.where(front, px[b] * px[b], np.inf).reshape(-1)
        assert src[b][cell] == int(np.argmin(r2))                       # argmin: the first of equals, the lower index
        assert len(set(np.round(np.sqrt(r2[np.isfinite(r2)]), 1))) > 2  # several distinct depths contended


def test_every_row_of_the_table_is_reached():
    for name in TC.CASES:
        for kind in TC.POSES:
            r = TC.step(name, kind)
            counts = np.bincount(r["B"]["row"].reshape(-1), minlength=5)
            print(f"[temporal] {name} {kind}: " + ", ".join(f"{n} {int(k)}" for n, k in zip(TC.ROWS, counts)))
            if TC.CASES[name]["bad"]:
                assert (counts > 0).all(), (name, kind, counts)
            else:
                assert counts[3] > 0 and counts[2] > 0                  # without bad values: fused pixels and the empty patch
    # the rows' outputs on one case, spelled out
    r = TC.step("waves", "rigid")
    Bs, inp = r["B"], r["inp"]
    row = Bs["row"]
    assert np.array_equal(Bs["fused"][row == 0].view(np.uint32), inp["cur_inv"][row == 0].view(np.uint32))          # passed through as it is
    assert np.isposinf(Bs["var"][row == 0]).all() and (Bs["age"][row == 0] == 0).all()
    assert np.array_equal(Bs["fused"][row == 1], Bs["warped_inv"][row == 1]) and np.array_equal(Bs["var"][row == 1], Bs["warped_var"][row == 1])
    for k in (2, 4):
        assert np.array_equal(Bs["fused"][row == k], inp["cur_inv"][row == k]) and (Bs["age"][row == k] == 1).all()
        assert np.array_equal(Bs["var"][row == k], np.square(inp["cur_std"][row == k]))
    both = row == 3
    assert (Bs["var"][both] <= Bs["warped_var"][both]).all() and (Bs["var"][both] <= np.square(inp["cur_std"][both]) * F32(1.0001)).all()
    lo, hi = np.minimum(Bs["warped_inv"], inp["cur_inv"]), np.maximum(Bs["warped_inv"], inp["cur_inv"])
    assert ((Bs["fused"][both] >= lo[both] * F32(0.9999)) & (Bs["fused"][both] <= hi[both] * F32(1.0001))).all()
    s_age = inp["prev_age"].reshape(inp["prev_age"].shape[0], -1)
    for b in range(row.shape[0]):
        assert np.array_equal(Bs["age"][b][both[b]], np.minimum(s_age[b][Bs["src"][b][both[b]]].astype(int) + 1, 255))
    assert (Bs["age"][both] == 255).any() or (inp["prev_age"] == 255).sum() < 2


@pytest.mark.parametrize("bf", TC.BFS)
def test_the_gate_margin_leaves_out_at_most_one_per_cent(bf):
    """The GPU test asks for the same decision where the float64 restatement is further than GATE_MARGIN from the gate: the seeds
    are chosen so that this leaves out at most 1 % of a case's pixels."""
    for name in TC.CASES:
        for kind in TC.POSES:
            m = TC.step(name, kind, bf)["B"]["margin"]
            out = int((m <= TC.GATE_MARGIN).sum())
            print(f"[temporal] {name} {kind} bf {bf:g}: {out} of {m.size} pixels within {TC.GATE_MARGIN:g} of the gate")
            assert out <= 0.01 * m.size, (name, kind, out)


def test_three_steps_of_a_static_scene_confirm_every_pixel():
    name = "b2"
    c = TC.CASES[name]
    aff, ray_table = TC.affine(c["ranges"], c["hw"]), TC.rays(name)
    scene = TC.make_inputs(name)["prev_inv"]
    scene = np.where(np.isfinite(scene) & (scene > 0), scene, F32(12.0)).astype(F32)                # a clean static scene
    std = (F32(0.02) * scene).astype(F32)
    state = (np.zeros_like(scene), np.zeros_like(scene), np.zeros(scene.shape, np.uint8))
    T = TC.poses("identity", name)
    variances = []
    for n in range(1, 4):
        A = TC.splat(state[0], state[2], ray_table, T, 96.0, aff)
        out = TC.fuse(A["zkey"], state, scene, std, 96.0, q_var=0.0)
        assert (out["row"] == (2 if n == 1 else 3)).all(), n            # the first step has no prior: measurement only
        assert (out["age"] == n).all()
        state = (out["fused"], out["var"], out["age"])
        variances.append(out["var"])
    assert (variances[1] < variances[0]).all() and (variances[2] < variances[1]).all()
    assert np.abs(state[0] / scene - 1).max() < 1e-5
