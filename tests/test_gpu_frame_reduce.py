"""GPU (MI355X): the order of the shared per-frame reduction (csrc/frame_reduce.hpp) pinned bit for bit, for each of the three tables
that use it: validation metrics, losses, photometric consistency.  Each op runs with a caller-owned workspace; the slab is copied back
and its records are summed here in numpy float64 -- the two-sum merge (sum_add, sum_merge, sum_value) restated, frame b's G records
in index order, then the frames' sums in frame order -- and put through the row formulas.  A float64 add, division and square root
in numpy are the IEEE operations the device runs, so rows 0 .. B are compared by their bits: no tolerance.  The shapes are the
smallest with G > 1 and B > 1, so that both orders matter.  The metrics' SSIM columns come from tile sums, not from records: they
are left out."""
import numpy as np
import pytest
import torch

import guard_arena
import losses_cases as LC
import metrics_cases as MC
import photo_cases as PC
import reproject_cases as RC
from mvs_gi_amd import dropin, hip_ops as H
from mvs_gi_amd.dropin import sweep_grids as SG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    yield from guard_arena.fixture_body(request)


# ------------------------------------------------------------------------------ csrc/frame_reduce.hpp, restated
def sum_add(h, l, x):
    t = h + x
    bp = t - h
    return t, l + ((h - (t - bp)) + (x - bp))


def sum_merge(h, l, bh, bl):
    h, l = sum_add(h, l, bh)
    return h, l + bl


def sum_value(h, l):
    return h + l if l - l == 0.0 else h


def sum_records(recs, pairs, counts):
    """recs [n, REC] float64 in index order -> the summed record: (hi, lo) index pairs by sum_merge, count indexes by a plain add."""
    x = np.zeros(recs.shape[1], np.float64)
    for r in recs:
        for h, l in pairs:
            x[h], x[l] = sum_merge(x[h], x[l], r[h], r[l])
        for c in counts:
            x[c] = x[c] + r[c]
    return x


def table_from_records(recs, pairs, counts, write_row):
    """recs [B, G, REC] -> (rows 0 .. B by the finaliser's order, the frames' sums [B, REC])"""
    with np.errstate(all="ignore"):
        frames = np.stack([sum_records(r, pairs, counts) for r in recs])
        return np.stack([write_row(x) for x in list(frames) + [sum_records(frames, pairs, counts)]]), frames


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    return got.shape == want.shape and bool(((got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))).all())


def _d(t):
    return t.to(DEV)


# ------------------------------------------------------------------------------ the three tables
def test_metrics_rows_are_the_records_summed_in_order():
    B, Hh, W = 2, 65, 67                       # 4355 pixels: two records per frame, and H * W % 4 != 0 (frame 1 starts off a 16-byte boundary)
    lay = H.metrics_ws_layout(B, Hh, W)
    assert lay["G"] == 2
    g = torch.Generator().manual_seed(65067)
    target = (2.0 + 60.0 * torch.rand(B, 1, Hh, W, generator=g, dtype=torch.float64) ** 3).to(torch.float32)
    preds = torch.clamp(target * (1.0 + 0.05 * torch.randn(B, 1, Hh, W, generator=g)) + 0.3 * torch.randn(B, 1, Hh, W, generator=g), min=0.3)
    cmin, cmax = MC.clamp_range()
    ws = torch.zeros(lay["total"], dtype=torch.float64, device=DEV)
    out = torch.full((B + 1, 9), float("nan"), dtype=torch.float64, device=DEV)
    H.metrics(_d(preds), _d(target), MC.BF, cmin, cmax, label_range=MC.LABEL_RANGE, thresh=MC.THRESH, thresh_dist=MC.THRESH_DIST, ws=ws, out=out)
    slab, got = ws.cpu().numpy(), out.cpu().numpy()
    S2H, S2L, S1H, S1L, NB, N = range(6)      # of a form's ten fields; the extrema feed the SSIM only
    rows, sums = [], []
    for f in range(2):                         # a record is [form][field]: each form is summed on its own, the same way
        def write_row(x):
            n = x[N]
            return [np.sqrt(sum_value(x[S2H], x[S2L]) / n), sum_value(x[S1H], x[S1L]) / n, x[NB] / n if n > 0.0 else 1.0, n]
        recs = slab[lay["records"]:lay["frame_sums"]].reshape(B, lay["G"], 2, 10)[:, :, f]
        r, s = table_from_records(recs, [(S2H, S2L), (S1H, S1L)], [NB, N], write_row)
        rows.append(r)
        sums.append(s)
        kept = slab[lay["frame_sums"]:lay["consts"]].reshape(B, 2, 10)[:, f, :6]
        assert same_bits(kept, s[:, :6]), f"form {f}: the frames' sums in the slab"
    assert int(rows[0][B, 3]) == int(rows[0][:B, 3].sum()) > 0 and 0 < rows[0][0, 3] < Hh * W       # the range selects some pixels, not all
    for f in range(2):
        assert same_bits(got[:, 4 * f:4 * f + 3], rows[f][:, :3]), f"form {f}: rmse, mae, bad"
    assert same_bits(got[:, 8], rows[0][:, 3])


def test_losses_rows_are_the_records_summed_in_order():
    B, D, OH, OW = 2, 4, 20, 30                # 600 pixels: three records per frame
    lay = H.losses_ws_layout(B, OH, OW)
    assert lay["G"] == 3
    g = torch.Generator().manual_seed(42030)
    lst = LC.inv_list(D)
    probs = torch.softmax(torch.randn(B, D, OH, OW, generator=g), dim=1).contiguous()
    labels = (0.2 + 229.8 * torch.rand(B, 1, OH, OW, generator=g, dtype=torch.float64)).to(torch.float32)
    pred = (labels + 0.8 * torch.randn(B, 1, OH, OW, generator=g)).contiguous()
    near, far = np.float32(1.0 / LC.NEAR_DIST), np.float32(1.0 / LC.FAR_DIST)
    ws = torch.zeros(lay["total"], dtype=torch.float64, device=DEV)
    out = torch.full((B + 1, 5), float("nan"), dtype=torch.float64, device=DEV)
    H.losses(_d(labels), _d(lst), pred=_d(pred), pred_cost=_d(probs), label_max=LC.LABEL_MAX, inbounds=(float(near), float(far)), ws=ws, out=out)
    VH, VL, SH, SL, NV, NP, MM, PAD = range(8)

    def write_row(x):
        return [sum_value(x[VH], x[VL]) / x[NV], sum_value(x[SH], x[SL]) / x[NP], 100.0 * x[MM] / x[NP], x[NV], x[NP]]
    slab = ws.cpu().numpy()
    recs = slab[lay["records"]:lay["frame_sums"]].reshape(B, lay["G"], 8)
    rows, sums = table_from_records(recs, [(VH, VL), (SH, SL)], [NV, NP, MM, PAD], write_row)
    assert same_bits(slab[lay["frame_sums"]:lay["total"]].reshape(B, 8), sums), "the frames' sums in the slab"
    assert rows[B, 3] == B * D * OH * OW and 0 < rows[0, 4] < OH * OW and rows[B, 2] > 0.0          # label_max selects some pixels, not all
    assert same_bits(out.cpu().numpy(), rows)


def test_photo_rows_are_the_records_summed_in_order():
    name = "waves_f32"                         # B = 3, 48 x 100: 1200 quads, five records per frame
    s, inp = PC.spec(name), PC.make_inputs(name)
    B, (Ho, Wo) = s["B"], s["hw"]
    lay = H.photo_ws_layout(B, Ho, Wo)
    assert lay["G"] == 5 and B == 3
    makers = [SG.EquirectangularSampleGridMaker() if s["all_eq"] or k % 2 else SG.DoubleSphereSampleGridMaker(RC.DS_PARAMS, RC.DS_CALIB)
              for k in range(s["N"])]
    rp = dropin.Reprojector(makers, RC.poses(s["base"]), s["hw"], RC.LON, RC.LAT, bf=RC.BF, device=DEV)
    ws = torch.zeros(lay["total"], dtype=torch.float64, device=DEV)
    table = torch.full((B + 1, 14), float("nan"), dtype=torch.float64, device=DEV)
    H.photo_consistency(_d(inp["inv"]), rp.rays, rp.T, rp.cams, rp.bf, _d(inp["imgs"]), cam_masks=_d(inp["cam_masks"]), mask=_d(inp["mask"]),
                        thresh=PC.THRESH, want=("table",), ws=ws, table=table)
    SH, SL, VH, VL, NB, N, NM, V0 = range(8)

    def write_row(x):
        n, nan = x[N], float("nan")
        return [n, sum_value(x[SH], x[SL]) / n if n > 0.0 else nan, np.sqrt(sum_value(x[VH], x[VL]) / n) if n > 0.0 else nan,
                x[NB] / n if n > 0.0 else nan, n / x[NM]] + list(x[V0:V0 + 9])
    slab = ws.cpu().numpy()
    recs = slab[lay["records"]:lay["frame_sums"]].reshape(B, lay["G"], 16)
    rows, sums = table_from_records(recs, [(SH, SL), (VH, VL)], list(range(NB, 16)), write_row)
    assert same_bits(slab[lay["frame_sums"]:lay["total"]].reshape(B, 16), sums), "the frames' sums in the slab"
    assert rows[B, 0] == rows[:B, 0].sum() > 0 and rows[B, 3] > 0.0
    assert same_bits(table.cpu().numpy(), rows)
