#!/usr/bin/env python3
"""Time of the validation losses (vol_loss + distance_loss: VolumeCrossEntropy on norm_costs, smooth-L1 on inv_dist) behind the
regressor at 64 frames of the operating shape (costs [64, 16, 80, 320], x2 -> 160 x 640), three ways:

  (a) fused     soft-argmin without norm_costs, then LossEvaluator.evaluate(costs=...): the softmax is walked again per pixel,
                no [B, D, OH, OW] tensor exists
  (b) given     soft-argmin storing norm_costs, then LossEvaluator.evaluate(norm_costs=...)
  (c) torch     soft-argmin storing norm_costs, then the reference's composition with torch ops on the device (clamp, bucketize,
                two index selects, divide, zeros_like, two scatter_, binary_cross_entropy; smooth_l1_loss), unmasked: boolean indexing
                synchronises the host and cannot be captured

Every variant is captured into a hipGraph and the graphs are replayed alternately in one process (rounds of `--steps` replays
between two hipEvents, the median round is reported), so that clocks and neighbours are the same for all.  The parts are timed
alone as well.

    python tools/losses_probe.py [--frames 64] [--steps 10] [--rounds 7] [--out profiles/losses_probe.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mvs_gi_amd import dropin, hip_ops as H  # noqa: E402

DEV = "cuda:0"
BF = 96.0


def torch_losses(pred_cost, inv, lab, lst, flipped, widths):
    x = torch.clamp(lab, lst[-1], lst[0])
    b = len(lst) - torch.bucketize(x, flipped)
    b = torch.clamp(b - 1, min=0, max=len(lst) - 2).to(torch.long)
    flat = b.flatten()
    d = (x - lst[flat].view_as(b)) / widths[flat].view_as(b)
    t = torch.zeros_like(pred_cost)
    t.scatter_(1, b, 1 - d)
    t.scatter_(1, b + 1, d)
    return torch.stack((F.binary_cross_entropy(pred_cost, t, reduction="mean"), F.smooth_l1_loss(inv, lab)))


def capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fn()
    return g, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses_probe.txt"))
    a = ap.parse_args()
    B, D, Hh, W, s = a.frames, 16, 80, 320, 2
    OH, OW = Hh * s, W * s
    gen = torch.Generator().manual_seed(B)
    costs = torch.randn(B, D, Hh, W, generator=gen).to(DEV)
    lab = (0.2 + 229.8 * torch.rand(B, 1, OH, OW, generator=gen)).to(DEV)
    dist = [float(v) for v in np.geomspace(0.5, 100.0, D)]
    reg = dropin.DistanceRegressorWithFixedCandidates(bf=BF, dist_cands=dist, interp_scale_factor=s, pre_interp=True).to(DEV)
    lst = reg.inv_dist_idx.reshape(-1).contiguous()
    flipped, widths = torch.flip(lst, [0]), torch.diff(lst)
    ev = dropin.LossEvaluator.from_regressor(reg)
    inv, pr = H.softargmin(costs, lst, s, True)
    variants = {
        "soft-argmin, no norm_costs": lambda: H.softargmin(costs, lst, s, False)[0],
        "soft-argmin, norm_costs stored": lambda: H.softargmin(costs, lst, s, True)[0],
        "evaluate, fused": lambda: ev.evaluate(lab, pred=inv, costs=costs),
        "evaluate, given": lambda: ev.evaluate(lab, pred=inv, norm_costs=pr),
        "torch composition": lambda: torch_losses(pr, inv, lab, lst, flipped, widths),
        "(a) fused": lambda: ev.evaluate(lab, pred=H.softargmin(costs, lst, s, False)[0], costs=costs).clone(),
        "(b) given": lambda: (lambda r: ev.evaluate(lab, pred=r[0], norm_costs=r[1]).clone())(H.softargmin(costs, lst, s, True)),
        "(c) torch": lambda: (lambda r: torch_losses(r[1], r[0], lab, lst, flipped, widths))(H.softargmin(costs, lst, s, True)),
    }
    graphs = {k: capture(fn) for k, fn in variants.items()}
    for g, _ in graphs.values():            # a capture runs nothing: the results exist after a replay
        g.replay()
    torch.cuda.synchronize()
    fa, fb, fc = graphs["(a) fused"][1][-1, :2], graphs["(b) given"][1][-1, :2], graphs["(c) torch"][1]
    times = {k: [] for k in graphs}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for k, (g, _) in graphs.items():
            t0.record()
            for _ in range(a.steps):
                g.replay()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1000.0 / a.steps)
    mb = 1.0 / (1 << 20)
    vol, low, img = 4 * B * D * OH * OW * mb, 4 * B * D * Hh * W * mb, 4 * B * OH * OW * mb
    moved = {
        "soft-argmin, no norm_costs": f"reads costs {low:.0f} MiB, writes inv_dist {img:.0f} MiB",
        "soft-argmin, norm_costs stored": f"reads costs {low:.0f} MiB, writes inv_dist {img:.0f} + norm_costs {vol:.0f} MiB",
        "evaluate, fused": f"reads costs {low:.0f} (every tap of a pixel, from cache after the first) + labels, pred {2 * img:.0f} MiB",
        "evaluate, given": f"reads norm_costs {vol:.0f} + labels, pred {2 * img:.0f} MiB",
        "torch composition": f"reads norm_costs {vol:.0f} MiB, writes and reads true_cost {vol:.0f} MiB three times over (zeros_like, two scatter_, "
                             "the cross-entropy), and its image temporaries",
    }
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# tools/losses_probe.py on {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), torch {torch.__version__}; "
             f"costs [{B}, {D}, {Hh}, {W}] x{s} -> {OH} x {OW}, hipGraph replays, {a.rounds} alternating rounds of {a.steps}, median round",
             f"# pooled (vol, smooth_l1): fused {[float(v) for v in fa]}, given {[float(v) for v in fb]}, torch {[float(v) for v in fc]}"]
    for k, v in times.items():
        lines.append(f"  {k:32s} {statistics.median(v):10.1f} us   rounds {min(v):.1f} .. {max(v):.1f}   {moved.get(k, '')}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
