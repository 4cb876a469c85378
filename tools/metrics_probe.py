#!/usr/bin/env python3
"""Time of one validation-metric evaluation (dropin.Evaluator: csrc/metrics.hip, all eight metrics of every frame and pooled) against
the six metrics of configs/base_model.yaml written with torch ops on the same device, at 1, 16 and 128 frames of 160 x 640.

The torch chain lives here, not in the package: clamp and scale, the label-range mask, RMSE / MAE as masked fp32 sums (torch.where
instead of the reference's boolean indexing, which synchronises the host and cannot be captured), the SSIM as a grouped 11 x 11
Gaussian convolution behind a reflect padding -- pooled over the batch, the direct and the distance form.  Both variants are
captured into a hipGraph each and replayed alternately in one process (rounds of `--steps` replays, the median round is
reported), so that clocks and neighbours are the same for both.

    python tools/metrics_probe.py [--batches 1,16,128] [--steps 20] [--rounds 7]      ->  profiles/metrics_probe.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mvs_gi_amd import dropin  # noqa: E402

DEV = "cuda:0"
BF, DIST_LIST = 96.0, [0.5, 1, 1.5, 2, 5, 10, 20, 30, 50, 100]


def torch_chain(preds, target, lo, hi, cmin, cmax, kernel):
    """-> [6] fp32: ssim, rmse, mae, ssim_dist, rmse_dist, mae_dist (pooled over the batch)"""
    v = (target >= lo) & (target <= hi)
    n = v.sum()
    out = []
    for inverse in (False, True):
        p, t = (1.0 / preds, 1.0 / target) if inverse else (preds, target)
        P, T = p / BF, torch.clamp(t, cmin, cmax) / BF
        e = torch.where(v, P - T, torch.zeros_like(P))
        R = torch.maximum(P.max() - P.min(), T.max() - T.min())
        c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        x = F.pad(torch.cat((P, T, P * P, T * T, P * T)), (5, 5, 5, 5), mode="reflect")
        mu_p, mu_t, pp, tt, pt = F.conv2d(x, kernel).split(P.shape[0])
        s_p, s_t, s_pt = pp - mu_p * mu_p, tt - mu_t * mu_t, pt - mu_p * mu_t
        m = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_p + s_t + c2))
        out += [m[..., 5:-5, 5:-5].mean(), torch.sqrt((e * e).sum() / n), e.abs().sum() / n]
    return torch.stack(out)


def capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fn()
    return g, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,128")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_probe.txt"))
    a = ap.parse_args()
    Hh, W = 160, 640
    k = torch.arange(-5, 6, dtype=torch.float32)
    g = torch.exp(-((k / 1.5) ** 2) / 2)
    g = (g / g.sum()).unsqueeze(0)
    kernel = (g.t() @ g).view(1, 1, 11, 11).to(DEV)
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# tools/metrics_probe.py on {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), torch {torch.__version__}; "
             f"{Hh} x {W}, hipGraph replays, {a.rounds} alternating rounds of {a.steps}, median round",
             f"# {'B':>4s} {'evaluator us':>13s} {'torch chain us':>15s} {'ratio':>7s} {'us/frame':>9s}   (evaluator: 8 metrics per frame + pooled; "
             "chain: 6 pooled metrics)"]
    for B in (int(b) for b in a.batches.split(",")):
        gen = torch.Generator().manual_seed(B)
        target = (2.0 + 60.0 * torch.rand(B, 1, Hh, W, generator=gen)).to(DEV)
        preds = torch.clamp(target * (1.0 + 0.05 * torch.randn(B, 1, Hh, W, generator=gen).to(DEV)), min=0.3)
        ev = dropin.Evaluator(bf=BF, dist_list=DIST_LIST, label_range=(0.96, 192.0), range_scope="batch")
        graphs = [capture(lambda: ev.evaluate(preds, target)),
                  capture(lambda: torch_chain(preds, target, 0.96, 192.0, ev.clamp_min, ev.clamp_max, kernel))]
        table, chain = graphs[0][1], graphs[1][1]
        for gr, _ in graphs:             # a capture runs nothing: the results exist after a replay
            gr.replay()
        torch.cuda.synchronize()
        agree = float((table[-1, [3, 0, 1, 7, 4, 5]].float() - chain).abs().max())
        times = ([], [])
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.rounds):
            for i, (gr, _) in enumerate(graphs):
                t0.record()
                for _ in range(a.steps):
                    gr.replay()
                t1.record()
                torch.cuda.synchronize()
                times[i].append(t0.elapsed_time(t1) * 1000.0 / a.steps)
        ours, theirs = statistics.median(times[0]), statistics.median(times[1])
        lines.append(f"  {B:4d} {ours:13.1f} {theirs:15.1f} {theirs / ours:7.2f} {ours / B:9.2f}   max |evaluator - chain| {agree:.2e}; "
                     f"rounds evaluator {min(times[0]):.1f} .. {max(times[0]):.1f}, chain {min(times[1]):.1f} .. {max(times[1]):.1f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
