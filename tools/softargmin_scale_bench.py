#!/usr/bin/env python3
"""A/B of the soft-argmin kernels at one scale factor on one box, interleaved in one process:

    python tools/softargmin_scale_bench.py [--scale 4] [--shape 128 16 80 320] [--rounds 5] [--iters 20]

Arms: the row-band kernel and the thread-per-pixel kernel (hip_ops.softargmin variant=SA_BAND | SA_PIXEL), each with
inv_dist only and with norm_costs, plus the x2 row-pair kernel on the same costs as the reference point.  Time: device events
around `iters` back-to-back launches, median over `rounds` (the arms alternate inside a round).  Bytes: the tensors once
(costs read + outputs written), which is what an ideal kernel moves."""
import argparse
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvs_gi_amd import hip_ops as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=4)
    ap.add_argument("--shape", type=int, nargs=4, default=[128, 16, 80, 320], metavar=("B", "D", "H", "W"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    B, D, Hh, W = a.shape
    g = torch.Generator(device="cuda").manual_seed(0)
    c = torch.randn((B, D, Hh, W), device="cuda", generator=g) * 4
    inv_idx = 96.0 / torch.logspace(-0.30103, 2, D, device="cuda")
    arms = {}
    for vname, variant in (("band", H.SA_BAND), ("pixel", H.SA_PIXEL)):
        for want in (False, True):
            arms[f"x{a.scale:g} {vname} {'+norm_costs' if want else 'inv_dist only'}"] = (a.scale, want, variant)
    for want in (False, True):
        arms[f"x2 row-pair {'+norm_costs' if want else 'inv_dist only'}"] = (2, want, H.SA_AUTO)

    def run(scale, want, variant):
        return H.softargmin(c, inv_idx, scale, want, variant=variant)

    ib, pb = run(a.scale, True, H.SA_BAND)
    ip, pp = run(a.scale, True, H.SA_PIXEL)
    for tag, x, y in (("inv_dist", ib, ip), ("norm_costs", pb, pp)):
        n = int((x != y).sum())
        ulp = int((x.view(torch.int32).long() - y.view(torch.int32).long()).abs().max()) if n else 0
        print(f"band vs pixel {tag}: {n} of {x.numel()} elements differ, max {ulp} ulp, max abs {float((x - y).abs().max()):.3e}")
    del ib, pb, ip, pp
    times = {k: [] for k in arms}
    for k, v in arms.items():                                  # warm-up: code objects, kernel attributes, the allocator's blocks
        for _ in range(3):
            run(*v)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, v in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                run(*v)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    print(f"costs [{B}, {D}, {Hh}, {W}] fp32, {a.rounds} rounds x {a.iters} launches, device events; us per launch")
    print(f"{'arm':34s} {'median':>9s} {'min':>9s} {'max':>9s} {'tensor MB':>10s} {'GB/s':>8s}")
    for k, (scale, want, _) in arms.items():
        OH, OW = int(Hh * scale), int(W * scale)
        mb = 4 * (B * D * Hh * W + B * OH * OW + (B * D * OH * OW if want else 0)) / 1e6
        med = statistics.median(times[k])
        print(f"{k:34s} {med:9.1f} {min(times[k]):9.1f} {max(times[k]):9.1f} {mb:10.1f} {mb / med * 1e3:8.0f}")


if __name__ == "__main__":
    main()
