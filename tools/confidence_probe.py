#!/usr/bin/env python3
"""What do the confidence maps cost next to the soft-argmin?  

    timeout -k 10 600 python tools/confidence_probe.py [--out profiles/confidence_probe.json]

Costs [128, 16, 80, 320] (G16V's cost head output, 128 frames) at x2 and x4, four calls timed with HIP events in ONE process:
  (a) hip_ops.softargmin(want_norm_costs=False)            what inference runs today
  (b) hip_ops.softargmin(want_norm_costs=True)             the only way to the softmax before mvsgi_confidence_f32
                                                           (the torch reductions it then needs are NOT counted)
  (c) hip_ops.confidence, all four maps
  (d) hip_ops.confidence, max_prob only
20 warm-up and 200 timed launches per call and repetition, the four calls alternating within a repetition, median of 5
repetitions.  Condition: (a) + (c) <= (b) at both factors.  (c)'s achieved bytes/s counts its own traffic: the costs once plus
the maps it stores.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mvs_gi_amd import hip_ops as H  # noqa: E402

SHAPE = (128, 16, 80, 320)
WARMUP, TIMED, REPS = 20, 200, 5


def timed_us(fn) -> float:
    for _ in range(WARMUP):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(TIMED):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / TIMED


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confidence_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("confidence_probe: needs a GPU")
    dev = "cuda:0"
    B, D, Hh, W = SHAPE
    g = torch.Generator(device=dev).manual_seed(16)
    costs = torch.randn(SHAPE, device=dev, generator=g) * 4.0
    inv_idx = (96.0 / torch.logspace(-0.30103, 2.0, D, device=dev)).contiguous()
    res = {"shape": list(SHAPE), "warmup": WARMUP, "timed": TIMED, "repetitions": REPS, "device": torch.cuda.get_device_name(0),
           "factors": {}}
    for s in (2, 4):
        OH, OW = Hh * s, W * s
        out = {n: torch.empty((B, 1, OH, OW), device=dev, dtype=torch.int32 if n == "argmax" else torch.float32) for n in H.CONFIDENCE_MAPS}
        calls = {
            "a_softargmin": lambda: H.softargmin(costs, inv_idx, s, False),
            "b_softargmin_norm_costs": lambda: H.softargmin(costs, inv_idx, s, True),
            "c_confidence_all": lambda: H.confidence(costs, inv_idx, s, out=out),
            "d_confidence_max_prob": lambda: H.confidence(costs, inv_idx, s, want=("max_prob",), out=out),
        }
        runs = {k: [] for k in calls}
        for _ in range(REPS):
            for k, fn in calls.items():
                runs[k].append(timed_us(fn))
        med = {k: statistics.median(v) for k, v in runs.items()}
        bytes_c = costs.numel() * 4 + 4 * B * OH * OW * 4
        row = {"median_us": med, "runs_us": runs, "a_plus_c_us": med["a_softargmin"] + med["c_confidence_all"],
               "condition_a_plus_c_le_b": med["a_softargmin"] + med["c_confidence_all"] <= med["b_softargmin_norm_costs"],
               "c_bytes": bytes_c, "c_bytes_per_s": bytes_c / (med["c_confidence_all"] * 1e-6),
               "norm_costs_bytes": B * D * OH * OW * 4}
        res["factors"][f"x{s}"] = row
        print(f"x{s}: " + "  ".join(f"{k} {v:.1f} us" for k, v in med.items()) +
              f"  (a)+(c) {row['a_plus_c_us']:.1f} us {'<=' if row['condition_a_plus_c_le_b'] else '>'} (b);  "
              f"(c) moves {bytes_c / 1e6:.0f} MB at {row['c_bytes_per_s'] / 1e12:.2f} TB/s", flush=True)
        del out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
