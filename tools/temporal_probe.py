#!/usr/bin/env python3
"""The temporal fusion (csrc/temporal.hip) on the device, against the composition it is defined by; one process, hipGraph replays, the
routes alternated round by round; one JSON line per measurement, also written to profiles/temporal_probe.txt (started afresh by every
run).  It also writes profiles/temporal_resources.txt: registers, scratch and LDS of the kernels of csrc/temporal.hip, by
tools/kernel_resources.py on the build's object.

    python tools/temporal_probe.py [--frames 1,16,128] [--rounds 5] [--steps 20]
    python tools/temporal_probe.py --resources-only          # the resources file alone; needs no GPU

  F independent sequences of inverse distance at 160 x 640 on the full sphere, a smooth surface with depth steps; the pose of every
  step is a 5 cm translation plus a 1 degree yaw:
    stage        TemporalFusion.step(inv, std) with the staged pose: fill, splat, fuse and the three copies into the state -- the stage
                 as a consumer uses it (its state moves on with every replay)
    splat        hip_ops.temporal_splat alone on a fixed state (fill + splat): atomics_per_us is what the 64-bit integer minimum
                 achieved in this shape
    fuse         hip_ops.temporal_fuse alone on that state's zkey
    composition  TemporalFusion.evaluate_chain on the same fixed state: Reprojector.reproject(want = xyz), the transform and
                 equirectangular grid kernels, torch's scatter_reduce(amin) on int64 keys and the fuse in torch
  bits_equal: zkey, src and age of splat + fuse and of the composition on the fixed state are the same bits, before and after the
  timed replays; differing: the elements of fused and var that differ (torch's own root is in the composition).
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mvs_gi_amd import dropin, hip_ops as H  # noqa: E402
from mvs_gi_amd.dropin import sweep_grids as SG  # noqa: E402

DEV = "cuda:0"
LON, LAT = (-math.pi, math.pi), (0.0, math.pi)
LOG = os.path.join(ROOT, "profiles", "temporal_probe.txt")
RESOURCES = os.path.join(ROOT, "profiles", "temporal_resources.txt")
KERNELS = ("temporal_fill_kernel", "temporal_splat_kernel", "temporal_fuse_kernel")
EXACT = ("zkey", "src", "age")


def emit(**row):
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")


class Replay:
    """fn() captured into a hipGraph after a warm-up; us(steps) = microseconds per replay (device events)."""

    def __init__(self, fn):
        fn()
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = fn()
        for _ in range(3):
            self.graph.replay()
        torch.cuda.synchronize()

    def us(self, steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            self.graph.replay()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / steps


def alternate(routes, rounds, steps, window_us=100e3):
    """Median over `rounds` of each route's time per replay, the routes alternated; every timed window holds at least `steps`
    replays and about `window_us` of device time (a window of a few replays of a few microseconds measures the clock)."""
    n = {k: min(20000, max(steps, int(window_us / max(r.us(10), 0.5)))) for k, r in routes.items()}
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, r in routes.items():
            t[k].append(r.us(n[k]))
    return {k: statistics.median(v) for k, v in t.items()}, {k: [round(x, 1) for x in v] for k, v in t.items()}


def step_pose(B):
    """5 cm forward and to the side, 1 degree of yaw"""
    a = math.radians(1.0)
    T = np.eye(4)
    T[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    T[:3, 3] = [0.03, 0.0, 0.04]
    return torch.from_numpy(T.astype(np.float32)).repeat(B, 1, 1).to(DEV)


def same_bits(a, b):
    return all(bool(torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8))) for k in EXACT)


def rows(frames, rounds, steps):
    g = torch.Generator(device=DEV).manual_seed(0)
    out_hw = (160, 640)
    rp = dropin.Reprojector([SG.EquirectangularSampleGridMaker()], [torch.eye(4, dtype=torch.float64)], out_hw, LON, LAT, bf=96.0, device=DEV)
    for Fr in frames:
        tf = dropin.TemporalFusion(rp, q_var=1e-6)
        # a smooth surface with depth steps: the scenes the stage is for
        lat = torch.linspace(0.0, 3.0, out_hw[0], device=DEV).view(1, -1, 1)
        lon = torch.linspace(0.0, 12.0, out_hw[1], device=DEV).view(1, 1, -1)
        ph = torch.rand((Fr, 1, 1), device=DEV, generator=g) * 6.28
        d = 8.0 + 3.0 * torch.sin(lon + ph) * torch.cos(lat) + torch.where(torch.sin(3.0 * lon + 2.0 * ph) > 0.6, -3.5, 0.0)
        inv = (torch.full_like(d, 96.0) / d).contiguous()
        std = (0.02 * inv).contiguous()
        T = step_pose(Fr)
        state = (inv.clone(), (0.03 * inv) ** 2, torch.ones(inv.shape, device=DEV, dtype=torch.uint8))
        tf.step(inv, std)                                                # the sequences start: the state is the measurement
        tf.set_pose(T)
        zkey = torch.empty(inv.shape, device=DEV, dtype=torch.int64)
        outs = H.temporal_fuse(H.temporal_splat(state[0], state[2], rp.rays, T, rp.bf, tf.affine, out=zkey), *state, inv, rp.bf, gate=tf.gate,
                               q_var=tf.q_var, cur_std=std)
        routes = {"stage": Replay(lambda: tf.step(inv, std)),
                  "splat": Replay(lambda: H.temporal_splat(state[0], state[2], rp.rays, T, rp.bf, tf.affine, out=zkey)),
                  "fuse": Replay(lambda: H.temporal_fuse(zkey, *state, inv, rp.bf, gate=tf.gate, q_var=tf.q_var, cur_std=std, out=outs)),
                  "composition": Replay(lambda: tf.evaluate_chain(inv, std, T=T, state=state))}
        chain = routes["composition"].out
        mine = dict(outs, zkey=zkey)
        same = same_bits(mine, chain)
        med, raw = alternate(routes, rounds, steps)
        same = same and same_bits(mine, chain)
        differing = {k: int((mine[k] != chain[k]).sum()) for k in ("warped_inv", "fused", "var")}
        cells = Fr * out_hw[0] * out_hw[1]
        emit(what="temporal", frames=Fr, out_hw=out_hw, gate=tf.gate, cells_filled=round(float((zkey != H.TEMPORAL_EMPTY).float().mean()), 4),
             fused_share=round(float((outs["age"] >= 2).float().mean()), 4), us_stage=round(med["stage"], 1), us_splat=round(med["splat"], 1),
             us_fuse=round(med["fuse"], 1), us_composition=round(med["composition"], 1),
             composition_over_stage=round(med["composition"] / med["stage"], 2), us_stage_per_frame=round(med["stage"] / Fr, 2),
             atomics_per_us=round(cells / med["splat"], 1), atomic_GB_per_s=round(8e-3 * cells / med["splat"], 1), bits_equal=same,
             differing=differing, rounds=raw)
        del inv, std, d, state, zkey, outs, routes, chain, mine, tf
        torch.cuda.empty_cache()


def write_resources():
    """tools/kernel_resources.py on the object of the build (build/obj, where build() leaves it), the rows of this stage's kernels ->
    profiles/temporal_resources.txt; None where the object is not at hand (a tree that received the library alone)"""
    objs = [os.path.join(ROOT, "build", "obj", "temporal.hip.o")]
    if not all(os.path.isfile(o) for o in objs):
        return None
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")] + objs, check=True, capture_output=True,
                         text=True).stdout
    rows = [line for line in txt.split("\n") if any(f"::{k}" in line for k in KERNELS)]
    if not rows:
        raise SystemExit(f"no kernel of csrc/temporal.hip in {objs}")
    os.makedirs(os.path.dirname(RESOURCES), exist_ok=True)
    with open(RESOURCES, "w") as f:
        f.write("# tools/temporal_probe.py: tools/kernel_resources.py on build/obj/temporal.hip.o (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off),\n"
                "# the kernels of csrc/temporal.hip.  Scratch 0 and no spills are expected in every row.\n")
        f.write("\n".join(rows) + "\n")
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,16,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    n = write_resources()
    print(f"{RESOURCES}: {n} kernels" if n else f"{RESOURCES}: left as it is (no build/obj objects here)", flush=True)
    if a.resources_only:
        return
    if not torch.cuda.is_available():
        raise SystemExit("temporal_probe needs a GPU")
    if os.path.exists(LOG):
        os.remove(LOG)
    emit(what="library", path=os.environ.get("MVSGI_LIB", "default"), device=torch.cuda.get_device_name(0))
    rows([int(f) for f in a.frames.split(",")], a.rounds, a.steps)


if __name__ == "__main__":
    main()
