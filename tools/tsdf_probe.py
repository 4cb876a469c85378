#!/usr/bin/env python3
"""The volumetric fusion (csrc/tsdf.hip) on the device, against the composition it is defined by; one process, hipGraph replays, the
routes alternated round by round; one JSON line per measurement, also written to profiles/tsdf_probe.txt (started afresh by every
run).  It also writes profiles/tsdf_resources.txt: registers, scratch and LDS of the kernels of csrc/tsdf.hip, by
tools/kernel_resources.py on the build's object.

    python tools/tsdf_probe.py [--sequences 1,8,64] [--rounds 5] [--steps 20] [--chain-up-to 64]
    python tools/tsdf_probe.py --resources-only          # the resources file alone; needs no GPU

  S independent sequences of inverse distance at 160 x 640 on the full sphere (a smooth surface 2 ... 5 m away with depth steps) and a
  volume of 256 x 256 x 64 voxels of 5 cm around the rig (32 MiB per sequence); the rig has moved 5 cm and yawed 1 degree:
    integrate    hip_ops.tsdf_integrate on a volume that already holds the scene, with std (the weighted form), at rest
    raycast      hip_ops.tsdf_raycast of that volume, all three outputs (t0 = 0.1 m, step = voxel / 2, K samples to 6.4 m)
    stage        TsdfVolume.integrate + raycast as the pipeline runs them, at the staged pose (a scroll costs nothing extra: the fresh
                 test is evaluated for every slot of every integrate)
    chain_integrate, chain_raycast   TsdfVolume.integrate_chain / raycast_chain on the same volume: the composition in torch -- the
                 yardstick of a stage that has no predecessor (only up to --chain-up-to sequences: the chain's dense
                 temporaries are 1 GiB each at 64 sequences)
  bits_equal: the ray-cast of the kernels and of raycast_chain are the same bits, before and after the timed replays; differing: the
  values of the integrated volume that differ from integrate_chain's (torch's own root is in the composition).
  Numbers are reported, not asserted.
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
LOG = os.path.join(ROOT, "profiles", "tsdf_probe.txt")
RESOURCES = os.path.join(ROOT, "profiles", "tsdf_resources.txt")
KERNELS = ("tsdf_integrate_kernel", "tsdf_raycast_kernel")
DIMS, VOXEL, OUT_HW = (256, 256, 64), 0.05, (160, 640)


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
    n = {k: min(20000, max(steps, int(window_us / max(r.us(3), 0.5)))) for k, r in routes.items()}
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, r in routes.items():
            t[k].append(r.us(n[k]))
    return {k: statistics.median(v) for k, v in t.items()}, {k: [round(x, 1) for x in v] for k, v in t.items()}


def step_pose(S, n):
    """The rig after n steps of 5 cm forward and to the side and 1 degree of yaw"""
    a = math.radians(1.0 * n)
    P = np.eye(4)
    P[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    P[:3, 3] = [0.03 * n, 0.0, 0.04 * n]
    return torch.from_numpy(P.astype(np.float32)).repeat(S, 1, 1).to(DEV)


def rows(sequences, rounds, steps, chain_up_to):
    g = torch.Generator(device=DEV).manual_seed(0)
    rp = dropin.Reprojector([SG.EquirectangularSampleGridMaker()], [torch.eye(4, dtype=torch.float64)], OUT_HW, LON, LAT, bf=96.0, device=DEV)
    for S in sequences:
        march = (0.1, 6.4, None)
        v, moving = dropin.TsdfVolume(rp, DIMS, VOXEL, march=march), dropin.TsdfVolume(rp, DIMS, VOXEL, march=march)
        lat = torch.linspace(0.0, 3.0, OUT_HW[0], device=DEV).view(1, -1, 1)
        lon = torch.linspace(0.0, 12.0, OUT_HW[1], device=DEV).view(1, 1, -1)
        ph = torch.rand((S, 1, 1), device=DEV, generator=g) * 6.28
        d = 3.5 + 1.2 * torch.sin(lon + ph) * torch.cos(lat) + torch.where(torch.sin(3.0 * lon + 2.0 * ph) > 0.6, -1.0, 0.0)
        inv = (torch.full_like(d, 96.0) / d).contiguous()
        std = (0.02 * inv).contiguous()
        for vol in (v, moving):                                           # the volumes hold the scene, seen from two places
            vol.integrate(inv, std)
            vol.integrate(inv, std, P=step_pose(S, 1))
        b = v.buffers(S)
        outs = {k: torch.empty_like(t) for k, t in b["out"].items()}
        scratch = b["vol"].clone()                                        # the integrate alone runs on a copy: the volume stays as it is

        def stage():
            moving.integrate(inv, std)
            return moving.raycast(B=S)
        args = (rp.bf, v.affine, v.voxel, v.trunc, v.w_max, v.r_range)
        routes = {"integrate": Replay(lambda: H.tsdf_integrate(scratch, inv, b["T"], b["origin"], b["origin_prev"], *args, std=std)),
                  "raycast": Replay(lambda: H.tsdf_raycast(b["vol"], rp.rays, b["P"], b["origin_prev"], rp.bf, v.voxel, v.t0, v.step, v.K, v.w_min,
                                                           out=outs)),
                  "stage": Replay(stage)}
        chains = S <= chain_up_to
        if chains:
            routes["chain_integrate"] = Replay(lambda: v.integrate_chain(b["vol"], inv, std)["vol"])
            routes["chain_raycast"] = Replay(lambda: v.raycast_chain(b["vol"]))
        same = lambda: all(bool(torch.equal(outs[k].view(torch.uint8), routes["chain_raycast"].out[k].contiguous().view(torch.uint8))) for k in outs)
        ok = same() if chains else None
        med, raw = alternate(routes, rounds, steps)
        ok = (ok and same()) if chains else None
        row = dict(what="tsdf", sequences=S, out_hw=OUT_HW, dims=DIMS, voxel=VOXEL, K=v.K, hit_share=round(float((outs["steps"] < v.K).float().mean()), 4),
                   mean_steps=round(float(outs["steps"].float().mean()), 1), us_integrate=round(med["integrate"], 1), us_raycast=round(med["raycast"], 1),
                   us_stage=round(med["stage"], 1), us_integrate_per_sequence=round(med["integrate"] / S, 2),
                   integrate_GB_per_s=round(16e-3 * S * DIMS[0] * DIMS[1] * DIMS[2] / med["integrate"], 1),
                   voxels_per_us=round(S * DIMS[0] * DIMS[1] * DIMS[2] / med["integrate"], 1))
        if chains:
            once = H.tsdf_integrate(b["vol"].clone(), inv, b["T"], b["origin"], b["origin_prev"], *args, std=std)
            row.update(us_chain_integrate=round(med["chain_integrate"], 1), us_chain_raycast=round(med["chain_raycast"], 1),
                       chain_over_integrate=round(med["chain_integrate"] / med["integrate"], 2),
                       chain_over_raycast=round(med["chain_raycast"] / med["raycast"], 2), bits_equal=ok,
                       differing=int((once != routes["chain_integrate"].out).sum()))
        emit(rounds=raw, **row)
        del routes, v, moving, b, outs, scratch, inv, std, d
        torch.cuda.empty_cache()


def write_resources():
    """tools/kernel_resources.py on the object of the build (build/obj, where build() leaves it), the rows of this stage's kernels ->
    profiles/tsdf_resources.txt; None where the object is not at hand (a tree that received the library alone)"""
    objs = [os.path.join(ROOT, "build", "obj", "tsdf.hip.o")]
    if not all(os.path.isfile(o) for o in objs):
        return None
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")] + objs, check=True, capture_output=True,
                         text=True).stdout
    rows = [line for line in txt.split("\n") if any(f"::{k}" in line for k in KERNELS)]
    if not rows:
        raise SystemExit(f"no kernel of csrc/tsdf.hip in {objs}")
    os.makedirs(os.path.dirname(RESOURCES), exist_ok=True)
    with open(RESOURCES, "w") as f:
        f.write("# tools/tsdf_probe.py: tools/kernel_resources.py on build/obj/tsdf.hip.o (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off),\n"
                "# the kernels of csrc/tsdf.hip.  Scratch 0, LDS 0 and no spills are expected in every row.\n")
        f.write("\n".join(rows) + "\n")
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", default="1,8,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--chain-up-to", type=int, default=64)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    n = write_resources()
    print(f"{RESOURCES}: {n} kernels" if n else f"{RESOURCES}: left as it is (no build/obj objects here)", flush=True)
    if a.resources_only:
        return
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_probe needs a GPU")
    if os.path.exists(LOG):
        os.remove(LOG)
    emit(what="library", path=os.environ.get("MVSGI_LIB", "default"), device=torch.cuda.get_device_name(0))
    rows([int(s) for s in a.sequences.split(",")], a.rounds, a.steps, a.chain_up_to)


if __name__ == "__main__":
    main()
