#!/usr/bin/env python3
"""The camera range images and the visibility test (csrc/visibility.hip) on the device, against the composition they are defined by;
one process, hipGraph replays, the routes alternated round by round; one JSON line per measurement, also written to
profiles/visibility_probe.txt (started afresh by every run).  It also writes profiles/visibility_resources.txt: registers, scratch
and LDS of the kernels of csrc/visibility.hip and csrc/photo.hip, by tools/kernel_resources.py on the build's objects.

    python tools/visibility_probe.py [--frames 1,16,128] [--rounds 5] [--steps 20] [--no-pipeline]
    python tools/visibility_probe.py --resources-only          # the resources file alone; needs no GPU

  F frames of inverse distance at 160 x 640, three equirectangular cameras on a ring, buffer 320 x 640 (the default, (2 H, W)):
    fused        Visibility.evaluate(want = visible + n_visible): fill, splat, test -- the stage as a consumer uses it
    fused_all    the same with the range image too (one more launch)
    splat        hip_ops.camera_range alone (fill + splat): atomics_per_us is what the integer minimum achieved in this shape
    composition  Visibility.evaluate_chain(want = z2 + visible + n_visible): Reprojector.reproject(want = xyz + grid + valid), the
                 transform kernel per camera, torch's scatter_reduce(amin) and the comparison
  bits_equal: z2, visible and n_visible of the two routes are the same bits, before and after the timed replays.
  The pipeline rows: one frame of G16V (bf16 split) through InferencePipeline's captured graph with a reprojector, and with the stage
  behind it.
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

from mvs_gi_amd import dropin, hip_ops as H, synth  # noqa: E402
from mvs_gi_amd.configs import CONFIGS  # noqa: E402
from mvs_gi_amd.dropin import sweep_grids as SG  # noqa: E402
from mvs_gi_amd.pipeline import InferencePipeline  # noqa: E402

DEV = "cuda:0"
CAMS = 3
LON, LAT = (0.0, 2 * math.pi), (-math.pi / 2, 0.0)
LOG = os.path.join(ROOT, "profiles", "visibility_probe.txt")
RESOURCES = os.path.join(ROOT, "profiles", "visibility_resources.txt")
KERNELS = ("fill_kernel", "range_splat_kernel", "visibility_kernel", "range_kernel", "photo_reduce", "photo_finalise")
EXACT = ("z2", "visible", "n_visible")


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


def ring_poses(n, radius=0.1):
    poses = []
    for i in range(n):
        a = 2 * math.pi * i / n
        T = np.eye(4)
        T[:3, :3] = np.array([[math.cos(0.3 * a), 0, math.sin(0.3 * a)], [0, 1, 0], [-math.sin(0.3 * a), 0, math.cos(0.3 * a)]])
        T[:3, 3] = [radius * math.cos(a), 0.02 * i, radius * math.sin(a)]
        poses.append(torch.from_numpy(T))
    return poses


def reprojector(out_hw, bf, cams=CAMS):
    return dropin.Reprojector([SG.EquirectangularSampleGridMaker() for _ in range(cams)], ring_poses(cams), out_hw, LON, LAT, bf=bf, device=DEV)


def same_bits(a, b):
    return all(bool(torch.equal(a[k].view(torch.uint8), b[k].contiguous().view(torch.uint8))) for k in EXACT)


def rows(frames, rounds, steps):
    g = torch.Generator(device=DEV).manual_seed(0)
    out_hw = (160, 640)
    rp = reprojector(out_hw, 96.0)
    vis = dropin.Visibility(rp)
    for Fr in frames:
        # a smooth surface with depth steps: the scenes the stage is for (white noise would occlude almost everything)
        lat = torch.linspace(0.0, 3.0, out_hw[0], device=DEV).view(1, -1, 1)
        lon = torch.linspace(0.0, 12.0, out_hw[1], device=DEV).view(1, 1, -1)
        ph = torch.rand((Fr, 1, 1), device=DEV, generator=g) * 6.28
        d = 8.0 + 3.0 * torch.sin(lon + ph) * torch.cos(lat) + torch.where(torch.sin(3.0 * lon + 2.0 * ph) > 0.6, -3.5, 0.0)
        inv = (torch.full_like(d, 96.0) / d).contiguous()
        out = {k: v.clone() for k, v in vis.evaluate(inv).items()}
        few = {k: out[k] for k in ("visible", "n_visible", "z2")}
        z2_alone = out["z2"].clone()
        routes = {"fused": Replay(lambda inv=inv: vis.evaluate(inv, want=("visible", "n_visible"), out=few)),
                  "fused_all": Replay(lambda inv=inv: vis.evaluate(inv, out=out)),
                  "splat": Replay(lambda inv=inv: H.camera_range(inv, rp.rays, rp.T, rp.cams, rp.bf, vis.zshape, out=z2_alone)),
                  "composition": Replay(lambda inv=inv: vis.evaluate_chain(inv, want=EXACT))}
        chain = routes["composition"].out
        same = same_bits(out, chain)
        med, raw = alternate(routes, rounds, steps)
        same = same and same_bits(out, chain)
        pairs = Fr * CAMS * out_hw[0] * out_hw[1]
        emit(what="visibility", frames=Fr, cams=CAMS, out_hw=out_hw, zshape=vis.zshape, tol=vis.tol, footprint=vis.footprint,
             visible_share=round(float(out["visible"].float().mean()), 4), cells_filled=round(float(torch.isfinite(out["z2"]).float().mean()), 4),
             us_fused=round(med["fused"], 1), us_fused_all=round(med["fused_all"], 1), us_splat=round(med["splat"], 1),
             us_composition=round(med["composition"], 1), composition_over_fused=round(med["composition"] / med["fused"], 2),
             us_fused_per_frame=round(med["fused"] / Fr, 2), atomics_per_us=round(pairs / med["splat"], 1),
             atomic_GB_per_s=round(4e-3 * pairs / med["splat"], 1), bits_equal=same, rounds=raw)
        del inv, d, out, few, z2_alone, routes, chain
        torch.cuda.empty_cache()


def pipeline_rows(rounds, steps):
    # random images through synthetic weights leave the fp16 split's range (the range report raises); the bf16 split has fp32's range,
    # and what the stage adds behind the soft-argmin does not depend on the convolutions' arithmetic
    H.set_conv_mode("bf16x3")
    cfg = CONFIGS["G16V"]
    w = synth.make_weights(cfg, seed=0)
    w["feature_extractor"] = synth.make_extractor_weights(0)
    inp = synth.make_inputs(cfg, seed=0, batch=1)
    g = torch.Generator(device=DEV).manual_seed(1)
    views = torch.randint(0, 256, (cfg.num_cams, 4 * cfg.feat_hw[0], 4 * cfg.feat_hw[1], 3), device=DEV, generator=g, dtype=torch.uint8)
    out_hw = tuple(InferencePipeline(cfg, w, inp, device=DEV).forward_device(views).shape[-2:])
    rp = reprojector(out_hw, 1.0, cfg.num_cams)
    plain = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp)
    with_v = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp, visibility=dropin.Visibility(rp))
    routes = {"pipeline_reprojector": Replay(lambda: plain.forward_device(views)),
              "pipeline_visibility": Replay(lambda: with_v.forward_device(views))}
    med, raw = alternate(routes, rounds, steps)
    emit(what="pipeline", config=cfg.tag, mode=H.get_conv_mode(), out_hw=out_hw, us={k: round(v, 1) for k, v in med.items()},
         us_difference=round(med["pipeline_visibility"] - med["pipeline_reprojector"], 1), rounds=raw)


def write_resources():
    """tools/kernel_resources.py on the two objects of the build (build/obj, where build() leaves them), the rows of this stage's
    kernels -> profiles/visibility_resources.txt; None where the objects are not at hand (a tree that received the library alone)"""
    objs = [os.path.join(ROOT, "build", "obj", s + ".o") for s in ("visibility.hip", "photo.hip")]
    if not all(os.path.isfile(o) for o in objs):
        return None
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")] + objs, check=True, capture_output=True,
                         text=True).stdout
    rows = [line for line in txt.split("\n") if any(f"::{k}" in line for k in KERNELS)]
    if not rows:
        raise SystemExit(f"no kernel of csrc/visibility.hip in {objs}")
    os.makedirs(os.path.dirname(RESOURCES), exist_ok=True)
    with open(RESOURCES, "w") as f:
        f.write("# tools/visibility_probe.py: tools/kernel_resources.py on build/obj/{visibility,photo}.hip.o (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off),\n"
                "# the kernels of csrc/visibility.hip and csrc/photo.hip.  Scratch 0 and no spills are expected in every row.\n")
        f.write("\n".join(rows) + "\n")
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,16,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    n = write_resources()
    print(f"{RESOURCES}: {n} kernels" if n else f"{RESOURCES}: left as it is (no build/obj objects here)", flush=True)
    if a.resources_only:
        return
    if not torch.cuda.is_available():
        raise SystemExit("visibility_probe needs a GPU")
    if os.path.exists(LOG):
        os.remove(LOG)
    emit(what="library", path=os.environ.get("MVSGI_LIB", "default"), device=torch.cuda.get_device_name(0))
    rows([int(f) for f in a.frames.split(",")], a.rounds, a.steps)
    if not a.no_pipeline:
        pipeline_rows(a.rounds, a.steps)


if __name__ == "__main__":
    main()
