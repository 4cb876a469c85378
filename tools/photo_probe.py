#!/usr/bin/env python3
"""The photometric consistency (csrc/photo.hip) on the device, against the composition it is defined by; one process, hipGraph
replays, the routes alternated round by round; one JSON line per measurement, also appended to profiles/photo_probe.txt.

    python tools/photo_probe.py [--frames 1,16,128] [--rounds 5] [--steps 20]

  F frames of inverse distance at 160 x 640 with three 512 x 2048 uint8 surrogate views (equirectangular cameras) and with three
  1028 x 1224 raw frames (double-sphere cameras behind R_raw_fisheye):
    fused_std    PhotoConsistency.evaluate(want = photo_std + table): the reduce and the finalise launch; 4 bytes per pixel leave it
    fused_all    the same with every plane (n_views, photo_var, photo_std, mean_colour): 21 bytes per pixel
    composition  PhotoConsistency.evaluate_chain(want = the four planes): Reprojector.reproject(want = warped + valid) -- 39 bytes
                 per pixel and three cameras written, then read back -- and the fusion rule as torch launches.  Its table is left
                 out of the replay (evaluate_chain's docstring says why) and evaluated once, eagerly, for table_max_rel_diff.
  bits_equal: n_views, photo_var and mean_colour of fused_all and of the composition are the same bits, before and after the
  timed replays.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mvs_gi_amd import dropin, hip_ops as H  # noqa: E402
from mvs_gi_amd.dropin import sweep_grids as SG  # noqa: E402

DEV = "cuda:0"
CAMS = 3
LON, LAT = (0.0, 2 * math.pi), (-math.pi / 2, 0.0)
DS = (-0.203, 0.589, 232.0, 232.0, 611.5, 513.5)
LOG = os.path.join(ROOT, "profiles", "photo_probe.txt")


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
        T[:3, :3] = rotation_y(0.3 * a)
        T[:3, 3] = [radius * math.cos(a), 0.02 * i, radius * math.sin(a)]
        poses.append(torch.from_numpy(T))
    return poses


def rotation_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def make_reprojector(kind, out_hw, bf):
    poses = ring_poses(CAMS)
    if kind == "views_512x2048":
        rp = dropin.Reprojector([SG.EquirectangularSampleGridMaker() for _ in range(CAMS)], poses, out_hw, LON, LAT, bf=bf, device=DEV)
        img_hw = (512, 2048)
    else:
        rp = dropin.Reprojector([SG.DoubleSphereSampleGridMaker(DS, (1028, 1224)) for _ in range(CAMS)], poses, out_hw, LON, LAT, bf=bf,
                                R_raw=[rotation_y(2 * math.pi * k / CAMS) for k in range(CAMS)], device=DEV)
        img_hw = (1028, 1224)
    return rp, img_hw


def rows(frames, rounds, steps):
    g = torch.Generator(device=DEV).manual_seed(0)
    out_hw = (160, 640)
    for kind in ("views_512x2048", "raw_1028x1224"):
        rp, img_hw = make_reprojector(kind, out_hw, 96.0)
        pc = dropin.PhotoConsistency(rp)
        for Fr in frames:
            imgs = torch.randint(0, 256, (Fr * CAMS, *img_hw, 3), device=DEV, generator=g, dtype=torch.uint8)
            d = torch.exp(torch.rand((Fr, *out_hw), device=DEV, generator=g) * math.log(200.0) + math.log(0.5))
            inv = torch.full_like(d, 96.0) / d
            out = {k: v.clone() for k, v in pc.evaluate(inv, imgs).items()}
            std_only = {k: out[k].clone() for k in ("photo_std", "table")}
            routes = {"fused_std": Replay(lambda inv=inv, imgs=imgs: pc.evaluate(inv, imgs, want=("photo_std", "table"), out=std_only)),
                      "fused_all": Replay(lambda inv=inv, imgs=imgs: pc.evaluate(inv, imgs, out=out)),
                      "composition": Replay(lambda inv=inv, imgs=imgs: pc.evaluate_chain(inv, imgs, want=H.PHOTO_MAPS))}
            chain = routes["composition"].out
            same = all(bool(torch.equal(out[k], chain[k])) for k in ("n_views", "photo_var", "mean_colour"))
            med, raw = alternate(routes, rounds, steps)
            same = same and all(bool(torch.equal(out[k], chain[k])) for k in ("n_views", "photo_var", "mean_colour"))
            chain = dict(chain, table=pc.evaluate_chain(inv, imgs, want=("table",))["table"])
            t = out["table"][-1].tolist()
            emit(what="photo", frames=Fr, cams=CAMS, out_hw=out_hw, images=kind, scored_share=round(t[0] / (Fr * out_hw[0] * out_hw[1]), 3),
                 mean_std=round(t[1], 4), us_fused_std=round(med["fused_std"], 1), us_fused_all=round(med["fused_all"], 1),
                 us_composition=round(med["composition"], 1), composition_over_fused_std=round(med["composition"] / med["fused_std"], 2),
                 composition_over_fused_all=round(med["composition"] / med["fused_all"], 2), bits_equal=same,
                 table_max_rel_diff=float(((out["table"] - chain["table"]).abs() / out["table"].abs().clamp_min(1.0)).nan_to_num(0.0).max()),
                 pooled_fused=[round(v, 9) for v in t[:5]], pooled_composition=[round(v, 9) for v in chain["table"][-1].tolist()[:5]],
                 rounds=raw)
            del imgs, d, inv, out, std_only, routes, chain
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,16,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photo_probe needs a GPU")
    emit(what="library", path=os.environ.get("MVSGI_LIB", "default"), device=torch.cuda.get_device_name(0))
    rows([int(f) for f in a.frames.split(",")], a.rounds, a.steps)


if __name__ == "__main__":
    main()
