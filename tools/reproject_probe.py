#!/usr/bin/env python3
"""The back-projection (csrc/reproject.hip) on the device: one process, hipGraph replays, the routes alternated round by
round; one JSON line per measurement, also appended to profiles/reproject_probe.txt.

    python tools/reproject_probe.py [--frames 1,16,128] [--rounds 5] [--steps 20] [--no-pipeline]

  reproject  F frames of inverse distance at G16V's output geometries (160 x 640, and 320 x 1280 for interp_scale_factor = 4)
             -> point cloud + three warped views + validity, with three 512 x 2048 uint8 surrogate views (equirectangular
             cameras) and with three 1028 x 1224 raw frames (double-sphere cameras behind R_raw_fisheye):
               fused   one launch of mvsgi_reproject_f32
               chain   Reprojector.reproject_chain, the launches it is defined by: divide, multiply, N x (transform, projection,
                       validity), stack, resample
             Bytes per frame (fused): inv read, xyz + warped + valid written; the image gathers are counted as the
             images' size (an upper bound of the HBM traffic: the taps of one frame's map touch a fraction of them).
  pipeline   the one-frame InferencePipeline replay with a reprojector against the same replay without one.
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

from mvs_gi_amd import dropin, hip_ops as H, synth  # noqa: E402
from mvs_gi_amd.configs import CONFIGS  # noqa: E402
from mvs_gi_amd.dropin import sweep_grids as SG  # noqa: E402
from mvs_gi_amd.pipeline import InferencePipeline  # noqa: E402

DEV = "cuda:0"
CAMS = 3
LON, LAT = (0.0, 2 * math.pi), (-math.pi / 2, 0.0)
DS = (-0.203, 0.589, 232.0, 232.0, 611.5, 513.5)
LOG = os.path.join(ROOT, "profiles", "reproject_probe.txt")


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


def reproject_rows(frames, rounds, steps):
    g = torch.Generator(device=DEV).manual_seed(0)
    for out_hw in ((160, 640), (320, 1280)):
        for kind in ("views_512x2048", "raw_1028x1224"):
            rp, img_hw = make_reprojector(kind, out_hw, 96.0)
            for Fr in frames:
                imgs = torch.randint(0, 256, (Fr * CAMS, *img_hw, 3), device=DEV, generator=g, dtype=torch.uint8)
                d = torch.exp(torch.rand((Fr, *out_hw), device=DEV, generator=g) * math.log(200.0) + math.log(0.5))
                inv = torch.full_like(d, 96.0) / d
                out = {k: v for k, v in rp.reproject(inv, imgs).items()}
                routes = {"fused": Replay(lambda inv=inv, imgs=imgs, out=out: rp.reproject(inv, imgs, out=out)),
                          "chain": Replay(lambda inv=inv, imgs=imgs: rp.reproject_chain(inv, imgs))}
                same = all(bool(torch.equal(out[k], routes["chain"].out[k])) for k in ("xyz", "warped", "valid"))
                med, raw = alternate(routes, rounds, steps)
                px = Fr * out_hw[0] * out_hw[1]
                nbytes = px * (4 + 12 + CAMS * (12 + 1)) + 3 * out_hw[0] * out_hw[1] * 4 + Fr * CAMS * img_hw[0] * img_hw[1] * 3
                emit(what="reproject", frames=Fr, cams=CAMS, out_hw=out_hw, images=kind, valid_share=round(float(out["valid"].float().mean()), 3),
                     us_fused=round(med["fused"], 1), us_chain=round(med["chain"], 1), chain_over_fused=round(med["chain"] / med["fused"], 2),
                     bits_equal=same, bytes_upper_bound=nbytes, effective_TB_per_s_fused=round(nbytes / med["fused"] / 1e6, 3), rounds=raw)
                del imgs, d, inv, out, routes
                torch.cuda.empty_cache()


def pipeline_rows(rounds, steps):
    cfg = CONFIGS["G16V"]
    w = synth.make_weights(cfg, seed=0)
    w["feature_extractor"] = synth.make_extractor_weights(0)
    inp = synth.make_inputs(cfg, seed=0, batch=1)
    g = torch.Generator(device=DEV).manual_seed(1)
    views = torch.randint(0, 256, (cfg.num_cams, 4 * cfg.feat_hw[0], 4 * cfg.feat_hw[1], 3), device=DEV, generator=g, dtype=torch.uint8)
    plain = InferencePipeline(cfg, w, inp, device=DEV)
    out_hw = tuple(plain.forward_device(views).shape[-2:])
    rp = dropin.Reprojector([SG.EquirectangularSampleGridMaker() for _ in range(cfg.num_cams)], ring_poses(cfg.num_cams), out_hw, LON, LAT,
                            bf=1.0, device=DEV)
    with_r = InferencePipeline(cfg, w, inp, device=DEV, reprojector=rp)
    routes = {"pipeline_plain": Replay(lambda: plain.forward_device(views)),
              "pipeline_reprojector": Replay(lambda: with_r.forward_device(views))}
    med, raw = alternate(routes, rounds, steps)
    emit(what="pipeline", config=cfg.tag, mode=H.get_conv_mode(), out_hw=out_hw, us={k: round(v, 1) for k, v in med.items()},
         us_difference=round(med["pipeline_reprojector"] - med["pipeline_plain"], 1), rounds=raw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,16,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reproject_probe needs a GPU")
    emit(what="library", path=os.environ.get("MVSGI_LIB", "default"), device=torch.cuda.get_device_name(0))
    reproject_rows([int(f) for f in a.frames.split(",")], a.rounds, a.steps)
    if not a.no_pipeline:
        pipeline_rows(a.rounds, a.steps)


if __name__ == "__main__":
    main()
