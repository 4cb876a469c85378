#!/usr/bin/env python3
"""The packed point cloud (csrc/cloud.hip) on the device, against the torch composition it replaces; one process, the routes
alternated round by round; one JSON line per measurement, also appended to profiles/cloud_probe.txt.

    python tools/cloud_probe.py [--frames 1,128] [--kept 0.1,0.5,1.0] [--rounds 5] [--steps 20]

  hip     the three launches of mvsgi_cloud_pack_f32 (flags, scan, scatter) at 160 x 640, records of R = 7 floats (xyz, the colour
          of the first valid of three cameras, one attribute), one gate that keeps the given share of the pixels:
            replay  a hipGraph replay, device events (what the stage costs inside InferencePipeline's captured graph)
            eager   hip_ops.pack_cloud with caller-owned buffers, wall clock around call + synchronize
  torch   xyz.permute(...)[keep] and friends on dense tensors: the composition of tests/test_gpu_cloud.py -- comparisons, a
          first-valid gather, cat, permute, nonzero (which synchronises the host) and an index_select per frame; wall clock,
          it cannot be captured.
  Byte model of the three launches, per launch of B frames with K kept points in all:
            flags    B * H * W * (4 inv + 4 per gate + 1 mask) read, B * H * W / 8 written (the bit words)
            scatter  B * H * W / 8 read, K * (4 inv + 12 rays + N valid bytes at most + 4 C colour + 4 A attributes) read,
                     K * 4 R written (+ 4 K for the index)
          (tile counts and offsets: 8 bytes per 1024 pixels, left out).  Printed beside the bandwidth the replay achieves with it.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mvs_gi_amd import hip_ops as H  # noqa: E402

DEV = "cuda:0"
CAMS, C, A = 3, 3, 1
R = 3 + C + A
HW = (160, 640)
LOG = os.path.join(ROOT, "profiles", "cloud_probe.txt")


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


class Wall:
    """fn() + synchronize under the wall clock; us(steps) = microseconds per call."""

    def __init__(self, fn):
        self.fn = fn
        for _ in range(3):
            fn()
        torch.cuda.synchronize()

    def us(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps


def alternate(routes, rounds, steps, window_us=100e3):
    """Median over `rounds` of each route's time per call, the routes alternated; every timed window holds at least `steps` calls and
    about `window_us` (a window of a few calls of a few microseconds measures the clock)."""
    n = {k: min(20000, max(steps, int(window_us / max(r.us(10), 0.5)))) for k, r in routes.items()}
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, r in routes.items():
            t[k].append(r.us(n[k]))
    return {k: statistics.median(v) for k, v in t.items()}, {k: [round(x, 1) for x in v] for k, v in t.items()}


def torch_composition(inv, rays, bf, gate, hi, warped, valid, attr):
    """What a consumer writes today on dense tensors -> (list of [kept_b, R] tensors, kept per frame)."""
    B, Hh, W = inv.shape
    d = torch.full_like(inv, bf) / inv
    xyz = rays.unsqueeze(0) * d.unsqueeze(1)
    keep = torch.isfinite(d) & (d >= H.CLOUD_D_RANGE[0]) & (d <= H.CLOUD_D_RANGE[1]) & (gate >= 0.0) & (gate <= hi)
    first = (valid.to(torch.int32).cumsum(dim=1) == 0).sum(dim=1).clamp(max=CAMS - 1)
    col = warped.gather(1, first[:, None, None].expand(B, 1, C, Hh, W))[:, 0]
    col = torch.where(valid.any(dim=1)[:, None], col, torch.zeros_like(col))
    rec = torch.cat([xyz, col, attr[:, None]], dim=1).permute(0, 2, 3, 1).reshape(B, Hh * W, R)
    out = [rec[b][keep[b].reshape(-1).nonzero()[:, 0]] for b in range(B)]
    return out


def rows(frames, shares, rounds, steps):
    Hh, W = HW
    g = torch.Generator(device=DEV).manual_seed(0)
    rays = torch.nn.functional.normalize(torch.randn((3, Hh, W), device=DEV, generator=g), dim=0).contiguous()
    for B in frames:
        d = torch.exp(torch.rand((B, Hh, W), device=DEV, generator=g) * math.log(200.0) + math.log(0.5))
        inv = torch.full_like(d, 96.0) / d
        gate = torch.rand((B, Hh, W), device=DEV, generator=g)
        attr = torch.rand((B, Hh, W), device=DEV, generator=g)
        warped = torch.rand((B, CAMS, C, Hh, W), device=DEV, generator=g)
        valid = torch.rand((B, CAMS, Hh, W), device=DEV, generator=g) < 0.6
        ws = H.cloud_ws(B, Hh, W, DEV)
        out = dict(points=torch.empty((B, Hh * W, R), device=DEV), counts=torch.empty((B, 2), device=DEV, dtype=torch.int32))
        for share in shares:
            hi = float(share)
            kw = dict(d_range=H.CLOUD_D_RANGE, gates=[(gate, 0.0, hi)], warped=warped, valid=valid, attrs=[attr], ws=ws, out=out)

            def hip():
                return H.pack_cloud(inv, rays, 96.0, **kw)
            routes = {"hip_replay": Replay(hip), "hip_eager": Wall(hip),
                      "torch": Wall(lambda: torch_composition(inv, rays, 96.0, gate, hi, warped, valid, attr))}
            counts = out["counts"].cpu()
            want = torch_composition(inv, rays, 96.0, gate, hi, warped, valid, attr)
            same = all(torch.equal(out["points"][b, :int(counts[b, 0])].view(torch.int32), want[b].contiguous().view(torch.int32))
                       for b in (0, B - 1)) and [int(c) for c in counts[:, 1]] == [w.shape[0] for w in want]
            med, raw = alternate(routes, rounds, steps)
            K, px = int(counts[:, 1].sum()), B * Hh * W
            flags = px * (4 + 4) + px // 8
            scatter = px // 8 + K * (4 + 12 + CAMS + 4 * C + 4 * A) + K * 4 * R
            emit(what="cloud", frames=B, hw=HW, record_floats=R, kept_share=round(K / px, 4), bits_equal=bool(same),
                 us_hip_replay=round(med["hip_replay"], 1), us_hip_eager_wall=round(med["hip_eager"], 1), us_torch_wall=round(med["torch"], 1),
                 torch_over_hip_eager=round(med["torch"] / med["hip_eager"], 1), model_bytes=dict(flags=flags, scatter=scatter),
                 model_TB_per_s_replay=round((flags + scatter) / med["hip_replay"] / 1e6, 3), rounds=raw)
            del routes, want
        del d, inv, gate, attr, warped, valid, ws, out
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,128")
    ap.add_argument("--kept", default="0.1,0.5,1.0")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cloud_probe needs a GPU")
    emit(what="library", path=os.environ.get("MVSGI_LIB", "default"), device=torch.cuda.get_device_name(0))
    rows([int(f) for f in a.frames.split(",")], [float(s) for s in a.kept.split(",")], a.rounds, a.steps)


if __name__ == "__main__":
    main()
