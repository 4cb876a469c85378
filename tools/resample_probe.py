#!/usr/bin/env python3
"""The fisheye -> surrogate-view resampler (csrc/resample.hip) on the device: one process, hipGraph replays, the variants
alternated round by round; one JSON line per measurement, also appended to profiles/resample_probe.txt.

    python tools/resample_probe.py [--frames 1,16,128] [--rounds 5] [--steps 20] [--no-pipeline]

  resample   F frames of 3 x 1028 x 1224 uint8 -> 3 x 512 x 2048 fp32 per launch (G16V), one rig table shared by the frames.
             Bytes per frame: 3 x 3 x 512 x 2048 x 4 written (37.7 MB), the raw images (11.3 MB), and the rig table
             (3 x 512 x 2048 x 9 B = 28.3 MB, read once per launch from HBM at most); "effective TB/s" is that count over
             the time.  The same job through torch.nn.functional.grid_sample (uint8 -> float / 255 conversion and the
             validity select included) is there for the record only: it is on no product path.
  pipeline   one-frame InferencePipeline replay with samplers (raw uint8 in) against without samplers on pre-resampled
             uint8 views: the difference holds the resample launch AND the fp32 RGB stem replacing the uint8 matrix-core
             stem; the two stems are timed alone so that their share can be taken out.  The row without samplers is the
             path as it was before samplers existed, measured in the same process.
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
import torch.nn.functional as F  # noqa: E402

from mvs_gi_amd import dropin, hip_ops as H, synth  # noqa: E402
from mvs_gi_amd.configs import CONFIGS  # noqa: E402
from mvs_gi_amd.dropin.feature_extractor import lower_conv2d_block  # noqa: E402
from mvs_gi_amd.pipeline import InferencePipeline  # noqa: E402

DEV = "cuda:0"
RAW, OUT, CAMS = (1028, 1224), (512, 2048), 3
LOG = os.path.join(ROOT, "profiles", "resample_probe.txt")


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


def alternate(routes, rounds, steps):
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, r in routes.items():
            t[k].append(r.us(steps))
    return {k: statistics.median(v) for k, v in t.items()}, {k: [round(x, 1) for x in v] for k, v in t.items()}


def rotation_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def make_samplers():
    return [dropin.DoubleSphereToEquirectSampler((-0.203, 0.589, 232.0, 232.0, 611.5, 513.5), RAW, OUT,
                                                 rotation_y(2 * math.pi * k / CAMS), device=DEV) for k in range(CAMS)]


def resample_rows(samplers, frames, rounds, steps):
    grid, valid = dropin.stack_tables(samplers)
    share = float(valid.float().mean())
    per_frame = CAMS * 3 * OUT[0] * OUT[1] * 4 + CAMS * RAW[0] * RAW[1] * 3
    table = CAMS * OUT[0] * OUT[1] * 9
    g = torch.Generator(device=DEV).manual_seed(0)
    for Fr in frames:
        imgs = torch.randint(0, 256, (Fr * CAMS, *RAW, 3), device=DEV, generator=g, dtype=torch.uint8)
        out = torch.empty((Fr * CAMS, 3, *OUT), device=DEV)
        gB = grid.repeat(Fr, 1, 1, 1) if Fr <= 16 else None              # grid_sample wants one grid per image

        def torch_route(imgs=imgs, gB=gB, Fr=Fr):
            x = imgs.permute(0, 3, 1, 2).float() / 255.0
            s = F.grid_sample(x, gB, mode="bilinear", padding_mode="zeros", align_corners=False)
            return torch.where(valid.repeat(Fr, 1, 1).unsqueeze(1), s, torch.zeros((), device=DEV))
        routes = {"hip": Replay(lambda imgs=imgs, out=out: H.resample_bilinear(imgs, grid, valid, out=out))}
        if gB is not None:
            routes["torch_grid_sample"] = Replay(torch_route)
            v = valid.repeat(Fr, 1, 1).unsqueeze(1).expand(-1, 3, -1, -1)
            diff = float((routes["hip"].out - routes["torch_grid_sample"].out)[v].abs().max())
        med, raw = alternate(routes, rounds, max(3, steps // (1 if Fr <= 16 else 4)))
        nbytes = Fr * per_frame + table
        row = dict(what="resample", frames=Fr, cams=CAMS, raw_hw=RAW, out_hw=OUT, valid_share=round(share, 3), us=round(med["hip"], 1),
                   us_per_frame=round(med["hip"] / Fr, 1), bytes=nbytes, effective_TB_per_s=round(nbytes / med["hip"] / 1e6, 3),
                   rounds=raw["hip"])
        if gB is not None:
            row.update(us_torch_grid_sample=round(med["torch_grid_sample"], 1), rounds_torch=raw["torch_grid_sample"],
                       max_abs_diff_to_torch_on_valid=diff)
        emit(**row)
        del imgs, out, gB, routes
        torch.cuda.empty_cache()


def pipeline_rows(samplers, rounds, steps):
    cfg = CONFIGS["G16V"]
    assert (4 * cfg.feat_hw[0], 4 * cfg.feat_hw[1]) == OUT and cfg.num_cams == CAMS
    w = synth.make_weights(cfg, seed=0)
    w["feature_extractor"] = synth.make_extractor_weights(0)
    inp = synth.make_inputs(cfg, seed=0, batch=1)
    g = torch.Generator(device=DEV).manual_seed(1)
    raw = torch.randint(0, 256, (CAMS, *RAW, 3), device=DEV, generator=g, dtype=torch.uint8)
    with_s = InferencePipeline(cfg, w, inp, device=DEV, samplers=samplers)
    plain = InferencePipeline(cfg, w, inp, device=DEV)
    views_f32 = H.resample_bilinear(raw, *dropin.stack_tables(samplers))
    views_u8 = (views_f32 * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    first = lower_conv2d_block(plain.feature_extractor.first)
    # the stem as the extractor launches it: in the 16-bit splits it writes the 2-D split-padded format for the residual blocks
    split = H.split2d_buffer(CAMS, OUT[0] // 2, OUT[1] // 2, DEV) if H.split_mode() else None
    routes = {
        "pipeline_samplers_raw_u8": Replay(lambda: with_s.forward_device(raw)),
        "pipeline_plain_views_u8": Replay(lambda: plain.forward_device(views_u8)),
        "resample_alone": Replay(lambda: H.resample_bilinear(raw, *with_s._table)),
        "stem_f32_alone": Replay(lambda: first.run(views_f32, in_nchw=True, out_split=split)),
        "stem_u8_alone": Replay(lambda: first.run(views_u8, in_nchw=True, out_split=split)),
    }
    med, rawt = alternate(routes, rounds, steps)
    d = med["pipeline_samplers_raw_u8"] - med["pipeline_plain_views_u8"]
    emit(what="pipeline", config=cfg.tag, mode=H.get_conv_mode(), us={k: round(v, 1) for k, v in med.items()},
         us_difference=round(d, 1), us_stem_share=round(med["stem_f32_alone"] - med["stem_u8_alone"], 1), rounds=rawt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,16,128")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_probe needs a GPU")
    emit(what="library", path=os.environ.get("MVSGI_LIB", "default"), device=torch.cuda.get_device_name(0))
    samplers = make_samplers()
    resample_rows(samplers, [int(f) for f in a.frames.split(",")], a.rounds, a.steps)
    if not a.no_pipeline:
        pipeline_rows(samplers, a.rounds, a.steps)


if __name__ == "__main__":
    main()
