#!/usr/bin/env python3
"""The masked-variance sweep for rigs of 5 to 8 cameras (sweep_std_nhwc_v_kernel<N>, N > 4) against the route such a rig had before:
the plane-gather kernel on NCHW features, fp32 vol_raw, streaming post_vol.  One process, hipGraph replays, the two routes
alternated round by round on the same device; one JSON line per measurement.

    python tools/wide_rig_probe.py [--cams 6,8] [--batches 16,128] [--rounds 3] [--steps 20] [--sweep-only]

  sweep      16 frames of G16V geometry (feats 16 x 128 x 512, 16 candidates, 80 x 320), one rig shared by the batch:
             validity-byte kernel (channels-last feats; and with the NCHW -> channels-last transposition in front) vs
             H.sweep_std(layout="nchw"), and against the 3-camera launch of sweep_std_nhwc_v_kernel: measured time over
             N / 3 x the 3-camera time (the "time proportional to the cameras gathered" model of DESIGN.md K1), with the
             (voxel, camera) pairs each rig really needs
  front/step sweep + post_vol and the whole step (f16x3) for a 6-camera G16V: this route vs the former one (the predicate
             of the validity-byte kernels put back to N <= 4 for that HotPath: plane-gather sweep, streaming post_vol)
MVSGI_LIB=<diagnostic build> measures another library (e.g. -DMVSGI_SWEEP_WIDE_WAVES=3).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mvs_gi_amd import hip_ops as H, synth  # noqa: E402
from mvs_gi_amd.configs import CONFIGS, PathConfig  # noqa: E402
from mvs_gi_amd.pipeline import HotPath  # noqa: E402

DEV = "cuda:0"


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
    """{name: Replay} -> {name: median us over `rounds` rounds}, the routes taken in turn within every round."""
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, r in routes.items():
            t[k].append(r.us(steps))
    return {k: statistics.median(v) for k, v in t.items()}, {k: [round(x, 1) for x in v] for k, v in t.items()}


def rig(N, B):
    cfg = PathConfig(**{**CONFIGS["G16V"].__dict__, "tag": f"G16V-{N}cam", "num_cams": N})
    inp = synth.make_inputs(cfg, seed=0, batch=1)
    g, gm, m = (torch.from_numpy(inp[k]).to(DEV) for k in ("grids", "grid_masks", "masks"))
    f = torch.from_numpy(inp["feats"]).to(DEV)
    feats = (f.expand(B, *f.shape[1:]) + torch.linspace(0, 1, B, device=DEV).view(B, 1, 1, 1, 1)).contiguous()
    return cfg, inp, feats, g, gm, m


def needed_pairs(vm, N):
    """(voxel, camera) pairs the kernel gathers per voxel: camera valid and at least two cameras valid."""
    bits = torch.stack([(vm >> c) & 1 for c in range(N)]).to(torch.int32)
    n = bits.sum(0)
    return float((bits * (n > 1)).sum()) / vm.numel()


def sweep_rows(cams, B, rounds, steps):
    routes, meta = {}, {}
    for N in (3, *cams):
        _, _, feats, g, gm, m = rig(N, B)
        vm = H.sweep_validity(g, gm, m)
        f_cl = feats.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        meta[N] = needed_pairs(vm, N)
        routes[f"valid_cl_{N}"] = Replay(lambda f=f_cl, g=g, vm=vm: H.sweep_std_valid(f, g, vm))
        if N > 3:
            gB, gmB, mB = (t.expand(B, *t.shape[1:]).contiguous() for t in (g, gm, m))
            routes[f"valid_nchw_feats_{N}"] = Replay(lambda f=feats, g=g, vm=vm: H.sweep_std_valid(f, g, vm))
            routes[f"nchw_{N}"] = Replay(lambda f=feats, a=gB, b=gmB, c=mB: H.sweep_std(f, a, b, c, layout="nchw"))
            assert torch.equal(routes[f"valid_cl_{N}"].out, routes[f"nchw_{N}"].out), "the two routes differ"
    med, raw = alternate(routes, rounds, steps)
    t3 = med["valid_cl_3"]
    print(json.dumps(dict(what="sweep", frames=B, cams=3, us=round(t3, 1), needed_pairs_per_voxel=round(meta[3], 3), rounds=raw["valid_cl_3"])), flush=True)
    for N in cams:
        a, b, c = med[f"valid_cl_{N}"], med[f"valid_nchw_feats_{N}"], med[f"nchw_{N}"]
        print(json.dumps(dict(what="sweep", frames=B, cams=N, us_valid_channels_last=round(a, 1), us_valid_with_transposition=round(b, 1),
                              us_plane_gather=round(c, 1), speedup=round(c / a, 2), speedup_with_transposition=round(c / b, 2),
                              over_cameras_model=round(a / (N / 3.0 * t3), 3), needed_pairs_per_voxel=round(meta[N], 3),
                              over_needed_pairs_model=round(a / (meta[N] / meta[3] * t3), 3),
                              rounds=dict(valid=raw[f"valid_cl_{N}"], plane_gather=raw[f"nchw_{N}"]))), flush=True)


def path_rows(N, B, rounds, steps):
    cfg, inp, feats, _, _, _ = rig(N, B)
    w = synth.make_weights(cfg, seed=0)
    H.set_conv_mode("f16x3")
    real = H.valid_sweep_ok
    hps = {}
    try:
        for name, pred in (("wide", real), ("former", lambda f: real(f) and f.shape[1] <= 4)):
            H.valid_sweep_ok = pred
            hp = HotPath(cfg, w, inp, device=DEV)
            hp(feats)
            torch.cuda.synchronize()
            g, gm, m = hp._rig_views[1:]
            hps[name] = (hp, Replay(lambda hp=hp, a=g, b=gm, c=m: hp.cv_builder(feats, a, b, c)), Replay(lambda hp=hp: hp(feats)))
        assert ("_mvsgi_rs_vol" in hps["wide"][0].cv_builder.__dict__) and ("_mvsgi_rs_vol" not in hps["former"][0].cv_builder.__dict__)
        err = float((hps["wide"][2].out[0] - hps["former"][2].out[0]).abs().max() / hps["former"][2].out[0].abs().max())
        for what, i in (("front", 1), ("step", 2)):
            med, raw = alternate({k: v[i] for k, v in hps.items()}, rounds, steps)
            print(json.dumps(dict(what=what, mode="f16x3", cams=N, frames=B, frames_per_s_wide=round(B * 1e6 / med["wide"], 1),
                                  frames_per_s_former=round(B * 1e6 / med["former"], 1), ratio=round(med["former"] / med["wide"], 3),
                                  inv_dist_max_rel_between_routes=err, us_rounds=raw)), flush=True)
    finally:
        H.valid_sweep_ok = real
    del hps
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", default="6,8")
    ap.add_argument("--batches", default="16,128")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sweep-only", action="store_true")
    a = ap.parse_args()
    cams = [int(c) for c in a.cams.split(",")]
    print(json.dumps(dict(what="library", path=os.environ.get("MVSGI_LIB", "default"), device=torch.cuda.get_device_name(0))), flush=True)
    sweep_rows(cams, 16, a.rounds, a.steps)
    torch.cuda.empty_cache()
    if not a.sweep_only:
        for B in (int(b) for b in a.batches.split(",")):
            path_rows(6, B, a.rounds, max(3, a.steps // (1 if B <= 16 else 4)))


if __name__ == "__main__":
    main()
