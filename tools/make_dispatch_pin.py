"""Records tests/golden/conv3d_dispatch_pin.json: the conv3d dispatcher's answer (mvsgi_conv3d_variant_f32 /
mvsgi_conv3d_up2_variant_f32) for every conv / fused-upsample layer of the BASELINE configurations at B in {1, ..., 128}, in
every weight layout that applies and in both splits (and the exact-fp32 choice), plus hand-picked shapes that reach the
variants no configuration layer does.  tests/test_gpu_dispatch_pin.py replays it.

  python tools/make_dispatch_pin.py [out.json]      (on the GPU the table is meant for: the dispatcher reads its CU count)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mvs_gi_amd import _lib, hip_ops as H                  # noqa: E402
from mvs_gi_amd.configs import CONFIGS                      # noqa: E402

BATCHES = (1, 2, 4, 8, 16, 32, 64, 128)
PIN_CONFIGS = ("E8", "G16V", "G16VV", "4cam-32")            # BASELINE.json configs (G16V batched is G16V)
LAYOUTS = {"generic": H.CONV_BF16X3, "c16": H.CONV_BF16X3_C16, "v32": H.CONV_BF16X3_V32, "d32": H.CONV_BF16X3_D32}

# (B, Cin, Cout, D, H, W, stride) of convs, ("up2", B, Cin, Cout, Dl, Hl, Wl) of fused upsample + conv: shapes no configuration
# layer reaches (small / ragged / one-plane volumes, odd channel counts)
EXTRA = [
    (1, 16, 32, 8, 16, 16, 2), (1, 16, 32, 7, 9, 13, 2), (1, 128, 128, 2, 5, 9, 1), (2, 64, 64, 4, 8, 16, 1),
    (32, 128, 128, 2, 10, 40, 1), (32, 64, 64, 3, 15, 21, 1), (32, 32, 96, 4, 10, 40, 1), (24, 32, 128, 1, 10, 40, 1),
    (64, 16, 192, 1, 10, 40, 1), (96, 16, 128, 1, 7, 21, 1), (1, 32, 384, 1, 10, 40, 1), (2, 32, 384, 1, 10, 40, 1),
    (40, 64, 64, 3, 10, 24, 1), (48, 32, 96, 2, 15, 40, 1), (40, 64, 64, 3, 15, 21, 1), (6, 64, 64, 4, 20, 80, 1),
    (8, 128, 128, 2, 10, 40, 1), (64, 16, 96, 8, 16, 24, 2), (48, 32, 128, 7, 17, 23, 2), (64, 16, 192, 8, 16, 24, 2),
    (20, 64, 96, 4, 20, 80, 1), (40, 64, 96, 3, 15, 21, 1), (40, 32, 96, 4, 10, 24, 1), (96, 32, 128, 1, 7, 21, 1),
    (24, 64, 128, 1, 15, 21, 1), (64, 32, 192, 1, 15, 21, 1), (64, 32, 192, 1, 10, 40, 1), (5, 64, 128, 2, 10, 40, 1),
    (48, 32, 64, 4, 20, 80, 1), (44, 32, 96, 4, 18, 70, 1), (8, 64, 128, 4, 20, 80, 2),
    (4, 16, 48, 8, 40, 160, 1), (64, 16, 48, 8, 40, 160, 2), (64, 16, 192, 16, 80, 320, 2), (64, 16, 128, 16, 80, 320, 2),
    (4, 64, 96, 16, 80, 320, 1), (4, 64, 384, 1, 10, 40, 1), (1, 64, 192, 1, 10, 40, 1),
    (128, 64, 64, 2, 15, 32, 1), (1, 3, 8, 4, 8, 8, 1), (1, 16, 1, 4, 8, 8, 1), (1, 8, 1, 4, 8, 8, 1),
    ("up2", 4, 16, 32, 4, 20, 80), ("up2", 1, 16, 32, 4, 20, 80), ("up2", 1, 32, 48, 2, 10, 40), ("up2", 16, 64, 96, 2, 10, 40),
    ("up2", 1, 128, 64, 2, 10, 40), ("up2", 1, 32, 16, 4, 20, 80), ("up2", 2, 64, 128, 2, 10, 40), ("up2", 8, 64, 64, 4, 20, 80),
    ("up2", 1, 16, 32, 2, 10, 40),
]


def _half(n):
    return (n - 1) // 2 + 1


def config_layers(cfg):
    """(conv | up2, Cin, Cout, input dims, stride) of post_vol and every regulator layer (configs.regulator_conv_specs)."""
    D, (Hh, W) = cfg.num_cands, cfg.cv_hw
    dims = [(D, Hh, W)]
    for _ in range(3):
        dims.append(tuple(_half(n) for n in dims[-1]))
    f, C, cin = cfg.reg_f_int_chs, cfg.vol_chs, cfg.reg_in_chs
    chs = [f, 2 * f, 4 * f]
    out = [("conv", C, C, dims[0], 1), ("conv", cin, 1, dims[0], 1)]        # post_vol, out_costs.1 (the head)
    for lvl in range(3):
        out.append(("conv", cin, chs[lvl], dims[lvl], 2))                    # down_blks.lvl.first
        out.append(("conv", chs[lvl], chs[lvl], dims[lvl + 1], 1))          # down_blks.lvl.blks.*
        cin = chs[lvl]
    for lo, hi, ci, co in ((3, 2, chs[2], chs[1]), (2, 1, chs[1], chs[0]), (1, 0, chs[0], cfg.reg_in_chs)):
        if tuple(2 * n for n in dims[lo]) == dims[hi]:                       # upBlks.0, upBlks.1, out_costs.0
            out.append(("up2", ci, co, dims[lo], 1))
    return out


def queries():
    qs = []
    for tag in PIN_CONFIGS:
        for kind, cin, cout, (d, h, w), s in config_layers(CONFIGS[tag]):
            for b in BATCHES:
                qs.append((kind, b, cin, cout, d, h, w, s) if kind == "conv" else ("up2", b, cin, cout, d, h, w, 1))
    for e in EXTRA:
        qs.append(("conv",) + e if e[0] != "up2" else e + (1,))
    return list(dict.fromkeys(qs))


def rows():
    lib = _lib.load()
    out = []
    for kind, b, cin, cout, d, h, w, s in queries():
        if kind == "conv":
            lays = ["generic"] + (["c16"] if cout == 16 and s == 1 else []) + \
                (["v32"] if lib.mvsgi_conv3d_v32_applies(b, cin, d, h, w, cout, s) else []) + \
                (["d32"] if lib.mvsgi_conv3d_d32_applies(b, cin, d, h, w, cout, s) else [])
            cases = [("auto", "f32", H.CONV_AUTO)] + [(lay, sp, LAYOUTS[lay] | (H.CONV_F16 if sp == "f16" else 0))
                                                       for lay in lays for sp in ("bf16", "f16")]
            for lay, sp, impl in cases:
                if sp == "f16" and (cin % 16 or cout % 16):
                    continue
                name = lib.mvsgi_conv3d_variant_f32(b, cin, d, h, w, cout, s, impl)
                out.append(["conv", b, cin, d, h, w, cout, s, lay, sp, name.decode() if name else None])
        else:
            if cin % 16 or cout % 16:
                continue
            lays = ["generic"] + (["c16"] if cout == 16 else []) + \
                (["v32"] if lib.mvsgi_conv3d_v32_applies(b, cin, 2 * d, 2 * h, 2 * w, cout, 1) else []) + \
                (["d32"] if lib.mvsgi_conv3d_up2_d32_applies(b, cin, d, h, w, cout) else [])
            for lay in lays:
                for sp in ("bf16", "f16"):
                    name = lib.mvsgi_conv3d_up2_variant_f32(b, cin, d, h, w, cout, LAYOUTS[lay] | (H.CONV_F16 if sp == "f16" else 0))
                    out.append(["up2", b, cin, d, h, w, cout, 1, lay, sp, name.decode() if name else None])
    return out


def device_cus() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 0


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv3d_dispatch_pin.json")
    r = rows()
    doc = {"cus": device_cus(),
           "fields": ["fn", "B", "Cin", "D", "H", "W", "Cout", "stride", "layout", "split", "variant"],
           "note": "fn conv: mvsgi_conv3d_variant_f32 at the input size (D, H, W); fn up2: mvsgi_conv3d_up2_variant_f32 at the "
                   "low-resolution size.  layout auto = the exact-fp32 choice (MVSGI_CONV_AUTO); split f16 = | MVSGI_CONV_F16",
           "rows": r}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v)}' for k, v in doc.items() if k != "rows") + ',\n"rows": [\n' +
                ",\n".join(json.dumps(x) for x in r) + "\n]}\n")
    names = sorted({x[-1] for x in r if x[-1]})
    print(f"{path}: {len(r)} queries, {len(names)} distinct variants, cus {doc['cus']}")
