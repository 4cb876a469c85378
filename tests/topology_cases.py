"""Seeded cases of the regulator-topology goldens, shared by tools/make_topology_goldens.py (which runs the REFERENCE's
regulators built with each case's constructor arguments) and tests/test_topology_host.py / tests/test_gpu_topology.py (which build
the drop-in's with the same arguments and regenerate bit-identical inputs and weights).  Names, seeds and shapes only: no tensors.

A case is (class, constructor arguments, seed).  `Base` is UNetCostVolumeRegulatorBase, `Old` the older UNetCostVolumeRegulator
(widths in * 2 / 4 / 8).  Arguments not listed keep the constructor's defaults."""
import numpy as np

_OLD = dict(in_chs=16, final_chs=1, u_depth=3, blk_width=4, stage_factor=2, cost_k_sz=3, keep_last_chs=[], deconv_k_sz=3,
            num_cams=3, sweep_fuse_ch_reduce=2)

# name -> (class, kwargs); the seed of a case is its position in this table
_TABLE = [
    ("default", "Base", {}),
    ("depth1", "Base", dict(u_depth=1)),
    ("depth2", "Base", dict(u_depth=2)),
    ("depth4", "Base", dict(u_depth=4)),
    ("width1", "Base", dict(blk_width=1)),
    ("width2", "Base", dict(blk_width=2)),
    ("width3", "Base", dict(blk_width=3)),
    ("factor1", "Base", dict(stage_factor=1)),
    ("factor3", "Base", dict(stage_factor=3)),
    ("keep1", "Base", dict(keep_last_chs=[1])),
    ("keep2", "Base", dict(keep_last_chs=[2])),
    ("keep12", "Base", dict(keep_last_chs=[1, 2])),
    ("final2", "Base", dict(final_chs=2)),
    ("relu", "Base", dict(relu_type="original")),
    ("linear", "Base", dict(relu_type="none")),
    ("nonorm", "Base", dict(norm_type="none")),
    ("nonorm_relu", "Base", dict(norm_type="none", relu_type="original")),
    ("in8_f24", "Base", dict(in_chs=8, f_int_chs=24)),
    ("in16_f16", "Base", dict(f_int_chs=16)),
    ("in32_f32", "Base", dict(in_chs=32, f_int_chs=32)),
    ("in48_f32_w2", "Base", dict(in_chs=48, f_int_chs=32, blk_width=2)),
    ("old_3cam", "Old", dict(_OLD)),
    ("old_one_cam", "Old", dict(_OLD, only_one_cam=True)),
    ("old_4cam_d2_w2", "Old", dict(_OLD, num_cams=4, u_depth=2, blk_width=2)),
]
CASES = {name: dict(cls=cls, kwargs=kw, seed=i) for i, (name, cls, kw) in enumerate(_TABLE)}

# (D, H, W) of the input volume [2, in_chs, D, H, W]
S1 = (8, 8, 32)          # every case
S2 = (5, 7, 19)          # every case: an odd pyramid (the second resize to the skip's size; the output is (6, 8, 20))
S3 = (16, 8, 64)         # level 0 is (8, 4, 32): the smallest volume the Winograd form and the Winograd-form polyphase tail accept
SHAPES = {"S1": S1, "S2": S2, "S3": S3}
BATCH = 2
ROUTE_CASES = ["default", "depth2", "depth4", "width2", "width3", "factor1", "keep1", "keep12", "final2", "relu", "linear",
               "old_one_cam"]
# file -> [(case, shape name)]
FILES = {
    "topology": [(c, s) for s in ("S1", "S2") for c in CASES],
    "topology_routes": [(c, "S3") for c in ROUTE_CASES],
}

# builder -> regulator on the geometry and inputs of the std_d8 golden case (synth.make_inputs on its cfg, batch 2);
# SphericalSweepStdMasked takes the regulator's relu_type / norm_type
COMPOSED = {
    "width2": dict(kwargs=dict(blk_width=2), seed=40),
    "width1": dict(kwargs=dict(blk_width=1), seed=41),
    "relu": dict(kwargs=dict(relu_type="original"), seed=42),
}
COMPOSED_BATCH = 2
BUILDER_SEED_OFFSET = 500        # the builder's weights: draw_state_dict(cvb, seed + BUILDER_SEED_OFFSET)

# the regulator classes a reference class name stands for: {"Base": ..., "Old": ...} of whichever package builds the module
CLASS_NAMES = {"Base": "UNetCostVolumeRegulatorBase", "Old": "UNetCostVolumeRegulator"}


def make_module(namespace, case):
    """The case's regulator from `namespace` (mvs_gi_amd.dropin, or the reference's unet_regulator module)."""
    return getattr(namespace, CLASS_NAMES[case["cls"]])(**{k: (list(v) if isinstance(v, list) else v) for k, v in case["kwargs"].items()})


def builder_kwargs(case, cfg):
    kw = case["kwargs"]
    return dict(num_cams=cfg.num_cams, feat_chs=cfg.vol_chs, post_k_sz=3, norm_type=kw.get("norm_type", "batch"),
                relu_type=kw.get("relu_type", "leaky"))


def input_seed(case, shape_name: str) -> int:
    return 1000 * int(shape_name[1:]) + case["seed"]


def make_input(case, shape_name: str, in_chs: int) -> np.ndarray:
    """x [2, in_chs, D, H, W]: two different frames."""
    shape = (BATCH, in_chs) + SHAPES[shape_name]
    return np.random.default_rng(input_seed(case, shape_name)).standard_normal(shape).astype(np.float32)


def draw_state_dict(module, seed: int):
    """Seeded values for every entry of module.state_dict(), in its order, by key suffix (the recipe of synth._conv_block).
    Two modules with equal key lists and shapes -- the reference's and the drop-in's -- get equal draws."""
    rng = np.random.default_rng(30_000 + seed)
    out = {}
    for key, t in module.state_dict().items():
        shape = tuple(t.shape)
        if key.endswith("conv_layer.weight"):
            b = float(np.sqrt(6.0 / (27 * shape[1])))
            v = rng.uniform(-b, b, shape).astype(np.float32)
        elif key.endswith("conv_layer.bias") or key.endswith("norm_layer.bias") or key.endswith("running_mean"):
            v = rng.normal(0, 0.1, shape).astype(np.float32)
        elif key.endswith("norm_layer.weight") or key.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif key.endswith("num_batches_tracked"):
            v = np.asarray(1, np.int64)
        else:
            raise KeyError(f"draw_state_dict: no rule for {key!r}")
        out[key] = v
    return out


def load_drawn(module, seed: int):
    """draw_state_dict into the module (strict); returns the drawn arrays."""
    import torch
    sd = draw_state_dict(module, seed)
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return sd


def signature(module):
    return [f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items()]
