"""Seeded cases of the builder-argument goldens, shared by tools/make_builder_goldens.py (which runs the REFERENCE's two cost-volume
builders built with each case's constructor arguments) and tests/test_builder_args_host.py / tests/test_gpu_builder_args.py (which
build the drop-in's with the same arguments and regenerate bit-identical inputs and weights).  Names, seeds, shapes and the
hip_ops entry points each case is expected to call (expected_route): no tensors.

A case is (class, num_cams N, channels per camera C, constructor keywords, grid-mask dtype); its seed is its position in the table.
`Std` is SphericalSweepStdMasked (feat_chs = C), `Cat` SphericalSweep (feat_chs = N * C).  Arguments not listed keep the defaults
(post_k_sz = 3, batch norm, leaky ReLU).  Inputs are wide_rig_cases.small_case (a uniformly drawn count of valid cameras per voxel),
weights topology_cases.draw_state_dict."""
import numpy as np

import topology_cases as T
import wide_rig_cases as W

# name -> (class, N, C, kwargs, grid-mask dtype)
_TABLE = [
    # Std, cameras at C = 16 (N = 1: summed_mask > 1 never holds, vol_raw is zero and vol the activation of the shift)
    ("n1", "Std", 1, 16, {}, "bool"),
    ("n2", "Std", 2, 16, {}, "bool"),
    ("default", "Std", 3, 16, {}, "bool"),
    ("n4", "Std", 4, 16, {}, "bool"),
    ("n5", "Std", 5, 16, {}, "bool"),
    ("n8", "Std", 8, 16, {}, "bool"),
    # Std, channels at N = 3: C % 4 == 0 but no multiple of 16 (validity byte -> exact-fp32 conv), multiples of 16 above 16
    # (streaming split conv), C % 4 != 0 (plane-gather sweep, direct conv)
    ("c4", "Std", 3, 4, {}, "bool"),
    ("c8", "Std", 3, 8, {}, "bool"),
    ("c12", "Std", 3, 12, {}, "bool"),
    ("c24", "Std", 3, 24, {}, "bool"),
    ("c32", "Std", 3, 32, {}, "bool"),
    ("c48", "Std", 3, 48, {}, "bool"),
    ("c64", "Std", 3, 64, {}, "bool"),
    ("c5", "Std", 3, 5, {}, "bool"),
    ("c6", "Std", 3, 6, {}, "bool"),
    ("n6_c5", "Std", 6, 5, {}, "bool"),
    ("n6_c8", "Std", 6, 8, {}, "bool"),
    # Std, norm and activation
    ("relu", "Std", 3, 16, dict(relu_type="original"), "bool"),
    ("linear", "Std", 3, 16, dict(relu_type="none"), "bool"),
    ("nonorm", "Std", 3, 16, dict(norm_type="none"), "bool"),
    ("nonorm_relu", "Std", 3, 16, dict(norm_type="none", relu_type="original"), "bool"),
    ("instance", "Std", 3, 16, dict(norm_type="instance"), "bool"),
    ("instance_c8", "Std", 3, 8, dict(norm_type="instance"), "bool"),
    # Std, grid masks: one byte per sample as uint8, fp32 of 0 / 1, fp32 whose true entries are 1.0, 0.5 and -2.0
    ("gm_u8", "Std", 3, 16, {}, "u8"),
    ("gm_f32", "Std", 3, 16, {}, "f32"),
    ("gm_f32_values", "Std", 3, 16, {}, "f32_values"),
    # Cat
    ("cat_1x16", "Cat", 1, 16, {}, "bool"),
    ("cat_2x8", "Cat", 2, 8, {}, "bool"),
    ("cat_3x4", "Cat", 3, 4, {}, "bool"),
    ("cat_3x5", "Cat", 3, 5, {}, "bool"),
    ("cat_3x16", "Cat", 3, 16, {}, "bool"),
    ("cat_4x8", "Cat", 4, 8, {}, "bool"),
    ("cat_4x32", "Cat", 4, 32, {}, "bool"),
    ("cat_8x16", "Cat", 8, 16, {}, "bool"),
    ("cat_relu", "Cat", 3, 16, dict(relu_type="original"), "bool"),
    ("cat_nonorm", "Cat", 3, 16, dict(norm_type="none"), "bool"),
    ("cat_instance", "Cat", 3, 16, dict(norm_type="instance"), "bool"),
]
CASES = {name: dict(name=name, cls=cls, n=n, c=c, kwargs=kw, gm=gm, seed=i) for i, (name, cls, n, c, kw, gm) in enumerate(_TABLE)}

# (B, Hi, Wi, D, Ho, Wo, Hm, Wm)
S1 = (2, 7, 11, 3, 3, 67, 14, 22)      # every case: Wo crosses the sweep's 64-voxel tile with a 3-wide rest; every extent odd; masks at 2x
S2 = (2, 3, 5, 1, 1, 2, 3, 5)          # every case but the instance-norm ones: every voxel a border voxel of every brick
S3 = (5, 7, 11, 5, 7, 37, 14, 22)      # the C = 16 Std cases: the ragged RS16_SHAPES volume at a batch above a chunk of 2
SHAPES = {"S1": S1, "S2": S2, "S3": S3}
MODES = ("f32", "bf16x3", "f16x3")
WEIGHT_SEED_OFFSET = 600               # the builder's weights: draw_state_dict(module, seed + WEIGHT_SEED_OFFSET)
CLASS_NAMES = {"Std": "SphericalSweepStdMasked", "Cat": "SphericalSweep"}
MAX_FILE_BYTES = 1_000_000


def kwargs_of(case) -> dict:
    kw = dict(num_cams=case["n"], feat_chs=feat_chs(case), post_k_sz=3, norm_type="batch", relu_type="leaky")
    kw.update(case["kwargs"])
    return kw


def feat_chs(case) -> int:
    return case["c"] if case["cls"] == "Std" else case["n"] * case["c"]


def is_instance(case) -> bool:
    return case["kwargs"].get("norm_type") == "instance"


def shapes_of(case):
    out = ["S1"]
    if not is_instance(case):
        out.append("S2")           # over one or two voxels an instance norm's variance is zero: the case would test nothing but eps
    if case["cls"] == "Std" and case["c"] == 16:
        out.append("S3")
    return out


RUNS = [(c, s) for c in CASES for s in shapes_of(CASES[c])]
# The masked sweeps of more than four cameras, carved out of "bit for bit against the reference" by name: the kernels add the
# cameras in camera order, ATen's sum associates differently from five addends on (tests/test_gpu_wide_rig.py has the same finding),
# so a handful of voxels differ in the last bit.  They are compared bit for bit with the oracle in camera order
# (sweep_std_masked(camera_order=True): the same operations) and with the reference's association to WIDE_BAR of the maximum with
# the same zeros.
WIDE_CASES = ["n5", "n8", "n6_c5", "n6_c8"]
WIDE_BAR = 1e-6            # test_gpu_wide_rig.py's; two associations of <= 8 fp32 addends differ by < 8 x 2^-24 = 4.8e-7 of the largest partial sum


def vol_shape(case, shape_name: str):
    b, _, _, d, ho, wo, _, _ = SHAPES[shape_name]
    return (b, feat_chs(case), d, ho, wo)


def _pack_files():
    """file -> [(case, shape name)]: the runs of a family in table order, a new file whenever the stored volumes (fp32, which
    hardly compress) would pass 900 000 bytes -- every file stays below MAX_FILE_BYTES."""
    files, budget = {}, 900_000
    for family, pick in (("std", lambda c, s: c["cls"] == "Std" and s != "S3"), ("std_s3", lambda c, s: s == "S3"),
                         ("cat", lambda c, s: c["cls"] == "Cat")):
        part, used = 1, 0
        for cname, sname in RUNS:
            if not pick(CASES[cname], sname):
                continue
            n = 4 * int(np.prod(vol_shape(CASES[cname], sname)))
            if used and used + n > budget:
                part, used = part + 1, 0
            files.setdefault(f"builder_args_{family}_{part}", []).append((cname, sname))
            used += n
    return files


FILES = _pack_files()
FILE_OF = {run: f for f, entries in FILES.items() for run in entries}


def make_module(namespace, case, **override):
    """The case's builder from `namespace` (mvs_gi_amd.dropin, or any object that has the reference's two classes under their names)."""
    return getattr(namespace, CLASS_NAMES[case["cls"]])(**dict(kwargs_of(case), **override))


def load_drawn(module, case, seed=None):
    return T.load_drawn(module, WEIGHT_SEED_OFFSET + (case["seed"] if seed is None else seed))


# (case, shape) -> the seed that stands for the case's position where that draw left the conditions tools/make_builder_goldens.py
# asserts (S2 is four voxels: a vol_raw that is all zero, or a volume whose maximum is below 0.1)
INPUT_SEEDS = {("n2", "S2"): 201, ("c24", "S2"): 109, ("c5", "S2"): 113, ("nonorm", "S2"): 119}


def input_seed(case, shape_name: str, seed=None) -> int:
    if seed is None:
        seed = INPUT_SEEDS.get((case["name"], shape_name), case["seed"])
    return 50_000 + 1000 * int(shape_name[1:]) + seed


def make_inputs(case, shape_name: str, seed=None, batch=None) -> dict:
    """feats [B, N, C, Hi, Wi], grids [B, N, D, Ho, Wo, 2], grid_masks [B, N, D, Ho, Wo, 1] in the case's dtype, masks
    [B, N, 1, Hm, Wm] (wide_rig_cases.small_case).  `seed` replaces the case's seed (another rig, other feats), `batch` the shape's."""
    shape = SHAPES[shape_name] if batch is None else (batch,) + SHAPES[shape_name][1:]
    inp = W.small_case(case["n"], case["c"], shape, seed=input_seed(case, shape_name, seed))
    gm = inp["grid_masks"]
    if case["gm"] == "u8":
        gm = gm.astype(np.uint8)
    elif case["gm"] == "f32":
        gm = gm.astype(np.float32)
    elif case["gm"] == "f32_values":
        # true entries that are not 1.0: the reference's logical_and and the kernels' `!= 0.0f` both count them as valid
        values = np.asarray([1.0, 0.5, -2.0], np.float32)
        pick = np.random.default_rng(input_seed(case, shape_name, seed) + 7).integers(0, 3, gm.shape)
        gm = np.where(gm, values[pick], np.float32(0.0)).astype(np.float32)
    else:
        assert case["gm"] == "bool" and gm.dtype == np.bool_
    inp["grid_masks"] = np.ascontiguousarray(gm)
    return inp


ARGS = ("feats", "grids", "grid_masks", "masks")
signature = T.signature


def raw_digest(vol_raw: np.ndarray) -> str:
    """sha256 of a vol_raw [B, Cv, D, Ho, Wo] fp32 with -0.0 read as 0.0 (x + 0.0): equal digests <=> np.array_equal."""
    from mvs_gi_amd import synth
    assert vol_raw.dtype == np.float32
    return synth.digest({"vol_raw": np.ascontiguousarray(vol_raw) + np.float32(0.0)})


# ---- routes -------------------------------------------------------------------------------------------------------------
# One forward as the sequence of hip_ops entry points it calls, read from dropin/cost_volume_builder.py (_std_front,
# std_sweep_ndhwc, cat_forward), common_modules.ConvLaunch.run / _run_conv and hip_ops.sweep_std.  'conv3d split' is H.conv3d with
# one of the streaming split kernel's layouts (CONV_BF16X3 | _C16 | _D32, CONV_F16 or not), 'conv3d f32' H.conv3d with CONV_AUTO:
# the exact-fp32 matrix-core kernel for channel counts that are multiples of 16, else the direct kernel.
FRONT_CHUNK = 16              # cost_volume_builder._FRONT_CHUNK's default


def front_ok(case, mode: str, cache: bool = True) -> bool:
    """_std_front serves the forward: a split mode, 16 -> 16, no instance norm, a slope in [0, 1] (every relu_type), the rig's
    validity byte usable (C % 4 == 0, 1 <= N <= 8, the cache on)."""
    return case["cls"] == "Std" and mode != "f32" and case["c"] == 16 and not is_instance(case) and cache and 1 <= case["n"] <= 8


def conv_route(case, mode: str):
    """post_vol through ConvLaunch.run: the streaming split kernel in a split mode when feat_chs % 16 == 0 (an instance norm does not
    change that: the conv then writes conv + bias and the norm launch follows)."""
    chs = feat_chs(case)
    return ["conv3d split" if mode != "f32" and chs % 16 == 0 else "conv3d f32"] + (["instance_norm"] if is_instance(case) else [])


def expected_route(case, mode: str, shape_name: str, cache: bool = True, first: bool = True, chunk: int = FRONT_CHUNK,
                   shared_rig: bool = False, batch: int = None):
    """cache: module.cache_rig_constants; first: the first forward on this rig (later ones find the validity byte cached);
    chunk / shared_rig / batch: _FRONT_CHUNK, the rig given as stride-0 views, another batch than the shape's."""
    assert mode in MODES
    if case["cls"] == "Cat":
        return ["sweep_cat"] + conv_route(case, mode)
    n, c = case["n"], case["c"]
    b = SHAPES[shape_name][0] if batch is None else batch
    valid = c % 4 == 0 and 1 <= n <= 8                 # H.valid_sweep_ok
    byte = ["sweep_validity"] if first else []
    if front_ok(case, mode, cache):
        chunks = -(-b // chunk) if chunk > 0 and b > chunk and shared_rig else 1
        return byte + ["sweep_std_valid_split", "conv3d_rs16"] * chunks
    if cache and valid:
        return byte + ["sweep_std_valid"] + conv_route(case, mode)
    # H.sweep_std(layout='auto'): the channels-last kernel that samples the masks itself at C % 4 == 0, N <= 4; for 5 to 8 cameras
    # with C % 4 == 0 it computes the validity byte and calls sweep_std_valid itself (every call); else the plane-gather kernel
    nested = ["sweep_validity", "sweep_std_valid"] if valid and n > 4 else []
    return ["sweep_std"] + nested + conv_route(case, mode)


def sweep_route(case, cache: bool = True, first: bool = True):
    """module.sweep(): expected_route's sweep part in 'f32' mode (the split-padded output belongs to forward alone)."""
    return [t for t in expected_route(case, "f32", "S1", cache=cache, first=first) if t.startswith("sweep")]
