"""Seeded cases of the extractor-argument goldens, shared by tools/make_extractor_goldens.py (which runs the REFERENCE's two
feature extractors built with each case's constructor arguments) and tests/test_extractor_args_host.py /
tests/test_gpu_extractor_args.py (which build the drop-in's with the same arguments and regenerate bit-identical images and
weights).  Names, seeds, shapes and the launches each case is expected to make (expected_route): no tensors.

A case is (class, constructor arguments, gain); its seed is its position in the table.  `Simple` is SimpleFeatExtraction, `Sphere`
SphereEquirectFeatExtraction.  Arguments not listed keep the constructor's defaults (chs = 8, k_sz = 3, layers = [5, 10], batch
norm, leaky ReLU).  `gain` scales the conv weights' uniform bound: 0.7 where the chain is long (or linear) enough that unit gain
takes the features' maximum out of [0.1, 100], the range in which a relative-to-maximum bar still says something."""
import numpy as np

# name -> (class, kwargs, gain)
_TABLE = [
    ("default", "Simple", {}, 0.7),
    ("chs16", "Simple", dict(chs=16), 0.7),
    ("chs6", "Simple", dict(chs=6, layers=[2, 2]), 1.0),
    ("chs32", "Simple", dict(chs=32, layers=[2, 2]), 1.0),
    ("chs48", "Simple", dict(chs=48, layers=[1, 2]), 1.0),
    ("chs64", "Simple", dict(chs=64, layers=[1, 1]), 1.0),
    ("chs80", "Simple", dict(chs=80, layers=[1, 1]), 1.0),
    ("k1", "Simple", dict(chs=16, k_sz=1, layers=[2, 2]), 1.0),
    ("k5", "Simple", dict(chs=16, k_sz=5, layers=[2, 2]), 1.0),
    ("k7", "Simple", dict(chs=16, k_sz=7, layers=[1, 1]), 1.0),
    ("layers_none", "Simple", dict(chs=16, layers=[]), 1.0),
    ("layers_3", "Simple", dict(chs=16, layers=[3]), 1.0),
    ("layers_0_3", "Simple", dict(chs=16, layers=[0, 3]), 1.0),
    ("layers_3_0", "Simple", dict(chs=16, layers=[3, 0]), 1.0),
    ("layers_1_1", "Simple", dict(chs=16, layers=[1, 1]), 1.0),
    ("layers_2_0_2", "Simple", dict(chs=16, layers=[2, 0, 2]), 1.0),
    ("layers_2_2_2", "Simple", dict(chs=16, layers=[2, 2, 2]), 1.0),
    ("gray", "Simple", dict(chs=16, in_chs=1, layers=[2, 2]), 1.0),
    ("in4", "Simple", dict(chs=16, in_chs=4, layers=[2, 2]), 1.0),
    ("relu", "Simple", dict(chs=16, relu_type="original"), 0.7),
    ("linear", "Simple", dict(chs=16, relu_type="none", layers=[2, 2]), 0.7),
    ("nonorm", "Simple", dict(chs=16, norm_type="none"), 0.7),
    ("nonorm_relu", "Simple", dict(chs=16, norm_type="none", relu_type="original", layers=[2, 2]), 1.0),
    ("instance", "Simple", dict(chs=16, norm_type="instance", layers=[2, 2]), 1.0),
    ("instance_c8", "Simple", dict(norm_type="instance", layers=[1, 1]), 1.0),
    ("sphere", "Sphere", dict(chs=16), 0.7),
    ("sphere_default", "Sphere", {}, 0.7),
    ("sphere_k5", "Sphere", dict(chs=16, k_sz=5, layers=[2, 2]), 1.0),
    ("sphere_l3", "Sphere", dict(chs=16, layers=[3]), 1.0),
    ("sphere_c32", "Sphere", dict(chs=32, layers=[1, 1]), 1.0),
    ("sphere_instance", "Sphere", dict(chs=16, norm_type="instance", layers=[1, 1]), 1.0),
    ("sphere_relu", "Sphere", dict(chs=16, relu_type="original", layers=[2, 2]), 0.8),     # 63 % zeros at unit gain, 60 % here
]
CASES = {name: dict(name=name, cls=cls, kwargs=kw, gain=g, seed=i) for i, (name, cls, kw, g) in enumerate(_TABLE)}

# (H, W) of the images [M, H, W, in_chs]
S1 = (30, 50)      # levels 15 x 25 and 8 x 13: 15 crosses resblock2d's 14-row tile; W % 4 = 2 sends uint8 images to the fp32 stem kernel
S2 = (46, 100)     # levels 23 x 50 (ragged against 14 x 30 both ways) and 12 x 25 (ragged against conv2d_s2_split's 8 x 16 units);
#                    W % 4 = 0: uint8 images take the matrix-core stem, three row blocks
S3 = (3, 5)        # levels 2 x 3 and 1 x 2: every pixel a border pixel, every tile partial
SHAPES = {"S1": S1, "S2": S2, "S3": S3}
M = 3
S2_CASES = ["default", "chs16", "chs48", "k5", "layers_0_3", "layers_2_2_2", "instance", "sphere"]


def kwargs_of(case) -> dict:
    kw = dict(in_chs=3, chs=8, k_sz=3, layers=[5, 10], norm_type="batch", relu_type="leaky")
    kw.update(case["kwargs"])
    return kw


def _has_s3(case) -> bool:
    """Not the three-step `layers` cases (a third halving of 1 x 2) and not instance norm: over one or two pixels its variance is
    zero and the case would test nothing but eps."""
    kw = kwargs_of(case)
    return len(kw["layers"]) < 3 and kw["norm_type"] != "instance"


# file -> [(case, shape name)]
FILES = {
    "extractor_args": [(c, "S1") for c in CASES] + [(c, "S3") for c in CASES if _has_s3(CASES[c])],
    "extractor_args_routes": [(c, "S2") for c in S2_CASES],
}
SIZES_OF = {c: [s for entries in FILES.values() for cc, s in entries if cc == c] for c in CASES}
FILE_OF = {"S1": "extractor_args", "S3": "extractor_args", "S2": "extractor_args_routes"}

CLASS_NAMES = {"Simple": "SimpleFeatExtraction", "Sphere": "SphereEquirectFeatExtraction"}


def make_module(namespace, case, shape_name: str):
    """The case's extractor for images of SHAPES[shape_name], from `namespace`: mvs_gi_amd.dropin, or any object that has the
    reference's two classes under their names."""
    kw = {k: (list(v) if isinstance(v, list) else v) for k, v in case["kwargs"].items()}
    return getattr(namespace, CLASS_NAMES[case["cls"]])(in_size=SHAPES[shape_name], **kw)


def out_shape(case, shape_name: str):
    kw = kwargs_of(case)
    h, w = ((s - 1) // 2 + 1 for s in SHAPES[shape_name])               # the 5x5 stride-2 stem, padding 2
    for _ in range(max(len(kw["layers"]) - 1, 0)):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1                         # 3x3 stride 2, padding 1
    return (M, kw["chs"], h, w)


def input_seed(case, shape_name: str) -> int:
    return 1000 * int(shape_name[1:]) + case["seed"]


def make_images(case, shape_name: str) -> np.ndarray:
    """uint8 [M, H, W, in_chs] camera images; the float input is to_float(images), as the reference's inference class converts."""
    Hh, W = SHAPES[shape_name]
    return np.random.default_rng(input_seed(case, shape_name)).integers(0, 256, (M, Hh, W, kwargs_of(case)["in_chs"]), dtype=np.uint8)


def to_float(imgs_u8):
    """torch uint8 [M, H, W, C] -> fp32 [M, C, H, W] in [0, 1]."""
    return imgs_u8.permute(0, 3, 1, 2).float() / 255.0


_CONV_W = ("conv_layer.weight", "blk.0.weight")
_SHIFT = ("conv_layer.bias", "blk.0.bias", "norm_layer.bias", "blk.1.bias", "running_mean")
_SCALE = ("norm_layer.weight", "blk.1.weight", "running_var")


def draw_state_dict(module, seed: int, gain: float = 1.0):
    """Seeded values for every entry of module.state_dict() but the sphere conv's `offset` buffer (which keeps the constructor's
    value), in its order, by key suffix.  Two modules with equal key lists and shapes -- the reference's and the drop-in's -- get
    equal draws."""
    rng = np.random.default_rng(30_000 + seed)
    out = {}
    for key, t in module.state_dict().items():
        shape = tuple(t.shape)
        if key.endswith(_CONV_W):
            b = gain * float(np.sqrt(6.0 / (shape[1] * shape[2] * shape[3])))
            v = rng.uniform(-b, b, shape).astype(np.float32)
        elif key.endswith(_SHIFT):
            v = rng.normal(0, 0.1, shape).astype(np.float32)
        elif key.endswith(_SCALE):
            v = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif key.endswith("num_batches_tracked"):
            v = np.asarray(1, np.int64)
        elif key.endswith("blk.0.offset"):
            continue
        else:
            raise KeyError(f"draw_state_dict: no rule for {key!r}")
        out[key] = v
    return out


def load_drawn(module, seed: int, gain: float = 1.0):
    """draw_state_dict into the module (strict: `offset` is handed back as the module has it); returns the drawn arrays."""
    import torch
    sd = draw_state_dict(module, seed, gain)
    full = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    full.update({k: v for k, v in module.state_dict().items() if k not in full})
    module.load_state_dict(full, strict=True)
    return sd


def signature(module):
    return [f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items()]


# ---- launch routes ------------------------------------------------------------------------------------------------------
# A forward as the list of its launches.  A conv2d launch reads 'conv k<k> s<stride> <Cin>-><Cout> <impl>' plus ' nchw' | ' u8'
# (input layout / dtype), ' packed' (w_packed given) and ' ->split' (out_split given); 'rbs' is resblock2d_split ('rbs ->f32'
# without out_split), 'rb' the fused resblock2d, 's2s' conv2d_s2_split, 'deform' and 'inorm' the deformable conv and instance norm.
def _conv(k, stride, cin, cout, split, inorm, nchw=False, u8=False, out_split=False):
    """One BaseConvBlk2d as Conv2dLaunch.run launches it: the split-bf16 kernel for a 3x3 layer on multiples of 16 channels in the
    split modes (never under instance norm), the fp32 MFMA kernel for 3x3, Cin % 16 == 0, Cout of 16 | 32, else CONV_AUTO (the
    direct kernel, the stem kernels).  w_packed goes with the two matrix-core forms and with the uint8 3 -> 16 stem."""
    m16 = k == 3 and cin % 16 == 0 and not nchw and not u8
    if split and not inorm and m16 and cout % 16 == 0:
        impl, packed = "b3", True
    elif m16 and cout in (16, 32):
        impl, packed = "mfma", True
    else:
        impl, packed = "auto", u8
    t = f"conv k{k} s{stride} {cin}->{cout} {impl}" + (" u8" if u8 else " nchw" if nchw else "")
    return [t + (" packed" if packed else "") + (" ->split" if out_split else "")] + (["inorm"] if inorm else [])


def expected_route(name: str, mode: str, u8: bool = False):
    """The launches of one forward, restated from the case's arguments alone (what _split_chain_forward and the two *_forward
    functions decide): in the split modes a run of 16 -> 16 3x3 residual blocks (batch norm or none, an activation of slope 0 ... 1)
    is served on pre-split activations when the layer in front of it can write the split format -- the (5, 2, 3, 16) stem, a 3x3
    16 -> 16 layer on fp32 input, or conv2d_s2_split between two runs; a run with no such layer in front (another in_chs) takes the
    fused resblock2d; every other residual block is two convs."""
    kw = kwargs_of(CASES[name])
    cin, chs, k, layers = kw["in_chs"], kw["chs"], kw["k_sz"], kw["layers"]
    split, inorm, sphere = mode != "f32", kw["norm_type"] == "instance", CASES[name]["cls"] == "Sphere"
    u8_stem = u8 and (cin, chs) == (3, 16)             # any other stem gets torch's conversion in front: fp32 NCHW
    fused = split and not inorm and k == 3 and chs == 16
    items = ["stem"]
    for step, n in enumerate(layers):
        items += ["res"] * n + (["s2"] if step != len(layers) - 1 else [])
    if not sphere:
        items.append("final")

    def run_len(i):
        n = 0
        while fused and i + n < len(items) and items[i + n] == "res":
            n += 1
        return n
    out, i, in_split = [], 0, False
    while i < len(items):
        it = items[i]
        if it == "res":
            out += ["rb"] if fused else _conv(k, 1, chs, chs, split, inorm) + _conv(k, 1, chs, chs, split, inorm)
            i += 1
            continue
        n = run_len(i + 1)
        kk, st, ci = {"stem": (5, 2, cin), "s2": (3, 2, chs), "final": (k, 1, chs)}[it]
        can = (cin, chs) == (3, 16) if it == "stem" else kk == 3
        if in_split:
            out.append("s2s")
        else:
            out += _conv(kk, st, ci, chs, split, inorm, nchw=it == "stem" and not u8_stem, u8=it == "stem" and u8_stem,
                         out_split=n > 0 and can)
        if n > 0 and (can or in_split):
            j = i + 1 + n
            in_split = j < len(items) and items[j] == "s2" and run_len(j + 1) > 0
            out += ["rbs"] * (n - 1) + ["rbs" if in_split else "rbs ->f32"]
            i = j
        else:
            i += 1
    if sphere:
        out += ["deform"] + (["inorm"] if inorm else [])
    return out


# what was read from the code when these tests were planned, written out (split modes, float images): the restated walk must say
# the same (tests/test_extractor_args_host.py)
_STEM = "conv k5 s2 3->16 auto nchw"
_FINAL = "conv k3 s1 16->16 b3 packed"
_S2 = "conv k3 s2 16->16 b3 packed"
LITERAL_ROUTES = {
    "chs16": [_STEM + " ->split"] + ["rbs"] * 5 + ["s2s"] + ["rbs"] * 9 + ["rbs ->f32", _FINAL],
    "sphere": [_STEM + " ->split"] + ["rbs"] * 5 + ["s2s"] + ["rbs"] * 9 + ["rbs ->f32", "deform"],
    "layers_none": [_STEM, _FINAL],
    "layers_3": [_STEM + " ->split", "rbs", "rbs", "rbs ->f32", _FINAL],
    "layers_0_3": [_STEM, _S2 + " ->split", "rbs", "rbs", "rbs ->f32", _FINAL],
    "layers_3_0": [_STEM + " ->split", "rbs", "rbs", "rbs ->f32", _S2, _FINAL],
    "layers_1_1": [_STEM + " ->split", "rbs", "s2s", "rbs ->f32", _FINAL],
    "layers_2_0_2": [_STEM + " ->split", "rbs", "rbs ->f32", _S2, _S2 + " ->split", "rbs", "rbs ->f32", _FINAL],
    "layers_2_2_2": [_STEM + " ->split", "rbs", "rbs", "s2s", "rbs", "rbs", "s2s", "rbs", "rbs ->f32", _FINAL],
    "gray": ["conv k5 s2 1->16 auto nchw", "rb", "rb", _S2 + " ->split", "rbs", "rbs ->f32", _FINAL],
    "in4": ["conv k5 s2 4->16 auto nchw", "rb", "rb", _S2 + " ->split", "rbs", "rbs ->f32", _FINAL],
    "k5": [_STEM] + ["conv k5 s1 16->16 auto"] * 4 + [_S2] + ["conv k5 s1 16->16 auto"] * 5,
    "chs6": ["conv k5 s2 3->6 auto nchw"] + ["conv k3 s1 6->6 auto"] * 4 + ["conv k3 s2 6->6 auto"] + ["conv k3 s1 6->6 auto"] * 5,
    "chs48": ["conv k5 s2 3->48 auto nchw"] + ["conv k3 s1 48->48 b3 packed"] * 2 + ["conv k3 s2 48->48 b3 packed"]
             + ["conv k3 s1 48->48 b3 packed"] * 5,
    "instance_c8": ["conv k5 s2 3->8 auto nchw", "inorm"] + ["conv k3 s1 8->8 auto", "inorm"] * 2 + ["conv k3 s2 8->8 auto", "inorm"]
                   + ["conv k3 s1 8->8 auto", "inorm"] * 3,
}
# the split kernel's template arguments per (Cout / 16, stride): one tile; two tiles (32 and 48 channels: a remainder of one tile at
# 48); the two-by-two form (64 and 80: a remainder at 80); the two stride-2 forms (32 | 48 and above)
B3_TEMPLATE = {(1, 1): "<1, 4, 4, 1, 1, 16, 16, 1, 1,", (2, 1): "<2, 4, 4, 1, 1, 16, 16, 1, 1,", (3, 1): "<2, 4, 4, 1, 1, 16, 16, 1, 1,",
               (4, 1): "<2, 4, 2, 2, 1, 8, 16, 1, 1,", (5, 1): "<2, 4, 2, 2, 1, 8, 16, 1, 1,",
               (1, 2): "<2, 1, 4, 1, 1, 4, 16, 2, 1,", (2, 2): "<2, 1, 4, 1, 1, 4, 16, 2, 1,", (3, 2): "<2, 2, 2, 2, 1, 4, 16, 2, 1,",
               (4, 2): "<2, 2, 2, 2, 1, 4, 16, 2, 1,", (5, 2): "<2, 2, 2, 2, 1, 4, 16, 2, 1,"}
