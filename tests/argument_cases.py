"""One canonical call per public entry point of mvs_gi_amd.hip_ops that reaches a launching symbol of include/mvsgi.h (plus the free
functions of dropin/ that call the library themselves), at the smallest shape its own test uses, with the ROLE of every tensor
argument.  tests/test_gpu_argument_forms.py walks this table.

roles
  act        an activation: hip_ops._dev takes it in any strides / at any offset and copies where the kernel needs it otherwise
  mask       the same for a bool / uint8 mask
  param      a parameter (scale, shift, weights in any layout, plans): read in place, never copied -- hip_ops._arg
  out, res   a caller-owned output / residual of the exact output shape: read or written in place -- hip_ops._arg
  split      a SplitAct the kernel reads or writes in place (its storage is a caller-owned buffer)
An argument "a/k" is the entry k of the dict argument a.

A row's builder returns a fresh Case each time (same seed, same values): outputs the caller supplies are never shared between two
calls that are compared.  Optional caller-owned buffers of the entry points that already checked every tensor before this table
existed (`ws` / `out` of metrics, losses, pack_cloud, photo_consistency, reproject, confidence) are left to the wrapper.

ACCEPTED: (row, argument, bad form) the wrapper legitimately takes, with the reason; everything else in BAD_FORMS must raise.
  conv3d_direct / conv2d_auto_packed, w_packed "short": size not checkable -- CONV_DIRECT (and conv2d's CONV_AUTO on fp32 input)
  never reads w_packed and no query tells which layout a caller may have at hand; its form (device, dtype, contiguity, alignment) is
  still checked.
  rays_panorama, dist "short": the candidate count is dist's own length.
REFUSED: (row, argument, awkward form) of an ACTIVATION a wrapper refuses by design instead of copying -- it must raise (no launch),
never compute something else.
  pack_cloud (every tensor) and photo_consistency's mask go through hip_ops._cloud_plane: "nothing is copied or converted", so that
  a call with `ws` and `out` allocates nothing (a documented contract of those two entry points); they take an offset view (their
  kernels need the element's alignment only; photo's mask 4 bytes when W % 4 == 0) and refuse a non-contiguous one.

EXEMPT: launching symbols no Python wrapper reaches, each with its reason (test_every_launching_symbol_has_a_row).
"""
from __future__ import annotations

import zlib
from collections import namedtuple

import numpy as np
import torch

from mvs_gi_amd import hip_ops as H

DEV = "cuda:0"
Case = namedtuple("Case", "fn args roles cl")

BAD_FORMS = ("cpu", "float64", "float16", "short", "long", "strided", "offset")      # "long" for out / res only
SPLIT_BAD_FORMS = ("cpu", "shape", "dtype", "strided", "offset")                      # of a SplitAct's buf
ACT_FORMS = ("transposed", "offset", "expand", "channels_last")

ACCEPTED = {
    ("conv3d_direct", "w_packed", "short"): "size not checkable: CONV_DIRECT never reads w_packed",
    ("conv2d_auto_packed", "w_packed", "short"): "size not checkable: CONV_AUTO on fp32 input never reads w_packed",
    ("rays_panorama", "dist", "short"): "the number of candidates IS the length of dist: one fewer is another valid call",
}

REFUSED = {}
for _name in ("inv", "rays", "mask", "warped", "valid", "gates/0", "attrs/0"):
    for _form in ("transposed", "expand"):
        REFUSED[("pack_cloud", _name, _form)] = "pack_cloud copies nothing (hip_ops._cloud_plane): a non-contiguous tensor is refused"
for _form in ("transposed", "expand"):
    REFUSED[("photo_consistency", "mask", _form)] = "photo_consistency's mask is read in place (hip_ops._cloud_plane)"
REFUSED[("photo_consistency", "mask", "offset")] = "photo_consistency's mask must be 4-byte aligned when W % 4 == 0 (read as words)"

EXEMPT = {
    "mvsgi_softargmin_f32": "mvsgi_softargmin_div_f32 with post_div 1: hip_ops.softargmin calls the _div form",
    "mvsgi_sweep_std_nhwc_valid_split": "bf16-only predecessor of mvsgi_sweep_std_nhwc_valid_split_fmt",
    "mvsgi_act_f32_to_split": "bf16-only predecessor of mvsgi_act_f32_to_split_fmt",
    "mvsgi_act_split_to_f32": "bf16-only predecessor of mvsgi_act_split_to_f32_fmt",
    "mvsgi_conv3d_f32_out_split": "bf16-only predecessor of mvsgi_conv3d_f32_out_split_fmt",
    "mvsgi_conv3d_rs_pack_weights": "bf16-only predecessor of mvsgi_conv3d_rs_pack_weights_fmt",
    "mvsgi_conv3d_rs_split": "bf16-only predecessor of mvsgi_conv3d_rs_split_fmt",
    "mvsgi_conv3d_rs16_split": "bf16-only predecessor of mvsgi_conv3d_rs16_split_fmt (fp32 output)",
    "mvsgi_conv3d_rs16_split_out_split": "bf16-only predecessor of mvsgi_conv3d_rs16_split_fmt (split-padded output)",
    "mvsgi_conv3d_s2rs_pack_weights": "bf16-only predecessor of mvsgi_conv3d_s2rs_pack_weights_fmt",
    "mvsgi_conv3d_s2rs": "bf16-only predecessor of mvsgi_conv3d_s2rs_out_fmt",
    "mvsgi_conv3d_s2rs_fmt": "mvsgi_conv3d_s2rs_out_fmt with y_f32p 0: hip_ops.conv3d_s2rs calls the _out form",
    "mvsgi_conv3d_up2_poly_split": "bf16-only predecessor of mvsgi_conv3d_up2_poly_fmt (y_is_split 1)",
    "mvsgi_conv3d_up2_poly_f32": "bf16-only predecessor of mvsgi_conv3d_up2_poly_fmt (y_is_split 0)",
    "mvsgi_conv3d_pack_weights_bf16x3": "per-layout predecessor of mvsgi_conv3d_pack_weights_split (tests/test_gpu_pack_split.py compares the bytes)",
    "mvsgi_conv3d_pack_weights_bf16x3_v32": "per-layout predecessor of mvsgi_conv3d_pack_weights_split",
    "mvsgi_conv3d_pack_weights_bf16x3_c16": "per-layout predecessor of mvsgi_conv3d_pack_weights_split",
}


# ------------------------------------------------------------------------------ values
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _r(rng, *shape, s=1.0):
    return _g((rng.standard_normal(shape) * s).astype(np.float32))


def _bn(rng, c):
    return _g(rng.uniform(0.5, 1.5, c).astype(np.float32)), _g((rng.standard_normal(c) * 0.1).astype(np.float32))


def _w(rng, cout, cin, *k):
    k = k or (3, 3, 3)
    return _g((rng.standard_normal((cout, cin) + k) / np.sqrt(cin * np.prod(k))).astype(np.float32))


def _empty(*shape, dtype=torch.float32):
    return torch.empty(shape, device=DEV, dtype=dtype)


def _split(rng, B, D, Hh, W, C, fmt="bf16"):
    return H.act_to_split(_r(rng, B, D, Hh, W, C), fmt=fmt)


def _case(fn, args, roles, cl=None):
    assert set(roles) <= {p for p in _paths(args)}, (sorted(roles), sorted(_paths(args)))
    return Case(fn, args, roles, cl or {})


def _paths(args):
    for k, v in args.items():
        if isinstance(v, dict):
            for kk in v:
                yield f"{k}/{kk}"
        elif isinstance(v, (list, tuple)):
            for i in range(len(v)):
                yield f"{k}/{i}"
        else:
            yield k


def get(args, path):
    k, _, sub = path.partition("/")
    v = args[k]
    if not sub:
        return v
    return v[sub] if isinstance(v, dict) else v[int(sub)]


def put(args, path, value):
    """args with the tensor at `path` replaced (containers copied, gates' (tensor, lo, hi) triples kept)."""
    k, _, sub = path.partition("/")
    args = dict(args)
    if not sub:
        args[k] = value
    elif isinstance(args[k], dict):
        args[k] = dict(args[k], **{sub: value})
    else:
        seq = list(args[k])
        seq[int(sub)] = value
        args[k] = type(args[k])(seq) if isinstance(args[k], tuple) else seq
    return args


# ------------------------------------------------------------------------------ forms
def bad_form(t: torch.Tensor, form: str):
    """A tensor with t's role in one of BAD_FORMS (values do not matter: no kernel may see it)."""
    n = t.numel()
    if form == "cpu":
        return torch.zeros(t.shape, dtype=t.dtype)
    if form == "float64":
        return torch.zeros(t.shape, device=t.device, dtype=torch.float64)
    if form == "float16":
        return torch.zeros(t.shape, device=t.device, dtype=torch.float16)
    if form == "short":
        return torch.zeros(n - 1, device=t.device, dtype=t.dtype)
    if form == "long":
        return torch.zeros(n + 1, device=t.device, dtype=t.dtype)
    if form == "strided":              # [::2] of a tensor twice as long in its last axis: t's shape, every second element
        big = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), device=t.device, dtype=t.dtype)
        v = big[..., ::2]
        assert v.shape == t.shape and (not v.is_contiguous() or n <= 1)
        return v
    if form == "offset":               # t[1:] of a tensor with numel + 1 elements: contiguous, t's shape, one element off alignment
        v = torch.zeros(n + 1, device=t.device, dtype=t.dtype)[1:].view(t.shape)
        assert v.data_ptr() % 16 == t.element_size() % 16 and v.is_contiguous()
        return v
    raise KeyError(form)


def bad_split(s: "H.SplitAct", form: str) -> "H.SplitAct":
    """A copy of the SplitAct whose buf has been replaced after construction (the constructor would refuse it)."""
    shp = (s.B, s.D + 2, s.H + 2, s.W + 2, s.C)
    if form == "cpu":
        buf = torch.zeros(shp, dtype=torch.int32)
    elif form == "shape":
        buf = torch.zeros((s.B, s.D + 1, s.H + 2, s.W + 2, s.C), device=s.buf.device, dtype=torch.int32)
    elif form == "dtype":
        buf = torch.zeros(shp, device=s.buf.device, dtype=torch.float32)
    else:
        buf = bad_form(s.buf, form)
    t = H.SplitAct(s.B, s.D, s.H, s.W, s.C, s.buf.device)
    t.buf, t.fmt, t.rec = buf, s.fmt, s.rec
    return t


def act_form(t: torch.Tensor, form: str, cl=None):
    """t's values in an awkward form, or None where the form does not apply to this tensor.  "expand" changes the values (frame 0 in
    every frame): its baseline is expand_base(t)."""
    if form == "transposed":
        if t.dim() < 2 or t.shape[-1] == 1 or t.shape[-2] == 1:
            return None
        v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
        assert not v.is_contiguous()
    elif form == "offset":
        flat = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
        v = flat[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == t.element_size() % 16
    elif form == "expand":
        if t.dim() < 2 or t.shape[0] < 2:
            return None
        v = t[:1].expand(t.shape)
        assert v.stride(0) == 0
        return v
    elif form == "channels_last":
        if cl is None:
            return None
        v = cl(t)
        assert not v.is_contiguous()
    else:
        raise KeyError(form)
    assert v.shape == t.shape and torch.equal(v, t)
    return v


def expand_base(t: torch.Tensor) -> torch.Tensor:
    return t[:1].expand(t.shape).contiguous()


def _cl5(t):          # [B, C, D, H, W] in channels-last storage
    return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def _cl_feats(t):     # [B, N, C, H, W] with the channel innermost in storage
    return t.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)


def _cl4(t):          # [B, C, H, W] in channels-last storage
    return t.contiguous(memory_format=torch.channels_last)


def flatten(res):
    """result of a call -> list of tensors (a SplitAct by its storage)"""
    if res is None:
        return []
    if isinstance(res, H.SplitAct):
        return [res.buf]
    if isinstance(res, torch.Tensor):
        return [res]
    if isinstance(res, dict):
        return [t for k in sorted(res) for t in flatten(res[k])]
    if isinstance(res, (tuple, list)):
        return [t for r in res for t in flatten(r)]
    if isinstance(res, (int, float)):
        return []
    raise TypeError(type(res))


# ------------------------------------------------------------------------------ rows
ROWS = {}


def row(fn):
    ROWS[fn.__name__] = fn
    return fn


# ---- conv3d family: x (1, 3, 5, 7, 16), 16 -> 16 ----
def _conv3d(name, impl, pack):
    rng = _rng(name)
    x, w = _r(rng, 1, 3, 5, 7, 16), _w(rng, 16, 16)
    sc, sh = _bn(rng, 16)
    wp = pack(w)
    if isinstance(wp, tuple):           # an fp16 packing: (weights, unscale [Cout]), the unscale folded into the scale
        wp, sc = wp[0], (sc * wp[1]).contiguous()
    args = dict(x=x, w_oidhw=w, w_packed=wp, scale=sc, shift=sh, res=_r(rng, 1, 3, 5, 7, 16), out=_empty(1, 3, 5, 7, 16))
    return _case(lambda **a: H.conv3d(a["x"], a["w_oidhw"], a["w_packed"], a["scale"], a["shift"], res=a["res"], impl=impl, out=a["out"]), args,
                 dict(x="act", w_oidhw="param", w_packed="param", scale="param", shift="param", res="res", out="out"))


@row
def conv3d_mfma():
    return _conv3d("conv3d_mfma", H.CONV_MFMA, H.pack_conv_weights)


@row
def conv3d_auto():
    return _conv3d("conv3d_auto", H.CONV_AUTO, H.pack_conv_weights)


@row
def conv3d_direct():
    return _conv3d("conv3d_direct", H.CONV_DIRECT, H.pack_conv_weights)


@row
def conv3d_bf16x3():
    return _conv3d("conv3d_bf16x3", H.CONV_BF16X3, H.pack_conv_weights_bf16x3)


@row
def conv3d_c16_f16():
    return _conv3d("conv3d_c16_f16", H.CONV_BF16X3_C16 | H.CONV_F16, lambda w: H.pack_conv_weights_f16x3(w, H.CONV_BF16X3_C16))


def _up2(name, split):
    rng = _rng(name)
    x, w = _r(rng, 1, 2, 3, 4, 16), _w(rng, 16, 16)
    sc, sh = _bn(rng, 16)
    args = dict(x=x, w_packed_b3=H.pack_conv_weights_bf16x3(w), scale=sc, shift=sh, res=_r(rng, 1, 4, 6, 8, 16),
                out=H.SplitAct(1, 4, 6, 8, 16, DEV) if split else _empty(1, 4, 6, 8, 16))
    f = H.conv3d_up2_out_split if split else H.conv3d_up2
    return _case(lambda **a: f(a["x"], a["w_packed_b3"], a["scale"], a["shift"], res=a["res"], out=a["out"]), args,
                 dict(x="act", w_packed_b3="param", scale="param", shift="param", res="res", out="split" if split else "out"))


@row
def conv3d_up2():
    return _up2("conv3d_up2", False)


@row
def conv3d_up2_out_split():
    return _up2("conv3d_up2_out_split", True)


@row
def conv3d_out_split():
    rng = _rng("conv3d_out_split")
    x, w = _r(rng, 1, 3, 5, 7, 16), _w(rng, 16, 16)
    sc, sh = _bn(rng, 16)
    args = dict(x=x, w_packed_b3=H.pack_conv_weights_bf16x3(w), scale=sc, shift=sh, out=H.SplitAct(1, 3, 5, 7, 16, DEV), res=_r(rng, 1, 3, 5, 7, 16))
    return _case(lambda **a: H.conv3d_out_split(a["x"], a["w_packed_b3"], a["scale"], a["shift"], a["out"], res=a["res"]), args,
                 dict(x="act", w_packed_b3="param", scale="param", shift="param", res="res", out="split"))


@row
def act_to_split():
    rng = _rng("act_to_split")
    return _case(lambda **a: H.act_to_split(a["x"], out=a["out"], fmt="f16"), dict(x=_r(rng, 1, 2, 4, 16, 32), out=H.SplitAct(1, 2, 4, 16, 32, DEV)),
                 dict(x="act", out="split"))


@row
def act_from_split():
    rng = _rng("act_from_split")
    return _case(lambda **a: H.act_from_split(a["x"], out=a["out"]), dict(x=_split(rng, 1, 2, 4, 16, 32), out=_empty(1, 2, 4, 16, 32)),
                 dict(x="split", out="out"))


# ---- register-stationary kernels: (1, 2, 4, 16) voxels ----
def _rs(name, out_f32):
    rng = _rng(name)
    sc, sh = _bn(rng, 32)
    args = dict(x=_split(rng, 1, 2, 4, 16, 32), w_packed_rs=H.pack_conv_weights_rs(_w(rng, 32, 32)), scale=sc, shift=sh,
                res=_split(rng, 1, 2, 4, 16, 32), out=_empty(1, 2, 4, 16, 32) if out_f32 else H.SplitAct(1, 2, 4, 16, 32, DEV))
    return _case(lambda **a: H.conv3d_rs(a["x"], a["w_packed_rs"], a["scale"], a["shift"], res=a["res"], out=a["out"], out_f32=out_f32), args,
                 dict(x="split", w_packed_rs="param", scale="param", shift="param", res="split", out="out" if out_f32 else "split"))


@row
def conv3d_rs():
    return _rs("conv3d_rs", False)


@row
def conv3d_rs_out_f32():
    return _rs("conv3d_rs_out_f32", True)


def _rs16(name, split):
    rng = _rng(name)
    sc, sh = _bn(rng, 16)
    args = dict(x=_split(rng, 1, 2, 4, 16, 16), w_packed_rs=H.pack_conv_weights_rs(_w(rng, 16, 16)), scale=sc, shift=sh,
                out=H.SplitAct(1, 2, 4, 16, 16, DEV) if split else _empty(1, 2, 4, 16, 16))
    if split:
        fn = lambda **a: H.conv3d_rs16(a["x"], a["w_packed_rs"], a["scale"], a["shift"], out_split=a["out"])
    else:
        fn = lambda **a: H.conv3d_rs16(a["x"], a["w_packed_rs"], a["scale"], a["shift"], out=a["out"])
    return _case(fn, args, dict(x="split", w_packed_rs="param", scale="param", shift="param", out="split" if split else "out"))


@row
def conv3d_rs16():
    return _rs16("conv3d_rs16", False)


@row
def conv3d_rs16_out_split():
    return _rs16("conv3d_rs16_out_split", True)


@row
def conv3d_s2rs():
    rng = _rng("conv3d_s2rs")
    sc, sh = _bn(rng, 32)
    args = dict(x=_split(rng, 1, 2, 4, 16, 16), w_packed=H.pack_conv_weights_s2rs(_w(rng, 32, 16), sc), shift=sh, out=H.SplitAct(1, 1, 2, 8, 32, DEV))
    return _case(lambda **a: H.conv3d_s2rs(a["x"], a["w_packed"], a["shift"], a["out"]), args,
                 dict(x="split", w_packed="param", shift="param", out="split"))


@row
def conv3d_wino():
    rng = _rng("conv3d_wino")
    sc, sh = _bn(rng, 32)
    wp, un = H.pack_conv_weights_wino(_w(rng, 32, 32))
    args = dict(x=_split(rng, 1, 8, 2, 32, 32, "f16"), w_packed=wp, scale=(sc * un).contiguous(), shift=sh, res=_split(rng, 1, 8, 2, 32, 32, "f16"),
                out=H.SplitAct(1, 8, 2, 32, 32, DEV))
    return _case(lambda **a: H.conv3d_wino(a["x"], a["w_packed"], a["scale"], a["shift"], res=a["res"], out=a["out"]), args,
                 dict(x="split", w_packed="param", scale="param", shift="param", res="split", out="split"))


@row
def conv3d_wino_out_f32():
    rng = _rng("conv3d_wino_out_f32")
    sc, sh = _bn(rng, 32)
    wp, un = H.pack_conv_weights_wino(_w(rng, 32, 32))
    args = dict(x=_split(rng, 1, 8, 2, 32, 32, "f16"), w_packed=wp, scale=(sc * un).contiguous(), shift=sh, out=_empty(1, 8, 2, 32, 32))
    return _case(lambda **a: H.conv3d_wino(a["x"], a["w_packed"], a["scale"], a["shift"], out=a["out"], out_f32=True), args,
                 dict(x="split", w_packed="param", scale="param", shift="param", out="out"))


# ---- polyphase ResizeConv3d and the split cost head ----
def _poly(name, kind):
    """kind: 'f32' (fp32 output), 'split' (direct main kernel), 'rec32' (fp32 records: the Winograd form, D == 8, H even, W % 32 == 0)"""
    rng = _rng(name)
    d, h, w = (8, 2, 32) if kind == "rec32" else (2, 4, 16)
    fmt = "f16" if kind == "rec32" else "bf16"
    sc, sh = _bn(rng, 16)
    plan = H.conv3d_up2_poly_plan(_w(rng, 16, 32), d, h, w, fmt=fmt)
    if fmt == "f16":
        plan, un = plan
        sc = (sc * un).contiguous()
    out = _empty(1, 2 * d, 2 * h, 2 * w, 16) if kind == "f32" else H.SplitAct(1, 2 * d, 2 * h, 2 * w, 16, DEV)
    if kind == "rec32":
        out.rec = "f32"
    args = dict(x=_split(rng, 1, d, h, w, 32, fmt), plan=plan, scale=sc, shift=sh, out=out)
    if kind == "f32":
        fn = lambda **a: H.conv3d_up2_poly(a["x"], a["plan"], a["scale"], a["shift"], out=a["out"])
    else:
        fn = lambda **a: H.conv3d_up2_poly_split(a["x"], a["plan"], a["scale"], a["shift"], a["out"], direct=kind == "split")
    return _case(fn, args, dict(x="split", plan="param", scale="param", shift="param", out="out" if kind == "f32" else "split"))


@row
def conv3d_up2_poly():
    return _poly("conv3d_up2_poly", "f32")


@row
def conv3d_up2_poly_split():
    return _poly("conv3d_up2_poly_split", "split")


@row
def conv3d_up2_poly_rec32():
    return _poly("conv3d_up2_poly_rec32", "rec32")


def _head(name, kind):
    rng = _rng(name)
    w = _w(rng, 1, 16)
    if kind == "bf16":
        x, wp, un = _split(rng, 1, 2, 4, 16, 16), H.pack_head_split_weights(w), 1.0
    else:
        wp, un = H.pack_head_split_weights_f16(w)
        x = _split(rng, 1, 2, 4, 16, 16, "f16")
        if kind == "rec32":         # fp32 records in the padded geometry: C plain fp32 per voxel in the same bytes
            x.buf.view(torch.float32)[:, 1:-1, 1:-1, 1:-1] = _r(rng, 1, 2, 4, 16, 16)
            x.rec = "f32"
    args = dict(x=x, w_packed=wp, out=_empty(1, 2, 4, 16, 1))
    return _case(lambda **a: H.conv3d_head_split(a["x"], a["w_packed"], 1.0 * un, 0.37, out=a["out"], f16=kind != "bf16"), args,
                 dict(x="split", w_packed="param", out="out"))


@row
def conv3d_head_split():
    return _head("conv3d_head_split", "bf16")


@row
def conv3d_head_split_f16():
    return _head("conv3d_head_split_f16", "f16")


@row
def conv3d_head_rec32():
    return _head("conv3d_head_rec32", "rec32")


# ---- weight packers: the weight is copied where it is awkward (an activation to _dev) ----
def _packer(name, f, *wshape, extra=None):
    def build():
        rng = _rng(name)
        args = dict(w=_w(rng, *wshape))
        roles = dict(w="act")
        if extra:
            args["scale"] = _bn(rng, extra)[0]
            roles["scale"] = "act"
        return _case(lambda **a: f(*a.values()), args, roles)
    build.__name__ = name
    return row(build)


_packer("pack_conv_weights", H.pack_conv_weights, 16, 16)
_packer("pack_conv_weights_bf16x3", H.pack_conv_weights_bf16x3, 16, 16)
_packer("pack_conv_weights_rs", H.pack_conv_weights_rs, 32, 32)
_packer("pack_conv_weights_s2rs", H.pack_conv_weights_s2rs, 32, 16, extra=32)
_packer("pack_conv_weights_wino", H.pack_conv_weights_wino, 32, 32)
_packer("pack_head_split_weights", H.pack_head_split_weights, 1, 16)
_packer("pack_head_split_weights_f16", lambda w: H.pack_head_split_weights_f16(w)[0], 1, 16)
_packer("pack_conv2d_weights_bf16x3", H.pack_conv2d_weights_bf16x3, 16, 16, 3, 3)
_packer("pack_conv2d_weights_f32", H.pack_conv2d_weights_f32, 16, 16, 3, 3)
_packer("pack_conv2d_stem_weights", H.pack_conv2d_stem_weights, 16, 3, 5, 5)
_packer("pack_resblock2d_split_weights", H.pack_resblock2d_split_weights, 16, 16, 3, 3, extra=16)
_packer("pack_deform_conv2d_weights", H.pack_deform_conv2d_weights, 16, 16, 3, 3)


# ---- conv2d family: x (1, 5, 4, 16), 16 -> 16 ----
def _conv2d(name, impl, pack, out_split=False):
    rng = _rng(name)
    x, w = _r(rng, 1, 5, 4, 16), _w(rng, 16, 16, 3, 3)
    sc, sh = _bn(rng, 16)
    args = dict(x=x, w_oihw=w, w_packed=pack(w), scale=sc, shift=sh, res=_r(rng, 1, 5, 4, 16))
    roles = dict(x="act", w_oihw="param", w_packed="param", scale="param", shift="param", res="res")
    if out_split:
        args["out_split"] = H.split2d_buffer(1, 5, 4, DEV)
        roles["out_split"] = "out"
    return _case(lambda **a: H.conv2d(a["x"], a["w_oihw"], a["w_packed"], a["scale"], a["shift"], res=a["res"], impl=impl, out_split=a.get("out_split")),
                 args, roles)


@row
def conv2d_bf16x3():
    return _conv2d("conv2d_bf16x3", H.CONV_BF16X3, H.pack_conv2d_weights_bf16x3)


@row
def conv2d_mfma():
    return _conv2d("conv2d_mfma", H.CONV_MFMA, H.pack_conv2d_weights_f32)


@row
def conv2d_auto_packed():
    return _conv2d("conv2d_auto_packed", H.CONV_AUTO, H.pack_conv2d_weights_f32)


@row
def conv2d_out_split2d():
    return _conv2d("conv2d_out_split2d", H.CONV_BF16X3, H.pack_conv2d_weights_bf16x3, out_split=True)


def _stem(name, u8):
    rng = _rng(name)
    w = _w(rng, 16, 3, 5, 5)
    sc, sh = _bn(rng, 16)
    x = _g(rng.integers(0, 256, (1, 5, 4, 3), dtype=np.uint8)) if u8 else _g(rng.random((1, 3, 5, 4)).astype(np.float32))
    args = dict(x=x, w_oihw=w, scale=sc, shift=sh)
    roles = dict(x="act", w_oihw="param", scale="param", shift="param")
    if u8:
        args["w_packed"] = H.pack_conv2d_stem_weights(w)
        roles["w_packed"] = "param"
    return _case(lambda **a: H.conv2d(a["x"], a["w_oihw"], a.get("w_packed"), a["scale"], a["shift"], stride=2, in_nchw=not u8), args, roles,
                 None if u8 else dict(x=_cl4))


@row
def conv2d_stem_u8():
    return _stem("conv2d_stem_u8", True)


@row
def conv2d_stem_nchw():
    return _stem("conv2d_stem_nchw", False)


@row
def resblock2d():
    rng = _rng("resblock2d")
    (s1, h1), (s2, h2) = _bn(rng, 16), _bn(rng, 16)
    args = dict(x=_r(rng, 1, 5, 4, 16), wp1=H.pack_conv2d_weights_bf16x3(_w(rng, 16, 16, 3, 3)), scale1=s1, shift1=h1,
                wp2=H.pack_conv2d_weights_bf16x3(_w(rng, 16, 16, 3, 3)), scale2=s2, shift2=h2)
    return _case(lambda **a: H.resblock2d(*a.values()), args, dict(x="act", wp1="param", scale1="param", shift1="param", wp2="param",
                                                                   scale2="param", shift2="param"))


@row
def f32_to_split2d():
    rng = _rng("f32_to_split2d")
    return _case(lambda **a: H.f32_to_split2d(a["x"], out=a["out"]), dict(x=_r(rng, 1, 5, 4, 16), out=H.split2d_buffer(1, 5, 4, DEV)),
                 dict(x="act", out="out"))


@row
def split2d_to_f32():
    rng = _rng("split2d_to_f32")
    return _case(lambda **a: H.split2d_to_f32(a["x_split"]), dict(x_split=H.f32_to_split2d(_r(rng, 1, 5, 4, 16))), dict(x_split="param"))


def _resblock2d_split(name, split_out):
    rng = _rng(name)
    (s1, h1), (s2, h2) = _bn(rng, 16), _bn(rng, 16)
    args = dict(x_split=H.f32_to_split2d(_r(rng, 1, 5, 4, 16)), wp1=H.pack_resblock2d_split_weights(_w(rng, 16, 16, 3, 3), s1), shift1=h1,
                wp2=H.pack_resblock2d_split_weights(_w(rng, 16, 16, 3, 3), s2), shift2=h2)
    roles = dict(x_split="param", wp1="param", shift1="param", wp2="param", shift2="param")
    if split_out:
        args["out_split"] = H.split2d_buffer(1, 5, 4, DEV)
        roles["out_split"] = "out"
    return _case(lambda **a: H.resblock2d_split(a["x_split"], a["wp1"], a["shift1"], a["wp2"], a["shift2"], out_split=a.get("out_split")), args, roles)


@row
def resblock2d_split():
    return _resblock2d_split("resblock2d_split", False)


@row
def resblock2d_split_out_split():
    return _resblock2d_split("resblock2d_split_out_split", True)


@row
def conv2d_s2_split():
    rng = _rng("conv2d_s2_split")
    sc, sh = _bn(rng, 16)
    args = dict(x_split=H.f32_to_split2d(_r(rng, 1, 5, 4, 16)), w_packed=H.pack_resblock2d_split_weights(_w(rng, 16, 16, 3, 3), sc), shift=sh,
                out_split=H.split2d_buffer(1, 3, 2, DEV))
    return _case(lambda **a: H.conv2d_s2_split(*a.values()), args, dict(x_split="param", w_packed="param", shift="param", out_split="out"))


@row
def deform_conv2d():
    # the first row of test_deform_conv2d_vs_oracle: (N, Cin, Cout, H, W, k, stride, pad, dil, res, slope) = (2, 16, 16, 12, 40, 3, 1, 1, 1, True, 0.01)
    rng = _rng("deform_conv2d")
    sc, sh = _bn(rng, 16)
    args = dict(x=_r(rng, 2, 12, 40, 16), offset=_r(rng, 2, 18, 12, 40, s=1.5), w_packed=H.pack_deform_conv2d_weights(_w(rng, 16, 16, 3, 3)),
                scale=sc, shift=sh, res=_r(rng, 2, 12, 40, 16))
    return _case(lambda **a: H.deform_conv2d(a["x"], a["offset"], a["w_packed"], a["scale"], a["shift"], (3, 3), (1, 1), (1, 1), (1, 1),
                                             res=a["res"], neg_slope=0.01), args,
                 dict(x="act", offset="act", w_packed="param", scale="param", shift="param", res="res"))


# ---- resize, layout, soft-argmin, confidence, instance norm ----
@row
def resize_trilinear():
    return _case(lambda **a: H.resize_trilinear(a["x"], (5, 6, 9)), dict(x=_r(_rng("resize_trilinear"), 2, 2, 3, 5, 16)), dict(x="act"))


@row
def ncdhw_to_ndhwc():
    return _case(lambda **a: H.ncdhw_to_ndhwc(a["x"]), dict(x=_r(_rng("ncdhw_to_ndhwc"), 2, 16, 2, 3, 5)), dict(x="act"), dict(x=_cl5))


@row
def ndhwc_to_ncdhw():
    return _case(lambda **a: H.ndhwc_to_ncdhw(a["x"]), dict(x=_r(_rng("ndhwc_to_ncdhw"), 2, 2, 3, 5, 16)), dict(x="act"))


@row
def as_ndhwc():
    # the contiguous NCDHW volume of another producer: a transposed copy; in channels-last storage: the view itself
    return _case(lambda **a: H.as_ndhwc(a["vol"]).contiguous(), dict(vol=_r(_rng("as_ndhwc"), 2, 16, 2, 3, 5)), dict(vol="act"), dict(vol=_cl5))


def _costs(name, B=1):
    rng = _rng(name)
    return _r(rng, B, 4, 3, 5, s=4.0), _g((96.0 / np.geomspace(0.5, 100.0, 4)).astype(np.float32))


def _softargmin(name, scale):
    c, idx = _costs(name)
    return _case(lambda **a: H.softargmin(a["costs"], a["inv_idx"], scale, True, post_div=96.0), dict(costs=c, inv_idx=idx),
                 dict(costs="act", inv_idx="act"))


@row
def softargmin_x2():
    return _softargmin("softargmin_x2", 2)


@row
def softargmin_scaled():
    return _softargmin("softargmin_scaled", 3)


@row
def confidence():
    c, idx = _costs("confidence", B=2)
    return _case(lambda **a: H.confidence(a["costs"], a["inv_idx"], 2), dict(costs=c, inv_idx=idx), dict(costs="act", inv_idx="act"))


@row
def instance_norm():
    rng = _rng("instance_norm")
    g, b = _bn(rng, 16)
    args = dict(x=_r(rng, 2, 7, 16), res=_r(rng, 2, 7, 16), gamma=g, beta=b, out=_empty(2, 7, 16))
    return _case(lambda **a: H.instance_norm(a["x"], a["res"], a["gamma"], a["beta"], neg_slope=0.01, out=a["out"]), args,
                 dict(x="act", res="act", gamma="param", beta="param", out="out"))


# ---- sweeps: D 2, Ho 3, Wo 5, 3 cameras, C 16 ----
def _rig(name, N=3, C=16, B=2):
    rng = _rng(name)
    return dict(feats=_r(rng, B, N, C, 4, 6), grids=_g(rng.uniform(-1.2, 1.2, (B, N, 2, 3, 5, 2)).astype(np.float32)),
                grid_masks=_g(rng.random((B, N, 2, 3, 5, 1)) < 0.8), masks=_g((rng.random((B, N, 1, 8, 12)) < 0.8).astype(np.float32)))


_SWEEP_ROLES = dict(feats="act", grids="act", grid_masks="mask", masks="act")


def _sweep_std(name, layout, N=3):
    return _case(lambda **a: H.sweep_std(a["feats"], a["grids"], a["grid_masks"], a["masks"], layout=layout), _rig(name, N), _SWEEP_ROLES,
                 dict(feats=_cl_feats))


@row
def sweep_std_nchw():
    return _sweep_std("sweep_std_nchw", "nchw")


@row
def sweep_std_nhwc():
    return _sweep_std("sweep_std_nhwc", "auto")


@row
def sweep_std_five_cameras():
    return _sweep_std("sweep_std_five_cameras", "auto", N=5)


def _sweep_cat(name, layout):
    a = _rig(name)
    return _case(lambda **a: H.sweep_cat(a["feats"], a["grids"], layout=layout), dict(feats=a["feats"], grids=a["grids"]),
                 dict(feats="act", grids="act"), dict(feats=_cl_feats))


@row
def sweep_cat_nchw():
    return _sweep_cat("sweep_cat_nchw", "nchw")


@row
def sweep_cat_nhwc():
    return _sweep_cat("sweep_cat_nhwc", "auto")


@row
def sweep_validity():
    a = _rig("sweep_validity")
    return _case(lambda **a: H.sweep_validity(a["grids"], a["grid_masks"], a["masks"]), dict(grids=a["grids"], grid_masks=a["grid_masks"], masks=a["masks"]),
                 dict(grids="act", grid_masks="mask", masks="act"))


def _valid(name, rig_shared=False, split=False):
    a = _rig(name)
    vm = _g(_rng(name + "v").integers(0, 8, (2, 2, 3, 5), dtype=np.uint8))
    args = dict(feats=a["feats"], grids=a["grids"][:1].contiguous() if rig_shared else a["grids"], vmask=vm[:1].contiguous() if rig_shared else vm)
    roles = dict(feats="act", grids="act", vmask="mask")
    if split:
        args["out"] = H.SplitAct(2, 2, 3, 5, 16, DEV)
        roles["out"] = "split"
        return _case(lambda **a: H.sweep_std_valid_split(a["feats"], a["grids"], a["vmask"], a["out"], fmt="f16"), args, roles, dict(feats=_cl_feats))
    return _case(lambda **a: H.sweep_std_valid(a["feats"], a["grids"], a["vmask"]), args, roles, dict(feats=_cl_feats))


@row
def sweep_std_valid():
    return _valid("sweep_std_valid")


@row
def sweep_std_valid_rig():
    return _valid("sweep_std_valid_rig", rig_shared=True)


@row
def sweep_std_valid_split():
    return _valid("sweep_std_valid_split", split=True)


# ---- geometry: resampler, back-projection, photometric consistency, point cloud ----
def _cams(N):
    T = torch.eye(4).repeat(N, 1, 1)
    T[:, :3, 3] = torch.linspace(-0.05, 0.05, 3 * N).view(N, 3)
    cams = torch.zeros(N, H.REPROJECT_CAM_FLOATS)
    cams[:, 0] = 1.0                                    # equirectangular: the nine after the id are not read
    cams[0] = torch.tensor([0.0, -0.203, 0.589, 8.0, 8.0, 5.5, 3.5, 0.0, 7.0, 11.0])       # camera 0: double sphere on the 8 x 12 images
    alpha, xi = 0.589, -0.203
    w1 = (1 - alpha) / alpha
    cams[0, 7] = (w1 + xi) / (2 * w1 * xi + xi * xi + 1) ** 0.5
    return T, cams


def _view(name, B=2, N=2, u8=True):
    rng = _rng(name)
    lat, lon = np.meshgrid(np.linspace(-1.2, 1.2, 6), np.linspace(-2.5, 2.5, 8), indexing="ij")
    rays = np.stack([np.cos(lat) * np.cos(lon), np.sin(lat), -np.cos(lat) * np.sin(lon)]).astype(np.float32)
    imgs = _g(rng.integers(0, 256, (B * N, 8, 12, 3), dtype=np.uint8)) if u8 else _r(rng, B * N, 3, 8, 12)
    return dict(inv=_g(rng.uniform(2.0, 60.0, (B, 6, 8)).astype(np.float32)), rays=_g(rays), imgs=imgs)


@row
def reproject_u8():
    a = _view("reproject_u8")
    T, cams = _cams(2)
    return _case(lambda **a: H.reproject(a["inv"], a["rays"], T, cams, 96.0, imgs=a["imgs"], want=("xyz", "warped", "valid", "grid")), a,
                 dict(inv="act", rays="act", imgs="act"))


@row
def reproject_f32():
    a = _view("reproject_f32", u8=False)
    T, cams = _cams(2)
    return _case(lambda **a: H.reproject(a["inv"], a["rays"], T, cams, 96.0, imgs=a["imgs"]), a, dict(inv="act", rays="act", imgs="act"), dict(imgs=_cl4))


@row
def photo_consistency():
    rng = _rng("photo_consistency")
    a = _view("photo_consistency")
    T, cams = _cams(2)
    a.update(cam_masks=_g((rng.random((2, 1, 8, 12)) < 0.9).astype(np.float32)), mask=_g(rng.random((2, 6, 8)) < 0.8))
    return _case(lambda **a: H.photo_consistency(a["inv"], a["rays"], T, cams, 96.0, a["imgs"], cam_masks=a["cam_masks"], mask=a["mask"]), a,
                 dict(inv="act", rays="act", imgs="act", cam_masks="act", mask="mask"))


@row
def pack_cloud():
    rng = _rng("pack_cloud")
    a = _view("pack_cloud")
    args = dict(inv=a["inv"], rays=a["rays"], mask=_g(rng.random((2, 6, 8)) < 0.8), gates=[(_g(rng.random((2, 6, 8)).astype(np.float32)), 0.1, 0.9)],
                warped=_g(rng.random((2, 2, 3, 6, 8)).astype(np.float32)), valid=_g(rng.random((2, 2, 6, 8)) < 0.5),
                attrs=[_r(rng, 2, 6, 8)])
    # written rows only: rows >= counts[:, 0] of points / index are not written by contract
    def fn(**a):
        gates = [(g[0] if isinstance(g, (tuple, list)) else g, 0.1, 0.9) for g in a["gates"]]
        r = H.pack_cloud(a["inv"], a["rays"], 96.0, d_range=H.CLOUD_D_RANGE, gates=gates, mask=a["mask"], warped=a["warped"], valid=a["valid"],
                         attrs=a["attrs"], want_index=True)
        n = r["counts"][:, 0].tolist()
        return [r["counts"]] + [r[k][b, :n[b]].clone() for k in ("points", "index") for b in range(len(n))]
    args["gates"] = [args["gates"][0][0]]        # the table addresses the gate's plane; fn restores the (plane, lo, hi) triple
    return _case(fn, args, {"inv": "act", "rays": "act", "mask": "mask", "gates/0": "act", "warped": "act", "valid": "mask", "attrs/0": "act"})


def _resample(name, u8):
    rng = _rng(name)
    imgs = _g(rng.integers(0, 256, (4, 8, 12, 3), dtype=np.uint8)) if u8 else _r(rng, 4, 3, 8, 12)
    args = dict(imgs=imgs, grid=_g(rng.uniform(-1.1, 1.1, (2, 6, 8, 2)).astype(np.float32)), valid=_g(rng.random((2, 6, 8)) < 0.8), out=_empty(4, 3, 6, 8))
    return _case(lambda **a: H.resample_bilinear(a["imgs"], a["grid"], a["valid"], invalid_value=-3.5, out=a["out"]), args,
                 dict(imgs="act", grid="act", valid="mask", out="out"), None if u8 else dict(imgs=_cl4))


@row
def resample_bilinear_u8():
    return _resample("resample_bilinear_u8", True)


@row
def resample_bilinear_f32():
    return _resample("resample_bilinear_f32", False)


@row
def resample_validity():
    rng = _rng("resample_validity")
    return _case(lambda **a: H.resample_validity(a["grid"], a["in_fov"]),
                 dict(grid=_g(rng.uniform(-1.1, 1.1, (2, 6, 8, 2)).astype(np.float32)), in_fov=_g(rng.random((2, 6, 8)) < 0.8)), dict(grid="act", in_fov="mask"))


# ---- validation metrics and losses ----
@row
def metrics():
    rng = _rng("metrics")
    args = dict(preds=_g(rng.uniform(2.0, 150.0, (2, 1, 12, 13)).astype(np.float32)), target=_g(rng.uniform(2.0, 150.0, (2, 1, 12, 13)).astype(np.float32)),
                valid_mask=_g(rng.random((2, 1, 12, 13)) < 0.8))
    return _case(lambda **a: H.metrics(a["preds"], a["target"], 96.0, 0.96, 192.0, valid_mask=a["valid_mask"]), args,
                 dict(preds="act", target="act", valid_mask="mask"))


@row
def losses():
    rng = _rng("losses")
    idx = _g((96.0 / np.array([0.5, 1, 2, 5], np.float32)).astype(np.float32))
    args = dict(labels=_g(rng.uniform(10.0, 200.0, (2, 1, 6, 10)).astype(np.float32)), inv_idx=idx, pred=_g(rng.uniform(10.0, 200.0, (2, 1, 6, 10)).astype(np.float32)),
                costs=_r(rng, 2, 4, 3, 5, s=4.0), vol_mask=_g(rng.random((2, 1, 6, 10)) < 0.8), px_mask=_g(rng.random((2, 1, 6, 10)) < 0.8))
    return _case(lambda **a: H.losses(a["labels"], a["inv_idx"], pred=a["pred"], costs=a["costs"], scale=2, vol_mask=a["vol_mask"], px_mask=a["px_mask"],
                                      inbounds=(96.0, 1.0)), args,
                 dict(labels="act", inv_idx="act", pred="act", costs="act", vol_mask="mask", px_mask="mask"))


# ---- dropin/: the functions that call the library themselves ----
@row
def rays_panorama():
    from mvs_gi_amd.dropin import sweep_grids as SG

    def fn(**a):
        rm = SG.RayMaker_UEPanorama(np.zeros(1, np.float32), (0.0, 6.0), (-1.5, 0.0), device=DEV)
        rm.dist = a["dist"]
        return rm.make_rays_for_candidates((3, 5))
    return _case(fn, dict(dist=_g(np.array([0.5, 1.0, 2.0, 5.0], np.float32))), dict(dist="param"))


@row
def transform_3D_points():
    from mvs_gi_amd.dropin import sweep_grids as SG
    rng = _rng("transform_3D_points")
    T = torch.eye(4, device=DEV).repeat(2, 1, 1) + _r(rng, 2, 4, 4, s=0.05)
    return _case(lambda **a: SG.transform_3D_points_torch(a["T"], a["points"]), dict(T=T, points=_r(rng, 2, 3, 2, 3, 5)), dict(T="act", points="act"))


def _grid_maker(name, equirect):
    from mvs_gi_amd.dropin import sweep_grids as SG
    maker = SG.EquirectangularSampleGridMaker() if equirect else SG.DoubleSphereSampleGridMaker()
    return _case(lambda **a: maker.make_grid(a["points"]), dict(points=_r(_rng(name), 2, 3, 2, 3, 5)), dict(points="act"))


@row
def grid_double_sphere():
    return _grid_maker("grid_double_sphere", False)


@row
def grid_equirect():
    return _grid_maker("grid_equirect", True)


@row
def equirect_surrogate_rays():
    from mvs_gi_amd.dropin import image_sampler as IS
    return _case(lambda **a: IS.equirect_surrogate_rays(3, 5, DEV), {}, {})


@row
def extractor_nhwc():
    from mvs_gi_amd.dropin import feature_extractor as FE
    return _case(lambda **a: FE._nhwc(a["x"]).contiguous(), dict(x=_r(_rng("extractor_nhwc"), 2, 16, 5, 4)), dict(x="act"), dict(x=_cl4))
