"""Host-side mirror of the 3-D building blocks of dsta_mvs/model/common/common_modules.py
(NoOp :13-16, BaseConvBlk3d :82-115, ResConvBlk3d :186-244, ResizeConv3d :305-355) and of
the registries in dsta_mvs/model/common/__init__.py:7-23.

The classes keep the reference's constructor arguments, attribute names and child-module
names, so state dicts load unchanged and module objects pickled by the reference
(Lightning `save_hyperparameters()`, spherical_sweep_stereo.py:74) unpickle into them.
Their `forward` runs the hand-written HIP kernels through the C ABI; nothing here
computes on the CPU.
"""
from __future__ import annotations

import os

import copy
from typing import Dict, NamedTuple, Optional, Type

import torch
from torch import nn, Tensor

from .. import hip_ops as H


def module_getstate(self):
    """__getstate__ of the drop-in modules (and, in patch mode, of the reference's classes): the launch records, packed
    weights, polyphase plans and module-owned activation buffers cached on a module under `_mvsgi_*` keys are derived data
    -- they are rebuilt on the next forward and must not travel with a pickled module or a whole-module checkpoint
    (Lightning's save_hyperparameters() pickles module OBJECTS, spherical_sweep_stereo.py:74)."""
    return {k: v for k, v in self.__dict__.items() if not k.startswith("_mvsgi_")}


# ------------------------------------------------------------------------------------------
# module-owned activation buffers: a captured hipGraph holds their addresses
# ------------------------------------------------------------------------------------------
def _owned_split_buffer(owner, attr: str, key: tuple, make):
    """Module-owned split-padded buffers (owner.__dict__[attr], an `_mvsgi_*` name: module_getstate), one per shape key, NEVER
    replaced or freed while the module lives: a captured hipGraph holds their addresses, and their zero borders are written
    exactly once (at allocation) -- the kernels write interiors only.  `make` allocates the entry of a new key."""
    bufs = owner.__dict__.setdefault(attr, {})
    if key not in bufs:
        bufs[key] = make()
    return bufs[key]


def _owned_head_buffer(self, B, D, Hh, W, C, device):
    """The module-owned split-padded buffer between out_costs.0 and the split head: ONE allocation per frame geometry, sized for the
    largest batch seen, handed out as a view of its first B frames (the format is per frame: a prefix of the batch is a valid
    buffer).  A caller that varies its batch (batch sweeps, dataset tails) therefore holds one buffer, not one per batch size; a
    larger batch replaces it -- unless a captured hipGraph may hold its address (`_mvsgi_pinned`, set while capturing), in which
    case the old one stays alive beside the new."""
    bufs = self.__dict__.setdefault("_mvsgi_head_bufs", {})
    key = (D, Hh, W, C, device)
    ent = bufs.get(key)
    if ent is None or ent[0].B < B:
        big = H.SplitAct(B, D, Hh, W, C, device)
        keep = ent[1] + [ent[0]] if ent is not None and (ent[2] or ent[1]) else []      # graphs may hold the old buffers
        ent = bufs[key] = [big, keep, False]
    if torch.cuda.is_current_stream_capturing():
        ent[2] = True
    big = ent[0]
    if big.B == B:
        return big
    return H.SplitAct(B, D, Hh, W, C, device, buf=big.buf[:B])


class NoOp(nn.Identity):
    """Alias of nn.Identity, as in the reference (common_modules.py:13-16)."""
    def infer_size(self, in_size):
        return in_size


RELU_TYPE: Dict[str, Type[nn.Module]] = {"original": nn.ReLU, "leaky": nn.LeakyReLU, "none": NoOp}
NORM2D_TYPE: Dict[str, Type[nn.Module]] = {"batch": nn.BatchNorm2d, "instance": nn.InstanceNorm2d, "none": NoOp}
NORM3D_TYPE: Dict[str, Type[nn.Module]] = {"batch": nn.BatchNorm3d, "instance": nn.InstanceNorm3d, "none": NoOp}


# ------------------------------------------------------------------------------------------
# lowering of one conv block to the arguments of mvsgi_conv3d_f32
# ------------------------------------------------------------------------------------------
# MVSGI_D32=0: keep the Cin % 32 == 0 stride-1 layers of large launches on the tap-pair layout (default: 32-channel slices,
# csrc/conv3d_bf16x3.hpp D32 -- 27 k-steps per 32 channels instead of 28 and half the slices per unit: 6-9 % of those layers)
_USE_D32 = os.environ.get("MVSGI_D32", "1") != "0"
_D32_OK: Dict[tuple, bool] = {}       # (up2, cin, cout, B, D, H, W) -> mvsgi_conv3d_up2_d32_applies / mvsgi_conv3d_d32_applies


class Packed(NamedTuple):
    """What one kernel's launch needs of a layer: its packed weights and the epilogue constants that go with THAT packing (an fp16
    packing's power-of-two pre-scale is undone in `scale`, or, where the kernel has no per-channel multiplier, in `unscale`)."""
    wp: Tensor
    scale: object           # Tensor [Cout]; a float for the cost head; None where the scale is folded into the weights
    shift: object           # Tensor [Cout]; a float for the cost head
    unscale: float = 1.0


class ConvLaunch:
    """Device-resident launch arguments of one BaseConvBlk3d: PyTorch-layout weight, exact-fp32 packed MFMA weight (or None),
    per-channel scale/shift (eval BatchNorm3d or bias), stride, slope -- and, in ONE cache, every other packing of the weights
    a kernel has asked for, keyed ("stream", layout, fmt) | ("rs", fmt) | ("s2", fmt) | ("wino",) | ("head", fmt) |
    ("poly", D, H, W, fmt) with fmt the 16-bit split ('bf16' | 'f16').  The library's mode picks the key, so a mode switch can
    never meet another mode's weights; a changed parameter makes a new ConvLaunch (lower_conv_block)."""
    __slots__ = ("w", "wp", "scale", "shift", "stride", "neg_slope", "cin", "cout", "key", "inorm", "_cache")

    def __init__(self, w: Tensor, scale: Tensor, shift: Tensor, stride: int, neg_slope: float, inorm=None, key=None):
        self.w = w
        self.wp = H.pack_conv_weights(w)      # eager: a pack launch in the first forward could fall into a stream capture
        self.scale, self.shift = scale.contiguous(), shift.contiguous()
        self.stride, self.neg_slope, self.inorm, self.key = int(stride), neg_slope, inorm, key
        self.cout, self.cin = int(w.shape[0]), int(w.shape[1])
        self._cache: Dict[tuple, Packed] = {}

    def _cached(self, key: tuple, make) -> Packed:
        ent = self._cache.get(key)
        if ent is None:
            ent = self._cache[key] = make()
        return ent

    def _entry(self, packed) -> Packed:
        """Packed of a packer's result: the weights alone (bf16 split), or (weights, unscale [Cout]) (fp16 split)."""
        wp, unscale = packed if isinstance(packed, tuple) else (packed, None)
        return Packed(wp, self.scale if unscale is None else (self.scale * unscale).contiguous(), self.shift)

    def run(self, x_ndhwc: Tensor, res: Optional[Tensor] = None, impl: Optional[int] = None) -> Tensor:
        if self.inorm is not None:          # conv (+ bias) -> instance norm (+ res) -> act: two more launches
            return self.inorm.apply(self._run_conv(x_ndhwc, None, impl), res)
        return self._run_conv(x_ndhwc, res, impl)

    def _run_conv(self, x_ndhwc: Tensor, res: Optional[Tensor] = None, impl: Optional[int] = None) -> Tensor:
        wp, scale = self.wp, self.scale      # CONV_AUTO (and any explicit impl but CONV_BF16X3): the exact-fp32 weights
        if impl is None:
            impl = H.CONV_AUTO
            if H.split_mode() and self.cin % 16 == 0 and self.cout % 16 == 0:
                impl, wp, scale = self._stream(self._stream_layout(x_ndhwc.shape[:4]), H.mode_fmt())
        elif impl == H.CONV_BF16X3:
            wp = self._stream_packed(H.CONV_BF16X3, "bf16").wp
        return H.conv3d(x_ndhwc, self.w, wp, scale, self.shift, res=res, stride=self.stride, neg_slope=self.neg_slope, impl=impl)

    def _stream_layout(self, dims=None, up2: bool = False) -> int:
        """THE layout rule of the streaming split kernel: the plane schedule for Cout == 16, else 32-channel slices where the
        library says they serve a launch of dims = (B, D, H, W) (`up2`: the fused upsample + conv, low-resolution sizes; dims
        None: a kernel with no such form), else tap pairs.  One library query per launch shape, not per launch.  The plain
        conv asks only for stride-1 layers; in 'f32' mode (a direct run_up2 call: the bf16 split) the slices are never taken."""
        if self._c16():
            return H.CONV_BF16X3_C16
        if dims is not None and _USE_D32 and H.split_mode() and self.cin % 32 == 0 and (up2 or (self.stride == 1 and self.cout % 16 == 0)):
            key = (up2, self.cin, self.cout) + tuple(dims)
            ok = _D32_OK.get(key)
            if ok is None:
                ok = _D32_OK[key] = H.conv3d_up2_d32_applies(dims[0], self.cin, *dims[1:], self.cout) if up2 else \
                    H.conv3d_d32_applies(dims[0], self.cin, *dims[1:], self.cout, self.stride)
            if ok:
                return H.CONV_BF16X3_D32
        return H.CONV_BF16X3

    def _stream_packed(self, layout: int, fmt: str) -> Packed:
        """The streaming split kernel's weights in `layout` and the split `fmt`, with the scale that goes with them."""
        return self._cached(("stream", layout, fmt), lambda: self._entry(H._pack_conv3d_split(self.w, layout, fmt)))

    def _stream(self, layout: int, fmt: str):
        """(impl / w_layout, packed weights, scale) of the streaming split kernel in `layout` and the split `fmt`."""
        p = self._stream_packed(layout, fmt)
        return layout | (H.CONV_F16 if fmt == "f16" else 0), p.wp, p.scale

    def _c16(self) -> bool:
        """Cout == 16, stride 1: the plane-schedule kernel (MVSGI_CONV_BF16X3_C16)."""
        return self.cout == 16 and self.stride == 1 and self.cin % 16 == 0

    def rs_ok(self) -> bool:
        """The register-stationary kernel (csrc/conv3d_rs.hip) serves this layer."""
        return self.inorm is None and H.conv3d_rs_applies(self.cin, self.cout, self.stride, self.neg_slope)

    def _rs(self, fmt: str) -> Packed:
        """The register-stationary kernels' weights in the split `fmt` of the activations."""
        return self._cached(("rs", fmt), lambda: self._entry(H.pack_conv_weights_rs(self.w, fmt)))

    def wino_ok(self, D: int, Hh: int, W: int) -> bool:
        """The Winograd-form kernel (csrc/conv3d_wino.hip) serves this layer on a [D, Hh, W] volume (fp16 split only)."""
        return self.inorm is None and H.conv3d_wino_applies(self.cin, self.cout, D, Hh, W, self.stride, self.neg_slope)

    def _wino(self) -> Packed:
        return self._cached(("wino",), lambda: self._entry(H.pack_conv_weights_wino(self.w)))

    def s2rs_ok(self) -> bool:
        """The stride-2 16 -> 32 kernel on split-padded activations (csrc/conv3d_s2rs.hip) serves this layer."""
        return self.inorm is None and H.split_mode() and H.conv3d_s2rs_applies(self.cin, self.cout, self.stride, self.neg_slope)

    def _s2(self, fmt: str) -> Packed:
        """The stride-2 kernel on split-padded activations: the scale is folded into its weights; in the fp16 split one power of
        two `up` with them, carried by the shift and undone by `unscale` (H.pack_conv_weights_s2rs)."""
        def make():
            if fmt == "bf16":
                return Packed(H.pack_conv_weights_s2rs(self.w, self.scale), None, self.shift)
            wp, up, un = H.pack_conv_weights_s2rs(self.w, self.scale, "f16")
            return Packed(wp, None, (self.shift * up).contiguous(), un)
        return self._cached(("s2", fmt), make)

    def poly_ok(self) -> bool:
        """ResizeConv3d in polyphase form on the register-stationary kernel (csrc/conv3d_up2poly.hip)."""
        return self.inorm is None and H.split_mode() and self.stride == 1 and H.conv3d_up2_poly_applies(self.cin, self.cout, self.neg_slope)

    def _poly_plan(self, x_split) -> Packed:
        """Folded phase weights + face tables for the low-resolution split-padded input: built once per size and split, kept."""
        D, Hh, W, fmt = x_split.D, x_split.H, x_split.W, x_split.fmt
        return self._cached(("poly", D, Hh, W, fmt), lambda: self._entry(H.conv3d_up2_poly_plan(self.w, D, Hh, W, fmt=fmt)))

    def head_split_ok(self) -> bool:
        """The split cost head on a split-padded input (csrc/conv3d_headsplit.hip), in either 16-bit split."""
        return self.inorm is None and H.split_mode() and self.cout == 1 and self.cin % 16 == 0 and self.stride == 1

    def run_head_split(self, x_split) -> Tensor:
        def make():       # scale / shift as host floats: one host read at lowering time
            if x_split.fmt == "f16":
                wp, unscale = H.pack_head_split_weights_f16(self.w)
                return Packed(wp, float(self.scale[0]) * unscale, float(self.shift[0]))
            return Packed(H.pack_head_split_weights(self.w), float(self.scale[0]), float(self.shift[0]))
        p = self._cached(("head", x_split.fmt), make)
        return H.conv3d_head_split(x_split, p.wp, p.scale, p.shift, neg_slope=self.neg_slope, f16=x_split.fmt == "f16")

    def run_up2_poly_split(self, x_split, out) -> "H.SplitAct":
        p = self._poly_plan(x_split)
        return H.conv3d_up2_poly_split(x_split, p.wp, p.scale, self.shift, out=out, neg_slope=self.neg_slope)

    def run_up2_poly(self, x_split, out=None) -> Tensor:
        p = self._poly_plan(x_split)
        return H.conv3d_up2_poly(x_split, p.wp, p.scale, self.shift, neg_slope=self.neg_slope, out=out)

    def run_up2_split(self, x_lowres_ndhwc: Tensor, res: Optional[Tensor], out) -> "H.SplitAct":
        """conv(trilinear_x2(x)) (+ res) written split-padded into `out` (the polyphase layer's input, the split head's input);
        this kernel has no 32-channel-slice form."""
        _no_inorm(self, "run_up2_split")
        w_layout, wp, scale = self._stream(self._stream_layout(), H.mode_fmt())
        return H.conv3d_up2_out_split(x_lowres_ndhwc, wp, scale, self.shift, out=out, res=res, neg_slope=self.neg_slope, w_layout=w_layout)

    def can_fuse_up2(self) -> bool:
        """conv(trilinear_x2(x)) in one launch writing fp32 (run_up2): an instance norm follows it like any other conv."""
        return H.split_mode() and self.stride == 1 and self.cin % 16 == 0 and self.cout % 16 == 0

    def run_up2(self, x_lowres_ndhwc: Tensor, res: Optional[Tensor] = None) -> Tensor:
        """conv(trilinear_x2(x)) in one launch (mvsgi_conv3d_up2_f32)."""
        if self.inorm is not None:
            return self.inorm.apply(self._run_up2(x_lowres_ndhwc, None), res)
        return self._run_up2(x_lowres_ndhwc, res)

    def _run_up2(self, x_lowres_ndhwc: Tensor, res: Optional[Tensor] = None) -> Tensor:
        w_layout, wp, scale = self._stream(self._stream_layout(x_lowres_ndhwc.shape[:4], up2=True), H.mode_fmt())
        return H.conv3d_up2(x_lowres_ndhwc, wp, scale, self.shift, res=res, neg_slope=self.neg_slope, w_layout=w_layout)


def _is_identity(m) -> bool:
    return m is None or isinstance(m, nn.Identity)


def _fingerprint(blk) -> tuple:
    """Everything the lowered launch record depends on: parameter identity and in-place version (pointer and
    version as SEPARATE entries), the norm layer's mode / eps, the activation and the stride.  `training` is part
    of the key, so a later `model.train()` re-lowers and raises instead of silently reusing eval statistics."""
    conv = blk.conv_layer
    parts = [conv.weight.data_ptr(), conv.weight._version, tuple(conv.stride)]
    if conv.bias is not None:
        parts += [conv.bias.data_ptr(), conv.bias._version]
    parts += norm_key(blk.norm_layer)
    act = blk.activation
    parts += [type(act).__name__, float(getattr(act, "negative_slope", 0.0))]
    return tuple(parts)


_BN = (nn.BatchNorm3d, nn.BatchNorm2d)
_IN = (nn.InstanceNorm3d, nn.InstanceNorm2d)


def norm_key(norm) -> list:
    """The part of a launch record's key that the norm layer decides: type, mode, eps, affine / running-statistics tensors."""
    parts = [type(norm).__name__]
    if isinstance(norm, _BN + _IN):
        parts += [bool(norm.training), float(norm.eps), bool(getattr(norm, "track_running_stats", True))]
        for t in (norm.weight, norm.bias, norm.running_mean, norm.running_var):
            parts += [None, None] if t is None else [t.data_ptr(), t._version]
    return parts


class InstanceNormLaunch:
    """Instance norm with input statistics after a conv (F.instance_norm, use_input_stats): the conv writes conv + bias with no
    activation, then mvsgi_instance_norm_f32 normalises per (frame, channel) and adds the residual and the activation in place."""
    __slots__ = ("gamma", "beta", "eps", "neg_slope")

    def apply(self, y: Tensor, res: Optional[Tensor] = None) -> Tensor:
        return H.instance_norm(y, res=res, gamma=self.gamma, beta=self.beta, eps=self.eps, neg_slope=self.neg_slope, out=y)


def _no_inorm(L, what: str) -> None:
    if L.inorm is not None:
        raise RuntimeError(f"{what}: this layer has an instance norm (its epilogue does not fold); use the plain fp32 path")


def lower_norm(norm, conv_bias: Optional[Tensor], cout: int, device, slope: float, dims: int = 3):
    """-> (scale, shift, InstanceNormLaunch | None) of the conv epilogue for the block's norm layer (common_modules.py:107-115:
    conv -> norm -> (+ res) -> act).  Eval BatchNorm, and InstanceNorm with running statistics in eval mode (then the same
    formula), fold into scale / shift; InstanceNorm with input statistics leaves scale = 1, shift = bias and returns the record
    of the norm launch that follows the conv."""
    bias = conv_bias.detach().float() if conv_bias is not None else None
    name = type(norm).__name__
    use_running = isinstance(norm, _BN) or (isinstance(norm, _IN) and norm.track_running_stats)
    if use_running:
        if norm.training:
            raise RuntimeError(f"HIP path implements eval-mode {name} only: call model.eval()")
        if norm.running_mean is None or norm.running_var is None:
            raise NotImplementedError(f"{name} without running statistics")
        gamma = norm.weight.detach().float() if norm.weight is not None else torch.ones(cout, device=device)
        beta = norm.bias.detach().float() if norm.bias is not None else torch.zeros(cout, device=device)
        # ATen eval batch_norm: alpha = gamma / sqrt(var + eps); y = x * alpha + (beta - mean * alpha)
        alpha = gamma / torch.sqrt(norm.running_var.detach().float() + norm.eps)
        scale = alpha
        shift = beta - norm.running_mean.detach().float() * alpha
        if bias is not None:
            shift = shift + bias * alpha
        return scale, shift, None
    scale = torch.ones(cout, device=device, dtype=torch.float32)
    shift = bias.clone() if bias is not None else torch.zeros(cout, device=device, dtype=torch.float32)
    if _is_identity(norm):
        return scale, shift, None
    if isinstance(norm, _IN):
        if norm.affine and norm.num_features != cout:          # (as _InstanceNorm.forward: without affine tensors torch only warns)
            raise ValueError(f"{name}({norm.num_features}) after a conv with {cout} output channels")
        rec = InstanceNormLaunch()
        rec.gamma = norm.weight.detach().float().contiguous() if norm.affine and norm.weight is not None else None
        rec.beta = norm.bias.detach().float().contiguous() if norm.affine and norm.bias is not None else None
        rec.eps, rec.neg_slope = float(norm.eps), float(slope)
        return scale, shift, rec
    raise NotImplementedError(f"norm layer {name} has no HIP implementation "
                              f"(only BatchNorm{dims}d in eval mode, InstanceNorm{dims}d and NoOp)")


def act_slope(act) -> float:
    if isinstance(act, nn.LeakyReLU):
        return float(act.negative_slope)
    if isinstance(act, nn.ReLU):
        return 0.0
    if _is_identity(act):
        return 1.0
    raise NotImplementedError(f"activation {type(act).__name__} has no HIP implementation")


def lower_conv_block(blk) -> ConvLaunch:
    """Build (and cache on the module, keyed by parameter identity/version) the launch
    arguments of a BaseConvBlk3d-shaped module {conv_layer, norm_layer, activation}."""
    key = _fingerprint(blk)
    cached = blk.__dict__.get("_mvsgi_launch")
    if cached is not None and cached.key == key:
        return cached
    conv: nn.Conv3d = blk.conv_layer
    if not isinstance(conv, nn.Conv3d):
        raise NotImplementedError(f"conv_layer is {type(conv).__name__}, expected nn.Conv3d")
    if tuple(conv.kernel_size) != (3, 3, 3) or tuple(conv.padding) != (1, 1, 1) or tuple(conv.dilation) != (1, 1, 1) \
            or conv.groups != 1 or conv.padding_mode != "zeros" or len(set(conv.stride)) != 1 \
            or conv.stride[0] not in (1, 2):
        raise NotImplementedError(
            f"HIP conv3d supports kernel 3, padding 1, stride 1|2, dense; got kernel {tuple(conv.kernel_size)}, "
            f"padding {tuple(conv.padding)}, stride {tuple(conv.stride)}, groups {conv.groups}")
    w = conv.weight.detach()
    if not w.is_cuda:
        raise RuntimeError("mvs_gi_amd modules run on the GPU only: call .cuda() on the model "
                           "(there is no CPU fallback)")
    w = w.to(torch.float32).contiguous()
    cout = w.shape[0]
    if isinstance(blk.norm_layer, (nn.BatchNorm2d, nn.InstanceNorm2d)):
        raise NotImplementedError(f"norm layer {type(blk.norm_layer).__name__} after a Conv3d")
    slope = act_slope(blk.activation)
    scale, shift, inorm = lower_norm(blk.norm_layer, conv.bias, cout, w.device, slope)
    if inorm is not None:
        slope = 1.0                 # the conv writes conv + bias; the activation follows the norm
    L = ConvLaunch(w, scale, shift, conv.stride[0], slope, inorm, key)
    blk.__dict__["_mvsgi_launch"] = L
    return L


def _to_ncdhw_view(y_ndhwc: Tensor) -> Tensor:
    """[B, D, H, W, C] storage presented with the reference's [B, C, D, H, W] shape
    (channels_last_3d strides; no copy)."""
    return y_ndhwc.permute(0, 4, 1, 2, 3)


# ------------------------------------------------------------------------------------------
# blocks (ndhwc-level helpers are used by the regulator / builder forwards)
# ------------------------------------------------------------------------------------------
class BaseConvBlk3d(nn.Module):
    def __init__(self, in_chs: int, out_chs: int, kernel_size: int, stride: int = 1, extra_pad: int = 0,
                 bias_on: bool = False, norm_layer: nn.Module = NoOp(), activation: nn.Module = NoOp()):
        super().__init__()
        self.conv_layer = nn.Conv3d(in_chs, out_chs, kernel_size, padding=(kernel_size // 2) + extra_pad,
                                    bias=bias_on, stride=stride)
        self.norm_layer = norm_layer
        self.activation = activation

    __getstate__ = module_getstate

    def forward_ndhwc(self, x: Tensor, res: Optional[Tensor] = None) -> Tensor:
        return lower_conv_block(self).run(x, res)

    def forward(self, x: Tensor, res: Optional[Tensor] = None) -> Tensor:
        r = None if res is None else H.as_ndhwc(res)
        return _to_ncdhw_view(self.forward_ndhwc(H.as_ndhwc(x), r))


def res_block_ndhwc(blk, x: Tensor) -> Tensor:
    """ResConvBlk3d.forward (common_modules.py:231-244) for in_chs == out_chs."""
    if not _is_identity(blk.one_by_one):
        raise NotImplementedError("ResConvBlk3d with a 1x1x1 projection (in_chs != out_chs) is not on the hot path")
    if getattr(blk, "out_pad", 0) != 0:
        raise NotImplementedError("ResConvBlk3d out_pad != 0")
    r = lower_conv_block(blk.blk1).run(x)
    return lower_conv_block(blk.blk2).run(r, res=x)


class ResConvBlk3d(nn.Module):
    def __init__(self, in_chs: int, out_chs: int, kernel_size: int = 3, in_stride: int = 1, out_stride: int = 1,
                 out_pad: int = 0, activation: nn.Module = NoOp(), norm_layer: nn.Module = NoOp()):
        super().__init__()
        self.in_chs, self.out_chs, self.k_sz = in_chs, out_chs, kernel_size
        self.in_stride, self.out_stride, self.out_pad = in_stride, out_stride, out_pad
        self.blk1 = BaseConvBlk3d(in_chs, out_chs, kernel_size, stride=in_stride,
                                  activation=copy.deepcopy(activation), norm_layer=copy.deepcopy(norm_layer))
        self.blk2 = BaseConvBlk3d(out_chs, out_chs, kernel_size, stride=out_stride,
                                  activation=copy.deepcopy(activation), norm_layer=copy.deepcopy(norm_layer))
        if in_chs != out_chs:
            self.one_by_one = BaseConvBlk3d(in_chs, out_chs, 1, stride=out_stride * in_stride,
                                            activation=copy.deepcopy(activation),
                                            norm_layer=copy.deepcopy(norm_layer))
        else:
            self.one_by_one = NoOp()

    def forward(self, x: Tensor) -> Tensor:
        return _to_ncdhw_view(res_block_ndhwc(self, H.as_ndhwc(x)))


def resize_conv_ndhwc(blk, x: Tensor, res: Optional[Tensor] = None) -> Tensor:
    """ResizeConv3d.forward (common_modules.py:332-355): trilinear to int(scale*s)+out_pad,
    optional second resize to the skip's size, then conv(+res)."""
    up = [int(blk.scale * s) + blk.out_pad for s in x.shape[1:4]]
    L = lower_conv_block(blk.conv)
    if up == [2 * s for s in x.shape[1:4]] and (res is None or tuple(res.shape[1:4]) == tuple(up)) and L.can_fuse_up2():
        return L.run_up2(x, res)                  # upsample evaluated inside the conv's staging path
    x = H.resize_trilinear(x, up)
    if res is not None and tuple(x.shape[1:4]) != tuple(res.shape[1:4]):
        x = H.resize_trilinear(x, res.shape[1:4])
    return lower_conv_block(blk.conv).run(x, res)


class ResizeConv3d(nn.Module):
    def __init__(self, in_chs: int, out_chs: int, kernel_size: int, stride: int = 1, extra_pad: int = 0,
                 out_pad: int = 0, activation: nn.Module = NoOp(), norm_layer: nn.Module = NoOp()):
        super().__init__()
        self.scale = stride
        self.out_pad = out_pad
        self.conv = BaseConvBlk3d(in_chs, out_chs, kernel_size, stride=1, extra_pad=extra_pad,
                                  activation=copy.deepcopy(activation), norm_layer=copy.deepcopy(norm_layer))

    def forward(self, x: Tensor, res: Optional[Tensor] = None) -> Tensor:
        r = None if res is None else H.as_ndhwc(res)
        return _to_ncdhw_view(resize_conv_ndhwc(self, H.as_ndhwc(x), r))
