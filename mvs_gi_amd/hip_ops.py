"""Tensor-level wrappers over the C ABI: argument checking, output allocation (PyTorch is
only the device allocator and stream provider here) and the call through ctypes.

All activations are channels-last fp32 ("NDHWC": [B, D, H, W, C]) unless stated.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

import ctypes
import math
import os

CONV_AUTO, CONV_DIRECT, CONV_MFMA, CONV_BF16X3, CONV_BF16X3_C16, CONV_BF16X3_V32, CONV_BF16X3_D32 = 0, 1, 2, 3, 4, 5, 6
SPLIT_F16 = 1          # `fmt` of the *_fmt entry points (include/mvsgi.h MVSGI_SPLIT_F16): split-padded data / weights hold fp16 pairs
CONV_F16 = 0x100       # flag OR-ed into CONV_BF16X3 / _C16 / _V32: the same kernel in the fp16 split (include/mvsgi.h MVSGI_CONV_F16)

# Arithmetic of the conv layers:
#   "f16x3" (default) = split-fp16 MFMA (x = hi + lo, hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16, fp32 accumulate; 11 + 11
#                       significant bits per operand; operands saturate at +-65504 (never inf / nan); weights pre-scaled per output
#                       channel by a power of two).  Inverse distance ~8x closer to the reference than the bf16 split, and since the
#                       level-0 residual convs of the (16, 32) regulator run in Winograd form in this split (csrc/conv3d_wino.hip; exact
#                       for |activation| <= 16376) also the fastest mode;
#   "bf16x3"          = the same three products in the bf16 split (8 + 8 bits per operand, fp32's range): the answer for activations
#                       beyond fp16's range (HotPath.precision_check tells the two apart);
#   "f32"             = exact fp32 MFMA (v_mfma_f32_16x16x4_f32; bit-for-bit an fp32 fmaf chain, ~4x slower).
CONV_MODES = ("f32", "bf16x3", "f16x3")
_CONV_MODE = os.environ.get("MVSGI_CONV_MODE", "f16x3")
if _CONV_MODE not in CONV_MODES:
    raise ValueError(f"MVSGI_CONV_MODE={_CONV_MODE!r} not in {CONV_MODES}")


# The environment the package reads: MVSGI_CONV_MODE, MVSGI_RANGE_CHECK (below), MVSGI_RIG_CACHE, MVSGI_POLY, MVSGI_S2RS,
# MVSGI_HEAD_SPLIT, MVSGI_FRONT_CHUNK (each covered by tests/test_gpu_parity.py::test_product_switches_off), MVSGI_WINO
# (test_full_size_winograd_level0_vs_direct_kernel_and_reference_golden), MVSGI_D32 and MVSGI_LIB.


def set_conv_mode(mode: str) -> None:
    global _CONV_MODE
    if mode not in CONV_MODES:
        raise ValueError(f"conv mode {mode!r} not in {CONV_MODES}")
    _CONV_MODE = mode


def get_conv_mode() -> str:
    return _CONV_MODE


# ---- range report of the fp16 split (include/mvsgi.h: mvsgi_saturation_flags) ----
# The reference computes in fp32 with no clamp (common_modules.py:105-115); the default arithmetic saturates what it writes or stages
# in fp16 pieces.  Every kernel that clamps raises a sticky flag when a clamp ENGAGED; the wrappers below read it -- a load from
# pinned host memory, no stream operation -- and turn it into an exception (MVSGI_RANGE_CHECK=raise, the default), a warning (=warn,
# once per kind) or nothing (=off).  A flag says something about launches that have COMPLETED: the path's calls are asynchronous, so
# the entry checks of HotPath / the drop-in modules report the frames before the current one; HotPath.check_range() and
# InferencePipeline (which synchronise) report the frame itself.
SAT_SWEEP, SAT_SPLIT, SAT_WINO = 1, 2, 4
_SAT_TEXT = {SAT_SWEEP: "the sweep's cost volume reached +-65504 (un-normalised features?)",
             SAT_SPLIT: "an activation written or staged in fp16 pieces reached +-65504",
             SAT_WINO: "an activation of the Winograd-form level reached its +-16376 range (or a transformed sum +-65504)"}
RANGE_CHECKS = ("raise", "warn", "off")
_RANGE_CHECK = os.environ.get("MVSGI_RANGE_CHECK", "raise")
if _RANGE_CHECK not in RANGE_CHECKS:
    raise ValueError(f"MVSGI_RANGE_CHECK={_RANGE_CHECK!r} not in {RANGE_CHECKS}")
_RANGE_WARNED = set()
_RANGE_SEEN = 0             # OR of every flag check_range() has reported (and cleared) in this process


class MvsgiRangeError(RuntimeError):
    """The fp16 split left its range: results since the last check are saturated, not the reference's."""


def set_range_check(policy: str) -> None:
    global _RANGE_CHECK
    if policy not in RANGE_CHECKS:
        raise ValueError(f"range check policy {policy!r} not in {RANGE_CHECKS}")
    _RANGE_CHECK = policy


def get_range_check() -> str:
    return _RANGE_CHECK


def saturation_flags(clear: bool = False) -> int:
    """OR of the SAT_* bits raised by completed launches since the last clear (sticky; no synchronisation)."""
    import ctypes
    out = ctypes.c_uint(0)
    if _lib.load().mvsgi_saturation_flags(1 if clear else 0, ctypes.byref(out)) != 0:
        # the pinned words could not be allocated (no usable device): then no kernel has run either -- every launcher of a kernel
        # that can clamp refuses to launch without them -- and there is nothing to report
        return 0
    return int(out.value)


def saturation_words():
    """The raw report words (diagnostics): a kernel only ever stores 1 into the word of its kind."""
    import ctypes
    out = (ctypes.c_uint * 8)()
    if _lib.load().mvsgi_saturation_words(out) != 0:
        return [0] * 8
    return [int(v) for v in out]


def range_flags_seen() -> int:
    """OR of the flags check_range() has reported so far in this process (it clears the library's sticky words when it reports)."""
    return _RANGE_SEEN


def check_range(where: str = "", sync_device=None) -> int:
    """Apply the MVSGI_RANGE_CHECK policy to the flags raised so far (after synchronising `sync_device`, if given) and clear them.
    -> the flags that were raised."""
    if _RANGE_CHECK == "off":
        return 0
    if sync_device is not None:
        torch.cuda.synchronize(sync_device)
    f = saturation_flags(clear=False)
    if not f:
        return 0
    words = saturation_words()
    saturation_flags(clear=True)
    global _RANGE_SEEN
    _RANGE_SEEN |= f
    what = "; ".join(t for b, t in _SAT_TEXT.items() if f & b)
    msg = (f"mvs_gi_amd{' (' + where + ')' if where else ''}: the fp16 split (MVSGI_CONV_MODE=f16x3, the default) left its range (flags 0x{f:x}, words {words[:4]}) -- {what}. "
           "Results computed since the last check are saturated, not the reference's fp32 results "
           "(dsta_mvs/model/common/common_modules.py:105-115 has no clamp). Re-run with MVSGI_CONV_MODE=bf16x3 "
           "(hip_ops.set_conv_mode('bf16x3'): fp32's range, ~8x the rounding error) or 'f32'; HotPath.precision_check(frames) measures "
           "which arithmetic a checkpoint needs. MVSGI_RANGE_CHECK=warn|off relaxes this check.")
    if _RANGE_CHECK == "raise":
        raise MvsgiRangeError(msg)
    if f not in _RANGE_WARNED:
        _RANGE_WARNED.add(f)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=2)
    return f


def split_mode() -> bool:
    """The library's mode is one of the two 16-bit splits (the streaming split kernels serve the layer)."""
    return _CONV_MODE in ("bf16x3", "f16x3")


def mode_fmt() -> str:
    """Element type of the (hi | lo) pieces the library's mode writes into split-padded buffers."""
    return "f16" if _CONV_MODE == "f16x3" else "bf16"


def _fmt_code(fmt: str) -> int:
    if fmt not in ("bf16", "f16"):
        raise ValueError(f"split format {fmt!r} not in ('bf16', 'f16')")
    return SPLIT_F16 if fmt == "f16" else 0


def _pow2_unscale(amax: torch.Tensor):
    """k per entry such that amax * 2^k lies in (512, 1024] (0 for a zero entry) -> (2^k, 2^-k) as fp32 tensors."""
    k = torch.where(amax > 0, torch.floor(torch.log2(1024.0 / amax.clamp_min(1e-37))), torch.zeros_like(amax)).clamp(-100.0, 100.0)
    return torch.exp2(k), torch.exp2(-k)


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: mvs_gi_amd runs on the GPU only (tensor is on {t.device}); "
                           "there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _arg(t, name: str, device, dtype=torch.float32, shape=None, numel=None, nbytes=None) -> torch.Tensor:
    """A parameter or a caller-owned buffer -- scale, shift, weights in any layout, plans, `out`, `res`, the storage of a split-padded
    activation -- checked and handed on AS IT IS: a tensor on `device` (the activation's) of `dtype` (one, or a tuple to choose
    from), contiguous, 16-byte aligned, of the expected shape / element count / byte count (whichever the caller knows).  The
    message names the argument.  Never copies: the hot path does not allocate, and an address a captured graph holds stays the
    tensor's.  Attribute reads only: no synchronisation, no device query."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: mvs_gi_amd runs on the GPU only (tensor is on {t.device}); there is no CPU fallback")
    if device is not None and t.device != device and not (device.index is None and device.type == "cuda"):
        raise AssertionError(f"{name}: on {t.device}, the activation is on {device}")
    if t.dtype != dtype and (type(dtype) is not tuple or t.dtype not in dtype):
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise AssertionError(f"{name}: expected shape {list(shape)}, got {list(t.shape)}")
    if numel is not None and t.numel() != numel:
        raise AssertionError(f"{name}: expected {numel} elements, got {t.numel()} ({list(t.shape)})")
    if nbytes is not None and t.numel() * t.element_size() != nbytes:
        raise AssertionError(f"{name}: wrong size: expected {nbytes} bytes, got {t.numel() * t.element_size()} ({t.dtype} {list(t.shape)})")
    if not t.is_contiguous():
        raise AssertionError(f"{name}: must be contiguous (strides {t.stride()} of {list(t.shape)}); it is read in place, never copied")
    if t.data_ptr() % 16:
        raise AssertionError(f"{name}: must be 16-byte aligned (a view at an odd offset?); it is read in place, never copied")
    return t


def _opt(t, name: str, device, dtype=torch.float32, **kw) -> Optional[int]:
    """_arg of an argument that may be None -> its address or None."""
    return None if t is None else _arg(t, name, device, dtype, **kw).data_ptr()


def _scale_shift(scale, shift, device, cout=None, suffix: str = ""):
    """The epilogue's per-channel constants: fp32 [Cout] each -> (their addresses, Cout)."""
    scale = _arg(scale, "scale" + suffix, device, numel=cout)
    cout = scale.numel()
    return scale.data_ptr(), _arg(shift, "shift" + suffix, device, numel=cout).data_ptr(), cout


_PACKED = (torch.uint8, torch.float32)        # a packed weight whose layout the call does not tell: bytes or floats


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _call(name: str, *args) -> None:
    """One launch through the C ABI: lib.<name>(*args); a failure raises with the name of the symbol that failed."""
    _lib.check(getattr(_lib.load(), name)(*args), name)


# --------------------------------------------------------------------------------------
def _feats_nhwc(feats):
    """[B, N, C, Hi, Wi] -> channels-last storage [B, N, Hi, Wi, C] (no copy if it already is)."""
    if feats.dim() != 5:
        raise AssertionError(f"feats must be [B, N, C, Hi, Wi], got {tuple(feats.shape)}")
    v = feats.permute(0, 1, 3, 4, 2)
    if v.is_contiguous() and v.data_ptr() % 16 == 0 and v.is_cuda and v.dtype == torch.float32:
        return v
    f = _dev(feats, "feats")
    B, N, C, Hi, Wi = f.shape
    y = torch.empty((B, N, Hi, Wi, C), device=f.device, dtype=torch.float32)
    _call("mvsgi_ncv_to_nvc_f32", f.data_ptr(), y.data_ptr(), B * N, C, Hi * Wi, _stream_ptr(f))
    return y


def nhwc_sweep_ok(feats) -> bool:
    """The channels-last kernel that samples the masks itself (mvsgi_sweep_std_nhwc_f32) takes these feats: C % 4 == 0, N <= 4."""
    return feats.dim() == 5 and feats.shape[2] % 4 == 0 and feats.shape[1] <= 4


def sweep_max_cams() -> int:
    """Cameras the masked-variance sweep takes (one validity bit per camera in a byte); the library's own bound."""
    return int(_lib.load().mvsgi_sweep_max_cams())


def valid_sweep_ok(feats) -> bool:
    """The kernels that read the rig's validity byte (sweep_std_valid, sweep_std_valid_split) take these feats:
    C % 4 == 0 and N <= sweep_max_cams()."""
    return feats.dim() == 5 and feats.shape[2] % 4 == 0 and 1 <= feats.shape[1] <= sweep_max_cams()


def _rig_args(grids, grid_masks, masks, B: int, N: int):
    """The rig tensors of a masked sweep, checked against B frames of N cameras -> (grids, grid_masks, gm_f32, masks, sizes):
    gm_f32 = 1 when the grid masks are fp32 (any dtype but bool / uint8 is converted), 0 for one byte per sample;
    sizes = (D, Ho, Wo, Hm, Wm)."""
    grids = _dev(grids, "grids")
    masks = _dev(masks, "masks")
    if grid_masks.dtype in (torch.bool, torch.uint8):
        gm, gm_f32 = _dev(grid_masks, "grid_masks", grid_masks.dtype), 0
    else:
        gm, gm_f32 = _dev(grid_masks.to(torch.float32) if grid_masks.dtype != torch.float32 else grid_masks, "grid_masks"), 1
    Bg, Ng, D, Ho, Wo, two = grids.shape
    if (Bg, Ng, two) != (B, N, 2):
        raise AssertionError(f"grids {tuple(grids.shape)} must be [{B}, {N}, D, Ho, Wo, 2]")
    if tuple(gm.shape[:5]) != (B, N, D, Ho, Wo) or gm.numel() != B * N * D * Ho * Wo:
        raise AssertionError(f"grid_masks {tuple(gm.shape)} do not match grids {tuple(grids.shape)}")
    if masks.shape[0] != B or masks.shape[1] != N or masks.numel() != B * N * masks.shape[-2] * masks.shape[-1]:
        raise AssertionError(f"masks {tuple(masks.shape)} do not match grids {tuple(grids.shape)}")
    return grids, gm, gm_f32, masks, (D, Ho, Wo) + tuple(masks.shape[-2:])


def sweep_validity(grids, grid_masks, masks) -> torch.Tensor:
    """Rig-constant validity byte per voxel, [B, D, Ho, Wo] uint8 (bit cam = camera cam valid):
    (bilinear_grid_sample(masks) > 0) & grid_masks of spherical_sweep_avg.py:92-102."""
    B, N = grids.shape[:2]
    if N > sweep_max_cams():
        raise AssertionError(f"grids must be [B, N<={sweep_max_cams()}, D, Ho, Wo, 2], got {tuple(grids.shape)}")
    grids, gm, gm_f32, masks, (D, Ho, Wo, Hm, Wm) = _rig_args(grids, grid_masks, masks, B, N)
    vmask = torch.empty((B, D, Ho, Wo), device=grids.device, dtype=torch.uint8)
    _call("mvsgi_sweep_validity_u8", grids.data_ptr(), gm.data_ptr(), gm_f32, masks.data_ptr(), vmask.data_ptr(),
          B, N, Hm, Wm, D, Ho, Wo, _stream_ptr(grids))
    return vmask


def sweep_std_valid(feats, grids, vmask) -> torch.Tensor:
    """sweep_std with the cached validity byte (channels-last kernel only) -> vol_raw [B, D, Ho, Wo, C].
    grids / vmask with batch 1 against feats with batch B > 1 = one rig shared by the whole batch."""
    if not valid_sweep_ok(feats):
        raise AssertionError(f"sweep_std_valid needs C % 4 == 0 and num_cams in [1, {sweep_max_cams()}], got feats {tuple(feats.shape)}")
    B, N, C, Hi, Wi = feats.shape
    f = _feats_nhwc(feats)
    grids = _dev(grids, "grids")
    vmask = _dev(vmask, "vmask", torch.uint8)
    Bg, Ng, D, Ho, Wo, two = grids.shape
    if (Ng, two) != (N, 2) or Bg not in (1, B):
        raise AssertionError(f"grids {tuple(grids.shape)} do not match feats {tuple(feats.shape)}")
    if tuple(vmask.shape) != (Bg, D, Ho, Wo):
        raise AssertionError(f"vmask {tuple(vmask.shape)} does not match grids {tuple(grids.shape)}")
    vol = torch.empty((B, D, Ho, Wo, C), device=f.device, dtype=torch.float32)
    _call("mvsgi_sweep_std_nhwc_valid_rig_f32" if (Bg == 1 and B > 1) else "mvsgi_sweep_std_nhwc_valid_f32",
          f.data_ptr(), grids.data_ptr(), vmask.data_ptr(), vol.data_ptr(), B, N, C, Hi, Wi, D, Ho, Wo, _stream_ptr(f))
    return vol


def sweep_std_valid_split(feats, grids, vmask, out: "SplitAct", fmt: str = "bf16") -> "SplitAct":
    """sweep_std_valid with vol_raw written split-padded (C == 16) into `out` (B, D, Ho, Wo, 16), its pieces in the split `fmt`."""
    if not valid_sweep_ok(feats):
        raise AssertionError(f"sweep_std_valid_split needs C == 16 and num_cams in [1, {sweep_max_cams()}], got feats {tuple(feats.shape)}")
    B, N, C, Hi, Wi = feats.shape
    grids = _dev(grids, "grids")
    vmask = _dev(vmask, "vmask", torch.uint8)
    Bg, Ng, D, Ho, Wo, two = grids.shape
    if (Ng, two) != (N, 2) or Bg not in (1, B) or tuple(vmask.shape) != (Bg, D, Ho, Wo) or C != 16:
        raise AssertionError(f"grids {tuple(grids.shape)} / vmask {tuple(vmask.shape)} do not match feats {tuple(feats.shape)}")
    yp = _split_ptr(out, "out", grids.device, (B, D, Ho, Wo, C))       # before the transpose of NCHW feats launches
    f = _feats_nhwc(feats)
    _call("mvsgi_sweep_std_nhwc_valid_split_fmt", f.data_ptr(), grids.data_ptr(), vmask.data_ptr(), yp, B, N, C, Hi, Wi, D, Ho, Wo,
          Bg, _fmt_code(fmt), _stream_ptr(f))
    out.fmt = fmt
    return out


def sweep_std(feats, grids, grid_masks, masks, layout: str = "auto") -> torch.Tensor:
    """-> vol_raw [B, D, Ho, Wo, C] (masked variance over cameras).  layout: 'auto' uses the
    channels-last kernel when C % 4 == 0 and N <= 4 (transposing NCHW feats once) and, for rigs of 5 to
    sweep_max_cams() cameras with C % 4 == 0, the validity byte and the kernel that reads it (same bits); 'nchw'
    forces the plane-gather kernel."""
    if feats.dim() != 5:
        raise AssertionError(f"feats must be [B, N, C, Hi, Wi], got {tuple(feats.shape)}")
    if not 1 <= feats.shape[1] <= sweep_max_cams():
        raise AssertionError(f"sweep_std: num_cams {feats.shape[1]} not in [1, {sweep_max_cams()}]")
    nhwc = layout == "auto" and nhwc_sweep_ok(feats)
    if layout == "auto" and not nhwc and valid_sweep_ok(feats):
        if tuple(grids.shape[:2]) != tuple(feats.shape[:2]):
            raise AssertionError(f"grids {tuple(grids.shape)} must be [{feats.shape[0]}, {feats.shape[1]}, D, Ho, Wo, 2]")
        return sweep_std_valid(feats, grids, sweep_validity(grids, grid_masks, masks))
    B, N, C, Hi, Wi = feats.shape
    f = _feats_nhwc(feats) if nhwc else _dev(feats, "feats")
    grids, gm, gm_f32, masks, (D, Ho, Wo, Hm, Wm) = _rig_args(grids, grid_masks, masks, B, N)
    vol = torch.empty((B, D, Ho, Wo, C), device=f.device, dtype=torch.float32)
    _call("mvsgi_sweep_std_nhwc_f32" if nhwc else "mvsgi_sweep_std_f32", f.data_ptr(), grids.data_ptr(), gm.data_ptr(), gm_f32,
          masks.data_ptr(), vol.data_ptr(), B, N, C, Hi, Wi, Hm, Wm, D, Ho, Wo, _stream_ptr(f))
    return vol


def sweep_cat(feats, grids, layout: str = "auto") -> torch.Tensor:
    """-> vol_raw [B, D, Ho, Wo, N*C] (channel = cam*C + c)."""
    nhwc = layout == "auto" and feats.dim() == 5 and feats.shape[2] % 4 == 0
    f = _feats_nhwc(feats) if nhwc else _dev(feats, "feats")
    B, N, C, Hi, Wi = feats.shape
    grids = _dev(grids, "grids")
    Bg, Ng, D, Ho, Wo, two = grids.shape
    if (Bg, Ng, two) != (B, N, 2):
        raise AssertionError(f"grids {tuple(grids.shape)} do not match feats {tuple(feats.shape)}")
    vol = torch.empty((B, D, Ho, Wo, N * C), device=f.device, dtype=torch.float32)
    _call("mvsgi_sweep_cat_nhwc_f32" if nhwc else "mvsgi_sweep_cat_f32", f.data_ptr(), grids.data_ptr(), vol.data_ptr(), B, N, C, Hi, Wi,
          D, Ho, Wo, _stream_ptr(f))
    return vol


def pack_conv_weights(w_oidhw: torch.Tensor) -> Optional[torch.Tensor]:
    """[Cout, Cin, 3, 3, 3] -> MFMA lane-ordered layout, or None when the channel counts
    are not multiples of 16 (the direct kernel then reads w_oidhw itself)."""
    lib = _lib.load()
    w = _dev(w_oidhw, "conv weight")
    Cout, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3, 3):
        raise NotImplementedError(f"only 3x3x3 kernels are supported, got {tuple(w.shape[2:])}")
    if Cin % 16 or not (Cout % 16 == 0 or Cout == 1):
        return None
    wp = torch.empty(lib.mvsgi_conv3d_packed_weight_floats(Cout, Cin), device=w.device, dtype=torch.float32)
    _call("mvsgi_conv3d_pack_weights_f32", w.data_ptr(), wp.data_ptr(), Cout, Cin, _stream_ptr(w))
    return wp


def _pack_conv3d_split(w_oidhw: torch.Tensor, layout: int, fmt: str = "bf16"):
    """[Cout, Cin, 3, 3, 3] -> (weights of the streaming split kernel in `layout` (CONV_BF16X3 | _C16 | _V32 | _D32) and the split
    `fmt`, unscale [Cout] | None), or None when the layout does not take these channel counts.  fmt = 'f16': every output channel's
    weights are pre-scaled by a power of two so that its largest weight lies in (512, 1024] -- the lo parts (2^-11 of the weight)
    are then normal fp16 numbers instead of subnormals with an absolute quantum of 2^-24; `unscale` = 2^-k per channel goes into
    the epilogue's per-channel scale (exact: powers of two).  The bf16 split has fp32's range: no scaling, unscale None."""
    lib = _lib.load()
    w = _dev(w_oidhw, "conv weight")
    Cout, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3, 3) or Cin % 16 or Cout % 16 or (layout == CONV_BF16X3_C16 and Cout != 16) or \
            (layout == CONV_BF16X3_V32 and Cout % 32) or (layout == CONV_BF16X3_D32 and Cin % 32):
        return None
    unscale = None
    if fmt == "f16":
        up, unscale = _pow2_unscale(w.abs().amax(dim=(1, 2, 3, 4)))
        w = (w * up.view(-1, 1, 1, 1, 1)).contiguous()
    n = {CONV_BF16X3: lambda: lib.mvsgi_conv3d_packed_weight_bytes_bf16x3(Cout, Cin),
         CONV_BF16X3_C16: lambda: lib.mvsgi_conv3d_packed_weight_bytes_bf16x3_c16(Cin),
         CONV_BF16X3_D32: lambda: lib.mvsgi_conv3d_packed_weight_bytes_bf16x3(Cout, Cin),
         CONV_BF16X3_V32: lambda: lib.mvsgi_conv3d_packed_weight_bytes_bf16x3_v32(Cout, Cin)}[layout]()
    wp = torch.empty(n, device=w.device, dtype=torch.uint8)
    _call("mvsgi_conv3d_pack_weights_split", w.data_ptr(), wp.data_ptr(), Cout, Cin, layout | (CONV_F16 if _fmt_code(fmt) else 0),
          _stream_ptr(w))
    return wp, (None if unscale is None else unscale.contiguous())


# The public packers: (bf16) -> packed weights | None; (fp16) -> (packed weights, unscale [Cout]) | None.  The library's per-layout
# bf16 entry points (mvsgi_conv3d_pack_weights_bf16x3 / _c16 / _v32) launch the same kernels with the same arguments as
# mvsgi_conv3d_pack_weights_split (csrc/conv3d.hip); tests/test_gpu_pack_split.py compares the bytes.
def _pack_bf16(w_oidhw: torch.Tensor, layout: int) -> Optional[torch.Tensor]:
    p = _pack_conv3d_split(w_oidhw, layout)
    return None if p is None else p[0]


def pack_conv_weights_bf16x3(w_oidhw: torch.Tensor) -> Optional[torch.Tensor]:
    """[Cout, Cin, 3, 3, 3] -> split-bf16 (hi | lo) MFMA layout, or None when unsupported."""
    return _pack_bf16(w_oidhw, CONV_BF16X3)


def pack_conv_weights_f16x3(w_oidhw: torch.Tensor, layout: int = CONV_BF16X3):
    """-> (packed weights of the fp16 split in `layout`, unscale [Cout]) or None (_pack_conv3d_split)."""
    return _pack_conv3d_split(w_oidhw, layout, "f16")


def pack_conv_weights_bf16x3_d32(w_oidhw: torch.Tensor) -> Optional[torch.Tensor]:
    """-> the bf16 split's weights in the 32-channel-slice layout (CONV_BF16X3_D32), or None (Cin % 32, Cout % 16)."""
    return _pack_bf16(w_oidhw, CONV_BF16X3_D32)


def pack_conv_weights_bf16x3_v32(w_oidhw: torch.Tensor) -> Optional[torch.Tensor]:
    """[Cout % 32 == 0, Cin % 16 == 0, 3, 3, 3] -> 32x32x16-MFMA split-bf16 layout, or None when unsupported."""
    return _pack_bf16(w_oidhw, CONV_BF16X3_V32)


def pack_conv_weights_bf16x3_c16(w_oidhw: torch.Tensor) -> Optional[torch.Tensor]:
    """[16, Cin, 3, 3, 3] -> plane-schedule split-bf16 layout (impl CONV_BF16X3_C16), or None when unsupported."""
    return _pack_bf16(w_oidhw, CONV_BF16X3_C16)


def conv3d_d32_applies(B, Cin, Din, Hin, Win, Cout, stride=1) -> bool:
    """Whether the split kernel on 32-channel slices (impl CONV_BF16X3_D32: 27 k-steps per 32 channels instead of 28, half the
    slices per unit) serves this problem: Cin % 32 == 0, stride 1, a launch large enough for its 128- / 160-voxel bricks."""
    return bool(_lib.load().mvsgi_conv3d_d32_applies(B, Cin, Din, Hin, Win, Cout, stride))


def conv3d_up2_d32_applies(B, Cin, Dl, Hl, Wl, Cout) -> bool:
    """... and the fused upsample + conv (conv3d_up2 with w_layout CONV_BF16X3_D32; low-resolution sizes)."""
    return bool(_lib.load().mvsgi_conv3d_up2_d32_applies(B, Cin, Dl, Hl, Wl, Cout))


def conv3d_v32_applies(B, Cin, Din, Hin, Win, Cout, stride=1) -> bool:
    """Whether the 32x32x16-MFMA kernel (impl / w_layout CONV_BF16X3_V32) serves this problem
    (for conv3d_up2 pass the upsampled input size)."""
    return bool(_lib.load().mvsgi_conv3d_v32_applies(B, Cin, Din, Hin, Win, Cout, stride))


def _split_layout_bytes(layout: int, Cout: int, Cin: int) -> int:
    """Size of the streaming split kernel's weights in `layout` (CONV_BF16X3 | _C16 | _V32 | _D32, CONV_F16 or not: the two splits
    share the layouts), by the library's own queries."""
    lib = _lib.load()
    layout &= ~CONV_F16
    if layout == CONV_BF16X3_C16:
        return lib.mvsgi_conv3d_packed_weight_bytes_bf16x3_c16(Cin)
    if layout == CONV_BF16X3_V32:
        return lib.mvsgi_conv3d_packed_weight_bytes_bf16x3_v32(Cout, Cin)
    if layout in (CONV_BF16X3, CONV_BF16X3_D32):
        return lib.mvsgi_conv3d_packed_weight_bytes_bf16x3(Cout, Cin)
    raise ValueError(f"w_layout {layout} is not one of the streaming split kernel's layouts")


def _conv3d_packed(w_packed, name: str, device, impl: int, Cout: int, Cin: int) -> Optional[int]:
    """w_packed of conv3d, checked against the layout `impl` names -> its address or None.  A split layout (CONV_BF16X3 on channel
    counts the split kernel takes, _C16, _V32, _D32): bytes, sized by the library's query.  CONV_MFMA, CONV_AUTO (which resolves to
    the exact-fp32 tiled kernels or the direct one) and CONV_BF16X3 on channel counts that fall back to them: the fp32 layout of
    pack_conv_weights, sized where that packer serves the channel counts.  CONV_DIRECT never reads it: form only."""
    base = impl & ~CONV_F16
    split = base in (CONV_BF16X3_C16, CONV_BF16X3_V32, CONV_BF16X3_D32) or (base == CONV_BF16X3 and Cin % 16 == 0 and Cout % 16 == 0)
    if w_packed is None:
        if split:
            raise AssertionError(f"{name}: impl {impl} needs the packed weights of its layout")
        return None
    if split:
        return _arg(w_packed, name, device, torch.uint8, nbytes=_split_layout_bytes(base, Cout, Cin)).data_ptr()
    if base == CONV_DIRECT:
        return _arg(w_packed, name, device, _PACKED).data_ptr()
    packs = Cin % 16 == 0 and (Cout % 16 == 0 or Cout == 1)
    return _arg(w_packed, name, device, numel=_lib.load().mvsgi_conv3d_packed_weight_floats(Cout, Cin) if packs else None).data_ptr()


def conv3d(x, w_oidhw, w_packed, scale, shift, res=None, stride=1, neg_slope=0.01, impl=CONV_AUTO, out=None):
    """x [B, D, H, W, Cin] -> y [B, Do, Ho, Wo, Cout] = act(conv(x) * scale + shift (+ res));
    act(v) = v if v > 0 else v * neg_slope (1.0 = no activation)."""
    x = _dev(x, "x")
    B, Din, Hin, Win, Cin = x.shape
    dev = x.device
    sc, sh, Cout = _scale_shift(scale, shift, dev)
    Do, Ho, Wo = (Din - 1) // stride + 1, (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    shp = (B, Do, Ho, Wo, Cout)
    y = torch.empty(shp, device=dev, dtype=torch.float32) if out is None else _arg(out, "out", dev, shape=shp)
    _call("mvsgi_conv3d_f32", x.data_ptr(), _opt(w_oidhw, "w_oidhw", dev, shape=(Cout, Cin, 3, 3, 3)),
          _conv3d_packed(w_packed, "w_packed", dev, impl, Cout, Cin), sc, sh, _opt(res, "res", dev, shape=shp), y.data_ptr(), B, Cin, Din,
          Hin, Win, Cout, stride, float(neg_slope), impl, _stream_ptr(x))
    return y


def conv3d_up2(x, w_packed_b3, scale, shift, res=None, neg_slope=0.01, out=None, w_layout=CONV_BF16X3):
    """Fused trilinear x2 upsample + conv3d (split-bf16): x [B, Dl, Hl, Wl, Cin] -> y [B, 2Dl, 2Hl, 2Wl, Cout].
    w_layout: CONV_BF16X3 (pack_conv_weights_bf16x3) or CONV_BF16X3_C16 (pack_conv_weights_bf16x3_c16, Cout == 16)."""
    x = _dev(x, "x")
    B, Dl, Hl, Wl, Cin = x.shape
    dev = x.device
    sc, sh, Cout = _scale_shift(scale, shift, dev)
    shp = (B, 2 * Dl, 2 * Hl, 2 * Wl, Cout)
    wp = _arg(w_packed_b3, "w_packed_b3", dev, torch.uint8, nbytes=_split_layout_bytes(w_layout, Cout, Cin))
    y = torch.empty(shp, device=dev, dtype=torch.float32) if out is None else _arg(out, "out", dev, shape=shp)
    _call("mvsgi_conv3d_up2_f32", x.data_ptr(), wp.data_ptr(), w_layout, sc, sh, _opt(res, "res", dev, shape=shp), y.data_ptr(), B, Cin, Dl,
          Hl, Wl, Cout, float(neg_slope), _stream_ptr(x))
    return y


def conv3d_up2_out_split(x, w_packed_b3, scale, shift, out: "SplitAct", res=None, neg_slope=0.01, w_layout=CONV_BF16X3) -> "SplitAct":
    """conv3d_up2 with the result written split-padded into `out` (B, 2Dl, 2Hl, 2Wl, Cout)."""
    x = _dev(x, "x")
    B, Dl, Hl, Wl, Cin = x.shape
    dev = x.device
    sc, sh, Cout = _scale_shift(scale, shift, dev)
    shp = (B, 2 * Dl, 2 * Hl, 2 * Wl, Cout)
    yp = _split_ptr(out, "out", dev, shp)
    wp = _arg(w_packed_b3, "w_packed_b3", dev, torch.uint8, nbytes=_split_layout_bytes(w_layout, Cout, Cin))
    _call("mvsgi_conv3d_up2_f32_out_split", x.data_ptr(), wp.data_ptr(), w_layout, sc, sh, _opt(res, "res", dev, shape=shp),
          yp, B, Cin, Dl, Hl, Wl, Cout, float(neg_slope), _stream_ptr(x))
    out.fmt = "f16" if w_layout & CONV_F16 else "bf16"
    return out


def conv3d_up2_poly_applies(cin: int, cout: int, neg_slope: float) -> bool:
    """The polyphase ResizeConv3d kernel (csrc/conv3d_up2poly.hip) serves this layer (no skip input)."""
    return cin == 32 and cout == 16 and 0.0 <= neg_slope <= 1.0


def conv3d_up2_poly_plan(w_oidhw: torch.Tensor, D: int, H: int, W: int, fmt: str = "bf16"):
    """Lowering of a [16, 32, 3, 3, 3] ResizeConv3d weight for a low-resolution input of D x H x W voxels: folded phase weights in
    the register-stationary layout, face-correction weights and role tables (built on the host by the library, float64).
    fmt = 'f16': the plan in the fp16 split -> (plan, unscale [16]): the weights are pre-scaled per output channel by a power of two
    (the folded phase weights are linear in them) and `unscale` goes into the layer's scale."""
    lib = _lib.load()
    if tuple(w_oidhw.shape) != (16, 32, 3, 3, 3):
        raise AssertionError(f"polyphase plan needs a [16, 32, 3, 3, 3] weight, got {tuple(w_oidhw.shape)}")
    n = lib.mvsgi_conv3d_up2_poly_plan_bytes(D, H, W)
    if not n:
        raise RuntimeError("mvsgi_conv3d_up2_poly_plan_bytes: bad dims")
    wh = w_oidhw.detach().to("cpu", torch.float32).contiguous()
    unscale = None
    if fmt == "f16":
        up, un = _pow2_unscale(wh.abs().amax(dim=(1, 2, 3, 4)))
        wh = (wh * up.view(-1, 1, 1, 1, 1)).contiguous()
        unscale = un.to(w_oidhw.device)
    plan = torch.empty(n, dtype=torch.uint8)
    _call("mvsgi_conv3d_up2_poly_plan_fmt", wh.data_ptr(), plan.data_ptr(), D, H, W, _fmt_code(fmt))
    plan = plan.to(w_oidhw.device)
    return (plan, unscale) if fmt == "f16" else plan


def _poly_plan_ptr(plan, device, x: "SplitAct") -> int:
    """The polyphase plan for x's (low-resolution) geometry, on the device, sized by the library's query -> its address."""
    return _arg(plan, "plan", device, torch.uint8, nbytes=_lib.load().mvsgi_conv3d_up2_poly_plan_bytes(x.D, x.H, x.W)).data_ptr()


def conv3d_up2_poly(x: "SplitAct", plan: torch.Tensor, scale, shift, neg_slope=0.01, out=None) -> torch.Tensor:
    """act(conv(trilinear_x2(x)) * scale + shift) for Cin = 32, Cout = 16 in polyphase form: x split-padded (low resolution)
    -> fp32 [B, 2D, 2H, 2W, 16]."""
    xp = _split_ptr(x, "x")
    dev = x.buf.device
    if x.C != 32:
        raise AssertionError("conv3d_up2_poly is the 32 -> 16 kernel")
    sc, sh, _ = _scale_shift(scale, shift, dev, 16)
    shp = (x.B, 2 * x.D, 2 * x.H, 2 * x.W, 16)
    y = torch.empty(shp, device=dev, dtype=torch.float32) if out is None else _arg(out, "out", dev, shape=shp)
    _call("mvsgi_conv3d_up2_poly_fmt", xp, _poly_plan_ptr(plan, dev, x), sc, sh, y.data_ptr(), 0, x.B, x.D, x.H, x.W,
          float(neg_slope), _fmt_code(x.fmt), _stream_ptr(x.buf))
    return y


POLY_WINO = os.environ.get("MVSGI_POLY_WINO", "1") != "0"      # 0: the polyphase layer's main kernel stays the direct register-stationary one in the fp16 split too


def conv3d_up2_poly_wino_pays(B: int, D: int, Hh: int, W: int) -> bool:
    """conv3d_up2_poly_split on fp16 pairs of this (low-resolution) geometry and batch runs its main kernel in Winograd form
    (csrc/conv3d_wino_up2.hip): D == 8, H even, W a multiple of 32 and enough units to fill the chip."""
    return POLY_WINO and bool(_lib.load().mvsgi_conv3d_up2_poly_wino_pays(int(B), int(D), int(Hh), int(W)))


def conv3d_up2_poly_split(x: "SplitAct", plan: torch.Tensor, scale, shift, out: "SplitAct", neg_slope=0.01, direct: bool = False,
                          wino: bool = False) -> "SplitAct":
    """conv3d_up2_poly with the result written split-padded into `out` (B, 2D, 2H, 2W, 16).  In the fp16 split the library picks
    the main kernel: the Winograd form where conv3d_up2_poly_wino_pays(), else the direct kernel; `direct` (or MVSGI_POLY_WINO=0)
    keeps the direct kernel, `wino` forces the Winograd form (an error where it does not apply).  `out.rec == "f32"` (set by the
    caller): the Winograd form writes fp32 records for conv3d_head_split instead of pairs -- an error where that form cannot run."""
    xp = _split_ptr(x, "x")
    dev = x.buf.device
    if x.C != 32:
        raise AssertionError(f"conv3d_up2_poly_split: input {x.shape}: the 32 -> 16 kernel")
    yp = _split_ptr(out, "out", dev, (x.B, 2 * x.D, 2 * x.H, 2 * x.W, 16))
    sc, sh, _ = _scale_shift(scale, shift, dev, 16)
    pp = _poly_plan_ptr(plan, dev, x)
    if out.rec == "f32":          # the caller asked for fp32 records (SplitAct.rec): only the Winograd form writes them
        if x.fmt != "f16" or direct or not POLY_WINO:
            raise AssertionError(f"conv3d_up2_poly_split: fp32 records need the fp16 split's Winograd form (input holds {x.fmt} pieces, direct={direct})")
        _call("mvsgi_conv3d_up2_poly_rec32", xp, pp, sc, sh, yp,
              x.B, x.D, x.H, x.W, float(neg_slope), _stream_ptr(x.buf))
        out.fmt = x.fmt
        return out
    _call("mvsgi_conv3d_up2_poly_fmt", xp, pp, sc, sh, yp,
          5 if wino else (3 if (direct or not POLY_WINO) else 1), x.B, x.D, x.H, x.W, float(neg_slope), _fmt_code(x.fmt), _stream_ptr(x.buf))
    out.fmt = x.fmt
    return out


def pack_head_split_weights(w_oidhw: torch.Tensor) -> Optional[torch.Tensor]:
    """[1, Cin % 16 == 0, 3, 3, 3] -> the fragment layout of conv3d_head_split, or None when unsupported."""
    lib = _lib.load()
    w = _dev(w_oidhw, "conv weight")
    if w.shape[0] != 1 or tuple(w.shape[2:]) != (3, 3, 3) or w.shape[1] % 16:
        return None
    wp = torch.empty(lib.mvsgi_conv3d_head_split_packed_weight_bytes(int(w.shape[1])), device=w.device, dtype=torch.uint8)
    _call("mvsgi_conv3d_head_split_pack_weights", w.data_ptr(), wp.data_ptr(), int(w.shape[1]), _stream_ptr(w))
    return wp


def pack_head_split_weights_f16(w_oidhw: torch.Tensor):
    """[1, Cin % 16 == 0, 3, 3, 3] -> (fragment layout of conv3d_head_split in the fp16 split, unscale) or None: the weights
    pre-scaled by a power of two (largest in (512, 1024]), `unscale` its inverse for the head's scale."""
    lib = _lib.load()
    w = _dev(w_oidhw, "conv weight")
    if w.shape[0] != 1 or tuple(w.shape[2:]) != (3, 3, 3) or w.shape[1] % 16:
        return None
    # NOT _pow2_unscale: here 1024 / amax is a double quotient rounded to fp32 afterwards (two roundings, no clamps), there one fp32
    # division of a clamped amax -- not shown to floor to the same k for every amax (either k is exact, but the output bits differ)
    amax = float(w.abs().max())
    k = 0.0 if amax == 0.0 else float(torch.floor(torch.log2(torch.tensor(1024.0 / amax))))
    ws = (w * (2.0 ** k)).contiguous()
    wp = torch.empty(lib.mvsgi_conv3d_head_split_packed_weight_bytes(int(w.shape[1])), device=w.device, dtype=torch.uint8)
    _call("mvsgi_conv3d_head_split_pack_weights_f16", ws.data_ptr(), wp.data_ptr(), int(w.shape[1]), _stream_ptr(w))
    return wp, 2.0 ** -k


def conv3d_head_split(x: "SplitAct", w_packed, scale: float, shift: float, neg_slope=1.0, out=None, f16: bool = False) -> torch.Tensor:
    """Cost head (Cout = 1) on a split-padded input -> fp32 [B, D, H, W, 1] = act(conv(x) * scale + shift).  f16: input and weights
    in the fp16 split; a buffer of fp32 records (x.rec == 'f32') is split by the kernel as it loads."""
    if x.fmt != ("f16" if f16 else "bf16"):
        raise AssertionError(f"conv3d_head_split(f16={f16}) on a split-padded buffer holding {x.fmt} pieces")
    if x.rec == "f32" and not f16:
        raise AssertionError("conv3d_head_split: fp32 records are read in the fp16 split only")
    xp = _split_ptr(x, "x")
    dev = x.buf.device
    shp = (x.B, x.D, x.H, x.W, 1)
    y = torch.empty(shp, device=dev, dtype=torch.float32) if out is None else _arg(out, "out", dev, shape=shp)
    wp = _arg(w_packed, "w_packed", dev, torch.uint8, nbytes=_lib.load().mvsgi_conv3d_head_split_packed_weight_bytes(x.C))
    _call("mvsgi_conv3d_head_rec32_f16" if x.rec == "f32" else ("mvsgi_conv3d_head_split_f16" if f16 else "mvsgi_conv3d_head_split"),
          xp, wp.data_ptr(), float(scale),
          float(shift), y.data_ptr(), x.B, x.C, x.D, x.H, x.W, float(neg_slope), _stream_ptr(x.buf))
    return y


def conv3d_up2_variant(B, Cin, Dl, Hl, Wl, Cout, w_layout=CONV_BF16X3) -> str:
    lib = _lib.load()
    name = lib.mvsgi_conv3d_up2_variant_f32(B, Cin, Dl, Hl, Wl, Cout, w_layout)
    if name is None:
        raise RuntimeError("mvsgi_conv3d_up2_variant_f32: " + lib.mvsgi_last_error().decode())
    return name.decode()


def conv3d_variant(B, Cin, Din, Hin, Win, Cout, stride=1, impl=CONV_AUTO) -> str:
    """Name of the kernel mvsgi_conv3d_f32 will launch for this problem (as rocprofv3 prints it)."""
    lib = _lib.load()
    name = lib.mvsgi_conv3d_variant_f32(B, Cin, Din, Hin, Win, Cout, stride, impl)
    if name is None:
        raise RuntimeError("mvsgi_conv3d_variant_f32: " + lib.mvsgi_last_error().decode())
    return name.decode()


# --------------------------------------------------------------------------------------
# split-padded activations (csrc/conv3d_rs.hip): [B, D+2, H+2, W+2, C] int32 words, each word = (hi | lo) bf16 pieces laid
# out per 16-channel slice as [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15]; zero border
# --------------------------------------------------------------------------------------
class SplitAct:
    """A split-padded activation buffer plus its logical geometry (B, D, H, W, C)."""
    __slots__ = ("buf", "B", "D", "H", "W", "C", "fmt", "rec")

    def __init__(self, B, D, H, W, C, device, buf=None):
        self.B, self.D, self.H, self.W, self.C = int(B), int(D), int(H), int(W), int(C)
        self.fmt = "bf16"          # element type of the (hi | lo) pieces: set by the kernel that writes the buffer, checked by its reader
        # encoding of a voxel's record: "pairs" = (hi | lo) pieces of `fmt`; "f32" = C plain fp32 in the same bytes, the hand-over
        # conv3d_up2_poly_split (Winograd form) -> conv3d_head_split.  Set by the CALLER on the buffer before the writing call (`fmt`
        # keeps naming the split of the arithmetic around it); every other reader and writer takes pairs
        self.rec = "pairs"
        if buf is None:
            buf = torch.zeros((self.B, self.D + 2, self.H + 2, self.W + 2, self.C), device=device, dtype=torch.int32)
        else:         # caller-owned storage (a batch slice buf[:B] / buf[i:j] of a larger buffer qualifies): checked like any other buffer
            _arg(buf, "buf", torch.device(device), torch.int32, shape=(self.B, self.D + 2, self.H + 2, self.W + 2, self.C))
        self.buf = buf

    @property
    def shape(self):
        return (self.B, self.D, self.H, self.W, self.C)

    @property
    def device(self):
        return self.buf.device


def _split_ptr(s, name: str, device=None, shape=None) -> int:
    """A split-padded activation a kernel reads or writes in place: a SplitAct whose storage still is the int32, contiguous, 16-byte
    aligned [B, D + 2, H + 2, W + 2, C] device tensor its geometry says (`buf` is an attribute: it can be replaced after the
    constructor's check), on `device` and of the logical `shape` where given -> the storage's address."""
    if not isinstance(s, SplitAct):
        raise TypeError(f"{name}: expected a SplitAct, got {type(s)}")
    if shape is not None and s.shape != tuple(shape):
        raise AssertionError(f"{name}: split-padded buffer {s.shape} does not match {tuple(shape)}")
    return _arg(s.buf, f"{name}.buf", device, torch.int32, shape=(s.B, s.D + 2, s.H + 2, s.W + 2, s.C)).data_ptr()


def act_to_split(x_ndhwc: torch.Tensor, out: Optional[SplitAct] = None, fmt: str = "bf16") -> SplitAct:
    x = _dev(x_ndhwc, "x")
    B, D, Hh, W, C = x.shape
    y = out if out is not None else SplitAct(B, D, Hh, W, C, x.device)
    _call("mvsgi_act_f32_to_split_fmt", x.data_ptr(), _split_ptr(y, "out", x.device, (B, D, Hh, W, C)), B, C, D, Hh, W, _fmt_code(fmt), _stream_ptr(x))
    y.fmt = fmt
    return y


def act_from_split(x: SplitAct, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if x.rec != "pairs":
        raise AssertionError("act_from_split reads (hi | lo) pairs; this buffer holds fp32 records")
    xp = _split_ptr(x, "x")
    y = torch.empty(x.shape, device=x.buf.device, dtype=torch.float32) if out is None else _arg(out, "out", x.buf.device, shape=x.shape)
    _call("mvsgi_act_split_to_f32_fmt", xp, y.data_ptr(), x.B, x.C, x.D, x.H, x.W, _fmt_code(x.fmt), _stream_ptr(x.buf))
    return y


def pack_conv_weights_rs(w_oidhw: torch.Tensor, fmt: str = "bf16"):
    """[32, 32, 3, 3, 3] or [16, 16, 3, 3, 3] -> register-stationary layout (tap pairs in the kernel's own order), or None.
    fmt = 'f16': -> (packed weights of the fp16 split, unscale [Cout]) with the per-channel power-of-two pre-scaling of
    pack_conv_weights_f16x3."""
    lib = _lib.load()
    w = _dev(w_oidhw, "conv weight")
    unscale = None
    if fmt == "f16":
        up, unscale = _pow2_unscale(w.abs().amax(dim=(1, 2, 3, 4)))
        w = (w * up.view(-1, 1, 1, 1, 1)).contiguous()
    Cout, Cin = w.shape[:2]
    nbytes = lib.mvsgi_conv3d_rs_packed_weight_bytes(Cout, Cin) if tuple(w.shape[2:]) == (3, 3, 3) else 0
    if not nbytes:
        return None
    wp = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    _call("mvsgi_conv3d_rs_pack_weights_fmt", w.data_ptr(), wp.data_ptr(), Cout, Cin, _fmt_code(fmt), _stream_ptr(w))
    return (wp, unscale.contiguous()) if fmt == "f16" else wp


def conv3d_rs(x: SplitAct, w_packed_rs, scale, shift, res: Optional[SplitAct] = None, neg_slope=0.01,
              out=None, out_f32: bool = False):
    """Register-stationary split-bf16 conv (Cin = Cout = 32, stride 1) on split-padded activations.  `out_f32`: the
    result is a plain fp32 [B, D, H, W, 32] tensor instead of a SplitAct (hand-over to an fp32-reading kernel)."""
    xp = _split_ptr(x, "x")
    dev = x.buf.device
    sc, sh, Cout = _scale_shift(scale, shift, dev)
    shp = (x.B, x.D, x.H, x.W, Cout)
    if out_f32:
        y = torch.empty(shp, device=dev, dtype=torch.float32) if out is None else _arg(out, "out", dev, shape=shp)
        yp = y.data_ptr()
    else:
        y = out if out is not None else SplitAct(x.B, x.D, x.H, x.W, Cout, dev)
        yp = _split_ptr(y, "out", dev, shp)
    rp = None if res is None else _split_ptr(res, "res", dev, shp)
    if res is not None and res.fmt != x.fmt:
        raise AssertionError(f"residual {res.shape} ({res.fmt}) does not match the output ({x.fmt})")
    nb = _lib.load().mvsgi_conv3d_rs_packed_weight_bytes(Cout, x.C)
    if not nb:
        raise AssertionError(f"conv3d_rs: no register-stationary kernel for {x.C} -> {Cout} channels")
    _call("mvsgi_conv3d_rs_split_fmt", xp, _arg(w_packed_rs, "w_packed_rs", dev, torch.uint8, nbytes=nb).data_ptr(), sc, sh,
          rp, yp, int(out_f32), x.B, x.C, x.D, x.H, x.W, Cout, float(neg_slope), _fmt_code(x.fmt),
          _stream_ptr(x.buf))
    if not out_f32:
        y.fmt = x.fmt
    return y


def conv3d_wino_applies(cin, cout, D, Hh, W, stride, neg_slope) -> bool:
    """The Winograd-form 32 -> 32 kernel (csrc/conv3d_wino.hip) serves this layer on this geometry (fp16 split only)."""
    return bool(_lib.load().mvsgi_conv3d_wino32_applies(int(cin), int(cout), int(D), int(Hh), int(W), int(stride), float(neg_slope)))


def pack_conv_weights_wino(w_oidhw: torch.Tensor):
    """[32, 32, 3, 3, 3] -> (packed weights of the Winograd F(2x2, 3x3) x direct-D kernel in the fp16 split, unscale [32]), or None.
    U[a, b, kd] = sum_kh,kw G[a, kh] G[b, kw] w[.., kd, kh, kw], pre-scaled per cout by a power of two so that max |U| lies in
    (512, 1024] (the caller folds `unscale` into the epilogue's scale), split hi = fp16(U), lo = fp16(U - hi)."""
    lib = _lib.load()
    w = _dev(w_oidhw, "conv weight")
    if tuple(w.shape) != (32, 32, 3, 3, 3):
        return None
    wp = torch.empty(lib.mvsgi_conv3d_wino32_packed_weight_bytes(), device=w.device, dtype=torch.uint8)
    unscale = torch.empty(32, device=w.device, dtype=torch.float32)
    _call("mvsgi_conv3d_wino32_pack_weights", w.data_ptr(), wp.data_ptr(), unscale.data_ptr(), _stream_ptr(w))
    return wp, unscale


F32P_MAX = 16376.0       # range of fp32-padded activations: a Winograd layer sums four of them in front of its fp16 split (65504 / 4)


def act_to_f32p(x_ndhwc: torch.Tensor, out: Optional[SplitAct] = None) -> SplitAct:
    """fp32 NDHWC -> "fp32-padded": the split-padded geometry with plain fp32 records (tests / tools; torch copies)."""
    x = _dev(x_ndhwc, "x")
    B, D, Hh, W, C = x.shape
    y = out if out is not None else SplitAct(B, D, Hh, W, C, x.device)
    y.buf.view(torch.float32)[:, 1:-1, 1:-1, 1:-1, :] = x.clamp(-F32P_MAX, F32P_MAX)      # the format's range (its writers clamp to it)
    y.fmt = "f32p"
    return y


def act_from_f32p(x: SplitAct) -> torch.Tensor:
    if x.fmt != "f32p":
        raise AssertionError(f"buffer holds {x.fmt} records")
    return x.buf.view(torch.float32)[:, 1:-1, 1:-1, 1:-1, :].contiguous()


def conv3d_wino(x: SplitAct, w_packed, scale, shift, res: Optional[SplitAct] = None, neg_slope=0.01, out=None, out_f32: bool = False,
                ):
    """Winograd-form 32 -> 32 conv (stride 1) on padded activations, arithmetic in the fp16 split; D == 8 or 16, H even, W % 32 == 0.
    x (and res) are split-padded fp16 pairs (fmt 'f16') or fp32-padded ('f32p': plain fp32 records in the same padded geometry --
    the cheaper hand-over between Winograd layers); the output takes x's format.  `out_f32`: the result is a plain fp32
    [B, D, H, W, 32] tensor instead of a SplitAct."""
    lib = _lib.load()
    if x.fmt not in ("f16", "f32p") or x.C != 32:
        raise AssertionError(f"conv3d_wino: needs a 32-channel input in the fp16 split or fp32-padded (got {x.C}, {x.fmt})")
    xp = _split_ptr(x, "x")
    dev = x.buf.device
    if out_f32:
        y = torch.empty(x.shape, device=dev, dtype=torch.float32) if out is None else _arg(out, "out", dev, shape=x.shape)
        yp = y.data_ptr()
    else:
        y = out if out is not None else SplitAct(x.B, x.D, x.H, x.W, 32, dev)
        yp = _split_ptr(y, "out", dev, x.shape)
    rp = None if res is None else _split_ptr(res, "res", dev, x.shape)
    if res is not None and res.fmt != x.fmt:
        raise AssertionError(f"residual {res.shape} ({res.fmt}) does not match the input ({x.fmt})")
    wp = _arg(w_packed, "w_packed", dev, torch.uint8, nbytes=lib.mvsgi_conv3d_wino32_packed_weight_bytes())
    sc, sh, _ = _scale_shift(scale, shift, dev, 32)
    _call("mvsgi_conv3d_wino32_f16", xp, wp.data_ptr(), sc, sh,
          rp, yp, int(out_f32), int(x.fmt == "f32p"), x.B, x.D, x.H, x.W, float(neg_slope),
          _stream_ptr(x.buf))
    if not out_f32:
        y.fmt = x.fmt
    return y


def conv3d_out_split(x, w_packed_b3, scale, shift, out: "SplitAct", res=None, stride=1, neg_slope=0.01, fmt: str = "bf16") -> "SplitAct":
    """mvsgi_conv3d_f32 (streaming split kernel) with the output written split-padded into `out`; fmt = 'f16': weights packed by
    pack_conv_weights_f16x3 (scale carrying the unscale) and the output in the fp16 split."""
    x = _dev(x, "x")
    B, Din, Hin, Win, Cin = x.shape
    dev = x.device
    sc, sh, Cout = _scale_shift(scale, shift, dev)
    Do, Ho, Wo = (Din - 1) // stride + 1, (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    shp = (B, Do, Ho, Wo, Cout)
    yp = _split_ptr(out, "out", dev, shp)
    wp = _arg(w_packed_b3, "w_packed_b3", dev, torch.uint8, nbytes=_split_layout_bytes(CONV_BF16X3, Cout, Cin))
    _call("mvsgi_conv3d_f32_out_split_fmt", x.data_ptr(), wp.data_ptr(), sc, sh, _opt(res, "res", dev, shape=shp), yp,
          B, Cin, Din, Hin, Win, Cout, stride, float(neg_slope), _fmt_code(fmt), _stream_ptr(x))
    out.fmt = fmt
    return out


def conv3d_rs16(x: "SplitAct", w_packed_rs, scale, shift, neg_slope=0.01, out=None, out_split: Optional["SplitAct"] = None):
    """Register-stationary 16 -> 16 conv (post_vol) on a split-padded volume -> fp32 [B, D, H, W, 16], or (out_split) a
    split-padded volume of the same geometry (the hand-over to conv3d_s2rs)."""
    xp = _split_ptr(x, "x")
    dev = x.buf.device
    if x.C != 16:
        raise AssertionError("conv3d_rs16 is the 16 -> 16 kernel")
    sc, sh, _ = _scale_shift(scale, shift, dev, 16)
    wp = _arg(w_packed_rs, "w_packed_rs", dev, torch.uint8, nbytes=_lib.load().mvsgi_conv3d_rs_packed_weight_bytes(16, 16)).data_ptr()
    if out_split is not None:
        if _split_ptr(out_split, "out_split", dev, x.shape) == xp:
            raise AssertionError(f"split output {out_split.shape} must match the input {x.shape} and be another buffer")
        _call("mvsgi_conv3d_rs16_split_fmt", xp, wp, sc, sh, out_split.buf.data_ptr(),
              1, x.B, x.D, x.H, x.W, float(neg_slope), _fmt_code(x.fmt), _stream_ptr(x.buf))
        out_split.fmt = x.fmt
        return out_split
    y = torch.empty(x.shape, device=dev, dtype=torch.float32) if out is None else _arg(out, "out", dev, shape=x.shape)
    _call("mvsgi_conv3d_rs16_split_fmt", xp, wp, sc, sh, y.data_ptr(), 0, x.B, x.D,
          x.H, x.W, float(neg_slope), _fmt_code(x.fmt), _stream_ptr(x.buf))
    return y


def conv3d_s2rs_applies(cin: int, cout: int, stride: int, neg_slope: float) -> bool:
    return cin == 16 and cout == 32 and stride == 2 and 0.0 <= neg_slope <= 1.0


def pack_conv_weights_s2rs(w_oidhw: torch.Tensor, scale: torch.Tensor, fmt: str = "bf16"):
    """[32, 16, 3, 3, 3] weights with the per-channel scale folded in, in the lane order of csrc/conv3d_s2rs.hip.
    fmt = 'f16': -> (packed weights, up, unscale): the kernel's epilogue has no per-channel multiplier, so ONE power of two `up` for
    the layer (the largest |weight * scale| in (512, 1024]) is folded into the packed weights; the caller multiplies `shift` by `up`
    and passes `unscale` = 1 / up to conv3d_s2rs."""
    lib = _lib.load()
    w = _dev(w_oidhw, "w")
    scale = _dev(scale, "scale")
    if tuple(w.shape) != (32, 16, 3, 3, 3) or scale.numel() != 32:
        raise AssertionError(f"conv3d_s2rs is the 16 -> 32 channel stride-2 layer, got weights {tuple(w.shape)}")
    up = un = None
    if fmt == "f16":
        up_t, un_t = _pow2_unscale((w.abs().amax(dim=(1, 2, 3, 4)) * scale.abs()).max().reshape(1))
        up, un = float(up_t[0]), float(un_t[0])
        scale = (scale * up).contiguous()
    wp = torch.empty(lib.mvsgi_conv3d_s2rs_packed_weight_bytes(), device=w.device, dtype=torch.uint8)
    _call("mvsgi_conv3d_s2rs_pack_weights_fmt", w.data_ptr(), scale.data_ptr(), wp.data_ptr(), _fmt_code(fmt), _stream_ptr(w))
    return (wp, up, un) if fmt == "f16" else wp


def conv3d_s2rs(x: "SplitAct", w_packed, shift, out: "SplitAct", neg_slope=0.01, unscale: float = 1.0, out_f32p: bool = False) -> "SplitAct":
    """16 -> 32 channel 3x3x3 stride-2 conv + scale / shift + LeakyReLU, split-padded in and out (LDS-DMA staging).
    `out_f32p` (fp16 split): the output is fp32-padded (plain fp32 records, fmt 'f32p') for a Winograd-form level 0 behind it."""
    Do, Ho, Wo = (x.D - 1) // 2 + 1, (x.H - 1) // 2 + 1, (x.W - 1) // 2 + 1
    xp = _split_ptr(x, "x")
    dev = x.buf.device
    if x.C != 16:
        raise AssertionError(f"conv3d_s2rs: input {x.shape}: the 16 -> 32 kernel")
    yp = _split_ptr(out, "out", dev, (x.B, Do, Ho, Wo, 32))
    wp = _arg(w_packed, "w_packed", dev, torch.uint8, nbytes=_lib.load().mvsgi_conv3d_s2rs_packed_weight_bytes())
    _call("mvsgi_conv3d_s2rs_out_fmt", xp, wp.data_ptr(), _arg(shift, "shift", dev, numel=32).data_ptr(), yp, x.B, x.D, x.H, x.W,
          float(neg_slope), float(unscale), _fmt_code(x.fmt), int(out_f32p), _stream_ptr(x.buf))
    out.fmt = "f32p" if out_f32p else x.fmt
    return out


def conv3d_rs_applies(cin: int, cout: int, stride: int, neg_slope: float) -> bool:
    return cin == 32 and cout == 32 and stride == 1 and 0.0 <= neg_slope <= 1.0


def pack_conv2d_weights_bf16x3(w_oihw: torch.Tensor) -> Optional[torch.Tensor]:
    """[Cout, Cin, 3, 3] -> split-bf16 MFMA layout, or None when unsupported."""
    lib = _lib.load()
    w = _dev(w_oihw, "conv weight")
    Cout, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3) or Cin % 16 or Cout % 16:
        return None
    wp = torch.empty(lib.mvsgi_conv2d_packed_weight_bytes_bf16x3(Cout, Cin), device=w.device, dtype=torch.uint8)
    _call("mvsgi_conv2d_pack_weights_bf16x3", w.data_ptr(), wp.data_ptr(), Cout, Cin, _stream_ptr(w))
    return wp


def pack_conv2d_stem_weights(w_oihw: torch.Tensor) -> Optional[torch.Tensor]:
    """[16, 3, 5, 5] RGB-stem weights -> the matrix-core layout for uint8 images (w / 255 in three bf16 pieces), or None."""
    lib = _lib.load()
    w = _dev(w_oihw, "conv weight")
    if tuple(w.shape) != (16, 3, 5, 5):
        return None
    wp = torch.empty(lib.mvsgi_conv2d_stem_packed_weight_bytes(), device=w.device, dtype=torch.uint8)
    _call("mvsgi_conv2d_stem_pack_weights", w.data_ptr(), wp.data_ptr(), _stream_ptr(w))
    return wp


def pack_conv2d_weights_f32(w_oihw: torch.Tensor) -> Optional[torch.Tensor]:
    """[Cout, Cin, 3, 3] -> exact-fp32 MFMA layout (Cout in {16, 32}), or None when unsupported."""
    lib = _lib.load()
    w = _dev(w_oihw, "conv weight")
    Cout, Cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3) or Cin % 16 or Cout not in (16, 32):
        return None
    wp = torch.empty(lib.mvsgi_conv2d_packed_weight_floats(Cout, Cin), device=w.device, dtype=torch.float32)
    _call("mvsgi_conv2d_pack_weights_f32", w.data_ptr(), wp.data_ptr(), Cout, Cin, _stream_ptr(w))
    return wp


def conv2d(x, w_oihw, w_packed, scale, shift, res=None, stride=1, neg_slope=0.01, impl=CONV_AUTO, in_nchw=False, out_split=None):
    """x [B, H, W, Cin] (or [B, Cin, H, W] with in_nchw) -> y [B, Ho, Wo, Cout] = act(conv(x)*scale + shift (+res)).
    out_split: a zero-bordered 2-D split-padded buffer (split2d_buffer) that receives the output instead (Cout == 16)."""
    layout = int(bool(in_nchw))
    if x.dtype == torch.uint8:                 # camera images [B, H, W, 3]: converted (/255) inside the stem kernel
        x = _dev(x, "imgs", torch.uint8)
        B, Hin, Win, Cin = x.shape
        layout = 2
    else:
        x = _dev(x, "x")
        if in_nchw:
            B, Cin, Hin, Win = x.shape
        else:
            B, Hin, Win, Cin = x.shape
    dev = x.device
    sc, sh, Cout = _scale_shift(scale, shift, dev)
    if not isinstance(w_oihw, torch.Tensor) or w_oihw.dim() != 4:
        raise TypeError(f"w_oihw: expected a [Cout, Cin, k, k] tensor, got {getattr(w_oihw, 'shape', type(w_oihw))}")
    k = int(w_oihw.shape[-1])
    wo = _arg(w_oihw, "w_oihw", dev, shape=(Cout, Cin, k, k)).data_ptr()
    pad = k // 2
    Ho, Wo = (Hin + 2 * pad - k) // stride + 1, (Win + 2 * pad - k) // stride + 1
    wp = None
    if w_packed is not None:
        lib = _lib.load()
        # the layouts conv2d's impl names (include/mvsgi.h, K2-2D); with AUTO / DIRECT on fp32 input nothing reads w_packed: form only
        if impl == CONV_BF16X3 and k == 3 and Cin % 16 == 0 and Cout % 16 == 0:
            wp = _arg(w_packed, "w_packed", dev, torch.uint8, nbytes=lib.mvsgi_conv2d_packed_weight_bytes_bf16x3(Cout, Cin))
        elif impl == CONV_MFMA and k == 3 and Cin % 16 == 0 and Cout in (16, 32):
            wp = _arg(w_packed, "w_packed", dev, numel=lib.mvsgi_conv2d_packed_weight_floats(Cout, Cin))
        elif layout == 2:
            wp = _arg(w_packed, "w_packed", dev, torch.uint8, nbytes=lib.mvsgi_conv2d_stem_packed_weight_bytes())
        else:
            wp = _arg(w_packed, "w_packed", dev, _PACKED)
        wp = wp.data_ptr()
    rp = _opt(res, "res", dev, shape=(B, Ho, Wo, Cout))
    if out_split is not None:
        _check_split2d(out_split, B, Ho, Wo, dev)
        _call("mvsgi_conv2d_f32_out_split2d", x.data_ptr(), wo, wp, sc, sh, rp,
              out_split.data_ptr(), B, Cin, Hin, Win, Cout, k, stride, float(neg_slope), impl, layout, _stream_ptr(x))
        return out_split
    y = torch.empty((B, Ho, Wo, Cout), device=dev, dtype=torch.float32)
    _call("mvsgi_conv2d_f32", x.data_ptr(), wo, wp, sc, sh, rp, y.data_ptr(), B, Cin, Hin,
          Win, Cout, k, stride, float(neg_slope), impl, layout, _stream_ptr(x))
    return y


def conv2d_variant(Cin, Cout, k=3, stride=1, impl=CONV_AUTO, in_nchw=False) -> str:
    lib = _lib.load()
    name = lib.mvsgi_conv2d_variant_f32(Cin, Cout, k, stride, impl, int(bool(in_nchw)))
    if name is None:
        raise RuntimeError("mvsgi_conv2d_variant_f32: " + lib.mvsgi_last_error().decode())
    return name.decode()


def resize_trilinear(x, size) -> torch.Tensor:
    x = _dev(x, "x")
    B, Di, Hi, Wi, C = x.shape
    Do, Ho, Wo = (int(s) for s in size)
    y = torch.empty((B, Do, Ho, Wo, C), device=x.device, dtype=torch.float32)
    _call("mvsgi_resize_trilinear_f32", x.data_ptr(), y.data_ptr(), B, C, Di, Hi, Wi, Do, Ho, Wo, _stream_ptr(x))
    return y


def _images(imgs, m: str, count=None, device=None):
    """The images of resample_bilinear and reproject: uint8 [m, Hr, Wr, 3] or fp32 [m, C, Hr, Wr] on the device (`count` of them,
    on `device`, where given) -> (imgs, u8, C, Hr, Wr); `m` is the leading dimension's name in the messages."""
    if not isinstance(imgs, torch.Tensor) or imgs.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"imgs: expected a uint8 [{m}, Hr, Wr, 3] or fp32 [{m}, C, Hr, Wr] tensor, got {getattr(imgs, 'dtype', type(imgs))}")
    u8 = imgs.dtype == torch.uint8
    imgs = _dev(imgs, "imgs", imgs.dtype)
    if imgs.dim() != 4 or (u8 and imgs.shape[3] != 3) or (count is not None and imgs.shape[0] != count) or \
            (device is not None and imgs.device != device):
        lead = m if count is None else count
        where, got_where = ("", "") if device is None else (f" on {device}", f" on {imgs.device}")
        raise AssertionError(f"imgs must be uint8 [{lead}, Hr, Wr, 3] or fp32 [{lead}, C, Hr, Wr]{where}, got {imgs.dtype} "
                             f"{tuple(imgs.shape)}{got_where}")
    C, Hr, Wr = (imgs.shape[3], imgs.shape[1], imgs.shape[2]) if u8 else tuple(imgs.shape[1:])
    return imgs, u8, C, Hr, Wr


def resample_validity(grid, in_fov) -> torch.Tensor:
    """Validity of a sampling table: in_fov & |gx| <= 1 & |gy| <= 1 (a NaN coordinate is invalid) -> uint8 of in_fov's shape.
    grid [..., 2] fp32 in grid_sample coordinates; in_fov [...] bool or uint8 (the projection's field-of-view mask).  One launch
    on the grid's stream."""
    if not isinstance(grid, torch.Tensor) or grid.dtype != torch.float32:
        raise TypeError(f"grid: expected a fp32 tensor, got {getattr(grid, 'dtype', type(grid))}")
    if not isinstance(in_fov, torch.Tensor) or in_fov.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"in_fov: expected a bool or uint8 tensor, got {getattr(in_fov, 'dtype', type(in_fov))}")
    if grid.dim() < 2 or grid.shape[-1] != 2 or tuple(in_fov.shape) != tuple(grid.shape[:-1]) or in_fov.device != grid.device:
        raise AssertionError(f"grid must be [..., 2] and in_fov its leading shape on one device, got {tuple(grid.shape)} on {grid.device}, "
                             f"{tuple(in_fov.shape)} on {in_fov.device}")
    grid, in_fov = _dev(grid, "grid"), _dev(in_fov, "in_fov", in_fov.dtype)
    valid = torch.empty(in_fov.shape, device=grid.device, dtype=torch.uint8)
    _call("mvsgi_resample_validity_u8", grid.data_ptr(), in_fov.data_ptr(), valid.data_ptr(), valid.numel(), _stream_ptr(grid))
    return valid


def resample_bilinear(imgs, grid, valid, invalid_value: float = 0.0, out=None) -> torch.Tensor:
    """Raw camera images through a per-camera sampling table -> fp32 planar views [M, C, H, W]:
    out = valid ? bilinear_grid_sample(img, grid, align_corners=False) : invalid_value (backports.py:11-86 arithmetic).
    imgs: uint8 [M, Hr, Wr, 3] (each byte / 255 first) or fp32 [M, C, Hr, Wr]; grid [T, H, W, 2] fp32; valid [T, H, W] bool or
    uint8.  Image m uses table m % T.  One launch on the images' stream; `out`, when given, is written in place."""
    imgs, u8, C, Hr, Wr = _images(imgs, "M")
    M = imgs.shape[0]
    grid = _dev(grid, "grid")
    if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"valid: expected a bool or uint8 tensor, got {getattr(valid, 'dtype', type(valid))}")
    valid = _dev(valid, "valid", valid.dtype)
    if grid.dim() != 4 or grid.shape[3] != 2 or tuple(valid.shape) != tuple(grid.shape[:3]):
        raise AssertionError(f"grid must be [T, H, W, 2] and valid [T, H, W], got {tuple(grid.shape)}, {tuple(valid.shape)}")
    T, Ho, Wo = valid.shape
    if out is None:
        out = torch.empty((M, C, Ho, Wo), device=imgs.device, dtype=torch.float32)
    elif tuple(out.shape) != (M, C, Ho, Wo) or out.dtype != torch.float32 or out.device != imgs.device or not out.is_contiguous() \
            or out.data_ptr() % 16:
        raise AssertionError(f"out must be a contiguous, 16-byte aligned fp32 [{M}, {C}, {Ho}, {Wo}] tensor on {imgs.device}")
    if u8:
        _call("mvsgi_resample_bilinear_u8_f32", imgs.data_ptr(), grid.data_ptr(), valid.data_ptr(), out.data_ptr(), M, T, Hr, Wr, Ho, Wo,
              float(invalid_value), _stream_ptr(imgs))
    else:
        _call("mvsgi_resample_bilinear_f32", imgs.data_ptr(), grid.data_ptr(), valid.data_ptr(), out.data_ptr(), M, T, C, Hr, Wr, Ho, Wo,
              float(invalid_value), _stream_ptr(imgs))
    return out


REPROJECT_CAM_FLOATS = 10     # camera table row: model id (0 double sphere, 1 equirectangular), xi, alpha, fx, fy, cx, cy, w2, calib_h - 1, calib_w - 1


def _view_args(who: str, inv, rays, T, cams):
    """inv, rays, T and cams as reproject() takes them -> (inv [B, H, W], rays, T, cams, B, H, W, N)"""
    inv = _dev(inv, "inv")
    rays = _dev(rays, "rays")
    if inv.dim() == 4 and inv.shape[1] == 1:
        inv = inv.squeeze(1)
    if inv.dim() != 3 or rays.dim() != 3 or rays.shape[0] != 3 or tuple(rays.shape[1:]) != tuple(inv.shape[1:]) or rays.device != inv.device:
        raise AssertionError(f"inv must be [B, H, W] and rays [3, H, W] on one device, got {tuple(inv.shape)}, {tuple(rays.shape)}")
    T = torch.as_tensor(T)
    cams = torch.as_tensor(cams)
    if T.is_cuda or cams.is_cuda or T.dtype != torch.float32 or cams.dtype != torch.float32:
        raise TypeError("T and cams are fp32 host tensors (they travel in the kernel's arguments)")
    N = T.shape[0] if T.dim() == 3 else -1
    if tuple(T.shape) != (N, 4, 4) or tuple(cams.shape) != (N, REPROJECT_CAM_FLOATS):
        raise AssertionError(f"T must be [N, 4, 4] and cams [N, {REPROJECT_CAM_FLOATS}], got {tuple(T.shape)}, {tuple(cams.shape)}")
    if not 1 <= N <= sweep_max_cams():
        raise ValueError(f"{who}: {N} cameras (1 ... {sweep_max_cams()} are supported)")
    B, Ho, Wo = (int(v) for v in inv.shape)
    return inv, rays, T.contiguous(), cams.contiguous(), B, Ho, Wo, N


def _pixel_mask(mask, B: int, Ho: int, Wo: int, dev):
    """A pixel mask uint8 / bool [H, W] or [B, H, W], read in place -> (mask, mask_per_frame); (None, 0) without one"""
    if mask is None:
        return None, 0
    mask = _cloud_plane(mask, "mask", None, dev, (torch.uint8, torch.bool))
    if tuple(mask.shape) not in ((Ho, Wo), (B, Ho, Wo)):
        raise AssertionError(f"mask must be [{Ho}, {Wo}] or [{B}, {Ho}, {Wo}], got {list(mask.shape)}")
    if Wo % 4 == 0 and mask.data_ptr() % 4:
        raise AssertionError("mask must be 4-byte aligned when W % 4 == 0")
    return mask, 1 if mask.dim() == 3 else 0


def _wanted(want, names) -> tuple:
    """want as a tuple, checked to be a selection of names.  Apart from _outputs(): some shapes there come from arguments that are
    checked after the selection (the images' channels)"""
    want = tuple(want)
    if not want or set(want) - set(names) or len(set(want)) != len(want):
        raise ValueError(f"want: a non-empty selection of {', '.join(repr(k) for k in names)}, got {want}")
    return want


def _outputs(want, out, dev, shapes: dict) -> dict:
    """The wanted outputs, each out[k] where the caller gave one (checked against shapes[k] = (shape, dtype)), else a new tensor"""
    res = {}
    for k in want:
        shape, dtype = shapes[k]
        t = None if out is None else out.get(k)
        if t is None:
            t = torch.empty(shape, device=dev, dtype=dtype)
        elif tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.data_ptr() % 16:
            raise AssertionError(f"out['{k}'] must be a contiguous, 16-byte aligned {dtype} {list(shape)} tensor on {dev}")
        res[k] = t
    return res


def reproject(inv, rays, T, cams, bf: float, imgs=None, invalid_value: float = 0.0, want=("xyz", "warped", "valid"), out=None) -> dict:
    """Back-projection of an inverse-distance map (spherical_sweep_stereo.py:417-471; include/mvsgi.h: mvsgi_reproject_f32):
    d = bf / inv, xyz = rays * d, each camera's projection of T[n] xyz, its validity and the camera images sampled there.
    inv [B, H, W] (or [B, 1, H, W]) fp32 on the device; rays [3, H, W] fp32 on the device; T [N, 4, 4] and cams
    [N, REPROJECT_CAM_FLOATS] host tensors (fp32); imgs uint8 [B * N, Hr, Wr, 3] or fp32 [B * N, C, Hr, Wr] on the device,
    needed exactly when "warped" is wanted.  want: the outputs to compute, of "xyz" [B, 3, H, W], "warped" [B, N, C, H, W],
    "valid" [B, N, H, W] bool and "grid" [B, N, H, W, 2]; out: a dict with tensors to write in place (graph capture).
    One launch on inv's stream; there is no CPU fallback.  -> dict of the wanted outputs."""
    inv, rays, T, cams, B, Ho, Wo, N = _view_args("reproject", inv, rays, T, cams)
    want = _wanted(want, ("xyz", "warped", "valid", "grid"))
    kind, C, Hr, Wr = 0, 0, 0, 0
    if "warped" in want:
        imgs, u8, C, Hr, Wr = _images(imgs, "B*N", count=B * N, device=inv.device)
        kind = 0 if u8 else 1
    elif imgs is not None:
        raise ValueError("reproject: imgs given but 'warped' is not wanted")
    res = _outputs(want, out, inv.device, {"xyz": ((B, 3, Ho, Wo), torch.float32), "warped": ((B, N, C, Ho, Wo), torch.float32),
                                           "valid": ((B, N, Ho, Wo), torch.bool), "grid": ((B, N, Ho, Wo, 2), torch.float32)})
    _call("mvsgi_reproject_f32", inv.data_ptr(), rays.data_ptr(), _ptr(imgs) if "warped" in want else None, kind, T.data_ptr(),
          cams.data_ptr(), _ptr(res.get("xyz")), _ptr(res.get("warped")), _ptr(res.get("valid")), _ptr(res.get("grid")), B, N, C, Hr, Wr,
          Ho, Wo, float(bf), float(invalid_value), _stream_ptr(inv))
    return res


def instance_norm(x, res=None, gamma=None, beta=None, eps: float = 1e-5, neg_slope: float = 1.0, out=None) -> torch.Tensor:
    """Instance norm with input statistics on channels-last x [B, ..., C] (NDHWC or NHWC), per frame and channel over all spatial
    positions (F.instance_norm, biased variance): y = act((x - mean) / sqrt(var + eps) * gamma + beta (+ res)), act(v) = v if
    v > 0 else v * neg_slope.  gamma / beta [C] or None; `out` may be x itself (in place).  Two launches on x's stream; the
    workspace comes from torch's allocator, so the call can be captured into a hipGraph."""
    lib = _lib.load()
    x = _dev(x, "x")
    B, C = int(x.shape[0]), int(x.shape[-1])
    S = x.numel() // max(B * C, 1)
    if S < 2:
        # F.instance_norm -> _verify_spatial_size
        raise ValueError(f"Expected more than 1 spatial element when training, got input size "
                         f"{[B, C] + list(x.shape[1:-1])}")
    if res is not None:
        res = _dev(res, "res")
        if tuple(res.shape) != tuple(x.shape):
            raise AssertionError(f"residual {tuple(res.shape)} does not match {tuple(x.shape)}")
    gp, bp = _opt(gamma, "gamma", x.device, numel=C), _opt(beta, "beta", x.device, numel=C)
    if out is None:
        out = torch.empty_like(x)
    elif not (isinstance(out, torch.Tensor) and out.data_ptr() == x.data_ptr() and out.is_contiguous() and out.shape == x.shape):
        _arg(out, "out", x.device, shape=x.shape)       # written in place: a copy (what _dev makes of awkward strides) would take the result with it
    nbytes = lib.mvsgi_instance_norm_ws_bytes(B, S, C)
    ws = torch.empty(max(int(nbytes), 16), device=x.device, dtype=torch.uint8)
    _call("mvsgi_instance_norm_f32", x.data_ptr(), _ptr(res), gp, bp, out.data_ptr(), ws.data_ptr(), B, S, C, float(eps),
          float(neg_slope), _stream_ptr(x))
    return out


def _slab_layout(B: int, units: int, units_per_block: int, max_blocks: int, rec: int) -> dict:
    """The slab of csrc/frame_reduce.hpp, restated, in doubles: [B][G][rec] records | [B][rec] frame sums; a reduce block per
    units_per_block units of a frame, at least one and at most max_blocks."""
    G = min(max(-(-units // units_per_block), 1), max_blocks)
    fsum = B * G * rec
    return dict(G=G, records=0, frame_sums=fsum, total=fsum + B * rec)


def _ws(symbol: str, label: str, dims: dict, device, dtype) -> torch.Tensor:
    """A workspace of the size the library's `symbol` gives for dims (8-byte elements; 0 bytes: the shape is not supported)."""
    n = getattr(_lib.load(), symbol)(*dims.values())
    if n == 0:
        raise ValueError(f"{label}: unsupported shape ({', '.join(f'{k} {v}' for k, v in dims.items())})")
    return torch.empty(n // 8, device=device, dtype=dtype)


METRICS_COLUMNS = ("rmse", "mae", "bad", "ssim", "rmse_dist", "mae_dist", "bad_dist", "ssim_dist", "n")
METRICS_MASK_NONE, METRICS_MASK_TENSOR, METRICS_MASK_RANGE = 0, 1, 2        # MVSGI_METRICS_MASK_* of include/mvsgi.h
METRICS_RANGE_SCOPES = {"frame": 0, "batch": 1}                              # MVSGI_METRICS_RANGE_*
METRICS_EVALUATIONS = 0       # calls of mvsgi_metrics_f32 by this process (tests count evaluations with it)
# the slab of csrc/metrics.hip, restated: a reduce block per 4096 pixels of a frame (at most 64), 20 doubles per record; SSIM tiles
# of 16 x 32 windows
_METRICS_REC, _METRICS_PIX_PER_BLOCK, _METRICS_MAX_BLOCKS, _METRICS_TILE = 20, 4096, 64, (16, 32)


def metrics_ws_layout(B: int, H: int, W: int) -> dict:
    """The workspace of metrics(), in doubles: offsets of its four parts, reduce blocks per frame G, SSIM tiles per frame T."""
    slab = _slab_layout(B, H * W, _METRICS_PIX_PER_BLOCK, _METRICS_MAX_BLOCKS, _METRICS_REC)
    T = (-(-(H - 10) // _METRICS_TILE[0])) * (-(-(W - 10) // _METRICS_TILE[1])) if H >= 11 and W >= 11 else 0
    consts = slab["total"]
    tiles = consts + B * 4
    return dict(slab, T=T, consts=consts, tiles=tiles, total=tiles + 2 * B * T)


def metrics_ws(B: int, H: int, W: int, device) -> torch.Tensor:
    """A workspace for metrics() at this shape (float64; its owner keeps it: a captured graph holds its address)."""
    return _ws("mvsgi_metrics_ws_bytes", "metrics", dict(B=B, H=H, W=W), device, torch.float64)


def metrics(preds, target, bf: float, cmin: float, cmax: float, valid_mask=None, label_range=None, thresh: float = 0.1,
            thresh_dist: float = 0.1, range_scope: str = "frame", ws=None, out=None) -> torch.Tensor:
    """The validation metrics of dsta_mvs/support/loss_function/metrics.py for every frame and pooled (include/mvsgi.h,
    "validation metrics"): preds / target [B, 1, H, W] or [B, H, W] fp32 -> float64 [B + 1, 9] with METRICS_COLUMNS, row B pooled.
    valid_mask: [B, 1, H, W] bool / uint8, or label_range = (lo, hi) on the raw target, or neither.  At most four launches on
    preds' stream, nothing else: with `ws` (metrics_ws) and `out` given the call allocates nothing and can be captured."""
    global METRICS_EVALUATIONS
    preds = _image(preds, "preds")
    target = _image(target, "target")
    if tuple(target.shape) != tuple(preds.shape):
        raise AssertionError(f"target {tuple(target.shape)} does not match preds {tuple(preds.shape)}")
    B, Hh, W = (int(v) for v in preds.shape)
    if valid_mask is not None and label_range is not None:
        raise ValueError("metrics: a valid_mask or a label_range, not both")
    kind, lo, hi, mptr = METRICS_MASK_NONE, 0.0, 0.0, None
    if valid_mask is not None:
        if valid_mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"valid_mask: expected bool or uint8, got {valid_mask.dtype}")
        if valid_mask.numel() != preds.numel() or valid_mask.device != preds.device:
            raise AssertionError(f"valid_mask {tuple(valid_mask.shape)} on {valid_mask.device} does not match preds {tuple(preds.shape)}")
        valid_mask = valid_mask.contiguous()
        if valid_mask.dtype == torch.bool:
            valid_mask = valid_mask.view(torch.uint8)
        if valid_mask.data_ptr() % 4:
            valid_mask = valid_mask.clone()
        kind, mptr = METRICS_MASK_TENSOR, valid_mask.data_ptr()
    elif label_range is not None:
        kind, lo, hi = METRICS_MASK_RANGE, float(label_range[0]), float(label_range[1])
    if range_scope not in METRICS_RANGE_SCOPES:
        raise ValueError(f"range_scope: 'frame' or 'batch', got {range_scope!r}")
    if ws is None:
        ws = metrics_ws(B, Hh, W, preds.device)
    elif ws.device != preds.device or not ws.is_contiguous():
        raise AssertionError("ws must be a contiguous tensor on preds' device")
    if out is None:
        out = torch.empty((B + 1, len(METRICS_COLUMNS)), device=preds.device, dtype=torch.float64)
    elif out.dtype != torch.float64 or tuple(out.shape) != (B + 1, len(METRICS_COLUMNS)) or not out.is_contiguous() \
            or out.device != preds.device:
        raise AssertionError(f"out must be a contiguous float64 [{B + 1}, {len(METRICS_COLUMNS)}] tensor on {preds.device}")
    _call("mvsgi_metrics_f32", preds.data_ptr(), target.data_ptr(), mptr, kind, lo, hi, float(bf), float(cmin), float(cmax), float(thresh),
          float(thresh_dist), METRICS_RANGE_SCOPES[range_scope], ws.data_ptr(), ws.numel() * ws.element_size(), out.data_ptr(), B, Hh, W,
          _stream_ptr(preds))
    METRICS_EVALUATIONS += 1
    return out


LOSSES_COLUMNS = ("vol", "smooth_l1", "inbounds", "n_vol", "n_px")
LOSSES_P_NONE, LOSSES_P_GIVEN, LOSSES_P_FUSED = 0, 1, 2                      # MVSGI_LOSSES_P_* of include/mvsgi.h
LOSSES_VOL_NONE, LOSSES_VOL_PIXEL, LOSSES_VOL_VOLUME = 0, 1, 2              # MVSGI_LOSSES_VOL_*
LOSSES_PX_NONE, LOSSES_PX_TENSOR, LOSSES_PX_LABEL_MAX = 0, 1, 2             # MVSGI_LOSSES_PX_*
LOSSES_EVALUATIONS = 0        # calls of mvsgi_losses_f32 by this process
# the slab of csrc/losses.hip, restated: a reduce block per 256 pixels of a frame (at most 256), 8 doubles per record
_LOSSES_REC, _LOSSES_PIX_PER_BLOCK, _LOSSES_MAX_BLOCKS = 8, 256, 256


def losses_ws_layout(B: int, OH: int, OW: int) -> dict:
    """The workspace of losses(), in doubles: offsets of its two parts and the reduce blocks per frame G."""
    return _slab_layout(B, OH * OW, _LOSSES_PIX_PER_BLOCK, _LOSSES_MAX_BLOCKS, _LOSSES_REC)


def losses_ws(B: int, OH: int, OW: int, device) -> torch.Tensor:
    """A workspace for losses() at this output shape (float64; its owner keeps it: a captured graph holds its address)."""
    return _ws("mvsgi_losses_ws_bytes", "losses", dict(B=B, OH=OH, OW=OW), device, torch.float64)


def _image(t, name: str):
    """[B, 1, H, W] or [B, H, W] fp32 on the device -> contiguous [B, H, W]"""
    t = _dev(t, name)
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise AssertionError(f"{name} must be [B, 1, H, W] or [B, H, W], got {tuple(t.shape)}")
    return t


def _byte_mask(m, name: str, shape, device):
    if not isinstance(m, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(m)}")
    if m.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{name}: expected bool or uint8, got {m.dtype}")
    if tuple(m.shape) != tuple(shape) or m.device != device:
        raise AssertionError(f"{name} {tuple(m.shape)} on {m.device} must be {tuple(shape)} on {device}")
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _inv_list(inv_idx, device):
    inv_idx = _dev(inv_idx.reshape(-1), "inv_dist_idx")
    if inv_idx.numel() < 2:
        raise ValueError(f"losses: D = {inv_idx.numel()}: the volume labels need at least two candidates")
    if inv_idx.device != device:
        raise AssertionError(f"inv_dist_idx is on {inv_idx.device}, the labels on {device}")
    return inv_idx


def losses(labels, inv_idx=None, pred=None, pred_cost=None, costs=None, scale=None, vol_mask=None, px_mask=None, label_max=None,
           inbounds=None, true_cost=None, ws=None, out=None) -> torch.Tensor:
    """The forward values of dsta_mvs/support/loss_function/distance_loss.py for every frame and pooled (include/mvsgi.h, "loss
    functions") -> float64 [B + 1, 5] with LOSSES_COLUMNS, row B pooled.
    labels [B, 1, OH, OW] or [B, OH, OW] fp32; inv_idx [D] fp32 = bf / dist_list, strictly decreasing (the caller's to check: the
    drop-in layer raises ValueError on a list that is not); None where only the image losses are wanted.
    vol (VolumeCrossEntropy): on pred_cost [B, D, OH, OW] (given probabilities), or on the low-resolution costs [B, D, H, W] with the
    regressor's scale (the soft-argmin's softmax, never stored); neither: NaN.  vol_mask: [B, 1, OH, OW] (a pixel across all D) or
    [B, D, OH, OW], bool / uint8.
    smooth_l1 (MaskedSmoothL1Loss) and inbounds (InBoundsBCEDistanceLoss, inbounds = (near_inv, far_inv) as the fp32 thresholds) on
    pred [B, 1, OH, OW]; no pred: NaN.  px_mask [B, 1, OH, OW] bool / uint8, or label_max (labels <= label_max), not both.
    true_cost: an fp32 [B, D, OH, OW] tensor to receive the two-hot labels, or None.
    Two launches on labels' stream, nothing else: with `ws` (losses_ws) and `out` given the call allocates nothing and can be
    captured."""
    global LOSSES_EVALUATIONS
    labels = _image(labels, "labels")
    B, OH, OW = (int(v) for v in labels.shape)
    dev = labels.device
    if inv_idx is None:
        if pred_cost is not None or costs is not None or true_cost is not None:
            raise ValueError("losses: the volume loss and its labels need inv_idx")
        D = 0
    else:
        inv_idx = _inv_list(inv_idx, dev)
        D = inv_idx.numel()
    if pred is not None:
        pred = _image(pred, "pred")
        if tuple(pred.shape) != (B, OH, OW) or pred.device != dev:
            raise AssertionError(f"pred {tuple(pred.shape)} on {pred.device} does not match labels {(B, OH, OW)} on {dev}")
    if pred_cost is not None and costs is not None:
        raise ValueError("losses: pred_cost (given probabilities) or costs (the fused softmax), not both")
    p_kind, probs, Hh, W, sc = LOSSES_P_NONE, None, OH, OW, 1.0
    if pred_cost is not None:
        probs = _dev(pred_cost, "pred_cost")
        if tuple(probs.shape) != (B, D, OH, OW) or probs.device != dev:
            raise AssertionError(f"pred_cost {tuple(probs.shape)} on {probs.device} must be {(B, D, OH, OW)} on {dev}")
        p_kind = LOSSES_P_GIVEN
    elif costs is not None:
        if not isinstance(costs, torch.Tensor) or costs.dim() != 4:
            raise AssertionError("losses: costs must be a [B, D, H, W] tensor")
        sc, shape = confidence_shape(costs.shape, 1.0 if scale is None else scale)
        probs = _dev(costs, "costs")
        if int(probs.shape[0]) != B or int(probs.shape[1]) != D or probs.device != dev:
            raise AssertionError(f"costs {tuple(probs.shape)} on {probs.device} must be [{B}, {D}, H, W] on {dev}")
        if shape[2:] != (OH, OW):
            raise AssertionError(f"costs {tuple(probs.shape)} at scale {sc} give {shape[2]} x {shape[3]}, the labels are {OH} x {OW}")
        Hh, W = int(probs.shape[2]), int(probs.shape[3])
        p_kind = LOSSES_P_FUSED
    vol_kind, vptr = LOSSES_VOL_NONE, None
    if vol_mask is not None:
        pixel = isinstance(vol_mask, torch.Tensor) and vol_mask.dim() == 4 and vol_mask.shape[1] == 1
        vol_mask = _byte_mask(vol_mask, "vol_mask", (B, 1 if pixel else D, OH, OW), dev)
        vol_kind, vptr = (LOSSES_VOL_PIXEL if pixel else LOSSES_VOL_VOLUME), vol_mask.data_ptr()
    if px_mask is not None and label_max is not None:
        raise ValueError("losses: a px_mask or a label_max, not both")
    px_kind, pptr, hi = LOSSES_PX_NONE, None, 0.0
    if px_mask is not None:
        px_mask = _byte_mask(px_mask, "px_mask", (B, 1, OH, OW), dev)
        px_kind, pptr = LOSSES_PX_TENSOR, px_mask.data_ptr()
    elif label_max is not None:
        px_kind, hi = LOSSES_PX_LABEL_MAX, float(label_max)
    near, far = (0.0, 0.0) if inbounds is None else (float(inbounds[0]), float(inbounds[1]))
    if true_cost is not None:
        if not isinstance(true_cost, torch.Tensor) or true_cost.dtype != torch.float32 or tuple(true_cost.shape) != (B, D, OH, OW) \
                or not true_cost.is_contiguous() or true_cost.device != dev:
            raise AssertionError(f"true_cost must be a contiguous fp32 {(B, D, OH, OW)} tensor on {dev}")
    if ws is None:
        ws = losses_ws(B, OH, OW, dev)
    elif ws.device != dev or not ws.is_contiguous():
        raise AssertionError("ws must be a contiguous tensor on labels' device")
    if out is None:
        out = torch.empty((B + 1, len(LOSSES_COLUMNS)), device=dev, dtype=torch.float64)
    elif out.dtype != torch.float64 or tuple(out.shape) != (B + 1, len(LOSSES_COLUMNS)) or not out.is_contiguous() or out.device != dev:
        raise AssertionError(f"out must be a contiguous float64 [{B + 1}, {len(LOSSES_COLUMNS)}] tensor on {dev}")
    _call("mvsgi_losses_f32", labels.data_ptr(), _ptr(pred), _ptr(probs), p_kind, _ptr(inv_idx), vptr, vol_kind, pptr, px_kind, hi,
          int(inbounds is not None), near, far, _ptr(true_cost), ws.data_ptr(), ws.numel() * ws.element_size(), out.data_ptr(),
          B, D, Hh, W, sc, OH, OW, _stream_ptr(labels))
    LOSSES_EVALUATIONS += 1
    return out


def volume_labels(labels, inv_idx, out=None) -> torch.Tensor:
    """The two-hot labels of VolumeCrossEntropy (its true_cost): labels [B, 1, OH, OW], inv_idx [D] -> fp32 [B, D, OH, OW]."""
    lab = _image(labels, "labels")
    inv_idx = _inv_list(inv_idx, lab.device)
    B, OH, OW = (int(v) for v in lab.shape)
    if out is None:
        out = torch.empty((B, inv_idx.numel(), OH, OW), device=lab.device, dtype=torch.float32)
    losses(lab, inv_idx, true_cost=out)
    return out


PHOTO_MAPS = ("n_views", "photo_var", "photo_std", "mean_colour")           # the order of mvsgi_photo_consistency_f32's output pointers
PHOTO_COLUMNS = ("n", "mean_std", "rms", "bad", "coverage") + tuple(f"views_{k}" for k in range(9))
PHOTO_OUTPUTS = PHOTO_MAPS + ("table",)
PHOTO_EVALUATIONS = 0         # calls of mvsgi_photo_consistency_f32 by this process
# the slab of csrc/photo.hip, restated: a reduce block per 256 quads of a frame (a quad: four consecutive pixels of a row; at most 256
# blocks), 16 doubles per record
_PHOTO_REC, _PHOTO_QUADS_PER_BLOCK, _PHOTO_MAX_BLOCKS = 16, 256, 256


def photo_ws_layout(B: int, H: int, W: int) -> dict:
    """The workspace of photo_consistency(), in doubles: offsets of its two parts and the reduce blocks per frame G (a function of
    (H, W) alone).  Pure: no device, no library."""
    return _slab_layout(B, H * (-(-W // 4)), _PHOTO_QUADS_PER_BLOCK, _PHOTO_MAX_BLOCKS, _PHOTO_REC)


def photo_ws(B: int, H: int, W: int, device) -> torch.Tensor:
    """A workspace for photo_consistency() at this shape (float64; its owner keeps it: a captured graph holds its address)."""
    return _ws("mvsgi_photo_ws_bytes", "photo_consistency", dict(B=B, H=H, W=W), device, torch.float64)


def photo_consistency(inv, rays, T, cams, bf: float, imgs, cam_masks=None, mask=None, thresh: float = 0.1, want=PHOTO_OUTPUTS, out=None,
                      ws=None, table=None, cam_seen=None) -> dict:
    """Photometric consistency of an inverse-distance map (include/mvsgi.h, "photometric consistency"): the
    masked variance over the cameras that see the back-projected point, of the colours they show there -- reproject()'s valid and
    warped put through the cost volume's fusion rule without storing them.
    inv, rays, T, cams, bf, imgs as for reproject() (imgs uint8 [B * N, Hr, Wr, 3] or fp32 [B * N, C, Hr, Wr], required); cam_masks
    fp32 [N, 1, Hr, Wr] (a camera also has to see the point through its mask, sampled like the image, > 0); mask uint8 / bool [H, W]
    or [B, H, W]: the pixels the table scores; thresh: the bad-pixel threshold on photo_std; cam_seen bool / uint8 [B, N, H, W], read in
    place: a camera sees a pixel only where it is set -- visibility()'s `visible` keeps the cameras a nearer surface hides the point from
    out of the fusion (mvsgi_photo_consistency_seen_f32; None: the entry point without it).
    want: a selection of PHOTO_OUTPUTS -- n_views uint8 [B, H, W], photo_var / photo_std fp32 [B, H, W], mean_colour fp32
    [B, C, H, W], table float64 [B + 1, 14] with PHOTO_COLUMNS, row B pooled.  out: a dict with tensors to write in place; `table=`
    is out["table"].  Two launches on inv's stream (one without the table), nothing else: with `out` and `ws` (photo_ws; needed with
    the table only) given the call allocates nothing and can be captured.  There is no CPU fallback.  -> dict of the wanted outputs."""
    global PHOTO_EVALUATIONS
    inv, rays, T, cams, B, Ho, Wo, N = _view_args("photo_consistency", inv, rays, T, cams)
    dev = inv.device
    want = _wanted(want, PHOTO_OUTPUTS)
    imgs, u8, C, Hr, Wr = _images(imgs, "B*N", count=B * N, device=dev)
    if cam_masks is not None:
        cam_masks = _dev(cam_masks, "cam_masks")
        if tuple(cam_masks.shape) != (N, 1, Hr, Wr) or cam_masks.device != dev:
            raise AssertionError(f"cam_masks must be fp32 [{N}, 1, {Hr}, {Wr}] (the size of the images) on {dev}, got "
                                 f"{tuple(cam_masks.shape)} on {cam_masks.device}")
    mask, mask_per_frame = _pixel_mask(mask, B, Ho, Wo, dev)
    if cam_seen is not None:
        cam_seen = _cloud_plane(cam_seen, "cam_seen", (B, N, Ho, Wo), dev, (torch.uint8, torch.bool))
        if Wo % 4 == 0 and cam_seen.data_ptr() % 4:
            raise AssertionError("cam_seen must be 4-byte aligned when W % 4 == 0")
    if table is not None:
        if out is not None and out.get("table") is not None and out["table"] is not table:
            raise ValueError("photo_consistency: table= and out['table'] are two different tensors")
        out = dict(out or {}, table=table)
        if "table" not in want:
            raise ValueError("photo_consistency: a table was given but 'table' is not wanted")
    res = _outputs(want, out, dev, {"n_views": ((B, Ho, Wo), torch.uint8), "photo_var": ((B, Ho, Wo), torch.float32),
                                    "photo_std": ((B, Ho, Wo), torch.float32), "mean_colour": ((B, C, Ho, Wo), torch.float32),
                                    "table": ((B + 1, len(PHOTO_COLUMNS)), torch.float64)})
    ws_ptr, ws_bytes = None, 0
    if "table" in want:
        if ws is None:
            ws = photo_ws(B, Ho, Wo, dev)
        elif not isinstance(ws, torch.Tensor) or ws.device != dev or not ws.is_contiguous():
            raise AssertionError("ws must be a contiguous tensor on inv's device")
        ws_ptr, ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    args = (inv.data_ptr(), rays.data_ptr(), imgs.data_ptr(), 0 if u8 else 1, _ptr(cam_masks), T.data_ptr(), cams.data_ptr(), _ptr(mask),
            mask_per_frame, float(thresh), _ptr(res.get("n_views")), _ptr(res.get("photo_var")), _ptr(res.get("photo_std")),
            _ptr(res.get("mean_colour")), ws_ptr, ws_bytes, _ptr(res.get("table")), B, N, C, Hr, Wr, Ho, Wo, float(bf))
    if cam_seen is None:
        _call("mvsgi_photo_consistency_f32", *args, _stream_ptr(inv))
    else:
        _call("mvsgi_photo_consistency_seen_f32", *args, cam_seen.data_ptr(), _stream_ptr(inv))
    PHOTO_EVALUATIONS += 1
    return res


# ---- camera range images and visibility (csrc/visibility.hip; include/mvsgi.h, "camera range images and visibility") ----
VISIBILITY_OUTPUTS = ("visible", "n_visible", "range")                     # the order of mvsgi_visibility_f32's output pointers
VISIBILITY_TOL = 0.02


def visibility_k2(tol: float) -> float:
    """(1 + tol)^2 in double: the factor of the visibility test, which the call rounds to fp32 once."""
    tol = float(tol)
    if not 0.0 <= tol < float("inf"):
        raise ValueError(f"tol: 0 <= tol < inf, got {tol}")
    return (1.0 + tol) * (1.0 + tol)


def _zshape(zshape):
    try:
        Hz, Wz = (int(v) for v in zshape)
    except (TypeError, ValueError):
        raise ValueError(f"zshape: (Hz, Wz), got {zshape!r}") from None
    if not (1 <= Hz <= 1 << 24 and 1 <= Wz <= 1 << 24 and Hz * Wz < 1 << 31):
        raise ValueError(f"zshape: 1 <= Hz, Wz <= 2^24 and Hz * Wz < 2^31, got {(Hz, Wz)}")
    return Hz, Wz


def camera_range(inv, rays, T, cams, bf: float, zshape, mask=None, footprint: int = 1, out=None) -> torch.Tensor:
    """The prediction forward-rendered into every camera: z2 [B, N, Hz, Wz] fp32, per cell of camera n's buffer the smallest squared
    range (from that camera) of the back-projected points that land in it, +inf in an empty cell (include/mvsgi.h, "camera range
    images and visibility").  inv, rays, T, cams, bf as for reproject(); zshape = (Hz, Wz); mask uint8 / bool
    [H, W] or [B, H, W], read in place: the pixels that are rendered; footprint 1 (the nearest cell) or 2 (the four cells around the
    point); out: the tensor to write.  Two launches on inv's stream (fill, splat); the minimum is an integer atomic on the bit pattern,
    independent of the order of arrival: the same inputs give the same bits.  With `out` the call allocates nothing and can be
    captured.  There is no CPU fallback."""
    inv, rays, T, cams, B, Ho, Wo, N = _view_args("camera_range", inv, rays, T, cams)
    dev = inv.device
    Hz, Wz = _zshape(zshape)
    if footprint not in (1, 2):
        raise ValueError(f"footprint: 1 or 2, got {footprint!r}")
    mask, mask_per_frame = _pixel_mask(mask, B, Ho, Wo, dev)
    if out is None:
        out = torch.empty((B, N, Hz, Wz), device=dev, dtype=torch.float32)
    else:
        _arg(out, "out", dev, shape=(B, N, Hz, Wz))
    _call("mvsgi_camera_range_f32", inv.data_ptr(), rays.data_ptr(), T.data_ptr(), cams.data_ptr(), _ptr(mask), mask_per_frame,
          int(footprint), out.data_ptr(), B, N, Ho, Wo, Hz, Wz, float(bf), _stream_ptr(inv))
    return out


def visibility(inv, rays, T, cams, bf: float, z2, tol: float = VISIBILITY_TOL, want=VISIBILITY_OUTPUTS, out=None) -> dict:
    """Which cameras see each pixel's point: visible [B, N, H, W] bool = live & valid_n & (r2 <= z2[cell] * fp32((1 + tol)^2)) at the
    nearest cell of camera_range()'s z2 [B, N, Hz, Wz]; n_visible [B, H, W] uint8, their number; range [B, N, Hz, Wz] fp32 = sqrt(z2),
    the cameras' range images (+inf in an empty cell).  inv, rays, T, cams, bf as for camera_range(); want: a selection of
    VISIBILITY_OUTPUTS; out: a dict with tensors to write in place.  One launch for visible / n_visible, one for range, on inv's stream;
    with `out` the call allocates nothing and can be captured.  There is no CPU fallback.  -> dict of the wanted outputs."""
    inv, rays, T, cams, B, Ho, Wo, N = _view_args("visibility", inv, rays, T, cams)
    dev = inv.device
    z2 = _arg(z2, "z2", dev)
    if z2.dim() != 4 or tuple(z2.shape[:2]) != (B, N):
        raise AssertionError(f"z2 must be [{B}, {N}, Hz, Wz], got {list(z2.shape)}")
    Hz, Wz = _zshape(z2.shape[2:])
    k2 = visibility_k2(tol)
    want = _wanted(want, VISIBILITY_OUTPUTS)
    res = _outputs(want, out, dev, {"visible": ((B, N, Ho, Wo), torch.bool), "n_visible": ((B, Ho, Wo), torch.uint8),
                                    "range": ((B, N, Hz, Wz), torch.float32)})
    _call("mvsgi_visibility_f32", inv.data_ptr(), rays.data_ptr(), T.data_ptr(), cams.data_ptr(), z2.data_ptr(), k2,
          _ptr(res.get("visible")), _ptr(res.get("n_visible")), _ptr(res.get("range")), B, N, Ho, Wo, Hz, Wz, float(bf), _stream_ptr(inv))
    return res


# ---- temporal fusion (csrc/temporal.hip; include/mvsgi.h, "temporal fusion") ----
TEMPORAL_OUTPUTS = ("fused", "var", "age", "warped_inv", "warped_var", "src")   # the order of mvsgi_temporal_fuse_f32's output pointers
TEMPORAL_EMPTY = 0x7F800000FFFFFFFF                                             # an empty cell of zkey: +inf over the largest source index
TEMPORAL_GATE = 3.0


def temporal_affine(long_range, lat_range, shape) -> tuple:
    """(au, bu, av, bv, wrap) of a rig panorama of `shape` = (H, W) with these ranges in radians, in float64 (the calls round each to
    fp32 once): column = floor(gx * au + bu), row = floor(gy * av + bv) of an equirectangular grid coordinate, the inverse of
    RayMaker_UEPanorama's ray table; wrap: the longitude closes (|long1 - long0 - 2 pi| < 1e-6)."""
    try:
        (lo0, lo1), (la0, la1), (Hh, W) = (float(v) for v in long_range), (float(v) for v in lat_range), (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"temporal_affine: long_range and lat_range are pairs of radians and shape is (H, W), got {long_range!r}, "
                         f"{lat_range!r}, {shape!r}") from None
    if not (math.isfinite(lo0) and math.isfinite(lo1) and math.isfinite(la0) and math.isfinite(la1) and lo1 > lo0 and la1 > la0):
        raise ValueError(f"temporal_affine: need finite long0 < long1 and lat0 < lat1, got {(lo0, lo1)}, {(la0, la1)}")
    if Hh < 1 or W < 1:
        raise ValueError(f"temporal_affine: shape (H, W) with H, W >= 1, got {(Hh, W)}")
    # where the equirectangular model is the ray table's inverse: phi = lat + pi / 2 in [0, pi], and theta = lon in [-pi, pi] unless the
    # longitude closes (then the wrap brings a column home)
    eps = 1e-6
    closes = abs(lo1 - lo0 - 2 * math.pi) < eps
    if la0 < -eps or la1 > math.pi + eps or not (closes or (lo0 >= -math.pi - eps and lo1 <= math.pi + eps)):
        raise ValueError(f"temporal_affine: the closed-form inverse needs lat_range inside [0, pi] and long_range inside [-pi, pi] or a "
                         f"full turn, got {(lo0, lo1)}, {(la0, la1)}")
    return (math.pi * W / (lo1 - lo0), -lo0 * W / (lo1 - lo0), (math.pi / 2) * Hh / (la1 - la0), (math.pi / 2 - la0) * Hh / (la1 - la0),
            abs(lo1 - lo0 - 2 * math.pi) < 1e-6)


def temporal_gate2(gate: float) -> float:
    """gate^2 in double: the factor of the agreement test, which the call rounds to fp32 once."""
    gate = float(gate)
    if not 0.0 < gate < float("inf"):
        raise ValueError(f"gate: 0 < gate < inf, got {gate}")
    return gate * gate


def _pano_map(stage: str, index_bits: int, B: int, Hh: int, W: int) -> None:
    """What one launch of a stage over the rig panorama addresses: sides that are exact floats, a cell index of index_bits bits, and
    B frames of ceil(H * ceil(W / 4) / 256) blocks"""
    if Hh > 1 << 24 or W > 1 << 24 or Hh * W >= 1 << index_bits or B * -(-(Hh * -(-W // 4)) // 256) >= 1 << 31:
        raise ValueError(f"{stage}: map {B} x {Hh} x {W}: H, W <= 2^24, H * W < 2^{index_bits} and one launch's blocks")


def _affine_args(affine) -> tuple:
    """affine = temporal_affine(...) as the calls pass it -> (au, bu, av, bv, wrap01)"""
    try:
        au, bu, av, bv, wrap = affine
        au, bu, av, bv = (float(v) for v in (au, bu, av, bv))
    except (TypeError, ValueError):
        raise ValueError(f"affine: (au, bu, av, bv, wrap) of temporal_affine(), got {affine!r}") from None
    if not all(math.isfinite(v) for v in (au, bu, av, bv)):
        raise ValueError(f"affine: (au, bu, av, bv) must be finite, got {(au, bu, av, bv)}")
    return au, bu, av, bv, 1 if wrap else 0


def _pano_plane(t, name: str, shape, dev, dtype=torch.float32):
    """A map [B, H, W] (or [B, 1, H, W]) of the rig panorama: an activation, copied when its form is awkward; bool as uint8"""
    if dtype == torch.uint8 and isinstance(t, torch.Tensor) and t.dtype == torch.bool:
        t = t.view(torch.uint8)
    t = _dev(t, name, dtype)
    if t.dim() == 4 and t.shape[1] == 1:
        t = t.squeeze(1)
    if (shape is not None and tuple(t.shape) != shape) or t.dim() != 3 or not t.numel() or (dev is not None and t.device != dev):
        raise AssertionError(f"{name} must be {list(shape) if shape else '[B, H, W]'} on {dev}, got {list(t.shape)} on {t.device}")
    return t


def _temporal_state(prev_inv, prev_age, prev_var=None):
    """The state as the two calls take it: caller-owned [B, H, W] tensors read in place -> (B, H, W, device)"""
    prev_inv = _arg(prev_inv, "prev_inv", None)
    if prev_inv.dim() != 3 or not prev_inv.numel():
        raise AssertionError(f"prev_inv must be a non-empty [B, H, W], got {list(prev_inv.shape)}")
    shape, dev = tuple(int(v) for v in prev_inv.shape), prev_inv.device
    _pano_map("temporal fusion", 32, *shape)
    _arg(prev_age, "prev_age", dev, torch.uint8, shape=shape)
    if prev_var is not None:
        _arg(prev_var, "prev_var", dev, shape=shape)
    return shape + (dev,)


def temporal_splat(prev_inv, prev_age, rays, T, bf: float, affine, out=None) -> torch.Tensor:
    """Stage A of the temporal fusion (include/mvsgi.h, "temporal fusion"): the previous fused inverse distance
    back-projected, moved by T and splatted into the rig panorama's own cells: zkey [B, H, W] int64, per cell the smallest
    (bits(r2) << 32 | source index) of the live points that land in it, TEMPORAL_EMPTY in an empty cell.  prev_inv [B, H, W] fp32 and
    prev_age [B, H, W] uint8 (0: the pixel holds nothing): the state, read in place; rays [3, H, W] fp32; T [B, 4, 4] fp32 ON THE
    DEVICE (the pose of the previous rig frame in the current one; the launch reads it from memory, so a captured graph sees the value
    of each replay); affine = temporal_affine(long_range, lat_range, (H, W)); out: the tensor to write.  Two launches on prev_inv's
    stream (fill, splat); the minimum is an integer atomic, independent of the order of arrival: the same inputs give the same bits.
    With `out` the call allocates nothing and can be captured.  There is no CPU fallback."""
    B, Ho, Wo, dev = _temporal_state(prev_inv, prev_age)
    rays = _dev(rays, "rays")
    if tuple(rays.shape) != (3, Ho, Wo) or rays.device != dev:
        raise AssertionError(f"rays must be [3, {Ho}, {Wo}] on {dev}, got {list(rays.shape)} on {rays.device}")
    _arg(T, "T", dev, shape=(B, 4, 4))
    affine = _affine_args(affine)
    if out is None:
        out = torch.empty((B, Ho, Wo), device=dev, dtype=torch.int64)
    else:
        _arg(out, "out", dev, torch.int64, shape=(B, Ho, Wo))
    _call("mvsgi_temporal_splat_f32", prev_inv.data_ptr(), prev_age.data_ptr(), rays.data_ptr(), T.data_ptr(), out.data_ptr(), B, Ho, Wo,
          float(bf), *affine, _stream_ptr(prev_inv))
    return out


def temporal_fuse(zkey, prev_inv, prev_var, prev_age, cur_inv, bf: float, gate: float = TEMPORAL_GATE, q_var: float = 0.0, cur_std=None,
                  meas_std=None, want=TEMPORAL_OUTPUTS, out=None) -> dict:
    """Stage B of the temporal fusion: every target pixel resolves its cell of temporal_splat()'s zkey (warped_inv = bf / sqrt(r2), the
    variance carried along the ray plus q_var), and fuses it with the measurement cur_inv [B, H, W] whose standard deviation is cur_std
    [B, H, W] or the scalar meas_std > 0: a Kalman update where the two agree within gate standard deviations, the measurement alone
    where they do not or where there is no prior, the prior alone where there is no measurement.  -> dict of the wanted
    TEMPORAL_OUTPUTS: fused, var fp32, age uint8 (the new state), warped_inv, warped_var fp32 and src int32 (the prior and its source
    pixel; 0, +inf and -1 in an empty cell), each [B, H, W].  prev_inv, prev_var, prev_age: the state the splat read, read in place and
    gathered at the source index, so no output may be one of them; out: a dict with tensors to write in place.  One launch on
    cur_inv's stream; with `out` the call allocates nothing and can be captured.  There is no CPU fallback."""
    B, Ho, Wo, dev = _temporal_state(prev_inv, prev_age, prev_var)
    shape = (B, Ho, Wo)
    _arg(zkey, "zkey", dev, torch.int64, shape=shape)
    cur_inv = _pano_plane(cur_inv, "cur_inv", shape, dev)
    if cur_std is not None:
        if meas_std is not None:
            raise ValueError("temporal_fuse: cur_std or meas_std, not both")
        cur_std = _pano_plane(cur_std, "cur_std", shape, dev)
        sd = 0.0
    else:
        if meas_std is None:
            raise ValueError("temporal_fuse: the measurement's standard deviation, cur_std [B, H, W] or meas_std > 0")
        sd = float(meas_std)
        if not 0.0 < sd < float("inf"):
            raise ValueError(f"meas_std: 0 < meas_std < inf, got {sd}")
    g2 = temporal_gate2(gate)
    q_var = float(q_var)
    if not 0.0 <= q_var < float("inf"):
        raise ValueError(f"q_var: 0 <= q_var < inf, got {q_var}")
    want = _wanted(want, TEMPORAL_OUTPUTS)
    kinds = {"fused": torch.float32, "var": torch.float32, "age": torch.uint8, "warped_inv": torch.float32, "warped_var": torch.float32,
             "src": torch.int32}
    res = _outputs(want, out, dev, {k: (shape, d) for k, d in kinds.items()})
    state = {t.data_ptr() for t in (prev_inv, prev_var, prev_age)}
    for k, t in res.items():
        if t.data_ptr() in state:
            raise AssertionError(f"out['{k}'] is a tensor of the state: the state is gathered at the source index and cannot be written in place")
    _call("mvsgi_temporal_fuse_f32", zkey.data_ptr(), prev_inv.data_ptr(), prev_var.data_ptr(), prev_age.data_ptr(), cur_inv.data_ptr(),
          _ptr(cur_std), sd, *(_ptr(res.get(k)) for k in TEMPORAL_OUTPUTS), B, Ho, Wo, float(bf), g2, q_var, _stream_ptr(cur_inv))
    return res


# ---- volumetric fusion (csrc/tsdf.hip; include/mvsgi.h, "volumetric fusion") ----
TSDF_OUTPUTS = ("inv", "weight", "steps")                   # the order of mvsgi_tsdf_raycast_f32's output pointers
TSDF_MAX_STEPS = 4096
TSDF_FLT_MAX = 3.4028234663852886e+38


def _tsdf_volume(vol):
    """The volume as the two calls take it: a caller-owned [B, Nz, Ny, Nx, 2] fp32 tensor used in place -> (B, Nx, Ny, Nz, device)"""
    vol = _arg(vol, "vol", None)
    if vol.dim() != 5 or vol.shape[4] != 2 or not vol.numel():
        raise AssertionError(f"vol must be a non-empty [B, Nz, Ny, Nx, 2], got {list(vol.shape)}")
    B, Nz, Ny, Nx = (int(v) for v in vol.shape[:4])
    tsdf_dims(B, Nx, Ny, Nz)
    return B, Nx, Ny, Nz, vol.device


def tsdf_dims(B: int, Nx: int, Ny: int, Nz: int) -> None:
    """What one launch addresses: every N >= 1, Nx * Ny * Nz < 2^31 and B * ceil(Nx * Ny * Nz / 512) < 2^31."""
    if min(B, Nx, Ny, Nz) < 1:
        raise ValueError(f"volumetric fusion: B, Nx, Ny, Nz >= 1, got {(B, Nx, Ny, Nz)}")
    n = Nx * Ny * Nz
    if n >= 1 << 31 or B * -(-(n // 2 if n % 2 == 0 else n) // 256) >= 1 << 31:
        raise ValueError(f"volumetric fusion: {B} volumes of {Nx} x {Ny} x {Nz} voxels are too large for one launch")


def _tsdf_scalar(v, name: str, low_ok: bool = False) -> float:
    v = float(v)
    if not (0.0 <= v if low_ok else 0.0 < v) or not v <= TSDF_FLT_MAX:
        raise ValueError(f"{name}: {'0 <=' if low_ok else '0 <'} {name} <= FLT_MAX, got {v}")
    return v


def tsdf_integrate(vol, inv, T, origin, origin_prev, bf: float, affine, voxel: float, trunc: float, w_max: float = 64.0,
                   r_range=(0.0, TSDF_FLT_MAX), std=None, mask=None, r_out=None) -> torch.Tensor:
    """One prediction integrated into the rolling truncated signed distance volume, in place (include/mvsgi.h, "volumetric fusion";
    DESIGN.md section 24).  vol [B, Nz, Ny, Nx, 2] fp32, the pairs (f, w), toroidal: world voxel i lives in slot i mod N; T [B, 4, 4]
    fp32 (world -> rig), origin and origin_prev [B, 3] int32 (the coverage now and at the previous integrate: what scrolled in is
    cleared on the way), all ON THE DEVICE and read by the launch, so a captured graph sees the values of each replay.  inv [B, H, W]
    (or [B, 1, H, W]) fp32: the rig panorama's inverse distance; affine = temporal_affine(long_range, lat_range, (H, W)); std
    likewise (the standard deviation of inv: the observation's weight is trunc^2 / (trunc^2 + sigma_d^2)) or None (weight 1); mask
    [B, H, W] uint8 / bool or None (0: the pixel is not integrated); r_out [B, Nz, Ny, Nx] fp32 or None: every voxel centre's range.
    One launch on inv's stream; nothing is allocated: capturable.  There is no CPU fallback.  -> vol"""
    B, Nx, Ny, Nz, dev = _tsdf_volume(vol)
    inv = _pano_plane(inv, "inv", None, dev)
    if inv.shape[0] != B:
        raise AssertionError(f"inv must be [{B}, H, W], got {list(inv.shape)}")
    shape = tuple(int(v) for v in inv.shape)
    _pano_map("volumetric fusion", 31, *shape)
    if std is not None:
        std = _pano_plane(std, "std", shape, dev)
    if mask is not None:
        mask = _pano_plane(mask, "mask", shape, dev, torch.uint8)
    _arg(T, "T", dev, shape=(B, 4, 4))
    _arg(origin, "origin", dev, torch.int32, shape=(B, 3))
    _arg(origin_prev, "origin_prev", dev, torch.int32, shape=(B, 3))
    if r_out is not None:
        _arg(r_out, "r_out", dev, shape=(B, Nz, Ny, Nx))
    affine = _affine_args(affine)
    voxel, trunc, w_max = _tsdf_scalar(voxel, "voxel"), _tsdf_scalar(trunc, "trunc"), _tsdf_scalar(w_max, "w_max")
    t2 = _tsdf_scalar(trunc * trunc, "trunc^2")
    try:
        r_min, r_max = (float(v) for v in r_range)
    except (TypeError, ValueError):
        raise ValueError(f"r_range: (r_min, r_max), got {r_range!r}") from None
    r_max = min(r_max, TSDF_FLT_MAX)
    if not 0.0 <= r_min < r_max:
        raise ValueError(f"r_range: 0 <= r_min < r_max, got {(r_min, r_max)}")
    _call("mvsgi_tsdf_integrate_f32", vol.data_ptr(), inv.data_ptr(), _ptr(std), _ptr(mask), T.data_ptr(), origin.data_ptr(),
          origin_prev.data_ptr(), _ptr(r_out), B, Nx, Ny, Nz, shape[1], shape[2], voxel, trunc, t2, w_max, r_min, r_max, float(bf), *affine,
          _stream_ptr(inv))
    return vol


def tsdf_raycast(vol, rays, P, origin, bf: float, voxel: float, t0: float, step: float, K: int, w_min: float = 1.0, want=TSDF_OUTPUTS,
                 out=None) -> dict:
    """The volume ray-cast into the rig's view: every pixel of the panorama marches its ray, moved into the world by P [B, 4, 4] fp32
    (rig -> world, ON THE DEVICE, read by the launch), in K fixed steps t_k = t0 + k step through the nearest voxels, and stops at
    the first front-face zero crossing between two valid samples (weight >= w_min), interpolated linearly.  vol [B, Nz, Ny, Nx, 2]
    and origin [B, 3] int32 (the coverage of what the volume holds): caller-owned, on the device, read in place; rays [3, H, W] fp32.
    -> dict of the wanted TSDF_OUTPUTS, each [B, H, W]: inv fp32 (bf / t*, 0 without a crossing), weight fp32 (the weight of the
    sample behind the surface, 0 without), steps int32 (the index of that sample, K without).  out: a dict with tensors to write in
    place.  One launch on vol's stream; with `out` nothing is allocated: capturable.  There is no CPU fallback."""
    B, Nx, Ny, Nz, dev = _tsdf_volume(vol)
    rays = _dev(rays, "rays")
    if rays.dim() != 3 or rays.shape[0] != 3 or not rays.numel() or rays.device != dev:
        raise AssertionError(f"rays must be [3, H, W] on {dev}, got {list(rays.shape)} on {rays.device}")
    Ho, Wo = int(rays.shape[1]), int(rays.shape[2])
    _pano_map("volumetric fusion", 31, B, Ho, Wo)
    _arg(P, "P", dev, shape=(B, 4, 4))
    _arg(origin, "origin", dev, torch.int32, shape=(B, 3))
    voxel, step, t0 = _tsdf_scalar(voxel, "voxel"), _tsdf_scalar(step, "step"), _tsdf_scalar(t0, "t0", low_ok=True)
    inv_vs = _tsdf_scalar(1.0 / voxel, "1 / voxel")
    w_min = float(w_min)
    if not math.isfinite(w_min):
        raise ValueError(f"w_min must be finite, got {w_min}")
    if int(K) != K or not 1 <= int(K) <= TSDF_MAX_STEPS:
        raise ValueError(f"K: 1 <= K <= {TSDF_MAX_STEPS} march steps, got {K!r}")
    want = _wanted(want, TSDF_OUTPUTS)
    shape = (B, Ho, Wo)
    res = _outputs(want, out, dev, {"inv": (shape, torch.float32), "weight": (shape, torch.float32), "steps": (shape, torch.int32)})
    _call("mvsgi_tsdf_raycast_f32", vol.data_ptr(), rays.data_ptr(), P.data_ptr(), origin.data_ptr(),
          *(_ptr(res.get(k)) for k in TSDF_OUTPUTS), B, Nx, Ny, Nz, Ho, Wo, inv_vs, t0, step, int(K), w_min, float(bf), _stream_ptr(vol))
    return res


# the packed point cloud (csrc/cloud.hip), restated: tiles of 1024 consecutive pixels, 16 words of 64 bits each; at most 4 gates, 4 colour
# channels and 16 floats per record
CLOUD_TILE, CLOUD_WORDS_PER_TILE, CLOUD_MAX_GATES, CLOUD_MAX_CHANNELS, CLOUD_MAX_RECORD, CLOUD_MAX_BATCH = 1024, 16, 4, 4, 16, 65535
# the default distance range: every positive finite d.  Its lower end is the smallest normal fp32, not 0: inv = +inf gives d = 0, which it drops
# together with inv = 0 (d = inf), negative inv (d < 0) and NaN
CLOUD_D_RANGE = (float(torch.finfo(torch.float32).tiny), float(torch.finfo(torch.float32).max))


def _round16(n: int) -> int:
    return -(-n // 16) * 16


def cloud_ws_layout(B: int, H: int, W: int) -> dict:
    """The workspace of pack_cloud(), in bytes: tiles per frame, 64-bit words per frame, the offsets of its three parts (bit words
    [B, tiles, 16] uint64, tile counts [B, tiles] int32, tile offsets [B, tiles] int32) and the total.  Pure: no device, no library."""
    B, H, W = int(B), int(H), int(W)
    if not (1 <= B <= CLOUD_MAX_BATCH and H >= 1 and W >= 1 and H * W < 1 << 31):
        raise ValueError(f"pack_cloud: unsupported shape (B {B}, H {H}, W {W})")
    tiles = -(-(H * W) // CLOUD_TILE)
    words = 0
    counts = words + _round16(B * tiles * CLOUD_WORDS_PER_TILE * 8)
    offsets = counts + _round16(B * tiles * 4)
    return dict(tiles=tiles, words_per_frame=tiles * CLOUD_WORDS_PER_TILE, words=words, tile_counts=counts, tile_offsets=offsets,
                total=offsets + _round16(B * tiles * 4))


def cloud_ws(B: int, H: int, W: int, device) -> torch.Tensor:
    """A workspace for pack_cloud() at this shape (int64; its owner keeps it: a captured graph holds its address)."""
    return _ws("mvsgi_cloud_ws_bytes", "pack_cloud", dict(B=B, H=H, W=W), device, torch.int64)


def cloud_capacity(H: int, W: int, step=(1, 1)) -> int:
    """The default capacity of pack_cloud(): the pixels the step leaves, ceil(H / sy) * ceil(W / sx)."""
    return (-(-int(H) // int(step[0]))) * (-(-int(W) // int(step[1])))


def _cloud_plane(t, name: str, shape, device, dtypes=(torch.float32,)) -> torch.Tensor:
    """A tensor pack_cloud() reads or writes as it is: nothing is copied, so that a call with `ws` and `out` allocates nothing."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: mvs_gi_amd runs on the GPU only (tensor is on {t.device}); there is no CPU fallback")
    if t.dtype not in dtypes:
        raise TypeError(f"{name}: expected {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if device is not None and t.device != device:
        raise AssertionError(f"{name}: on {t.device}, inv is on {device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise AssertionError(f"{name}: expected shape {list(shape)}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise AssertionError(f"{name}: must be contiguous")
    if t.data_ptr() % t.element_size():
        raise AssertionError(f"{name}: must be aligned to its element size")
    return t


def pack_cloud(inv, rays, bf: float, *, d_range, gates=(), mask=None, step=(1, 1), warped=None, valid=None, require_colour: bool = False,
               no_colour: float = 0.0, attrs=(), capacity=None, want_index: bool = False, ws=None, out=None) -> dict:
    """The prediction as a packed list of points (include/mvsgi.h, "packed point cloud").
    inv [B, H, W] (or [B, 1, H, W]) fp32, rays [3, H, W] fp32: d = bf / inv, xyz = rays * d, the bits of reproject()'s xyz.
    A pixel p = i * W + j of frame b is kept iff i % sy == 0 and j % sx == 0, mask != 0 (uint8 / bool [H, W] or [B, H, W]), d is finite
    and d_range[0] <= d <= d_range[1], lo <= g <= hi for every gate (g [B, H, W] fp32, lo, hi) -- at most CLOUD_MAX_GATES --, and,
    with require_colour, some camera of valid [B, N, H, W] (bool / uint8) sees it.  warped [B, N, C, H, W] fp32 (C <= 4) and valid, as
    reproject() returns them, give the colour: that of the lowest valid camera, no_colour when there is none.  attrs: planes [B, H, W]
    fp32 appended to each record; R = 3 + C + A <= CLOUD_MAX_RECORD.
    -> dict(points [B, capacity, R] fp32: the kept points of a frame in ascending p; counts [B, 2] int32 = (written, kept), written =
    min(kept, capacity); index [B, capacity] int32, the source p, with want_index).  Rows >= written are not written.  capacity
    defaults to cloud_capacity(H, W, step).  Three launches on inv's stream, no host synchronisation; with `ws` (cloud_ws) and `out`
    (a dict of the outputs) given the call allocates nothing and can be captured.  Nothing is copied or converted: every tensor must
    be contiguous and on inv's device.  There is no CPU fallback."""
    if isinstance(inv, torch.Tensor) and inv.dim() == 4 and inv.shape[1] == 1:
        inv = inv[:, 0]
    inv = _cloud_plane(inv, "inv", None, None)
    if inv.dim() != 3:
        raise AssertionError(f"inv must be [B, H, W] or [B, 1, H, W], got {tuple(inv.shape)}")
    B, Hh, W = (int(v) for v in inv.shape)
    dev = inv.device
    cloud_ws_layout(B, Hh, W)                                   # the shape's limits
    rays = _cloud_plane(rays, "rays", (3, Hh, W), dev)
    sy, sx = (int(v) for v in step)
    if sy < 1 or sx < 1:
        raise ValueError(f"step: (sy, sx) >= 1, got {tuple(step)}")
    d_min, d_max = (float(v) for v in d_range)
    gates = tuple(gates)
    if len(gates) > CLOUD_MAX_GATES:
        raise ValueError(f"pack_cloud: {len(gates)} gates (at most {CLOUD_MAX_GATES})")
    gate_planes = [_cloud_plane(g, f"gates[{k}]", (B, Hh, W), dev) for k, (g, _, _) in enumerate(gates)]
    mask_per_frame = 0
    if mask is not None:
        mask = _cloud_plane(mask, "mask", None, dev, (torch.uint8, torch.bool))
        if tuple(mask.shape) not in ((Hh, W), (B, Hh, W)):
            raise AssertionError(f"mask must be [{Hh}, {W}] or [{B}, {Hh}, {W}], got {list(mask.shape)}")
        mask_per_frame = 1 if mask.dim() == 3 else 0
    if (warped is None) != (valid is None):
        raise ValueError("pack_cloud: warped and valid are given together (as reproject() returns them) or not at all")
    N = C = 0
    if warped is not None:
        warped = _cloud_plane(warped, "warped", None, dev)
        if warped.dim() != 5 or warped.shape[0] != B or tuple(warped.shape[3:]) != (Hh, W):
            raise AssertionError(f"warped must be [{B}, N, C, {Hh}, {W}], got {list(warped.shape)}")
        N, C = int(warped.shape[1]), int(warped.shape[2])
        if not 1 <= N <= sweep_max_cams():
            raise ValueError(f"pack_cloud: {N} cameras (1 ... {sweep_max_cams()} are supported)")
        if not 1 <= C <= CLOUD_MAX_CHANNELS:
            raise ValueError(f"pack_cloud: {C} colour channels (1 ... {CLOUD_MAX_CHANNELS} are supported)")
        valid = _cloud_plane(valid, "valid", (B, N, Hh, W), dev, (torch.bool, torch.uint8))
    elif require_colour:
        raise ValueError("pack_cloud: require_colour needs warped and valid")
    attrs = tuple(attrs)
    attr_planes = [_cloud_plane(a, f"attrs[{m}]", (B, Hh, W), dev) for m, a in enumerate(attrs)]
    R = 3 + C + len(attrs)
    if R > CLOUD_MAX_RECORD:
        raise ValueError(f"pack_cloud: a record of {R} floats (3 + {C} colour channels + {len(attrs)} attributes; at most {CLOUD_MAX_RECORD})")
    capacity = cloud_capacity(Hh, W, (sy, sx)) if capacity is None else int(capacity)
    if not 1 <= capacity < 1 << 31:
        raise ValueError(f"capacity: 1 <= capacity < 2^31, got {capacity}")
    shapes = {"points": ((B, capacity, R), torch.float32), "counts": ((B, 2), torch.int32)}
    if want_index:
        shapes["index"] = ((B, capacity), torch.int32)
    if out is not None:
        for k, (shape, dtype) in shapes.items():
            if out.get(k) is not None:
                _cloud_plane(out[k], f"out['{k}']", shape, dev, (dtype,))
    if ws is not None:
        if not isinstance(ws, torch.Tensor) or ws.device != dev or not ws.is_contiguous() or ws.data_ptr() % 16:
            raise AssertionError(f"ws must be a contiguous, 16-byte aligned tensor on {dev}")
    lib = _lib.load()
    if ws is None:
        ws = cloud_ws(B, Hh, W, dev)
    elif ws.numel() * ws.element_size() < lib.mvsgi_cloud_ws_bytes(B, Hh, W):
        raise AssertionError(f"ws holds {ws.numel() * ws.element_size()} bytes, this shape needs {lib.mvsgi_cloud_ws_bytes(B, Hh, W)} (cloud_ws)")
    res = {}
    for k, (shape, dtype) in shapes.items():
        t = None if out is None else out.get(k)
        res[k] = torch.empty(shape, device=dev, dtype=dtype) if t is None else t
    P, F = ctypes.c_void_p, ctypes.c_float
    gate_tab = (P * max(len(gates), 1))(*[g.data_ptr() for g in gate_planes])
    lo_tab = (F * max(len(gates), 1))(*[float(lo) for _, lo, _ in gates])
    hi_tab = (F * max(len(gates), 1))(*[float(hi) for _, _, hi in gates])
    attr_tab = (P * max(len(attrs), 1))(*[a.data_ptr() for a in attr_planes])
    _call("mvsgi_cloud_pack_f32", inv.data_ptr(), rays.data_ptr(), _ptr(mask), mask_per_frame, gate_tab, lo_tab, hi_tab, len(gates),
          _ptr(warped), _ptr(valid), N, C, 1 if require_colour else 0, float(no_colour), attr_tab, len(attrs), res["points"].data_ptr(),
          res["counts"].data_ptr(), _ptr(res.get("index")), capacity, ws.data_ptr(), ws.numel() * ws.element_size(), B, Hh, W, sy, sx,
          float(bf), d_min, d_max, _stream_ptr(inv))
    return res


SA_AUTO, SA_PIXEL, SA_BAND = 0, 1, 2        # MVSGI_SA_* of include/mvsgi.h


def softargmin(costs_bdhw, inv_idx, scale: float, want_norm_costs: bool, post_div: float = 1.0, variant: int = SA_AUTO):
    """costs [B, D, H, W], inv_idx [D] -> inv_dist [B, 1, OH, OW] (divided by post_div), norm_costs
    [B, D, OH, OW] | None, with OH = floor(H * scale), OW = floor(W * scale) as F.interpolate(scale_factor=scale) sizes them.
    scale 1 | 2: the fused x1 / x2 launches; integer factors >= 3: the row-band kernel; any other factor > 0: the
    thread-per-pixel kernel.  variant: SA_PIXEL | SA_BAND force one of the latter two (tests, A/B timing)."""
    c = _dev(costs_bdhw, "costs")
    inv_idx = _dev(inv_idx.reshape(-1), "inv_dist_idx")
    B, D, H, W = c.shape
    if inv_idx.numel() != D:
        raise AssertionError(f"{D} cost planes but {inv_idx.numel()} distance candidates")
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"softargmin: scale {scale} is not a finite positive factor")
    OH, OW = math.floor(H * scale), math.floor(W * scale)
    if OH < 1 or OW < 1:
        raise ValueError(f"softargmin: scale {scale} gives an empty {OH} x {OW} output for {H} x {W}")
    inv = torch.empty((B, 1, OH, OW), device=c.device, dtype=torch.float32)
    pr = torch.empty((B, D, OH, OW), device=c.device, dtype=torch.float32) if want_norm_costs else None
    if variant == SA_AUTO and scale in (1.0, 2.0):
        _call("mvsgi_softargmin_div_f32", c.data_ptr(), inv_idx.data_ptr(), inv.data_ptr(), _ptr(pr), B, D, H, W, int(scale), float(post_div),
              _stream_ptr(c))
    else:
        _call("mvsgi_softargmin_scaled_f32", c.data_ptr(), inv_idx.data_ptr(), inv.data_ptr(), _ptr(pr), B, D, H, W, scale, OH, OW, float(post_div),
              int(variant), _stream_ptr(c))
    return inv, pr


CONFIDENCE_MAPS = ("max_prob", "entropy", "spread", "argmax")      # the order of mvsgi_confidence_f32's output pointers


def confidence_shape(costs_shape, scale):
    """(B, D, H, W), scale -> (scale as float, the maps' shape (B, 1, OH, OW)); raises on what F.interpolate would not take."""
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"confidence: scale {scale} is not a finite positive factor")
    B, _, H, W = (int(v) for v in costs_shape)
    OH, OW = math.floor(H * scale), math.floor(W * scale)
    if OH < 1 or OW < 1:
        raise ValueError(f"confidence: scale {scale} gives an empty {OH} x {OW} output for {H} x {W}")
    return scale, (B, 1, OH, OW)


def confidence(costs_bdhw, inv_idx, scale: float, want=CONFIDENCE_MAPS, post_div: float = 1.0, normalize_entropy: bool = False,
               out=None) -> dict:
    """Confidence maps of the soft-argmin's softmax (include/mvsgi.h, mvsgi_confidence_f32):
    costs [B, D, H, W], inv_idx [D] -> {name: [B, 1, OH, OW]} for the names in `want`, at softargmin()'s output resolution.
    max_prob, entropy (natural log; divided by ln D with normalize_entropy) and spread (standard deviation of the candidates
    under the softmax, divided by post_div like inv_dist) are fp32, argmax is int32 (-1 where the others are NaN).
    want: a non-empty selection of CONFIDENCE_MAPS without repeats; only those maps are computed for storing and stored.
    out: {name: tensor} for every wanted name, written in place and returned; the call then allocates nothing.  One launch on
    costs' stream, no [B, D, OH, OW] tensor, capturable."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or not set(want) <= set(CONFIDENCE_MAPS):
        raise ValueError(f"confidence: want must be a non-empty selection of {CONFIDENCE_MAPS} without repeats, got {want!r}")
    if not isinstance(costs_bdhw, torch.Tensor) or costs_bdhw.dim() != 4:
        raise AssertionError("confidence: costs must be a [B, D, H, W] tensor")
    scale, shape = confidence_shape(costs_bdhw.shape, scale)
    if float(post_div) == 0.0:
        raise ValueError("confidence: post_div must be non-zero")
    if out is not None:
        for n in want:
            t = out.get(n)
            dt = torch.int32 if n == "argmax" else torch.float32
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"confidence: out[{n!r}] must be a tensor")
            if t.dtype != dt:
                raise TypeError(f"confidence: out[{n!r}]: expected {dt}, got {t.dtype}")
            if tuple(t.shape) != shape or not t.is_contiguous() or t.device != costs_bdhw.device:
                raise AssertionError(f"confidence: out[{n!r}] must be a contiguous {shape} tensor on {costs_bdhw.device}, got "
                                     f"{tuple(t.shape)} on {t.device}")
    c = _dev(costs_bdhw, "costs")
    inv_idx = _dev(inv_idx.reshape(-1), "inv_dist_idx")
    B, D, H, W = c.shape
    if inv_idx.numel() != D:
        raise AssertionError(f"{D} cost planes but {inv_idx.numel()} distance candidates")
    if out is None:
        out = {n: torch.empty(shape, device=c.device, dtype=torch.int32 if n == "argmax" else torch.float32) for n in want}
    _call("mvsgi_confidence_f32", c.data_ptr(), inv_idx.data_ptr(), *(_ptr(out[n]) if n in want else None for n in CONFIDENCE_MAPS),
          B, D, H, W, scale, shape[2], shape[3], float(post_div), int(bool(normalize_entropy)), _stream_ptr(c))
    return {n: out[n] for n in want}


def ncdhw_to_ndhwc(x) -> torch.Tensor:
    """contiguous [B, C, D, H, W] -> [B, D, H, W, C]."""
    x = _dev(x, "x")
    B, C, D, H, W = x.shape
    y = torch.empty((B, D, H, W, C), device=x.device, dtype=torch.float32)
    _call("mvsgi_ncv_to_nvc_f32", x.data_ptr(), y.data_ptr(), B, C, D * H * W, _stream_ptr(x))
    return y


def ndhwc_to_ncdhw(x) -> torch.Tensor:
    x = _dev(x, "x")
    B, D, H, W, C = x.shape
    y = torch.empty((B, C, D, H, W), device=x.device, dtype=torch.float32)
    _call("mvsgi_nvc_to_ncv_f32", x.data_ptr(), y.data_ptr(), B, C, D * H * W, _stream_ptr(x))
    return y


def as_ndhwc(vol: torch.Tensor) -> torch.Tensor:
    """Accepts the module-boundary volume [B, C, D, H, W] in either memory format and returns the
    [B, D, H, W, C] view (no copy when it already is channels-last, which is what our
    cv_builder hands over) or a transposed copy (contiguous NCDHW from another producer)."""
    if vol.dim() != 5:
        raise AssertionError(f"expected a [B, C, D, H, W] volume, got {tuple(vol.shape)}")
    v = vol.permute(0, 2, 3, 4, 1)
    if v.is_contiguous():
        return v
    return ncdhw_to_ndhwc(vol.contiguous())


# --------------------------------------------------------------------------------------
def pack_deform_conv2d_weights(w_oihw: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, Kh, Kw] -> [Kh*Kw, Cin, Cout] for mvsgi_deform_conv2d_f32."""
    w = _dev(w_oihw, "deform conv weight")
    Cout, Cin, Kh, Kw = w.shape
    wp = torch.empty((Kh * Kw, Cin, Cout), device=w.device, dtype=torch.float32)
    _call("mvsgi_deform_conv2d_pack_weights_f32", w.data_ptr(), wp.data_ptr(), Cout, Cin, Kh, Kw, _stream_ptr(w))
    return wp


def deform_conv2d(x_nhwc, offset, w_packed, scale, shift, kernel_size, stride=(1, 1), padding=(0, 0), dilation=(1, 1),
                  res=None, neg_slope=1.0) -> torch.Tensor:
    """x [N, H, W, Cin], offset [1 | N, 2*Kh*Kw, Ho, Wo] -> y [N, Ho, Wo, Cout] (torchvision.ops.deform_conv2d
    semantics + per-channel scale / shift, residual, LeakyReLU)."""
    x = _dev(x_nhwc, "x")
    offset = _dev(offset, "offset")
    N, Hh, W, Cin = x.shape
    Kh, Kw = kernel_size
    dev = x.device
    sc, sh, Cout = _scale_shift(scale, shift, dev)
    Ho = (Hh + 2 * padding[0] - (dilation[0] * (Kh - 1) + 1)) // stride[0] + 1
    Wo = (W + 2 * padding[1] - (dilation[1] * (Kw - 1) + 1)) // stride[1] + 1
    if offset.dim() != 4 or tuple(offset.shape[1:]) != (2 * Kh * Kw, Ho, Wo) or offset.shape[0] not in (1, N):
        raise AssertionError(f"offset {tuple(offset.shape)} does not match [1|{N}, {2 * Kh * Kw}, {Ho}, {Wo}]")
    wp = _arg(w_packed, "w_packed", dev, shape=(Kh * Kw, Cin, Cout))
    y = torch.empty((N, Ho, Wo, Cout), device=dev, dtype=torch.float32)
    _call("mvsgi_deform_conv2d_f32", x.data_ptr(), offset.data_ptr(), int(offset.shape[0] == N and N > 1), wp.data_ptr(), sc,
          sh, _opt(res, "res", dev, shape=(N, Ho, Wo, Cout)), y.data_ptr(), N, Cin, Hh, W, Cout, Kh, Kw, stride[0], stride[1], padding[0], padding[1], dilation[0],
          dilation[1], float(neg_slope), _stream_ptr(x))
    return y


# ---- the extractor's residual blocks on pre-split activations (csrc/resblock2d_rs.hip) ----
def split2d_buffer(N: int, H: int, W: int, device) -> torch.Tensor:
    """A zeroed 2-D split-padded activation buffer [N, H + 4, W + 4, 64] uint8 (the kernels write the interior only: the
    two-pixel zero border is the convolutions' padding and stays as allocated)."""
    return torch.zeros((N, H + 4, W + 4, 64), device=device, dtype=torch.uint8)


def _check_split2d(t: torch.Tensor, N: int, H: int, W: int, device, name: str = "out_split") -> None:
    """A caller-owned 2-D split-padded buffer (split2d_buffer) for N images of H x W pixels."""
    _arg(t, name, device, torch.uint8, shape=(N, H + 4, W + 4, 64))


def _split2d_dims(x_split, name: str):
    """A 2-D split-padded input, checked -> (N, H, W)."""
    if not isinstance(x_split, torch.Tensor) or x_split.dim() != 4:
        raise TypeError(f"{name}: expected a [N, H + 4, W + 4, 64] uint8 tensor, got {getattr(x_split, 'shape', type(x_split))}")
    N, Hp, Wp, _ = x_split.shape
    _arg(x_split, name, None, torch.uint8, shape=(N, Hp, Wp, 64))
    return N, Hp - 4, Wp - 4


def _rs2d_packed(wp, name: str, device) -> int:
    return _arg(wp, name, device, torch.uint8, nbytes=_lib.load().mvsgi_resblock2d_split_packed_weight_bytes()).data_ptr()


def f32_to_split2d(x_nhwc: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    x = _dev(x_nhwc, "x")
    N, Hh, W, C = x.shape
    if C != 16:
        raise AssertionError(f"the 2-D split-padded format holds 16 channels, got {tuple(x.shape)}")
    if out is None:
        out = split2d_buffer(N, Hh, W, x.device)
    _check_split2d(out, N, Hh, W, x.device, "out")
    _call("mvsgi_f32_to_split2d", x.data_ptr(), out.data_ptr(), N, Hh, W, _stream_ptr(x))
    return out


def split2d_to_f32(x_split: torch.Tensor) -> torch.Tensor:
    N, Hh, W = _split2d_dims(x_split, "x_split")
    y = torch.empty((N, Hh, W, 16), device=x_split.device, dtype=torch.float32)
    _call("mvsgi_split2d_to_f32", x_split.data_ptr(), y.data_ptr(), N, Hh, W, _stream_ptr(x_split))
    return y


def pack_resblock2d_split_weights(w_oihw: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """Lane-ordered split-bf16 weights of one conv of the block with the BatchNorm scale folded in."""
    lib = _lib.load()
    w = _dev(w_oihw, "w")
    scale = _dev(scale, "scale")
    if tuple(w.shape) != (16, 16, 3, 3) or scale.numel() != 16:
        raise AssertionError(f"resblock2d_split is the 16 -> 16 channel 3x3 block, got weights {tuple(w.shape)}")
    wp = torch.empty(lib.mvsgi_resblock2d_split_packed_weight_bytes(), device=w.device, dtype=torch.uint8)
    _call("mvsgi_resblock2d_split_pack_weights", w.data_ptr(), scale.data_ptr(), wp.data_ptr(), _stream_ptr(w))
    return wp


def resblock2d_split(x_split, wp1, shift1, wp2, shift2, neg_slope=0.01, out_split=None) -> torch.Tensor:
    """Fused 16 -> 16 residual block on a 2-D split-padded input [N, H + 4, W + 4, 64] uint8 (wp1 / wp2 carry the scales).
    out_split: the split-padded buffer that receives the output (returned); None: the output is a plain fp32 [N, H, W, 16]
    tensor."""
    N, Hh, W = _split2d_dims(x_split, "x_split")
    dev = x_split.device
    if out_split is not None:
        _check_split2d(out_split, N, Hh, W, dev)
        y = out_split
    else:
        y = torch.empty((N, Hh, W, 16), device=dev, dtype=torch.float32)
    _call("mvsgi_resblock2d_split", x_split.data_ptr(), _rs2d_packed(wp1, "wp1", dev), _arg(shift1, "shift1", dev, numel=16).data_ptr(),
          _rs2d_packed(wp2, "wp2", dev), _arg(shift2, "shift2", dev, numel=16).data_ptr(), y.data_ptr(),
          int(out_split is not None), N, Hh, W, float(neg_slope), _stream_ptr(x_split))
    return y


def conv2d_s2_split(x_split, w_packed, shift, out_split, neg_slope=0.01) -> torch.Tensor:
    """16 -> 16 channel 3x3 stride-2 layer on 2-D split-padded activations (weights from pack_resblock2d_split_weights)."""
    N, Hh, W = _split2d_dims(x_split, "x_split")
    dev = x_split.device
    _check_split2d(out_split, N, (Hh - 1) // 2 + 1, (W - 1) // 2 + 1, dev)
    _call("mvsgi_conv2d_s2_split", x_split.data_ptr(), _rs2d_packed(w_packed, "w_packed", dev), _arg(shift, "shift", dev, numel=16).data_ptr(),
          out_split.data_ptr(), N, Hh, W, float(neg_slope),
          _stream_ptr(x_split))
    return out_split


def resblock2d(x_nhwc, wp1, scale1, shift1, wp2, scale2, shift2, neg_slope=0.01) -> torch.Tensor:
    """Fused 16 -> 16 residual block (two 3x3 convs + BN + LeakyReLU + skip): x [N, H, W, 16] -> y, same shape."""
    x = _dev(x_nhwc, "x")
    N, Hh, W, C = x.shape
    if C != 16:
        raise AssertionError(f"resblock2d is the 16-channel block, got x {tuple(x.shape)}")
    dev = x.device
    nb = _lib.load().mvsgi_conv2d_packed_weight_bytes_bf16x3(16, 16)
    p1, p2 = (_arg(w, n, dev, torch.uint8, nbytes=nb).data_ptr() for w, n in ((wp1, "wp1"), (wp2, "wp2")))
    (sc1, sh1, _), (sc2, sh2, _) = _scale_shift(scale1, shift1, dev, 16, "1"), _scale_shift(scale2, shift2, dev, 16, "2")
    y = torch.empty_like(x)
    _call("mvsgi_resblock2d_f32", x.data_ptr(), p1, sc1, sh1, p2, sc2,
          sh2, y.data_ptr(), N, Hh, W, float(neg_slope), _stream_ptr(x))
    return y
