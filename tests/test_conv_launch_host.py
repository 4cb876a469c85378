"""The lowering rule of dropin.common_modules.ConvLaunch, on the CPU: which layout / weights / scale reach hip_ops.conv3d,
conv3d_up2 and conv3d_up2_out_split in every mode, with the packers and launchers replaced by recorders.

The expected tables are literals, read off ConvLaunch._run_conv / _run_up2 / run_up2_split as they stood before the class got
its constructor and single cache (commit 57b703b): plane schedule if Cout == 16 (stride 1), else 32-channel slices if the library
says they apply (Cin % 32 == 0; stride 1 and Cout % 16 == 0 for the plain conv), else tap pairs; CONV_AUTO with the exact-fp32
weights outside the split modes or with channel counts that are not multiples of 16.
"""
import pytest
import torch

from mvs_gi_amd import hip_ops as H
from mvs_gi_amd.dropin import common_modules as cm

AUTO, B3, C16, D32, F16 = H.CONV_AUTO, H.CONV_BF16X3, H.CONV_BF16X3_C16, H.CONV_BF16X3_D32, H.CONV_F16
MODES = ("f16x3", "bf16x3", "f32")
COMBOS = ((16, 16, 1), (32, 16, 1), (32, 32, 1), (64, 64, 1), (64, 128, 2), (48, 96, 1), (24, 16, 1))

# (cin, cout, stride) -> (layout with the library's D32 answer False, with the answer True, whether the library is asked)
RUN_SPLIT = {(16, 16, 1): (C16, C16, False),
             (32, 16, 1): (C16, C16, False),
             (32, 32, 1): (B3, D32, True),
             (64, 64, 1): (B3, D32, True),
             (64, 128, 2): (B3, B3, False),        # stride 2: never asked
             (48, 96, 1): (B3, B3, False),         # Cin % 32 != 0: never asked
             (24, 16, 1): (None, None, False)}     # not multiples of 16: CONV_AUTO, exact-fp32 weights
# the fused upsample + conv (stride-1 layers with multiples of 16, ConvLaunch.can_fuse_up2's domain)
UP2_SPLIT = {(16, 16, 1): (C16, C16, False),
             (32, 16, 1): (C16, C16, False),
             (32, 32, 1): (B3, D32, True),
             (64, 64, 1): (B3, D32, True),
             (48, 96, 1): (B3, B3, False)}
UP2_OUT_SPLIT = {(16, 16, 1): C16, (32, 16, 1): C16, (32, 32, 1): B3, (64, 64, 1): B3, (48, 96, 1): B3}      # never D32
UNSCALE = 0.25


class Recorder:
    def __init__(self, monkeypatch, d32_answer: bool):
        self.packs, self.queries, self.up2_queries, self.launches = [], [], [], []
        self.d32_answer = d32_answer
        monkeypatch.setattr(cm, "_D32_OK", {})
        monkeypatch.setattr(cm, "_USE_D32", True)
        monkeypatch.setattr(H, "pack_conv_weights", lambda w: ("exact", id(w)))
        monkeypatch.setattr(H, "_pack_conv3d_split", self.pack)
        for name in ("pack_conv_weights_bf16x3", "pack_conv_weights_f16x3", "pack_conv_weights_bf16x3_d32", "pack_conv_weights_bf16x3_v32",
                     "pack_conv_weights_bf16x3_c16"):
            monkeypatch.setattr(H, name, self.unexpected)
        monkeypatch.setattr(H, "conv3d_d32_applies", self.applies)
        monkeypatch.setattr(H, "conv3d_up2_d32_applies", self.up2_applies)
        monkeypatch.setattr(H, "conv3d", self.conv3d)
        monkeypatch.setattr(H, "conv3d_up2", self.conv3d_up2)
        monkeypatch.setattr(H, "conv3d_up2_out_split", self.conv3d_up2_out_split)
        self.mode = H.get_conv_mode()
        monkeypatch.setattr(H, "_CONV_MODE", self.mode)       # restored at teardown; set_conv_mode below writes it

    def unexpected(self, *a, **k):
        raise AssertionError("ConvLaunch packs the streaming kernel's weights through hip_ops._pack_conv3d_split alone")

    def pack(self, w, layout, fmt="bf16"):
        self.packs.append((id(w), layout, fmt))
        wp = ("packed", id(w), layout, fmt)
        return wp, (torch.full((w.shape[0],), UNSCALE) if fmt == "f16" else None)

    def applies(self, B, cin, D, Hh, W, cout, stride=1):
        self.queries.append((B, cin, D, Hh, W, cout, stride))
        return self.d32_answer

    def up2_applies(self, B, cin, D, Hh, W, cout):
        self.up2_queries.append((B, cin, D, Hh, W, cout))
        return self.d32_answer

    def conv3d(self, x, w_oidhw, w_packed, scale, shift, res=None, stride=1, neg_slope=0.01, impl=H.CONV_AUTO, out=None):
        self.launches.append(dict(fn="conv3d", w=w_oidhw, wp=w_packed, scale=scale, shift=shift, stride=stride, impl=impl))
        return "y"

    def conv3d_up2(self, x, w_packed_b3, scale, shift, res=None, neg_slope=0.01, out=None, w_layout=H.CONV_BF16X3):
        self.launches.append(dict(fn="conv3d_up2", wp=w_packed_b3, scale=scale, shift=shift, impl=w_layout))
        return "y"

    def conv3d_up2_out_split(self, x, w_packed_b3, scale, shift, out, res=None, neg_slope=0.01, w_layout=H.CONV_BF16X3):
        self.launches.append(dict(fn="conv3d_up2_out_split", wp=w_packed_b3, scale=scale, shift=shift, impl=w_layout))
        return out


def make_launch(cin, cout, stride):
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g)
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    return cm.ConvLaunch(w, scale, shift, stride, 0.01, None, ("key", cin, cout, stride))


def x_of(L, B=1, D=2, Hh=4, W=8):
    return torch.zeros(B, D, Hh, W, L.cin)


def check_weights_and_scale(call, L, layout, fmt):
    """The launch got the weights packed for (layout, fmt) and the scale that goes with them."""
    assert call["wp"] == ("packed", id(L.w), layout, fmt)
    assert call["shift"] is L.shift
    if fmt == "f16":
        assert call["scale"] is not L.scale and torch.equal(call["scale"], L.scale * UNSCALE)      # scale * unscale
    else:
        assert call["scale"] is L.scale                                                          # the very tensor


@pytest.mark.parametrize("d32_answer", [False, True])
@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("mode", MODES)
def test_run_layout_rule(monkeypatch, mode, combo, d32_answer):
    rec = Recorder(monkeypatch, d32_answer)
    H.set_conv_mode(mode)
    L = make_launch(*combo)
    assert L.wp == ("exact", id(L.w)) and not rec.packs          # the exact-fp32 layout is packed eagerly, nothing else
    shapes = [(1, 2, 4, 8), (3, 2, 4, 8)]
    for _ in range(3):
        for s in shapes:
            L.run(x_of(L, *s))
    layout_no, layout_yes, asked = RUN_SPLIT[combo]
    layout = layout_yes if d32_answer else layout_no
    assert len(rec.launches) == 6 and all(c["fn"] == "conv3d" and c["w"] is L.w and c["stride"] == combo[2] for c in rec.launches)
    if mode == "f32" or layout is None:
        assert not rec.packs and not rec.queries
        for c in rec.launches:
            assert c["impl"] == AUTO and c["wp"] == ("exact", id(L.w)) and c["scale"] is L.scale and c["shift"] is L.shift
        return
    fmt = "f16" if mode == "f16x3" else "bf16"
    for c in rec.launches:
        assert c["impl"] == (layout | F16 if fmt == "f16" else layout)
        check_weights_and_scale(c, L, layout, fmt)
    assert rec.packs == [(id(L.w), layout, fmt)]                                       # packed exactly once
    cin, cout, stride = combo
    assert rec.queries == ([(s[0], cin) + s[1:] + (cout, stride) for s in shapes] if asked else [])      # once per launch shape
    assert not rec.up2_queries


@pytest.mark.parametrize("d32_answer", [False, True])
@pytest.mark.parametrize("combo", sorted(UP2_SPLIT))
@pytest.mark.parametrize("mode", MODES)
def test_run_up2_layout_rule(monkeypatch, mode, combo, d32_answer):
    rec = Recorder(monkeypatch, d32_answer)
    H.set_conv_mode(mode)
    L = make_launch(*combo)
    shapes = [(1, 2, 4, 8), (2, 2, 4, 16)]
    for _ in range(3):
        for s in shapes:
            L.run_up2(x_of(L, *s))
    layout_no, layout_yes, asked = UP2_SPLIT[combo]
    # outside the split modes the fused launch never takes the 32-channel slices (it runs in the bf16 split)
    layout = layout_yes if (d32_answer and mode != "f32") else layout_no
    fmt = "f16" if mode == "f16x3" else "bf16"
    assert len(rec.launches) == 6
    for c in rec.launches:
        assert c["fn"] == "conv3d_up2" and c["impl"] == (layout | F16 if fmt == "f16" else layout)
        check_weights_and_scale(c, L, layout, fmt)
    assert rec.packs == [(id(L.w), layout, fmt)]
    cin, cout, _ = combo
    if mode != "f32":          # (asked with the LOW-resolution sizes, through mvsgi_conv3d_up2_d32_applies)
        assert rec.up2_queries == ([(s[0], cin) + s[1:] + (cout,) for s in shapes] if asked else [])
    assert not rec.queries


@pytest.mark.parametrize("d32_answer", [False, True])
@pytest.mark.parametrize("combo", sorted(UP2_OUT_SPLIT))
@pytest.mark.parametrize("mode", ("f16x3", "bf16x3"))
def test_run_up2_split_never_selects_d32(monkeypatch, mode, combo, d32_answer):
    rec = Recorder(monkeypatch, d32_answer)
    H.set_conv_mode(mode)
    L = make_launch(*combo)
    for _ in range(3):
        assert L.run_up2_split(x_of(L), None, "out") == "out"
    layout, fmt = UP2_OUT_SPLIT[combo], ("f16" if mode == "f16x3" else "bf16")
    for c in rec.launches:
        assert c["fn"] == "conv3d_up2_out_split" and c["impl"] == (layout | F16 if fmt == "f16" else layout)
        check_weights_and_scale(c, L, layout, fmt)
    assert rec.packs == [(id(L.w), layout, fmt)] and not rec.queries and not rec.up2_queries


@pytest.mark.parametrize("mode", MODES)
def test_explicit_impl_bypasses_the_rule(monkeypatch, mode):
    rec = Recorder(monkeypatch, True)
    H.set_conv_mode(mode)
    L = make_launch(64, 64, 1)
    L.run(x_of(L), impl=H.CONV_BF16X3)         # the tap-pair layout in the bf16 split, whatever the mode
    L.run(x_of(L), impl=H.CONV_MFMA)           # any other selector: the exact-fp32 weights
    L.run(x_of(L), impl=H.CONV_DIRECT)
    a, b, c = rec.launches
    assert a["impl"] == B3 and a["wp"] == ("packed", id(L.w), B3, "bf16") and a["scale"] is L.scale
    assert b["impl"] == H.CONV_MFMA and b["wp"] == ("exact", id(L.w)) and b["scale"] is L.scale
    assert c["impl"] == H.CONV_DIRECT and c["wp"] == ("exact", id(L.w)) and c["scale"] is L.scale
    assert rec.packs == [(id(L.w), B3, "bf16")] and not rec.queries


def test_each_mode_keeps_its_own_weights_across_switches(monkeypatch):
    rec = Recorder(monkeypatch, True)
    L = make_launch(32, 32, 1)
    seq = ["f16x3", "bf16x3", "f32", "f16x3", "bf16x3", "f32", "f16x3"]
    for mode in seq:
        H.set_conv_mode(mode)
        L.run(x_of(L))
        if mode != "f32":
            L.run_up2(x_of(L))
            L.run_up2_split(x_of(L), None, "out")
    it = iter(rec.launches)
    for mode in seq:
        c = next(it)
        if mode == "f32":
            assert c["impl"] == AUTO and c["wp"] == ("exact", id(L.w)) and c["scale"] is L.scale
            continue
        fmt, flag = ("f16", F16) if mode == "f16x3" else ("bf16", 0)
        assert c["impl"] == D32 | flag
        check_weights_and_scale(c, L, D32, fmt)
        c = next(it)
        assert c["fn"] == "conv3d_up2" and c["impl"] == D32 | flag
        check_weights_and_scale(c, L, D32, fmt)
        c = next(it)
        assert c["fn"] == "conv3d_up2_out_split" and c["impl"] == B3 | flag
        check_weights_and_scale(c, L, B3, fmt)
    # one pack per (layout, split) over all the switches, one query per (kernel, launch shape)
    assert sorted(rec.packs) == sorted((id(L.w), lay, fmt) for lay in (D32, B3) for fmt in ("f16", "bf16"))
    assert len(rec.queries) == 1 and len(rec.up2_queries) == 1
