"""hip_ops packs every layout of the streaming split kernel through ONE entry point, mvsgi_conv3d_pack_weights_split.  The
library's per-layout bf16 entry points (mvsgi_conv3d_pack_weights_bf16x3 / _bf16x3_c16 / _bf16x3_v32, still part of the C ABI)
must write the same bytes: a weight packed by either is valid for the same kernel."""
import pytest
import torch

from mvs_gi_amd import _lib, hip_ops as H

pytestmark = pytest.mark.gpu

CHANNELS = ((16, 16), (16, 32), (32, 16), (32, 32), (64, 48), (96, 128))      # (cout, cin)


def _dedicated(w, layout):
    """Packed bytes of the bf16 split from the layout's own C symbol (no wrapper of hip_ops in between)."""
    lib = _lib.load()
    cout, cin = w.shape[:2]
    s = torch.cuda.current_stream().cuda_stream
    if layout == H.CONV_BF16X3:
        wp = torch.empty(lib.mvsgi_conv3d_packed_weight_bytes_bf16x3(cout, cin), device=w.device, dtype=torch.uint8)
        _lib.check(lib.mvsgi_conv3d_pack_weights_bf16x3(w.data_ptr(), wp.data_ptr(), cout, cin, s), "mvsgi_conv3d_pack_weights_bf16x3")
    elif layout == H.CONV_BF16X3_C16:
        wp = torch.empty(lib.mvsgi_conv3d_packed_weight_bytes_bf16x3_c16(cin), device=w.device, dtype=torch.uint8)
        _lib.check(lib.mvsgi_conv3d_pack_weights_bf16x3_c16(w.data_ptr(), wp.data_ptr(), cin, s), "mvsgi_conv3d_pack_weights_bf16x3_c16")
    else:
        wp = torch.empty(lib.mvsgi_conv3d_packed_weight_bytes_bf16x3_v32(cout, cin), device=w.device, dtype=torch.uint8)
        _lib.check(lib.mvsgi_conv3d_pack_weights_bf16x3_v32(w.data_ptr(), wp.data_ptr(), cout, cin, s), "mvsgi_conv3d_pack_weights_bf16x3_v32")
    return wp


@pytest.mark.parametrize("cout,cin", CHANNELS)
def test_split_packers_one_entry_point(cout, cin):
    g = torch.Generator().manual_seed(cout * 100 + cin)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * torch.logspace(-3, 3, cout).view(-1, 1, 1, 1, 1)).cuda()
    wrappers = {H.CONV_BF16X3: H.pack_conv_weights_bf16x3, H.CONV_BF16X3_C16: H.pack_conv_weights_bf16x3_c16,
                H.CONV_BF16X3_V32: H.pack_conv_weights_bf16x3_v32, H.CONV_BF16X3_D32: H.pack_conv_weights_bf16x3_d32}
    applies = {H.CONV_BF16X3: True, H.CONV_BF16X3_C16: cout == 16, H.CONV_BF16X3_V32: cout % 32 == 0, H.CONV_BF16X3_D32: cin % 32 == 0}
    for layout, wrapper in wrappers.items():
        got = wrapper(w)
        if not applies[layout]:
            assert got is None and H.pack_conv_weights_f16x3(w, layout) is None
            continue
        assert got.dtype == torch.uint8 and got.is_cuda
        if layout != H.CONV_BF16X3_D32:          # (the 32-channel-slice layout never had a symbol of its own)
            want = _dedicated(w, layout)
            assert got.shape == want.shape and torch.equal(got, want), f"layout {layout}: the two entry points pack different bytes"
        # the fp16 split of the same layout: weights pre-scaled by 2^k per output channel, the inverse returned for the epilogue
        wp16, unscale = H.pack_conv_weights_f16x3(w, layout)
        up, un = H._pow2_unscale(w.abs().amax(dim=(1, 2, 3, 4)))
        assert wp16.shape == got.shape and torch.equal(unscale, un) and torch.equal(up * un, torch.ones_like(up))
        amax = (w * up.view(-1, 1, 1, 1, 1)).abs().amax(dim=(1, 2, 3, 4))
        assert bool(((amax > 512) & (amax <= 1024)).all())
