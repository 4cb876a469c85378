"""The conv3d dispatcher's choices, pinned: tests/golden/conv3d_dispatch_pin.json (tools/make_dispatch_pin.py) holds the variant
mvsgi_conv3d_variant_f32 / mvsgi_conv3d_up2_variant_f32 named for every conv / fused-upsample layer of the BASELINE configurations
at 1 ... 128 frames, in every weight layout that applies and both splits, plus shapes that reach the remaining variants.  Each query
must return the recorded name exactly.  Nothing is launched; the GPU only supplies the CU count the choices depend on."""
import json
import os

import pytest
import torch

import guard_arena
from mvs_gi_amd import _lib, hip_ops as H

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _guarded_allocations(request):
    """Every device tensor the library allocates during a test of this module sits between NaN-sentinel guards, and unwritten
    fp32 outputs read as NaN (tests/guard_arena.py: what is guarded, guard sizes, exemptions)."""
    yield from guard_arena.fixture_body(request)

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3d_dispatch_pin.json")
LAYOUTS = {"auto": H.CONV_AUTO, "generic": H.CONV_BF16X3, "c16": H.CONV_BF16X3_C16, "v32": H.CONV_BF16X3_V32,
           "d32": H.CONV_BF16X3_D32}


def test_conv3d_dispatch_pin():
    with open(PIN) as f:
        pin = json.load(f)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != pin["cus"]:
        pytest.skip(f"the table was recorded on a device of {pin['cus']} CUs, this one has {cus}")
    lib = _lib.load()
    wrong = []
    for fn, B, Cin, D, Hh, W, Cout, stride, layout, split, want in pin["rows"]:
        impl = LAYOUTS[layout] | (H.CONV_F16 if split == "f16" else 0)
        if fn == "conv":
            got = lib.mvsgi_conv3d_variant_f32(B, Cin, D, Hh, W, Cout, stride, impl)
        else:
            got = lib.mvsgi_conv3d_up2_variant_f32(B, Cin, D, Hh, W, Cout, impl)
        got = got.decode() if got else None
        if got != want:
            wrong.append(f"{fn} B={B} Cin={Cin} [{D},{Hh},{W}] Cout={Cout} s={stride} {layout}/{split}: {got} (pinned {want})")
    assert len(pin["rows"]) > 1000 and not wrong, f"{len(wrong)} of {len(pin['rows'])} choices moved:\n" + "\n".join(wrong[:40])
