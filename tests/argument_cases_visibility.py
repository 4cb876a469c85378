"""The rows of tests/argument_cases.py's table for the entry points of csrc/visibility.hip and for the photometric consistency with
cam_seen: one canonical call each, the role of every tensor argument, and the forms their wrappers refuse by design.

They live in a file of their own because the table's file is kept as it is; importing this module REGISTERS them in the table
(argument_cases.ROWS and argument_cases.REFUSED, through argument_cases.row), which is what
tests/test_gpu_argument_forms.py::test_every_launching_symbol_has_a_row reads when it runs.  tests/test_gpu_argument_forms_visibility.py
imports this module -- so a run that collects it has the rows -- and walks them with the table's own three checks; a run of
tests/test_gpu_argument_forms.py ALONE does not see them, and its completeness test then names the three symbols as missing.

camera_range's mask and photo_consistency's cam_seen are read in place like photo_consistency's mask (hip_ops._cloud_plane): a
non-contiguous one is refused, and so is one that is not 4-byte aligned on these maps (W % 4 == 0: read as words).
"""
import numpy as np

import argument_cases as AC
from mvs_gi_amd import hip_ops as H

ROWS = {}
REFUSED = {}
for _row, _argument in (("camera_range", "mask"), ("photo_consistency_seen", "mask"), ("photo_consistency_seen", "cam_seen")):
    for _form in ("transposed", "expand"):
        REFUSED[(_row, _argument, _form)] = f"{_row}'s {_argument} is read in place (hip_ops._cloud_plane)"
    REFUSED[(_row, _argument, "offset")] = f"{_row}'s {_argument} must be 4-byte aligned when W % 4 == 0 (read as words)"
AC.REFUSED.update(REFUSED)


def row(fn):
    ROWS[fn.__name__] = fn
    return AC.row(fn)


def _map(name):
    a = AC._view(name)
    del a["imgs"]
    return a


@row
def camera_range():
    a = _map("camera_range")
    T, cams = AC._cams(2)
    a.update(mask=AC._g(AC._rng("camera_range/mask").random((2, 6, 8)) < 0.8), out=AC._empty(2, 2, 12, 8))
    return AC._case(lambda **a: H.camera_range(a["inv"], a["rays"], T, cams, 96.0, (12, 8), mask=a["mask"], footprint=2, out=a["out"]), a,
                    dict(inv="act", rays="act", mask="mask", out="out"))


@row
def visibility():
    a = _map("visibility")
    T, cams = AC._cams(2)
    a.update(z2=H.camera_range(a["inv"], a["rays"], T, cams, 96.0, (12, 8)))          # its own row's entry point makes the buffer
    return AC._case(lambda **a: H.visibility(a["inv"], a["rays"], T, cams, 96.0, a["z2"]), a, dict(inv="act", rays="act", z2="param"))


@row
def photo_consistency_seen():
    rng = AC._rng("photo_consistency_seen")
    a = AC._view("photo_consistency_seen")
    T, cams = AC._cams(2)
    a.update(cam_masks=AC._g((rng.random((2, 1, 8, 12)) < 0.9).astype(np.float32)), mask=AC._g(rng.random((2, 6, 8)) < 0.8),
             cam_seen=AC._g(rng.random((2, 2, 6, 8)) < 0.7))
    return AC._case(lambda **a: H.photo_consistency(a["inv"], a["rays"], T, cams, 96.0, a["imgs"], cam_masks=a["cam_masks"], mask=a["mask"],
                                                    cam_seen=a["cam_seen"]), a,
                    dict(inv="act", rays="act", imgs="act", cam_masks="act", mask="mask", cam_seen="mask"))
