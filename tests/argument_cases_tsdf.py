"""The rows of tests/argument_cases.py's table for the entry points of csrc/tsdf.hip: one canonical call each and the role of every
tensor argument.

They live in a file of their own because the table's file is kept as it is; importing this module REGISTERS them in the table
(argument_cases.ROWS, through argument_cases.row), which is what tests/test_gpu_argument_forms.py::
test_every_launching_symbol_has_a_row reads when it runs.  tests/test_gpu_tsdf_args.py imports this module -- so a run that collects
it has the rows -- and walks them with the table's own three checks; a run of tests/test_gpu_argument_forms.py ALONE does not see
them, and its completeness test then names the two symbols as missing.

The volume, the poses T / P, the origins and the optional range output are caller-owned buffers used in place (hip_ops._arg: any
awkward form is refused); the measurement (inv, std, mask) and the rays are activations (hip_ops._dev: an awkward form is copied).
"""
import math

import numpy as np
import torch

import argument_cases as AC
from mvs_gi_amd import hip_ops as H

ROWS = {}
HW, DIMS, VOXEL = (6, 8), (10, 6, 5), 0.25
AFFINE = H.temporal_affine((-math.pi, math.pi), (0.0, math.pi), HW)


def row(fn):
    ROWS[fn.__name__] = fn
    return AC.row(fn)


def _rays():
    lat, lon = np.meshgrid((np.arange(HW[0]) + 0.5) / HW[0] * math.pi, (np.arange(HW[1]) + 0.5) / HW[1] * 2 * math.pi - math.pi, indexing="ij")
    return np.stack([np.sin(lat) * np.cos(lon), -np.cos(lat), -np.sin(lat) * np.sin(lon)]).astype(np.float32)


def _volume(name, B=2):
    rng = AC._rng(name)
    Nx, Ny, Nz = DIMS
    vol = np.empty((B, Nz, Ny, Nx, 2), np.float32)
    vol[..., 0] = rng.uniform(-1.0, 1.0, vol.shape[:-1])
    vol[..., 1] = rng.uniform(0.0, 4.0, vol.shape[:-1])
    pose = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    pose[:, :3, 3] = rng.uniform(-0.3, 0.3, (B, 3))
    origin = np.tile(np.asarray([-5, -3, -2], np.int32), (B, 1))
    return dict(vol=AC._g(vol), pose=AC._g(pose), origin=AC._g(origin))


@row
def tsdf_integrate():
    rng = AC._rng("tsdf_integrate/measurement")
    a = _volume("tsdf_integrate")
    inv = (96.0 / rng.uniform(0.4, 1.4, (2,) + HW)).astype(np.float32)
    a.update(T=a.pop("pose"), origin_prev=AC._g(np.tile(np.asarray([-6, -3, -1], np.int32), (2, 1))), inv=AC._g(inv),
             std=AC._g((0.2 * inv).astype(np.float32)), mask=AC._g((rng.uniform(size=inv.shape) > 0.2).astype(np.uint8)),
             r_out=AC._empty(2, DIMS[2], DIMS[1], DIMS[0]))
    return AC._case(lambda **a: H.tsdf_integrate(a["vol"], a["inv"], a["T"], a["origin"], a["origin_prev"], 96.0, AFFINE, VOXEL, 2 * VOXEL, 8.0,
                                                 (0.1, 5.0), std=a["std"], mask=a["mask"], r_out=a["r_out"]), a,
                    dict(vol="out", inv="act", std="act", mask="mask", T="param", origin="param", origin_prev="param", r_out="out"))


@row
def tsdf_raycast():
    a = _volume("tsdf_raycast")
    kinds = dict(inv=torch.float32, weight=torch.float32, steps=torch.int32)
    a.update(P=a.pop("pose"), rays=AC._g(_rays()), out={k: AC._empty(2, *HW, dtype=d) for k, d in kinds.items()})
    roles = dict(vol="param", rays="act", P="param", origin="param")
    roles.update({f"out/{k}": "out" for k in kinds})
    return AC._case(lambda **a: H.tsdf_raycast(a["vol"], a["rays"], a["P"], a["origin"], 96.0, VOXEL, 0.125, 0.125, 10, out=a["out"]), a, roles)
