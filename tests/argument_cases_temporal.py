"""The rows of tests/argument_cases.py's table for the entry points of csrc/temporal.hip: one canonical call each and the role of
every tensor argument.

They live in a file of their own because the table's file is kept as it is; importing this module REGISTERS them in the table
(argument_cases.ROWS, through argument_cases.row), which is what tests/test_gpu_argument_forms.py::
test_every_launching_symbol_has_a_row reads when it runs.  tests/test_gpu_temporal_args.py imports this module -- so a run that
collects it has the rows -- and walks them with the table's own three checks; a run of tests/test_gpu_argument_forms.py ALONE does
not see them, and its completeness test then names the two symbols as missing.

The state (prev_inv, prev_var, prev_age), the pose T and zkey are caller-owned buffers read in place (hip_ops._arg: any awkward form
is refused); the rays and the measurement (cur_inv, cur_std) are activations (hip_ops._dev: an awkward form is copied).
"""
import math

import numpy as np
import torch

import argument_cases as AC
from mvs_gi_amd import hip_ops as H

ROWS = {}
AFFINE = H.temporal_affine((-math.pi, math.pi), (0.0, math.pi), (6, 8))


def row(fn):
    ROWS[fn.__name__] = fn
    return AC.row(fn)


def _state(name, B=2):
    rng = AC._rng(name)
    lat, lon = np.meshgrid((np.arange(6) + 0.5) / 6 * math.pi, (np.arange(8) + 0.5) / 8 * 2 * math.pi - math.pi, indexing="ij")
    rays = np.stack([np.sin(lat) * np.cos(lon), -np.cos(lat), -np.sin(lat) * np.sin(lon)]).astype(np.float32)
    inv = rng.uniform(8.0, 48.0, (B, 6, 8)).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, :3, 3] = rng.uniform(-0.3, 0.3, (B, 3))
    return dict(prev_inv=AC._g(inv), prev_var=AC._g(np.square(0.03 * inv).astype(np.float32)),
                prev_age=AC._g(rng.integers(0, 4, (B, 6, 8)).astype(np.uint8)), rays=AC._g(rays), T=AC._g(T))


@row
def temporal_splat():
    a = _state("temporal_splat")
    del a["prev_var"]
    a.update(out=AC._empty(2, 6, 8, dtype=torch.int64))
    return AC._case(lambda **a: H.temporal_splat(a["prev_inv"], a["prev_age"], a["rays"], a["T"], 96.0, AFFINE, out=a["out"]), a,
                    dict(prev_inv="param", prev_age="param", rays="act", T="param", out="out"))


@row
def temporal_fuse():
    rng = AC._rng("temporal_fuse/measurement")
    a = _state("temporal_fuse")
    a.update(zkey=H.temporal_splat(a["prev_inv"], a["prev_age"], a["rays"], a["T"], 96.0, AFFINE))      # its own row's entry point makes the buffer
    del a["rays"], a["T"]
    cur = (a["prev_inv"].cpu().numpy() * rng.uniform(0.9, 1.1, (2, 6, 8))).astype(np.float32)
    kinds = dict(fused=torch.float32, var=torch.float32, age=torch.uint8, warped_inv=torch.float32, warped_var=torch.float32, src=torch.int32)
    a.update(cur_inv=AC._g(cur), cur_std=AC._g((0.02 * cur).astype(np.float32)), out={k: AC._empty(2, 6, 8, dtype=d) for k, d in kinds.items()})
    roles = dict(zkey="param", prev_inv="param", prev_var="param", prev_age="param", cur_inv="act", cur_std="act")
    roles.update({f"out/{k}": "out" for k in kinds})
    return AC._case(lambda **a: H.temporal_fuse(a["zkey"], a["prev_inv"], a["prev_var"], a["prev_age"], a["cur_inv"], 96.0, q_var=1e-6,
                                                cur_std=a["cur_std"], out=a["out"]), a, roles)
