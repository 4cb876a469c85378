"""The Python-to-C boundary of the volumetric fusion on the GPU: every argument of hip_ops.tsdf_integrate, hip_ops.tsdf_raycast and
dropin.TsdfVolume is refused before a pointer is taken -- CPU tensors, wrong dtypes, ranks and shapes, poses that are not [B, 4, 4],
origins that are not int32 [B, 3], voxel / trunc / w_max <= 0, an empty range window, K outside 1 ... 4096, non-contiguous buffers,
an `out` of the wrong shape, a ray-table reprojector -- the library's own refusals, each before a pointer is used, and the three
checks of tests/test_gpu_argument_forms.py on the rows of tests/argument_cases_tsdf.py (importing that module registers them in
tests/argument_cases.py's table, which the completeness test there reads when it runs)."""
import math

import numpy as np
import pytest
import torch

import abi_header
import argument_cases as AC
import argument_cases_tsdf as ACT
from mvs_gi_amd import dropin, hip_ops as H
from mvs_gi_amd.dropin import sweep_grids as SG
from test_gpu_argument_forms import ERRORS, arena, recorder  # noqa: F401  (fixtures: the guarded allocator, the recording library)
from test_gpu_argument_forms import test_awkward_activations_give_the_same_bits as _awkward_activations_give_the_same_bits
from test_gpu_argument_forms import test_bad_forms_raise_before_any_launch as _bad_forms_raise_before_any_launch

pytestmark = pytest.mark.gpu
DEV = AC.DEV
SYMBOLS = {"tsdf_integrate": "mvsgi_tsdf_integrate_f32", "tsdf_raycast": "mvsgi_tsdf_raycast_f32"}


def test_the_rows_are_in_the_table():
    assert set(ACT.ROWS) == set(SYMBOLS) and all(AC.ROWS[n] is ACT.ROWS[n] for n in ACT.ROWS)
    assert set(SYMBOLS.values()) <= abi_header.launching_symbols() and not set(SYMBOLS.values()) & set(AC.EXEMPT)


@pytest.mark.parametrize("name", sorted(ACT.ROWS))
def test_bad_forms_raise_before_any_launch(name, recorder):  # noqa: F811
    _bad_forms_raise_before_any_launch(name, recorder)


@pytest.mark.parametrize("name", sorted(ACT.ROWS))
def test_awkward_activations_give_the_same_bits(name):
    _awkward_activations_give_the_same_bits(name)


@pytest.mark.parametrize("name", sorted(ACT.ROWS))
def test_the_canonical_call_reaches_its_symbol(name, recorder):  # noqa: F811
    case = AC.ROWS[name]()
    del recorder.launched[:]
    case.fn(**case.args)
    assert recorder.launched == [SYMBOLS[name]], recorder.launched


def _refused(recorder, fn, **changes):  # noqa: F811
    del recorder.launched[:]
    with pytest.raises(ERRORS):
        fn(**changes)
    assert not recorder.launched, (changes, recorder.launched)


def test_integrate_refuses_what_it_cannot_take(recorder):  # noqa: F811
    a = AC.ROWS["tsdf_integrate"]().args

    def call(affine=ACT.AFFINE, voxel=0.25, trunc=0.5, w_max=8.0, r_range=(0.1, 5.0), **kw):
        b = dict(a, **kw)
        return H.tsdf_integrate(b["vol"], b["inv"], b["T"], b["origin"], b["origin_prev"], 96.0, affine, voxel, trunc, w_max, r_range,
                                std=b["std"], mask=b["mask"], r_out=b["r_out"])
    call()
    call(std=None, mask=None, r_out=None)
    call(mask=a["mask"].bool(), inv=a["inv"].unsqueeze(1), std=a["std"].unsqueeze(1), r_range=(0.0, float("inf")))
    assert recorder.launched == ["mvsgi_tsdf_integrate_f32"] * 3
    z = torch.zeros
    for changes in (
            dict(vol=a["vol"][0]), dict(vol=a["vol"][..., :1]), dict(vol=a["vol"].double()), dict(vol=a["vol"].cpu()),
            dict(vol=a["vol"].transpose(1, 2)), dict(vol=a["vol"].cpu().numpy()),
            dict(inv=a["inv"][0]), dict(inv=a["inv"][:1]), dict(inv=a["inv"].cpu()), dict(inv=a["inv"].double()), dict(inv=a["inv"].unsqueeze(2)),
            dict(std=a["std"][:, :5]), dict(std=a["std"].half()), dict(std=a["std"].cpu()),
            dict(mask=a["mask"].int()), dict(mask=a["mask"][:, :, :7]), dict(mask=a["mask"].cpu()),
            dict(T=a["T"][0]), dict(T=a["T"][:1]), dict(T=a["T"][:, :3]), dict(T=a["T"].cpu()), dict(T=a["T"].double()),
            dict(T=z((2, 4, 8), device=DEV)[:, :, ::2]), dict(T=a["T"].cpu().numpy()),
            dict(origin=a["origin"].long()), dict(origin=a["origin"].float()), dict(origin=a["origin"][:1]), dict(origin=a["origin"].cpu()),
            dict(origin=z((2, 4), device=DEV, dtype=torch.int32)), dict(origin_prev=a["origin_prev"].long()),
            dict(origin_prev=z((2, 6), device=DEV, dtype=torch.int32)[:, ::2]), dict(origin_prev=None),
            dict(r_out=z((2, 5, 6, 10, 2), device=DEV)), dict(r_out=z((2, 5, 6, 10), device=DEV, dtype=torch.float64)), dict(r_out=z((2, 5, 6, 10))),
            dict(affine=ACT.AFFINE[:4]), dict(affine=(float("nan"),) + ACT.AFFINE[1:]), dict(affine=None),
            dict(voxel=0.0), dict(voxel=-0.25), dict(voxel=float("nan")), dict(voxel=float("inf")),
            dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("nan")), dict(trunc=1e30),
            dict(w_max=0.0), dict(w_max=float("inf")), dict(w_max=float("nan")),
            dict(r_range=(1.0, 1.0)), dict(r_range=(-0.5, 1.0)), dict(r_range=(float("nan"), 1.0)), dict(r_range=(0.0, float("nan"))), dict(r_range=2.0)):
        _refused(recorder, call, **changes)


def test_raycast_refuses_what_it_cannot_take(recorder):  # noqa: F811
    a = AC.ROWS["tsdf_raycast"]().args

    def call(want=H.TSDF_OUTPUTS, voxel=0.25, t0=0.125, step=0.125, K=10, w_min=1.0, **kw):
        b = dict(a, **kw)
        return H.tsdf_raycast(b["vol"], b["rays"], b["P"], b["origin"], 96.0, voxel, t0, step, K, w_min, want=want, out=b["out"])
    call()
    call(want=("steps",), out=None, t0=0.0, K=1)
    call(K=4096)
    assert recorder.launched == ["mvsgi_tsdf_raycast_f32"] * 3
    z = torch.zeros
    for changes in (
            dict(vol=a["vol"][0]), dict(vol=a["vol"].half()), dict(vol=a["vol"].cpu()), dict(vol=a["vol"][:, :, :, ::2]),
            dict(rays=a["rays"][:2]), dict(rays=a["rays"][0]), dict(rays=a["rays"].cpu()), dict(rays=a["rays"].double()),
            dict(P=a["P"][0]), dict(P=a["P"][:1]), dict(P=a["P"].cpu()), dict(P=a["P"].double()), dict(P=a["P"].cpu().numpy()),
            dict(origin=a["origin"].long()), dict(origin=a["origin"][:1]), dict(origin=a["origin"].cpu()), dict(origin=None),
            dict(voxel=0.0), dict(voxel=float("nan")), dict(t0=-0.1), dict(t0=float("inf")), dict(step=0.0), dict(step=-0.1), dict(step=float("nan")),
            dict(K=0), dict(K=4097), dict(K=2.5), dict(w_min=float("nan")), dict(w_min=float("inf")),
            dict(want=()), dict(want=("inv", "inv")), dict(want=("inv", "vol")),
            dict(out=dict(a["out"], inv=z((2, 8, 6), device=DEV))), dict(out=dict(a["out"], steps=z((2, 6, 8), device=DEV, dtype=torch.int64))),
            dict(out=dict(a["out"], weight=z((2, 6, 8)))), dict(out=dict(a["out"], weight=z((2, 6, 16), device=DEV)[:, :, ::2])),
            dict(out=dict(a["out"], inv=z((3, 6, 8), device=DEV)))):
        _refused(recorder, call, **changes)


def test_the_library_refuses_before_a_pointer_is_used(recorder):  # noqa: F811
    """The real library, called with addresses it never reads: every refusal comes before any of them is used."""
    lib = recorder._real
    fake = 1 << 20                                                       # 16-byte aligned, never dereferenced
    st = torch.cuda.current_stream().cuda_stream
    names_i = ("vol", "inv", "std", "mask", "T", "origin", "origin_prev", "range", "B", "Nx", "Ny", "Nz", "H", "W", "vs", "trunc", "t2", "w_max",
               "r_min", "r_max", "bf", "au", "bu", "av", "bv", "wrap", "stream")
    base_i = [fake, fake, None, None, fake, fake, fake, None, 1, 10, 6, 5, 6, 8, 0.25, 0.5, 0.25, 8.0, 0.0, 5.0, 96.0, 1.0, 0.0, 1.0, 0.0, 0, st]
    names_r = ("vol", "rays", "P", "origin", "inv", "weight", "steps", "B", "Nx", "Ny", "Nz", "H", "W", "inv_vs", "t0", "step", "K", "w_min", "bf",
               "stream")
    base_r = [fake, fake, fake, fake, fake, None, None, 1, 10, 6, 5, 6, 8, 4.0, 0.125, 0.125, 10, 1.0, 96.0, st]

    def run(fn, names, base, **kw):
        args = list(base)
        for k, v in kw.items():
            args[names.index(k)] = v
        return fn(*args), lib.mvsgi_last_error().decode()
    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(vol=None), "null pointer"), (dict(origin_prev=None), "null pointer"), (dict(Nx=0), "non-positive"), (dict(B=0), "non-positive"),
                     (dict(Nx=1 << 11, Ny=1 << 10, Nz=1 << 10), "below 2^31"), (dict(B=1 << 40), "too large"), (dict(H=0), "non-positive"),
                     (dict(H=1 << 25, W=4), "2^24"), (dict(H=1 << 16, W=1 << 15), "below 2^31"),
                     (dict(vs=0.0), "vs ="), (dict(vs=nan), "vs ="), (dict(trunc=0.0), "trunc ="), (dict(t2=inf), "trunc ="), (dict(w_max=0.0), "w_max"),
                     (dict(r_min=-1.0), "r_min"), (dict(r_min=5.0), "r_min"), (dict(r_max=inf), "r_min"), (dict(r_max=nan), "r_min"),
                     (dict(wrap=2), "wrap = 2"), (dict(au=inf), "must be finite"), (dict(bv=nan), "must be finite"),
                     (dict(T=fake + 4), "16-byte aligned"), (dict(std=fake + 8), "16-byte aligned"), (dict(range=fake + 4), "16-byte aligned")):
        status, msg = run(lib.mvsgi_tsdf_integrate_f32, names_i, base_i, **kw)
        assert status == 1 and text in msg, (kw, msg)
    for kw, text in ((dict(rays=None), "null pointer"), (dict(inv=None), "every output is NULL"), (dict(Nz=0), "non-positive"), (dict(W=0), "non-positive"),
                     (dict(K=0), "K = 0"), (dict(K=4097), "K = 4097"), (dict(inv_vs=0.0), "inv_vs"), (dict(inv_vs=nan), "inv_vs"),
                     (dict(t0=-1.0), "t0 ="), (dict(step=0.0), "t0 ="), (dict(step=inf), "t0 ="), (dict(w_min=nan), "w_min"),
                     (dict(P=fake + 8), "16-byte aligned"), (dict(steps=fake + 4), "16-byte aligned"), (dict(B=1 << 40), "too large")):
        status, msg = run(lib.mvsgi_tsdf_raycast_f32, names_r, base_r, **kw)
        assert status == 1 and text in msg, (kw, msg)


def _reprojector(**kw):
    kw.setdefault("long_range", (-math.pi, math.pi))
    kw.setdefault("lat_range", (0.0, math.pi))
    return dropin.Reprojector([SG.EquirectangularSampleGridMaker()], [np.eye(4)], (6, 8), bf=1.0, device=DEV, **kw)


def test_the_volume_refuses_what_it_cannot_take(recorder):  # noqa: F811
    rp = _reprojector()
    table = _reprojector(rays=rp.rays.clone())                           # a bare ray table: no closed-form inverse
    with pytest.raises(ValueError):
        dropin.TsdfVolume(table, (10, 6, 5), 0.25)
    with pytest.raises(ERRORS):
        dropin.TsdfVolume(_reprojector(lat_range=(-math.pi / 2, 0.0)), (10, 6, 5), 0.25)
    v = dropin.TsdfVolume(rp, (10, 6, 5), 0.25)
    inv = torch.rand((2, 6, 8), device=DEV) + 0.5
    std = torch.full_like(inv, 0.01)
    eye = torch.eye(4).repeat(2, 1, 1)
    del recorder.launched[:]                                             # (the reprojectors made their ray tables on the device)
    for call in (lambda: v.integrate(inv.cpu()), lambda: v.integrate(inv.double()), lambda: v.integrate(inv[:, :5]), lambda: v.integrate(inv[0]),
                 lambda: v.integrate(inv, std.cpu()), lambda: v.integrate(inv, std[:1]), lambda: v.integrate(inv, std.half()),
                 lambda: v.integrate(inv, mask=torch.ones((2, 6, 8), device=DEV)), lambda: v.integrate(inv, mask=torch.ones((2, 6, 7), device=DEV, dtype=torch.uint8)),
                 lambda: v.integrate(inv, P=eye[:1]), lambda: v.integrate(inv, P=eye[:, :3]), lambda: v.integrate(inv, P=eye.double()),
                 lambda: v.integrate(inv, P=torch.eye(3)), lambda: v.integrate(inv, r_out=torch.zeros((2, 5, 6, 9), device=DEV)),
                 lambda: v.raycast(want=("inv", "nothing")), lambda: v.raycast(want=()), lambda: v.raycast(P=torch.eye(3)), lambda: v.raycast(P=eye.double()),
                 lambda: v.set_pose(torch.eye(3)), lambda: v.set_pose(eye.double()), lambda: v.set_pose(eye, B=3)):
        with pytest.raises(ERRORS):
            call()
    assert not recorder.launched
    v.integrate(inv, std, P=eye)
    v.integrate(inv.unsqueeze(1), std.unsqueeze(1), mask=torch.ones((2, 6, 8), device=DEV, dtype=torch.bool))
    v.raycast(B=2)
    v.raycast(P=torch.eye(4), B=2, want=("inv",))
    assert recorder.launched == ["mvsgi_tsdf_integrate_f32"] * 2 + ["mvsgi_tsdf_raycast_f32"] * 2
