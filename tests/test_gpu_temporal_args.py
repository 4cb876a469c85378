"""The Python-to-C boundary of the temporal fusion on the GPU: every argument of hip_ops.temporal_splat, hip_ops.temporal_fuse and
dropin.TemporalFusion is refused before a pointer is taken -- CPU tensors, wrong dtypes, ranks and shapes, a T that is not [B, 4, 4],
meas_std <= 0, gate <= 0, q_var < 0, non-contiguous buffers, an `out` of the wrong shape, a ray-table reprojector, H * W >= 2^32 --
and the three checks of tests/test_gpu_argument_forms.py run on the rows of tests/argument_cases_temporal.py (importing that module
registers them in tests/argument_cases.py's table, which the completeness test there reads when it runs)."""
import math

import numpy as np
import pytest
import torch

import abi_header
import argument_cases as AC
import argument_cases_temporal as ACT
from mvs_gi_amd import _lib, dropin, hip_ops as H
from mvs_gi_amd.dropin import sweep_grids as SG
from test_gpu_argument_forms import ERRORS, arena, recorder  # noqa: F401  (fixtures: the guarded allocator, the recording library)
from test_gpu_argument_forms import test_awkward_activations_give_the_same_bits as _awkward_activations_give_the_same_bits
from test_gpu_argument_forms import test_bad_forms_raise_before_any_launch as _bad_forms_raise_before_any_launch

pytestmark = pytest.mark.gpu
DEV = AC.DEV
SYMBOLS = {"temporal_splat": "mvsgi_temporal_splat_f32", "temporal_fuse": "mvsgi_temporal_fuse_f32"}


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
    assert recorder.launched[-1] == SYMBOLS[name], recorder.launched


def _refused(recorder, fn, **changes):  # noqa: F811
    del recorder.launched[:]
    with pytest.raises(ERRORS):
        fn(**changes)
    assert not recorder.launched, recorder.launched


def test_splat_refuses_what_it_cannot_take(recorder):  # noqa: F811
    case = AC.ROWS["temporal_splat"]()
    a = case.args

    def call(affine=ACT.AFFINE, **kw):
        b = dict(a, **kw)
        return H.temporal_splat(b["prev_inv"], b["prev_age"], b["rays"], b["T"], 96.0, affine, out=b["out"])
    call()
    assert recorder.launched == ["mvsgi_temporal_splat_f32"]
    z = torch.zeros
    for changes in (
            dict(prev_inv=a["prev_inv"][0]), dict(prev_inv=a["prev_inv"].unsqueeze(1)),                         # ranks
            dict(prev_age=a["prev_age"].bool()), dict(prev_age=a["prev_age"][:, :5]), dict(prev_age=a["prev_age"][:1]),
            dict(rays=a["rays"][:2]), dict(rays=a["rays"][:, :5]), dict(rays=a["rays"].cpu()), dict(rays=a["rays"].double()),
            dict(T=a["T"][0]), dict(T=a["T"][:1]), dict(T=a["T"][:, :3]), dict(T=a["T"].cpu()), dict(T=a["T"].double()),
            dict(T=z((2, 4, 8), device=DEV)[:, :, ::2]), dict(T=a["T"].cpu().numpy()),                         # strided; not a tensor
            dict(out=z((2, 6, 8), device=DEV, dtype=torch.int32)), dict(out=z((2, 8, 6), device=DEV, dtype=torch.int64)),
            dict(out=z((3, 6, 8), device=DEV, dtype=torch.int64)), dict(out=z((2, 6, 16), device=DEV, dtype=torch.int64)[:, :, ::2]),
            dict(affine=ACT.AFFINE[:4]), dict(affine=(float("nan"),) + ACT.AFFINE[1:]), dict(affine=None)):
        _refused(recorder, call, **changes)


def test_fuse_refuses_what_it_cannot_take(recorder):  # noqa: F811
    case = AC.ROWS["temporal_fuse"]()
    a = case.args

    def call(want=H.TEMPORAL_OUTPUTS, **kw):
        b = dict(a, **{k: v for k, v in kw.items() if k in a})
        more = {k: v for k, v in kw.items() if k not in a}
        more.setdefault("cur_std", b["cur_std"])
        return H.temporal_fuse(b["zkey"], b["prev_inv"], b["prev_var"], b["prev_age"], b["cur_inv"], 96.0, want=want, out=b["out"], **more)
    del recorder.launched[:]                                             # (the row's builder made zkey through temporal_splat)
    call()
    assert recorder.launched == ["mvsgi_temporal_fuse_f32"]
    z = torch.zeros
    for changes in (
            dict(zkey=a["zkey"].int()), dict(zkey=a["zkey"][:1]), dict(zkey=a["zkey"].cpu()), dict(zkey=a["zkey"].transpose(1, 2)),
            dict(prev_var=a["prev_var"][:, :5]), dict(prev_var=a["prev_var"].half()), dict(prev_age=a["prev_age"].int()),
            dict(cur_inv=a["cur_inv"][0]), dict(cur_inv=a["cur_inv"][:, :5]), dict(cur_inv=a["cur_inv"].cpu()), dict(cur_inv=a["cur_inv"].double()),
            dict(cur_inv=a["cur_inv"].unsqueeze(2)),
            dict(cur_std=a["cur_std"][:1]), dict(cur_std=a["cur_std"].cpu()), dict(cur_std=a["cur_std"].half()),
            dict(cur_std=None), dict(cur_std=None, meas_std=0.0), dict(cur_std=None, meas_std=-1.0), dict(cur_std=None, meas_std=float("inf")),
            dict(cur_std=None, meas_std=float("nan")), dict(meas_std=0.1),                                      # both given
            dict(gate=0.0), dict(gate=-3.0), dict(gate=float("inf")), dict(gate=float("nan")),
            dict(q_var=-1e-9), dict(q_var=float("inf")), dict(q_var=float("nan")),
            dict(want=()), dict(want=("fused", "fused")), dict(want=("fused", "zkey")),
            dict(out=dict(a["out"], fused=z((2, 8, 6), device=DEV))), dict(out=dict(a["out"], age=z((2, 6, 8), device=DEV, dtype=torch.int8))),
            dict(out=dict(a["out"], src=z((2, 6, 8), device=DEV, dtype=torch.int64))), dict(out=dict(a["out"], var=z((2, 6, 8)))),
            dict(out=dict(a["out"], var=z((2, 6, 16), device=DEV)[:, :, ::2])),
            dict(out=dict(a["out"], fused=a["prev_inv"])), dict(out=dict(a["out"], age=a["prev_age"]))):        # an output that is the state
        _refused(recorder, call, **changes)
    del recorder.launched[:]
    call(cur_std=None, meas_std=0.1)                                                                           # the scalar form
    assert recorder.launched == ["mvsgi_temporal_fuse_f32"]


def test_maps_whose_index_does_not_fit_a_key_are_refused(recorder):  # noqa: F811
    """H * W >= 2^32: refused by the wrapper's own check of the shape, and by the library before any pointer is used (the real
    library, called with addresses it never reads)."""
    for shape in ((1, 1 << 16, 1 << 16), (1, 1 << 25, 4), (1, 4, 1 << 25)):
        with pytest.raises(ValueError):
            H._pano_map("temporal fusion", 32, *shape)
    H._pano_map("temporal fusion", 32, 1, 1 << 16, (1 << 16) - 1)
    with pytest.raises(ValueError):
        H._pano_map("temporal fusion", 32, 1 << 20, 1 << 12, 1 << 12)      # too many blocks for one launch
    lib = recorder._real
    fake = 1 << 20                                                       # 16-byte aligned, never dereferenced: the dimensions are checked first
    st = torch.cuda.current_stream().cuda_stream
    for Hh, W, text in ((1 << 16, 1 << 16, "below 2^32"), (1 << 25, 4, "2^24"), (0, 8, "non-positive")):
        assert lib.mvsgi_temporal_splat_f32(fake, fake, fake, fake, fake, 1, Hh, W, 96.0, 1.0, 0.0, 1.0, 0.0, 0, st) == 1
        assert text in lib.mvsgi_last_error().decode()
        assert lib.mvsgi_temporal_fuse_f32(fake, fake, fake, fake, fake, None, 0.1, fake, None, None, None, None, None, 1, Hh, W, 96.0, 9.0,
                                           0.0, st) == 1
        assert text in lib.mvsgi_last_error().decode()
    # and the other refusals of the library itself, each before a pointer is used
    for args, text in (((None, fake, fake, fake, fake, 1, 6, 8, 96.0, 1.0, 0.0, 1.0, 0.0, 0, st), "null pointer"),
                       ((fake, fake, fake, fake, fake, 1, 6, 8, 96.0, 1.0, 0.0, 1.0, 0.0, 2, st), "wrap = 2"),
                       ((fake, fake, fake, fake, fake, 1, 6, 8, 96.0, float("inf"), 0.0, 1.0, 0.0, 0, st), "must be finite"),
                       ((fake, fake, fake, fake + 4, fake, 1, 6, 8, 96.0, 1.0, 0.0, 1.0, 0.0, 0, st), "16-byte aligned")):
        assert lib.mvsgi_temporal_splat_f32(*args) == 1 and text in lib.mvsgi_last_error().decode(), text
    base = [fake, fake, fake, fake, fake, None, 0.1, fake + 4096, None, None, None, None, None, 1, 6, 8, 96.0, 9.0, 0.0, st]

    def fuse(**kw):
        names = ("zkey", "prev_inv", "prev_var", "prev_age", "cur_inv", "cur_std", "meas_std", "fused", "var", "age", "warped_inv", "warped_var",
                 "src", "B", "H", "W", "bf", "gate2", "q_var", "stream")
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.mvsgi_temporal_fuse_f32(*a), lib.mvsgi_last_error().decode()
    for kw, text in ((dict(zkey=None), "null pointer"), (dict(fused=None), "every output is NULL"), (dict(gate2=0.0), "gate2"),
                     (dict(gate2=float("nan")), "gate2"), (dict(q_var=-1.0), "q_var"), (dict(meas_std=0.0), "meas_std"),
                     (dict(src=fake + 8), "16-byte aligned"), (dict(var=fake), "aliases the state")):
        status, msg = fuse(**kw)
        assert status == 1 and text in msg, (kw, msg)


def _reprojector(**kw):
    kw.setdefault("long_range", (-math.pi, math.pi))
    kw.setdefault("lat_range", (0.0, math.pi))
    return dropin.Reprojector([SG.EquirectangularSampleGridMaker()], [np.eye(4)], (6, 8), bf=1.0, device=DEV, **kw)


def test_temporal_fusion_refuses_what_it_cannot_take(recorder):  # noqa: F811
    rp = _reprojector()
    assert rp.long_range == (-math.pi, math.pi) and rp.lat_range == (0.0, math.pi)
    table = _reprojector(rays=rp.rays.clone())                           # a bare ray table: no closed-form inverse
    assert table.long_range is None and table.lat_range is None
    del recorder.launched[:]
    for make in (lambda: dropin.TemporalFusion(table), lambda: dropin.TemporalFusion(object()), lambda: dropin.TemporalFusion(rp, gate=0.0),
                 lambda: dropin.TemporalFusion(rp, gate=-1.0), lambda: dropin.TemporalFusion(rp, gate=float("nan")),
                 lambda: dropin.TemporalFusion(rp, q_var=-1e-6), lambda: dropin.TemporalFusion(rp, q_var=float("inf")),
                 lambda: dropin.TemporalFusion(rp, meas_std=0.0), lambda: dropin.TemporalFusion(rp, meas_std=-0.1),
                 lambda: dropin.TemporalFusion(rp, meas_std=float("nan")),
                 lambda: dropin.TemporalFusion(_reprojector(lat_range=(-math.pi / 2, 0.0))),                    # outside the inverse's domain
                 lambda: dropin.TemporalFusion(_reprojector(long_range=(0.0, 1.5 * math.pi)))):
        with pytest.raises(ERRORS):
            make()
    with pytest.raises(ValueError):
        dropin.TemporalFusion(table)
    tf = dropin.TemporalFusion(rp)
    inv = torch.rand((2, 6, 8), device=DEV) + 0.1
    std = torch.full_like(inv, 0.01)
    eye = torch.eye(4).repeat(2, 1, 1)
    del recorder.launched[:]
    for call in (lambda: tf.step(inv),                                                                          # no std, no meas_std
                 lambda: tf.step(inv.cpu(), std), lambda: tf.step(inv.double(), std), lambda: tf.step(inv[:, :5], std), lambda: tf.step(inv[0], std),
                 lambda: tf.step(inv, std.cpu()), lambda: tf.step(inv, std[:1]), lambda: tf.step(inv, std.half()),
                 lambda: tf.step(inv, std, T=eye[:1]), lambda: tf.step(inv, std, T=eye[:, :3]), lambda: tf.step(inv, std, T=eye.double()),
                 lambda: tf.step(inv, std, T=torch.eye(3)), lambda: tf.step(inv, std, want=("fused", "nothing")), lambda: tf.step(inv, std, want=()),
                 lambda: tf.set_pose(torch.eye(3)), lambda: tf.set_pose(eye.double()), lambda: tf.set_pose(eye, B=3)):
        with pytest.raises(ERRORS):
            call()
    assert not recorder.launched
    tf.step(inv, std, T=eye)
    tf.step(inv.unsqueeze(1), std.unsqueeze(1), T=torch.eye(4))
    tf.set_pose(eye)
    assert recorder.launched == ["mvsgi_temporal_splat_f32", "mvsgi_temporal_fuse_f32"] * 2
