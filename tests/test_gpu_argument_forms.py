"""The Python-to-C boundary of mvs_gi_amd.hip_ops on the GPU: what a wrapper does with a tensor in a form the kernel cannot take.
tests/argument_cases.py is the table (one canonical call per entry point, the role of every tensor argument, the exemptions).

1. Rejections (test_bad_forms_raise_before_any_launch).  With a proxy in place of the loaded library that forwards the size and
   dispatch queries and records -- never runs -- every launching symbol (classified by tests/abi_header.py from include/mvsgi.h),
   each parameter, caller-owned output, residual and SplitAct of each row arrives in each bad form: on the CPU, float64, float16,
   one element short, one element long (outputs and residuals), strided, offset by one element, and for a SplitAct a storage of the
   wrong shape, dtype or stride.  The call must raise TypeError / RuntimeError / AssertionError / ValueError and the proxy must have
   recorded nothing; what is accepted must be listed in argument_cases.ACCEPTED.  No kernel can start in this part: these inputs
   are never shown to the real library.
2. Accepted forms (test_awkward_activations_give_the_same_bits), real library.  Each activation or mask in a transposed-storage view,
   a view offset by one element, a stride-0 expand along the batch and channels-last storage gives the bits of the canonical call
   (compared as bytes, so NaNs compare too), and the input is bit-identical afterwards.  argument_cases.REFUSED lists what a
   wrapper refuses by design; that must raise.
3. Completeness (test_every_launching_symbol_has_a_row).  The symbols the canonical calls reach are the launching symbols of the
   header minus argument_cases.EXEMPT: a new entry point fails here until it has a row.
"""
import pytest
import torch

import abi_header
import argument_cases as AC
import guard_arena
from mvs_gi_amd import _lib, hip_ops as H

pytestmark = pytest.mark.gpu
ERRORS = (TypeError, RuntimeError, AssertionError, ValueError)
LAUNCHING = abi_header.launching_symbols()


@pytest.fixture(autouse=True)
def arena(request):
    yield from guard_arena.fixture_body(request)


class RecordingLibrary:
    """The loaded library with every launching symbol replaced by a recorder that returns 0 (enqueued)."""

    def __init__(self, real):
        self._real, self.launched = real, []

    def __getattr__(self, name):
        if name in LAUNCHING:
            def record(*args, _name=name):
                self.launched.append(_name)
                return 0
            return record
        return getattr(self._real, name)


@pytest.fixture
def recorder(monkeypatch):
    """hip_ops and every `from ..hip_ops import _call` site go through _lib.load(): replacing that reaches them all."""
    proxy = RecordingLibrary(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    assert _lib.load() is proxy
    return proxy


def _bits(t):
    return t.detach().contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _run(case, args=None):
    return AC.flatten(case.fn(**(case.args if args is None else args)))


# ------------------------------------------------------------------------------ 1. rejections
@pytest.mark.parametrize("name", sorted(AC.ROWS))
def test_bad_forms_raise_before_any_launch(name, recorder):
    case = AC.ROWS[name]()
    tried, accepted = 0, []
    for path, role in case.roles.items():
        if role in ("act", "mask"):
            continue
        t = AC.get(case.args, path)
        if role == "split":
            variants = [(f, AC.bad_split(t, f)) for f in AC.SPLIT_BAD_FORMS]
        else:
            forms = [f for f in AC.BAD_FORMS if f != "long" or role in ("out", "res")]
            variants = [(f, AC.bad_form(t, f)) for f in forms if not (f == "short" and t.numel() < 2)]
        for form, bad in variants:
            del recorder.launched[:]
            tried += 1
            try:
                case.fn(**AC.put(case.args, path, bad))
            except ERRORS as e:
                assert not recorder.launched, f"{name}: {path} as {form!r} raised {type(e).__name__} after launching {recorder.launched}"
                # one element short or long is a mismatch BETWEEN arguments (Cout is scale's length): either side may be named
                assert form in ("short", "long") or path.split("/")[0] in str(e), \
                    f"{name}: {path} as {form!r}: the message does not name the argument: {e}"
            else:
                accepted.append((name, path, form))
    unlisted = [a for a in accepted if a not in AC.ACCEPTED]
    assert not unlisted, f"accepted although not listed in argument_cases.ACCEPTED (launches: {recorder.launched}): {unlisted}"
    stale = [k for k in AC.ACCEPTED if k[0] == name and k not in accepted]
    assert not stale, f"listed in argument_cases.ACCEPTED but rejected: {stale}"
    if any(r not in ("act", "mask") for r in case.roles.values()):
        assert tried


def test_splitact_constructor_checks_its_buffer(recorder):
    good = torch.zeros((2, 4, 6, 18, 16), device=AC.DEV, dtype=torch.int32)
    s = H.SplitAct(2, 2, 4, 16, 16, AC.DEV, buf=good)
    assert s.buf is good
    big = torch.zeros((5, 4, 6, 18, 16), device=AC.DEV, dtype=torch.int32)
    for view in (big[:2], big[1:3], big[3:]):            # the batch slices dropin/ and tools/ hand in
        assert H.SplitAct(2, 2, 4, 16, 16, "cuda", buf=view).buf is view
    for form in AC.SPLIT_BAD_FORMS:
        with pytest.raises(ERRORS):
            H.SplitAct(2, 2, 4, 16, 16, AC.DEV, buf=AC.bad_split(s, form).buf)
    with pytest.raises(ERRORS):
        H.SplitAct(2, 2, 4, 16, 16, AC.DEV, buf=good.cpu().numpy())
    with pytest.raises(ERRORS):
        H.SplitAct(2, 2, 4, 16, 16, "cpu", buf=good)
    with pytest.raises(ERRORS):
        H.SplitAct(2, 2, 4, 16, 16, AC.DEV, buf=big[::2][:2])      # every second frame
    assert not recorder.launched


# ------------------------------------------------------------------------------ 2. accepted forms
@pytest.mark.parametrize("name", sorted(n for n, b in AC.ROWS.items()))
def test_awkward_activations_give_the_same_bits(name):
    build = AC.ROWS[name]
    base_case = build()
    acts = [p for p, r in base_case.roles.items() if r in ("act", "mask")]
    if not acts:
        return
    base = [t.clone() for t in _run(base_case)]
    assert base
    tried = 0
    for path in acts:
        for form in AC.ACT_FORMS:
            case = build()
            t = AC.get(case.args, path)
            v = AC.act_form(t, form, case.cl.get(path))
            if v is None:
                continue
            tried += 1
            want = base
            if form == "expand":        # other values (frame 0 in every frame): the baseline is the same call on their contiguous copy
                ref_case = build()
                want = [r.clone() for r in _run(ref_case, AC.put(ref_case.args, path, AC.expand_base(t)))]
            before = v.clone()
            args = AC.put(case.args, path, v)
            if (name, path, form) in AC.REFUSED:
                with pytest.raises(ERRORS):
                    case.fn(**args)
                continue
            got = _run(case, args)
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(got, want)):
                assert _same(a, b), f"{name}: {path} as {form!r}: output {i} differs from the canonical call"
            assert _same(v, before), f"{name}: {path} as {form!r}: the input was written"
    assert tried, f"{name}: no awkward form applied to any activation"
    stale = [k for k in AC.REFUSED if k[0] == name and (k[1] not in acts or k[2] not in AC.ACT_FORMS)]
    assert not stale, stale


# ------------------------------------------------------------------------------ 3. completeness
def test_every_launching_symbol_has_a_row(recorder):
    reached = set()
    for name in sorted(AC.ROWS):
        del recorder.launched[:]
        case = AC.ROWS[name]()           # the packers a row's builder runs count too: they are entry points with rows of their own
        case.fn(**case.args)
        assert recorder.launched, f"{name}: the canonical call reached no launching symbol"
        reached |= set(recorder.launched)
    assert set(AC.EXEMPT) <= LAUNCHING, sorted(set(AC.EXEMPT) - LAUNCHING)
    assert not reached & set(AC.EXEMPT), f"exempt although a wrapper reaches it: {sorted(reached & set(AC.EXEMPT))}"
    missing = LAUNCHING - reached - set(AC.EXEMPT)
    assert not missing, f"launching symbols of include/mvsgi.h without a row in tests/argument_cases.py: {sorted(missing)}"
    assert all(isinstance(r, str) and r for r in AC.EXEMPT.values())


def test_the_recorder_never_reaches_the_library(recorder):
    """The proxy forwards queries and swallows launches: the canonical conv3d call leaves its sentinel-filled output untouched."""
    case = AC.ROWS["conv3d_mfma"]()
    case.args["out"].fill_(float("nan"))
    case.fn(**case.args)
    torch.cuda.synchronize()
    assert recorder.launched[-1] == "mvsgi_conv3d_f32" and bool(case.args["out"].isnan().all())
    assert recorder.mvsgi_abi_version() == _lib.ABI_VERSION and recorder.mvsgi_conv3d_packed_weight_floats(16, 16) == 27 * 16 * 16
