"""The Python-to-C boundary of the visibility stage's wrappers (hip_ops.camera_range, hip_ops.visibility, hip_ops.photo_consistency
with cam_seen) on the GPU: the three checks of tests/test_gpu_argument_forms.py -- bad forms raise before any launch, awkward
activations give the canonical call's bits, every launching symbol has a row -- on the rows of tests/argument_cases_visibility.py.

Importing that module registers the rows in tests/argument_cases.py's table, which tests/test_gpu_argument_forms.py's completeness
test reads when it runs; the checks themselves are that module's functions, called here on the new rows (its own parametrisation was
made before the rows were registered)."""
import pytest

import abi_header
import argument_cases as AC
import argument_cases_visibility as ACV
from test_gpu_argument_forms import arena, recorder  # noqa: F401  (fixtures: the guarded allocator, the recording library)
from test_gpu_argument_forms import test_awkward_activations_give_the_same_bits as _awkward_activations_give_the_same_bits
from test_gpu_argument_forms import test_bad_forms_raise_before_any_launch as _bad_forms_raise_before_any_launch

pytestmark = pytest.mark.gpu
SYMBOLS = {"camera_range": "mvsgi_camera_range_f32", "visibility": "mvsgi_visibility_f32",
           "photo_consistency_seen": "mvsgi_photo_consistency_seen_f32"}


def test_the_rows_are_in_the_table():
    assert set(ACV.ROWS) == set(SYMBOLS) and all(AC.ROWS[n] is ACV.ROWS[n] for n in ACV.ROWS)
    assert all(AC.REFUSED[k] == v for k, v in ACV.REFUSED.items())
    assert set(SYMBOLS.values()) <= abi_header.launching_symbols() and not set(SYMBOLS.values()) & set(AC.EXEMPT)


@pytest.mark.parametrize("name", sorted(ACV.ROWS))
def test_bad_forms_raise_before_any_launch(name, recorder):  # noqa: F811
    _bad_forms_raise_before_any_launch(name, recorder)


@pytest.mark.parametrize("name", sorted(ACV.ROWS))
def test_awkward_activations_give_the_same_bits(name):
    _awkward_activations_give_the_same_bits(name)


@pytest.mark.parametrize("name", sorted(ACV.ROWS))
def test_the_canonical_call_reaches_its_symbol(name, recorder):  # noqa: F811
    case = AC.ROWS[name]()
    del recorder.launched[:]
    case.fn(**case.args)
    assert recorder.launched[-1] == SYMBOLS[name], recorder.launched
