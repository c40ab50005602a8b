'''
Export of solved racelines on the CPU: the twin of the export kernels (tests/native/export_hostcheck.cpp) against
the numpy oracle of tests/export_helpers.py. The same bodies run on the device in tests/test_gpu_export.py.
'''
import numpy as np
import pytest

from tests.export_helpers import CASES, ERRORS, check_batch, check_chain, check_error, check_parity, twin_export, twin_raw


@pytest.mark.parametrize('relative', (False, True), ids=('seconds', 'fractions'))
@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(map(str, c)))
def test_twin_matches_oracle(case, relative):
    check_parity(twin_export, case, relative)


def test_twin_sign_chain():
    check_chain(twin_export)


def test_twin_across_a_wave_and_batch_invariance():
    check_batch(twin_export)


@pytest.mark.parametrize('name', ERRORS)
def test_twin_error_codes_leave_the_outputs_untouched(name):
    check_error(twin_raw, np.ascontiguousarray, name)
