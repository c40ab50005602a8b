'''
Warm starts on the CPU: the twin of the warm-start kernels (tests/native/warmstart_hostcheck.cpp, the same
ws_node / ws_segment_map / ws_segment_apply the device runs) against raceline.warmstart.drone_guess_batch.
'''
import numpy as np
import pytest

from tests.warmstart_helpers import ERROR_CASES, LAYOUTS, POSES, SHAPES, check_error, check_lift, oracle_case, \
    shape_specs, twin_lift_rc


@pytest.mark.parametrize('turns', [0.75, 2.0])
@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('B', [1, 67])
@pytest.mark.parametrize('pose', POSES)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_twin_matches_oracle(shape, pose, B, layout, turns):
    check_lift(twin_lift_rc, shape, pose, B, layout, turns)


@pytest.mark.parametrize('name', ERROR_CASES)
def test_error_codes_leave_the_outputs_untouched(name):
    check_error(twin_lift_rc, name)


def test_inputs_drive_every_branch():
    ''' the swept headings flip quaternion signs along the chain and at the closure, unwrap Euler yaws, and at two
    turns make the Euler continuity fail '''
    shape, B = 'race-global-P28', 67
    esp, ypr = shape_specs(shape, 'esp')[0], shape_specs(shape, 'ypr')[0]
    W, _, _, flips, _ = oracle_case(shape, 'esp', B, 0.75)[1]
    assert np.count_nonzero(W[:, esp.N:].reshape(B, esp.P, esp.nv)[:, :, 6] < 0) > 100 and flips.all()
    assert not oracle_case(shape, 'esp', B, 2.0)[1][3].any()
    W, _, _, _, wraps = oracle_case(shape, 'ypr', B, 0.75)[1]
    assert np.count_nonzero(np.abs(W[:, ypr.N:].reshape(B, ypr.P, ypr.nv)[:, :, 3]) > np.pi) > 100
    assert np.all(np.abs(wraps) == 1)
    assert oracle_case(shape, 'ypr', B, 2.0)[1] is NotImplementedError
