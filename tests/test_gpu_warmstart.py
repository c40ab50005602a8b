'''
Warm starts on the device (ato_warmstart: k_ws_nodes, k_ws_chain): the cases of tests/test_warmstart_cpu.py through
NativeProblem.warmstart_rc against raceline.warmstart.drone_guess_batch, the error codes, the wrapper
drone_guess_batch_device and corridor_batch(lift='device').
'''
import functools

import numpy as np
import pytest

from aircraft_trajectory_optimization_amd import native
from tests.warmstart_helpers import ERROR_CASES, LAYOUTS, POSES, SHAPES, TOL, check_error, check_lift, from_layout, \
    lift_buffers, oracle_case, shape_specs, to_layout

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@functools.lru_cache(maxsize=None)
def problem(spec):
    return native.NativeProblem(spec.native_spec())


def device_lift_rc(drone, point, X, layout, batch=None, null=(), fill=np.nan):
    ''' ato_warmstart on device copies of the host arrays: tests.warmstart_helpers.twin_lift_rc's signature '''
    B = X.shape[0]
    names = ('w_drone', 'hlb', 'hub', 'info')
    bufs = {k: torch.as_tensor(v, device='cuda') for k, v in zip(names, lift_buffers(drone, B, layout, fill))}
    bufs['w_point'] = torch.as_tensor(np.array(to_layout(X, layout)), device='cuda')
    ptr = {k: 0 if k in null else v.data_ptr() for k, v in bufs.items()}
    rc = problem(drone).warmstart_rc(problem(point), B if batch is None else batch, ptr['w_point'], ptr['w_drone'],
                                     ptr['info'], ptr['hlb'], ptr['hub'], layout=layout)
    torch.cuda.synchronize()
    return (rc,) + tuple(from_layout(bufs[k].cpu().numpy(), layout) for k in names)


@pytest.mark.parametrize('turns', [0.75, 2.0])
@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('B', [1, 67])
@pytest.mark.parametrize('pose', POSES)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_device_matches_oracle(shape, pose, B, layout, turns):
    check_lift(device_lift_rc, shape, pose, B, layout, turns)


@pytest.mark.parametrize('name', ERROR_CASES)
def test_error_codes_leave_the_outputs_untouched(name):
    check_error(device_lift_rc, name)
    assert problem(shape_specs('fig8-gr-P9', 'esp')[0]).lib.ato_last_error().decode()


@pytest.mark.parametrize('pose,turns', [('esp', 0.75), ('ypr', 0.75), ('ypr', 2.0), ('dcm', 2.0)])
def test_wrapper_returns_or_raises_as_the_host_version(pose, turns):
    from aircraft_trajectory_optimization_amd.raceline.warmstart import drone_guess_batch_device
    shape, B = 'race-global-P28', 67
    drone, point = shape_specs(shape, pose)
    X, ref = oracle_case(shape, pose, B, turns)
    if ref is NotImplementedError:
        with pytest.raises(NotImplementedError):
            drone_guess_batch_device(drone, point, X)
        return
    out = drone_guess_batch_device(drone, point, torch.as_tensor(np.ascontiguousarray(X.T), device='cuda'))
    for a, r in zip(out[:3], ref[:3]):
        assert a.is_cuda and tuple(a.shape) == (drone.nw, B)
        np.testing.assert_allclose(a.T.cpu().numpy(), r, rtol=TOL, atol=TOL)
    assert np.array_equal(out[3], ref[3]) and np.array_equal(out[4], ref[4])
    bad = X.copy()
    bad[5, point.N + 6:point.N + 9] = 0.0            # no thrust at node 0 of instance 5
    with pytest.raises(ValueError, match='instance 5'):
        drone_guess_batch_device(drone, point, bad)


def test_corridor_batch_device_lift_equals_host_lift():
    from aircraft_trajectory_optimization_amd.raceline.batch_instances import corridor_batch
    kw = dict(track='fig8', frame='parametric', N=8, K=2, use_quat=True, global_r=True)
    spec, W, LBW, UBW, status, laps = corridor_batch(3, **kw)
    dspec, Wd, Ld, Ud, dstatus, dlaps = corridor_batch(3, lift='device', **kw)
    assert dstatus == status and (dspec.quat_flip, dspec.euler_wraps) == (spec.quat_flip, spec.euler_wraps)
    for a, r in ((Wd, W), (Ld, LBW), (Ud, UBW)):
        np.testing.assert_allclose(a.T.cpu().numpy(), r, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(dlaps, laps, rtol=TOL, atol=TOL)
