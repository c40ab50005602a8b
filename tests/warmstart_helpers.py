'''
Warm-start test fixtures: the CPU twin of the warm-start kernels (tests/native/warmstart_hostcheck.cpp), the
swept-heading inputs, the oracle (raceline.warmstart.drone_guess_batch, computed once per case) and the one test
body the CPU and the GPU tests share.
'''
import ctypes
import functools
import os

import numpy as np

from aircraft_trajectory_optimization_amd import native
from aircraft_trajectory_optimization_amd.raceline.warmstart import drone_guess_batch
from tests.helpers import REPO, build_twin, product_spec
from tests.replay_helpers import MODELS

WS_SRC = os.path.join(REPO, 'tests', 'native', 'warmstart_hostcheck.cpp')
WS_LIB = os.path.join(REPO, 'tests', 'native', 'libato_warmstartcheck.so')
IL, IM = native.ATO_LAYOUT_INTERLEAVED, native.ATO_LAYOUT_INSTANCE_MAJOR
LAYOUTS = {'interleaved': IL, 'instance_major': IM}
TOL = 1e-13                 # rtol = atol, the bound between the two host versions (tests/test_corridor_cpu.py)
MARGIN = 1e-6               # no oracle decision may lie this close to its threshold
G = 4                       # WS_G, the segments of the chain

# The smallest shapes at which the kernels can go wrong (P = N (K + 1) nodes against the G segments). A closed
# problem needs N >= 2 (ato_create rejects N = 1), so P < G, with empty segments, is the open line's.
SHAPES = {
    'fig8-gr-P4': dict(track='fig8', frame='parametric', global_r=True, N=2, K=1),       # one node per segment
    'fig8-gr-P9': dict(track='fig8', frame='parametric', global_r=True, N=3, K=2),       # P no multiple of G
    'race-global-P28': dict(track='race', frame='global', N=7, K=3),                     # several flips per segment
    'fig8-rel-P9': dict(track='fig8', frame='parametric', global_r=False, N=3, K=2),     # both Rp tables are read
    'fig8-open-P2': dict(track='fig8', frame='parametric', global_r=True, N=1, K=1, closed=False),   # P < G
}
POSES = ('esp', 'ypr', 'dcm')
GROUPS = ('position', 'attitude', 'body velocity', 'body rates', 'thrust')
worst = {g: 0.0 for g in GROUPS}       # largest deviation from the oracle per variable group, over the cases run


@functools.lru_cache(maxsize=None)
def shape_specs(shape, pose):
    ''' (drone, point) specs of a shape '''
    kw = SHAPES[shape]
    return product_spec(**kw, **MODELS[pose]), product_spec(**kw, **MODELS['point'])


def swept_inputs(point, B, turns, seed=11):
    ''' (B, nw) point-mass "solutions" whose heading sweeps `turns` turns along the lap '''
    rng = np.random.default_rng(seed)
    N, P = point.N, point.P
    phi = 2 * np.pi * turns * np.arange(P)[None] / P + rng.uniform(0, 2 * np.pi, (B, 1))
    node = np.zeros((B, P, point.nv))
    node[..., :3] = rng.normal(size=(B, P, 3))
    node[..., 3:6] = 8 * np.stack([np.cos(phi), np.sin(phi), 0 * phi], axis=2) + [0, 0, 0.5]
    node[..., 6:9] = 4 * np.stack([np.cos(phi + 0.3), np.sin(phi + 0.3), 0 * phi], axis=2) + [0, 0, 9.81] + \
        rng.normal(0, 0.3, (B, P, 3))
    node[..., 9:12] = rng.normal(size=(B, P, 3))
    X = np.zeros((B, point.nw))
    X[:, :N] = rng.uniform(0.05, 0.2, (B, N))
    X[:, N:N + P * point.nv] = node.reshape(B, -1)
    return X


@functools.lru_cache(maxsize=None)
def oracle_case(shape, pose, B, turns):
    ''' (inputs (B, nw_p), drone_guess_batch's result or the exception type it raises); computed once '''
    drone, point = shape_specs(shape, pose)
    X = swept_inputs(point, B, turns)
    X.setflags(write=False)
    try:
        with np.errstate(all='ignore'):
            ref = drone_guess_batch(drone, point, X)
    except NotImplementedError:
        return X, NotImplementedError
    for a in ref:
        a.setflags(write=False)
    return X, ref


def build_warmstartcheck(force=False):
    return build_twin(WS_SRC, WS_LIB, ('ato_sample.hpp', 'ato_warmstart.hpp'), force)


@functools.lru_cache(maxsize=None)
def _lib():
    lib = ctypes.CDLL(build_warmstartcheck())
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.atow_create.argtypes = [ctypes.POINTER(native.AtoProblemDesc), ctypes.POINTER(vp)]
    lib.atow_last_error.restype = ctypes.c_char_p
    lib.atow_destroy.argtypes = [vp]
    lib.atow_warmstart.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp]
    return lib


class _Problem:
    ''' a twin handle; kept for the test session (one per spec, _problem) '''

    def __init__(self, spec):
        self.lib, self.holder = _lib(), native.DescHolder(spec.native_spec())
        self.h = ctypes.c_void_p()
        if self.lib.atow_create(ctypes.byref(self.holder.desc), ctypes.byref(self.h)) != 0:
            raise RuntimeError(self.lib.atow_last_error().decode())

    def __del__(self):
        self.lib.atow_destroy(self.h)


@functools.lru_cache(maxsize=None)
def _problem(spec):
    return _Problem(spec)


def to_layout(a, layout):
    ''' host (B, n) -> the contiguous array a call in `layout` reads or writes '''
    return np.ascontiguousarray(a.T) if layout == IL else np.ascontiguousarray(a)


def from_layout(a, layout):
    return a.T.copy() if layout == IL else a


def lift_buffers(drone, B, layout, fill=np.nan):
    ''' (W, hlb, hub, info) in `layout`, filled: what a call leaves unwritten stays `fill` '''
    return [to_layout(np.full((B, n), fill), layout) for n in (drone.nw, drone.N, drone.N, 3)]


def twin_lift_rc(drone, point, X, layout, batch=None, null=(), fill=np.nan):
    ''' the twin's ato_warmstart: (rc, W (B, nw), hlb (B, N), hub (B, N), info (B, 3)); null: arguments passed as NULL '''
    lib, B = _lib(), X.shape[0]
    bufs = dict(zip(('w_drone', 'hlb', 'hub', 'info'), lift_buffers(drone, B, layout, fill)), w_point=to_layout(X, layout))
    ptr = {k: None if k in null else v.ctypes.data for k, v in bufs.items()}
    rc = lib.atow_warmstart(_problem(point).h, _problem(drone).h, B if batch is None else batch, layout,
                            ptr['w_point'], ptr['w_drone'], ptr['hlb'], ptr['hub'], ptr['info'])
    return (rc,) + tuple(from_layout(bufs[k], layout) for k in ('w_drone', 'hlb', 'hub', 'info'))


def _margins(drone, pose, W):
    ''' distance of every continuity decision of the oracle's result W from its threshold 1 '''
    if pose == 'dcm':
        return np.array([1.0])
    nr = 4 if pose == 'esp' else 3
    r = W[:, drone.N:].reshape(W.shape[0], drone.P, drone.nv)[:, :, 3:3 + nr]
    d = [np.roll(r, 1, axis=1) - s * r for s in (1, -1)] if pose == 'esp' else \
        [r - np.roll(r, 1, axis=1) + np.array([2 * np.pi * k, 0, 0]) for k in (-1, 0, 1)]
    if pose == 'ypr':           # first against last is no decision of the Euler chain
        d = [x[:, 1:] for x in d]
    return np.abs(np.linalg.norm(np.stack(d), axis=-1) - 1.0)


def check_lift(lift_rc, shape, pose, B, layout, turns):
    '''
    The body of the twin's and the device's test: lift_rc has twin_lift_rc's signature. hlb / hub bit for bit, info
    equal to the oracle's closure values, W within TOL of the oracle's, every element of W written; where the oracle
    raises, status 1 in some instance (what the wrapper turns into the same exception).
    '''
    drone, point = shape_specs(shape, pose)
    X, ref = oracle_case(shape, pose, B, turns)
    rc, W, hlb, hub, info = lift_rc(drone, point, X, LAYOUTS[layout])
    assert rc == 0
    h = X[:, :drone.N]
    assert np.array_equal(hlb, h / 100) and np.array_equal(hub, h * 10)
    if ref is NotImplementedError:
        assert pose == 'ypr' and np.any(info[:, 0] == 1) and not np.any(info[:, 0] == 2)
        return
    Wr, LBW, UBW, flips, wraps = ref
    assert np.array_equal(LBW[:, :drone.N], hlb) and np.array_equal(UBW[:, :drone.N], hub)
    assert _margins(drone, pose, Wr).min() > MARGIN, 'an oracle decision sits on its threshold: pick another seed'
    assert np.all(info[:, 0] == 0)
    assert np.array_equal(info[:, 1], flips.astype(float)) and np.array_equal(info[:, 2], wraps)
    nr = drone.nz - 9
    node = lambda A: A[:, drone.N:].reshape(B, drone.P, drone.nv)      # noqa: E731
    cuts = dict(zip(GROUPS, ((0, 3), (3, 3 + nr), (3 + nr, 6 + nr), (6 + nr, 9 + nr), (9 + nr, drone.nv))))
    for g, (i, j) in cuts.items():
        dev = float(np.max(np.abs(node(W)[..., i:j] - node(Wr)[..., i:j]) / np.maximum(1.0, np.abs(node(Wr)[..., i:j]))))
        worst[g] = max(worst[g], dev)
    print(f'warm start vs oracle {shape} {pose} B={B} {layout} turns={turns}: ' +
          ', '.join(f'{g} {worst[g]:.2e}' for g in GROUPS) + ' (largest so far)')
    np.testing.assert_allclose(W, Wr, rtol=TOL, atol=TOL)


def error_cases():
    ''' name -> (drone, point, keywords of lift_rc, expected code): the ATO_ERR_ARG / ATO_ERR_UNSUPPORTED cases '''
    d, p = shape_specs('fig8-gr-P9', 'esp')
    g = dict(track='race', frame='global', N=7, K=2)
    cpc = {'waypoints': None, 'tol': 0.3}
    A, U = native.ATO_ERR_ARG, native.ATO_ERR_UNSUPPORTED
    return {
        'batch_zero': (d, p, dict(batch=0), A),
        'layout': (d, p, dict(layout=7), A),
        'other_N': (product_spec(**{**SHAPES['fig8-gr-P9'], 'N': 4}), p, {}, A),
        'other_K': (product_spec(**{**SHAPES['fig8-gr-P9'], 'K': 3}), p, {}, A),
        'point_is_a_drone': (d, d, {}, A),
        'drone_is_a_point': (p, p, {}, A),
        'null_w_point': (d, p, dict(null=('w_point',)), A),
        'null_w_drone': (d, p, dict(null=('w_drone',)), A),
        'null_info': (d, p, dict(null=('info',)), A),
        'rk4_point': (d, product_spec(track='race', N=7, K=2, rk4=True, **MODELS['point']), {}, U),
        'rk4_drone': (product_spec(track='race', N=7, K=2, rk4=True), p, {}, U),
        'cpc_drone': (product_spec(**g, model='drone', cpc=cpc), product_spec(**g, **MODELS['point']), {}, U),
    }


ERROR_CASES = ['batch_zero', 'layout', 'other_N', 'other_K', 'point_is_a_drone', 'drone_is_a_point', 'null_w_point',
               'null_w_drone', 'null_info', 'rk4_point', 'rk4_drone', 'cpc_drone']


def check_error(lift_rc, name):
    ''' the code, and nothing written (W keeps its fill) '''
    drone, point, kw, code = error_cases()[name]
    kw = dict(kw)
    rc, W, hlb, hub, info = lift_rc(drone, point, np.ones((2, point.nw)), kw.pop('layout', IL), fill=123.5, **kw)
    assert rc == code
    assert all(np.all(a == 123.5) for a in (W, hlb, hub, info))
