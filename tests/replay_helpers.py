'''
Replay test fixtures: the CPU twin of the replay kernel (tests/native/replay_hostcheck.cpp), the
cases the CPU and the GPU tests share, and their inputs.
'''
import ctypes
import functools
import os

import numpy as np

from aircraft_trajectory_optimization_amd import native
from tests.helpers import REPO, build_twin, product_spec, random_w, rel_dev  # noqa: F401

REPLAY_SRC = os.path.join(REPO, 'tests', 'native', 'replay_hostcheck.cpp')
REPLAY_LIB = os.path.join(REPO, 'tests', 'native', 'libato_replaycheck.so')

# Twin / device against the numpy oracle, relative to max(1, |value|), over every case below.
# Measured once on the CPU twin: 2.014e-15 (the largest over zsim, err and traj of all the cases below, at
# ypr-global-K2-S1; contraction and summation order compounding over the 4 S model evaluations); the
# bound is 10 x that (it may not exceed 1e-9).
PARITY_TOL = 2.014e-14

MODELS = {
    'esp': dict(model='drone', use_quat=True),
    'ypr': dict(model='drone', use_quat=False),
    'dcm': dict(model='drone', use_dcm=True),
    'point': dict(model='point', use_quat=False),
}
# N = 3 is the base; the global frame rounds N up to a multiple of the track's 7 gate phases
FRAMES = {'global': dict(frame='global', N=7), 'parametric': dict(frame='parametric', N=3, global_r=True)}
CASES = [(m, f, K, S) for m in MODELS for f in FRAMES for K in (1, 2, 9) for S in (1, 4)]


def case_id(c):
    return f'{c[0]}-{c[1]}-K{c[2]}-S{c[3]}'


def build_replaycheck(force=False):
    return build_twin(REPLAY_SRC, REPLAY_LIB, ('ato_sample.hpp', 'ato_replay.hpp'), force)


class ReplayTwin:
    ''' ato_replay_set_lift / ato_replay on host arrays (CPU build of csrc/ato_replay.hpp) '''

    def __init__(self, spec):
        lib = ctypes.CDLL(build_replaycheck())
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.ator_create.argtypes = [ctypes.POINTER(native.AtoProblemDesc), ctypes.POINTER(vp)]
        lib.ator_last_error.restype = ctypes.c_char_p
        lib.ator_destroy.argtypes = [vp]
        lib.ator_set_lift.argtypes = [vp, vp]
        lib.ator_weights.argtypes = [vp, ci, vp]
        lib.ator_replay.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
        self.lib, self.spec = lib, spec
        self.holder = native.DescHolder(spec.native_spec())
        h = vp()
        if lib.ator_create(ctypes.byref(self.holder.desc), ctypes.byref(h)) != 0:
            raise RuntimeError(lib.ator_last_error().decode())
        self.h = h

    def set_lift(self, table):
        t = np.ascontiguousarray(table, np.float64)
        assert t.shape == (self.spec.N + 1, 12)
        self.lib.ator_set_lift(self.h, t.ctypes.data)

    def weights(self, S):
        lw = np.zeros((2 * S + 1, self.spec.K1))
        self.lib.ator_weights(self.h, S, lw.ctypes.data)
        return lw

    def replay_rc(self, W, S, layout=native.ATO_LAYOUT_INSTANCE_MAJOR, traj=False):
        ''' W (B, nw) -> (rc, zsim (B, N, NZ), err (B, N, 4), traj (B, N, S, NZ) or None) '''
        sp_ = self.spec
        W = np.ascontiguousarray(np.atleast_2d(W), np.float64)
        B = W.shape[0]
        il = layout == native.ATO_LAYOUT_INTERLEAVED
        Sa = max(int(S), 1)
        zs, er = np.zeros((B, sp_.N * sp_.nz)), np.zeros((B, sp_.N * 4))
        tj = np.zeros((B, sp_.N * Sa * sp_.nz)) if traj else None
        win = np.ascontiguousarray(W.T) if il else W
        if il:
            zs, er = np.ascontiguousarray(zs.T), np.ascontiguousarray(er.T)
            tj = np.ascontiguousarray(tj.T) if traj else None
        rc = self.lib.ator_replay(self.h, B, layout, win.ctypes.data, int(S), zs.ctypes.data, er.ctypes.data,
                                  tj.ctypes.data if traj else None)
        if il:
            zs, er = zs.T, er.T
            tj = tj.T if traj else None
        return (rc, zs.reshape(B, sp_.N, sp_.nz), er.reshape(B, sp_.N, 4),
                tj.reshape(B, sp_.N, Sa, sp_.nz) if traj else None)

    def replay(self, W, S, **kw):
        rc, zs, er, tj = self.replay_rc(W, S, **kw)
        if rc != 0:
            raise RuntimeError(f'twin replay error {rc}: {self.lib.ator_last_error().decode()}')
        return zs, er, tj

    def __del__(self):
        try:
            self.lib.ator_destroy(self.h)
        except Exception:  # pylint: disable=broad-except
            pass


@functools.lru_cache(maxsize=None)
def case_spec(model, frame, K):
    return product_spec(track='race', K=K, **MODELS[model], **FRAMES[frame])


def replay_inputs(spec, B, seed=0):
    ''' (B, nw) helpers.random_w vectors with h overwritten by values in [0.05, 0.3] '''
    rng = np.random.default_rng(seed)
    W = np.stack([random_w(spec, rng) for _ in range(B)])
    W[:, :spec.N] = 0.05 + 0.25 * rng.random((B, spec.N))
    return W
