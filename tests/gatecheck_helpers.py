'''
Gate-passage test fixtures: the CPU twin of the gate-check kernels (tests/native/gatecheck_hostcheck.cpp), the
cases the CPU and the GPU tests share (those of the clearance tests), their inputs and the hand-built cases.
'''
import ctypes
import functools
import os

import numpy as np

from aircraft_trajectory_optimization_amd import native
from aircraft_trajectory_optimization_amd.raceline.gates import gate_planes
from tests import gatecheck_oracle
from tests.audit_helpers import WAVE_CASES, _blank, _nodes, nonfinite_inputs, rel_dev  # noqa: F401
from tests.clearance_helpers import CASES, FRAMES, IL, IM, case_id, case_spec  # noqa: F401
from tests.helpers import REPO, build_twin, product_spec
from tests.replay_helpers import MODELS, replay_inputs

GATE_SRC = os.path.join(REPO, 'tests', 'native', 'gatecheck_hostcheck.cpp')
GATE_LIB = os.path.join(REPO, 'tests', 'native', 'libato_gatecheck.so')

NCH = 9
CH = {name: i for i, name in enumerate(('n_cross', 'margin', 'interval', 'x', 't', 'p2', 'p3', 'off', 'flag'))}
EXACT_CH = (CH['n_cross'], CH['interval'], CH['flag'])
CLOSE_CH = tuple(c for c in range(NCH) if c not in EXACT_CH)
SAMPLES = (1, 5, 16)

# Twin / device against the numpy oracle (tests/gatecheck_oracle.py): n_cross, interval and flag equal; x, t, p2, p3,
# off and margin relative to max(1, |value|), over every case of CASES at samples 1, 5, 16 and both layouts, the
# B = 65 / 130 inputs of WAVE_CASES at samples 5 and the hand-built cases. Measured once on the CPU twin
# (tests/test_gatecheck_cpu.py prints the figures): the largest at CLOSE_CASE; the bound is 10 x the measured value
# (it may not exceed 1e-9).
CLOSE_MEASURED = 1.7888e-14
CLOSE_CASE = 'obstacles-point-parametric-K9 (and its relative twin: the position does not depend on the attitude)'
CLOSE_TOL = 10 * CLOSE_MEASURED
# Global-frame identity: p2, p3 of the crossing at a gate node against ubg - g of the gate's rows in the CPU build of
# the programs (plain products there, fused multiply-adds here) and against the offsets the node was built with.
# Measured once on the CPU twin over both tracks: the largest at IDENTITY_CASE; asserted at 10 x.
IDENTITY_MEASURED = 8.1012e-16
IDENTITY_CASE = 'obstacles (circle gates), gate 8'
IDENTITY_TOL = 10 * IDENTITY_MEASURED

# The conditions the tests ask of the shared inputs (asserted in tests/test_gatecheck_cpu.py):
MIN_SLOPE = 1e-2        # every oracle crossing is transversal: |da/dx| >= 1e-2 m per unit abscissa
MIN_SAMPLE = 1e-9       # no sample has |a| below it
# and the oracle finds no pair of crossings inside one sample step -- asserted as stated at S = 16, the default and the
# finest of the three (PAIR_FREE), where a seed that keeps every step free of pairs exists for every case (SEEDS).
# At S = 1 and S = 5 no seed can do that: at N = 3 a step at S = 1 is a third of the lap and at S = 5 a fifteenth, and
# the lap crosses the planes of the far gates twice inside such a step wherever the perturbation puts the nodes
# (tests/test_gatecheck_cpu.py counts them over eight seeds: about 30 such steps each at S = 1, 1 to 3 at S = 5 on the
# race track). There the inputs are held to what the comparison needs: no step holds an ODD number above one of
# crossings (of those the bisection finds one and the definition does not say which). By the definition a pair shows
# no sign change and is no crossing; the oracle counts it so and n_cross is asserted equal, so these steps are checked.
PAIR_FREE = (16,)


def build_gatecheck(force=False):
    return build_twin(GATE_SRC, GATE_LIB, ('ato_sample.hpp', 'ato_clearance.hpp', 'ato_gatecheck.hpp'), force)


@functools.lru_cache(maxsize=None)
def _lib():
    lib = ctypes.CDLL(build_gatecheck())
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.atog_create.argtypes = [ctypes.POINTER(native.AtoProblemDesc), ctypes.POINTER(vp)]
    lib.atog_last_error.restype = ctypes.c_char_p
    lib.atog_destroy.argtypes = [vp]
    lib.atog_set_line.argtypes = [vp, ctypes.POINTER(native.AtoLineTable)]
    lib.atog_set_gates.argtypes = [vp, vp, ci]
    lib.atog_n_gates.argtypes = [vp]
    lib.atog_gates.argtypes = [vp, vp]
    lib.atog_gatecheck.argtypes = [vp, ci, ci, vp, ci, ctypes.c_double, vp]
    lib.atog_gate_rows.argtypes = [vp, vp]
    return lib


class GateTwin:
    ''' ato_gatecheck on host arrays (CPU build of csrc/ato_gatecheck.hpp) '''

    def __init__(self, spec, set_line=True):
        self.lib, self.spec = _lib(), spec
        self.holder = native.DescHolder(spec.native_spec())
        h = ctypes.c_void_p()
        if self.lib.atog_create(ctypes.byref(self.holder.desc), ctypes.byref(h)) != 0:
            raise RuntimeError(self.lib.atog_last_error().decode())
        self.h = h
        if set_line and spec.param and not spec.rk4:
            t, self._keep = native.line_table_struct(spec.line_table())
            self.lib.atog_set_line(self.h, ctypes.byref(t))

    def __del__(self):
        try:
            self.lib.atog_destroy(self.h)
        except Exception:  # pylint: disable=broad-except
            pass

    def last_error(self):
        return self.lib.atog_last_error().decode()

    def set_gates(self, planes):
        ''' planes as raceline.gates.gate_planes gives them, any number (the check rejects more than 64); None:
        the problem's own '''
        if planes is None:
            return self.lib.atog_set_gates(self.h, None, 0)
        c = np.asarray(planes['centre'], float).reshape(-1, 3)
        arr = (native.AtoGatePlane * max(len(c), 1))()
        for i in range(len(c)):
            arr[i].centre[:] = c[i].tolist()
            arr[i].R[:] = np.asarray(planes['R'][i], float).reshape(9).tolist()
            arr[i].d_max = float(planes['d_max'][i])
            arr[i].shape = int(planes['shape'][i])
        return self.lib.atog_set_gates(self.h, arr, len(c))

    def gate_rows(self):
        ''' first row in g of every gate of the problem '''
        rows = np.full(max(len(self.spec.gates), 1), -1, np.int32)
        self.lib.atog_gate_rows(self.h, rows.ctypes.data)
        return rows[:len(self.spec.gates)]

    def n_gates(self):
        return self.lib.atog_n_gates(self.h)

    def planes(self):
        ''' the planes in use, in gate_planes' form '''
        G = self.n_gates()
        arr = (native.AtoGatePlane * max(G, 1))()
        self.lib.atog_gates(self.h, arr)
        return {'centre': np.array([list(arr[i].centre) for i in range(G)]).reshape(G, 3),
                'R': np.array([list(arr[i].R) for i in range(G)]).reshape(G, 3, 3),
                'd_max': np.array([arr[i].d_max for i in range(G)]),
                'shape': np.array([arr[i].shape for i in range(G)], np.int32)}

    def raw(self, W, samples, axial_tol=1e-6, layout=IL, batch=None, fill=0.0):
        '''
        W (B, nw) -> (rc, val in the library's own layout: (NCH, G, B) interleaved, (B, G, NCH) instance-major),
        the output starting from `fill`. batch: the batch argument where it shall differ.
        '''
        W = np.ascontiguousarray(np.atleast_2d(W), np.float64)
        B, G = W.shape[0], min(self.n_gates(), 64)
        il = layout == IL
        val = np.full((NCH, G, B) if il else (B, G, NCH), fill)
        win = np.ascontiguousarray(W.T) if il else W
        rc = self.lib.atog_gatecheck(self.h, B if batch is None else batch, layout, win.ctypes.data, int(samples),
                                     float(axial_tol), val.ctypes.data)
        return rc, val

    def gatecheck(self, W, samples, axial_tol=1e-6, layout=IL):
        ''' W (B, nw) -> (NCH, G, B) '''
        rc, val = self.raw(W, samples, axial_tol, layout)
        if rc != 0:
            raise RuntimeError(f'twin gate check error {rc}: {self.last_error()}')
        return to_canonical(val, layout)


def to_canonical(val, layout):
    ''' the library's layout -> (NCH, G, B) '''
    return val if layout == IL else np.ascontiguousarray(np.transpose(val, (2, 1, 0)))


def conditions_hold(cond, sample=True):
    return cond['slope'] >= MIN_SLOPE and cond['odd'] == 0 and (not sample or cond['sample'] >= MIN_SAMPLE)


def gate_inputs(spec, B, seed):
    '''
    (B, nw) decision vectors around the cold start: replay_inputs, and in the global frame the node positions moved
    from the cold start's (the centreline at (n + k / K) / phase, uniform in k, whose interpolant through the
    Gauss nodes oscillates at K = 9 and crosses a gate's plane three times inside one sample step) to the
    centreline at the nodes' own abscissae (n + tau_k) / phase, the seed's perturbation kept.
    '''
    W = replay_inputs(spec, B, seed)
    if not spec.param:
        V, V0 = _nodes(spec, W), _nodes(spec, np.array(spec.w0, float)[None].copy())
        tau = np.asarray(spec.tau, float)
        for n in range(spec.N):
            for k in range(spec.K1):
                V[:, n, k, :3] += spec.line.p2xc((n + tau[k]) / spec.guess_phase_len) - V0[0, n, k, :3]
    return W


# The seed of a case's inputs: 0, or the first one whose inputs meet the conditions at every sample count, no pair of
# crossings in a step at S = 16 among them
SEEDS = {('race', 'esp', 'parametric', 9): 2, ('race', 'esp', 'relative', 9): 2, ('race', 'ypr', 'parametric', 9): 4,
         ('race', 'ypr', 'relative', 9): 4, ('race', 'dcm', 'parametric', 9): 3, ('race', 'dcm', 'relative', 9): 3,
         ('race', 'point', 'parametric', 1): 1, ('race', 'point', 'parametric', 9): 1, ('race', 'point', 'relative', 1): 1,
         ('race', 'point', 'relative', 9): 1, ('obstacles', 'esp', 'global', 9): 28, ('obstacles', 'esp', 'parametric', 9): 1,
         ('obstacles', 'esp', 'relative', 9): 1, ('obstacles', 'ypr', 'parametric', 9): 3,
         ('obstacles', 'ypr', 'relative', 9): 3, ('obstacles', 'dcm', 'global', 9): 3, ('obstacles', 'point', 'global', 9): 21,
         ('obstacles', 'point', 'parametric', 9): 1, ('obstacles', 'point', 'relative', 9): 1}
WAVE_SEED = 4


@functools.lru_cache(maxsize=None)
def case_inputs(track, model, frame, K, B=3):
    W = gate_inputs(case_spec(track, model, frame, K), B, SEEDS.get((track, model, frame, K), 0))
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def wave_inputs(case, B):
    ''' W (B, nw) of a wave-crossing case: B no multiple of the wave or the block '''
    W = gate_inputs(case_spec(*case), B, WAVE_SEED)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def oracle_val(track, model, frame, K, samples, B=3):
    ''' (the oracle's channels (NCH, G, B), the conditions) of one case and sample count; computed once '''
    spec = case_spec(track, model, frame, K)
    v, cond = gatecheck_oracle.gatecheck(spec, case_planes(track, model, frame, K), case_inputs(track, model, frame, K, B),
                                         samples)
    v.setflags(write=False)
    return v, cond


@functools.lru_cache(maxsize=None)
def case_planes(track, model, frame, K):
    spec = case_spec(track, model, frame, K)
    return gate_planes(spec)


def compare(val, ref):
    ''' (n_cross, interval and flag equal?, largest deviation of the other channels relative to max(1, |value|)) of
    two (NCH, G, B) results '''
    val, ref = np.asarray(val, float), np.asarray(ref, float)
    ex = list(EXACT_CH)
    same = bool(np.all((val[ex] == ref[ex]) | (np.isnan(val[ex]) & np.isnan(ref[ex]))))
    return same, rel_dev(val[list(CLOSE_CH)], ref[list(CLOSE_CH)])


# ------------------------------------------------------------------ the hand-built cases
def open_spec(K=2):
    ''' the race track as an open line in the global frame: a gate on the first point, one on the last '''
    return product_spec(track='race', K=K, frame='global', N=7, closed=False, **MODELS['point'])


def _smooth(spec):
    ''' one decision vector (1, nw) of a global-frame problem: h = 0.2, the positions on the centreline at the
    nodes' own abscissae (n + tau_k) / phase -- node 0 of a gate's interval is the gate's centre -- everything
    else the cold start '''
    W = np.array(spec.w0, float)[None].copy()
    W[:, :spec.N] = 0.2
    V = _nodes(spec, W)
    tau = np.asarray(spec.tau, float)
    for n in range(spec.N):
        for k in range(spec.K1):
            V[0, n, k, :3] = spec.line.p2xc((n + tau[k]) / spec.guess_phase_len)
    return W


def _axes(planes, g):
    R = np.asarray(planes['R'][g], float).reshape(3, 3)
    return planes['centre'][g], R[:, 0], R[:, 1], R[:, 2]


def _end_weights(spec):
    ''' l_j(1): the interval's end value is their sum over the nodes '''
    return gatecheck_oracle.lagrange(spec.tau, [1.0])[0]


@functools.lru_cache(maxsize=None)
def identity_case(track):
    '''
    (spec, W (1, nw), offsets (G, 2)) in the global frame at K = 2: every gate node Z[interval, 0] lies on its
    gate's plane, ON_PLANE = 1e-13 m to the side the lap leaves the gate on (so that the sign of its rounding is
    known), at lateral offsets (p2, p3) = offsets[g]; the last node of the interval before it is moved along e1
    so that the interval ends 0.05 m before the plane. The only sign change near the gate is then the junction
    (interval, 0), and the far crossings of the plane have larger offsets.
    '''
    spec = case_spec(track, 'point', 'global', 2)
    planes = gate_planes(spec)
    W = _smooth(spec)
    V = _nodes(spec, W)
    G = len(spec.gates)
    rng = np.random.default_rng(11)
    offsets = 0.1 * planes['d_max'][:, None] * (rng.random((G, 2)) - 0.5)
    lend = _end_weights(spec)
    for g, gate in enumerate(spec.gates):
        n = gate['interval']
        c, e1, e2, e3 = _axes(planes, g)
        ahead = float((V[0, n, 1, :3] - c) @ e1)                 # the side the lap leaves on
        side = 1.0 if ahead >= 0 else -1.0
        V[0, n, 0, :3] = c + offsets[g, 0] * e2 + offsets[g, 1] * e3 + side * ON_PLANE * e1
        m = (n - 1) % spec.N
        end = lend @ V[0, m, :, :3]
        V[0, m, -1, :3] += (-side * 0.05 - float((end - c) @ e1)) * e1 / lend[-1]
    W.setflags(write=False)
    return spec, W, offsets


ON_PLANE = 1e-13


@functools.lru_cache(maxsize=None)
def frozen_case():
    '''
    (spec, W (1, nw), gate, x*) -- what the check is for. The race track, parametric, K = 2, N = 3, from the
    audit's blank vector. Interval 1 holds gates 3 and 4 at the Lagrange points d3 = 2 / 7 and d4 = 5 / 7. The
    nodes' s of that interval are shifted by a linear function of the abscissa that vanishes at d4 and moves the
    true crossing of gate 3's plane from d3 to x* = d3 + 0.1; y is the parabola with y(d3) = y(d4) = 0 and
    y(x*) = 1.5 d_max. The NLP places gate 3 through y(d3) = n(d3) = 0 in the frame frozen at the gate's s: its
    rows hold exactly. The trajectory itself crosses the plane at x*, 1.5 d_max off the centre.
    '''
    spec = case_spec('race', 'point', 'parametric', 2)
    W = _blank(spec)
    V = _nodes(spec, W)
    tau = np.asarray(spec.tau, float)
    g, n = 3, 1
    d3 = float((spec.line.config.s[3] - spec.get_s(1, 0)) / (spec.get_s(2, 0) - spec.get_s(1, 0)))
    d4 = float((spec.line.config.s[4] - spec.get_s(1, 0)) / (spec.get_s(2, 0) - spec.get_s(1, 0)))
    xs = d3 + 0.1
    s_of = lambda x: float(gatecheck_oracle.lagrange(tau, [x])[0] @ V[0, n, :, 0])      # noqa: E731
    delta = (float(spec.line.config.s[3]) - s_of(xs)) * (d3 - d4) / (xs - d4)
    V[0, n, :, 0] += delta * (tau - d4) / (d3 - d4)
    amp = 1.5 * spec.gates[g]['d_max'] / ((xs - d3) * (xs - d4))
    V[0, n, :, 1] = amp * (tau - d3) * (tau - d4)
    W.setflags(write=False)
    return spec, W, g, xs


@functools.lru_cache(maxsize=None)
def triple_case():
    '''
    (spec, W (1, nw), gate, interval) on the open race line, global frame, K = 9: the lap rests 0.5 m before the
    plane of gate 1 up to its interval, rests 0.5 m behind it afterwards, and in the interval itself
    a(x) = 4 (x - 0.23) (x - 0.52) (x - 0.81) -- out, back, out, no root on a sample abscissa of S = 1, 5 or 16 -- at
    the lateral offset p2(x) = d_max (0.1 + 2 ((x - 0.52) / 0.29)^2): 2.1 d_max at the outer crossings, 0.1 d_max at
    the middle one.
    '''
    spec = open_spec(9)
    planes = gate_planes(spec)
    g = 1
    n = spec.gates[g]['interval']
    c, e1, e2, _ = _axes(planes, g)
    W = _smooth(spec)
    V = _nodes(spec, W)
    tau = np.asarray(spec.tau, float)
    V[0, :n, :, :3] = c - 0.5 * e1
    V[0, n + 1:, :, :3] = c + 0.5 * e1
    a = 4 * (tau - 0.23) * (tau - 0.52) * (tau - 0.81)
    p2 = planes['d_max'][g] * (0.1 + 2 * ((tau - 0.52) / 0.29) ** 2)
    V[0, n, :, :3] = c + a[:, None] * e1 + p2[:, None] * e2
    W.setflags(write=False)
    return spec, W, g, n


@functools.lru_cache(maxsize=None)
def junction_case():
    '''
    (spec, W (2, nw), gate, interval m) on the closed race track, global frame, K = 2: the lap rests 0.3 m behind
    the plane of gate 2 in intervals 0 .. m - 1 and 0.3 m before it from interval m on, so the plane is crossed
    at the junction (m, 0) and at the closed wrap (0, 0) and nowhere else. Instance 0 sits nearer the centre
    before the plane (the junction is the best crossing), instance 1 behind it (the wrap is).
    '''
    spec = case_spec('race', 'point', 'global', 2)
    planes = gate_planes(spec)
    g, m = 2, 4
    c, e1, e2, e3 = _axes(planes, g)
    W = np.repeat(_smooth(spec), 2, axis=0)
    V = _nodes(spec, W)
    near, far = 0.2 * planes['d_max'][g], 0.6 * planes['d_max'][g]
    for b, (behind, before) in enumerate(((far, near), (near, far))):
        V[b, :m, :, :3] = c + 0.3 * e1 + behind * e2 - 0.1 * e3
        V[b, m:, :, :3] = c - 0.3 * e1 + before * e3 + 0.1 * e2
    W.setflags(write=False)
    return spec, W, g, m


@functools.lru_cache(maxsize=None)
def open_case():
    '''
    (spec, W (1, nw), first gate, last gate) on the open race line, global frame, K = 2: the smooth lap with its
    first point OFF_PLANE = 1e-8 m off the first gate's plane on the side the lap leaves on, and the last node of
    the last interval moved along the last gate's e1 so that the lap ends 1e-8 m short of that gate's plane: no
    sign change at either, rounding on the wrong side.
    '''
    spec = open_spec(2)
    planes = gate_planes(spec)
    W = _smooth(spec)
    V = _nodes(spec, W)
    c, e1, _, _ = _axes(planes, 0)
    side = 1.0 if float((V[0, 0, 1, :3] - c) @ e1) >= 0 else -1.0
    V[0, 0, 0, :3] = c + side * OFF_PLANE * e1
    last = len(spec.gates) - 1
    c, e1, _, _ = _axes(planes, last)
    lend = _end_weights(spec)
    side = 1.0 if float((V[0, -1, 0, :3] - c) @ e1) >= 0 else -1.0       # the side the lap comes from
    end = lend @ V[0, -1, :, :3]
    V[0, -1, -1, :3] += (side * OFF_PLANE - float((end - c) @ e1)) * e1 / lend[-1]
    W.setflags(write=False)
    return spec, W, 0, last


OFF_PLANE = 1e-8
