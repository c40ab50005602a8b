'''
Replay of collocation solutions through the vehicle ODE, on the CPU: the twin of the device kernel
(tests/native/replay_hostcheck.cpp runs csrc/ato_replay.hpp's replay_interval) against the numpy
oracle (tests/replay_oracle.py), and properties that need no oracle (hover, RK4's order, the lift).
'''
import numpy as np
import pytest

from aircraft_trajectory_optimization_amd import native
from tests import replay_oracle
from tests.helpers import HostEvaluator, product_spec
from tests.replay_helpers import CASES, MODELS, PARITY_TOL, ReplayTwin, case_id, case_spec, rel_dev, replay_inputs

B = 3


def make_twin(spec):
    tw = ReplayTwin(spec)
    if spec.param:
        tw.set_lift(spec.lift_table())
    return tw


def test_parity_constant_is_capped():
    assert PARITY_TOL <= 1e-9


def test_weight_table_is_the_formula():
    for K in (1, 2, 9):
        spec = case_spec('point', 'parametric', K)
        tw = ReplayTwin(spec)
        for S in (1, 4):
            lw = tw.weights(S)
            assert np.array_equal(lw, replay_oracle.weights(spec.tau, S))
            assert np.abs(lw.sum(1) - 1).max() <= 1e-9
            # the interpolant of interpolate_collocation: l_j(tau_r) = delta_jr, l_j(1) = D_j
            assert np.allclose(lw[-1], spec.D, rtol=0, atol=1e-9 * np.abs(spec.D).max())


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_twin_matches_oracle(case):
    model, frame, K, S = case
    spec = case_spec(model, frame, K)
    W = replay_inputs(spec, B)
    zs, er, tj = make_twin(spec).replay(W, S, traj=True)
    dev = 0.0
    for b in range(B):
        zo, eo, to = replay_oracle.replay(spec, W[b], S)
        dev = max(dev, rel_dev(zs[b], zo), rel_dev(er[b], eo), rel_dev(tj[b], to))
    print(f'replay twin vs oracle {case_id(case)}: {dev:.3e}')
    assert np.array_equal(tj[:, :, -1], zs)
    assert dev <= PARITY_TOL, dev


def test_twin_layouts_agree():
    spec = case_spec('esp', 'parametric', 2)
    W = replay_inputs(spec, B)
    tw = make_twin(spec)
    a = tw.replay(W, 4, traj=True)
    b = tw.replay(W, 4, traj=True, layout=native.ATO_LAYOUT_INTERLEAVED)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('model', ['esp', 'ypr', 'dcm'])
def test_hover_stays_put(model):
    ''' identity attitude, zero velocities, every rotor at m g / 4, the same state at every node '''
    spec = case_spec(model, 'global', 2)
    v = spec.vehicle
    att = {'esp': [0, 0, 0, 1], 'ypr': [0, 0, 0], 'dcm': [1, 0, 0, 0, 1, 0, 0, 0, 1]}[model]
    z0 = np.array([0.3, -1.2, 2.0, *att, 0, 0, 0, 0, 0, 0], float)
    w = np.zeros(spec.nw)
    w[:spec.N] = np.linspace(0.05, 0.3, spec.N)
    nodes = w[spec.N:].reshape(spec.P, spec.nv)
    nodes[:, :spec.nz] = z0
    nodes[:, spec.nz:spec.nz + 4] = v.m * v.g / 4
    for S in (1, 4):
        zs, er, _ = make_twin(spec).replay(w[None], S)
        assert np.abs(zs[0] - z0).max() <= 1e-13
        assert er.max() <= 1e-13


def test_rk4_order():
    ''' Delta(S) = zsim(S) - zsim(8 S) on a smooth input: global error ~ (h / S)^4, ratio 16 '''
    spec = case_spec('esp', 'global', 2)
    W = replay_inputs(spec, 1, seed=3)
    W[:, :spec.N] = 0.3
    tw = make_twin(spec)
    z = {S: tw.replay(W, S)[0] for S in (2, 4, 16, 32)}
    ratio = np.linalg.norm(z[2] - z[16]) / np.linalg.norm(z[4] - z[32])
    print(f'replay RK4 order ratio: {ratio:.2f}')
    assert 8 <= ratio <= 32, ratio


@pytest.mark.parametrize('model', ['esp', 'point'])
def test_lift_matches_global_frame(model):
    ''' a parametric w and a global-frame w of the same track, N, K with the lifted start states and the
    same h and U replay to the same states '''
    K = 2
    sg = case_spec(model, 'global', K)
    sp_ = product_spec(track='race', K=K, frame='parametric', N=sg.N, global_r=True, **MODELS[model])
    assert (sp_.N, sp_.nz, sp_.nv) == (sg.N, sg.nz, sg.nv)
    wp = replay_inputs(sp_, 1, seed=5)[0]
    wg = wp.copy()
    Zp = wp[sp_.N:].reshape(sp_.N, sp_.K1, sp_.nv)
    Zg = wg[sg.N:].reshape(sg.N, sg.K1, sg.nv)
    Zg[:, 0, :sg.nz] = replay_oracle.lift(sp_, Zp[:, 0, :sp_.nz], sp_.interval_s[:sp_.N])
    for S in (1, 4):
        zp = make_twin(sp_).replay(wp[None], S)[0]
        zg = make_twin(sg).replay(wg[None], S)[0]
        dev = rel_dev(zp, zg)
        print(f'replay lift {model} S={S}: {dev:.3e}')
        assert dev <= PARITY_TOL, dev


def test_lift_table_rows():
    spec = case_spec('esp', 'parametric', 2)
    t = spec.lift_table()
    assert t.shape == (spec.N + 1, 12)
    assert spec.interval_s[-1] == pytest.approx(spec.line.s_max())
    for n in (0, spec.N):
        s = float(spec.interval_s[n])
        assert np.array_equal(t[n, :3], spec.line.p2xc(s))
        Rp = t[n, 3:].reshape(3, 3)
        assert np.array_equal(Rp[:, 1], spec.line.p2ey(s)) and np.array_equal(Rp[:, 2], spec.line.p2en(s))
        assert np.abs(Rp.T @ Rp - np.eye(3)).max() <= 1e-12
    # the node geometry of node (n, 0) carries the same frame
    assert np.allclose(t[:spec.N, 3:], spec.node_geom[::spec.K1, :9], rtol=0, atol=1e-14)


def test_error_codes():
    rk4 = product_spec(track='race', N=7, K=2, rk4=True)
    rel = product_spec(track='fig8', N=3, K=2, global_r=False)
    par = case_spec('esp', 'parametric', 2)
    for spec, code in ((rk4, native.ATO_ERR_UNSUPPORTED), (rel, native.ATO_ERR_UNSUPPORTED),
                       (par, native.ATO_ERR_STATE)):
        tw = ReplayTwin(spec)
        assert tw.replay_rc(np.array(spec.w0)[None], 4)[0] == code
    tw = make_twin(par)
    for S in (0, 65):
        assert tw.replay_rc(np.array(par.w0)[None], S)[0] == native.ATO_ERR_ARG
    assert tw.replay_rc(np.array(par.w0)[None], 64)[0] == native.ATO_OK


def test_cpc_variables_are_ignored():
    ''' CPC problems carry their progress variables after the node block: the replay does not read them '''
    spec = product_spec(track='race', frame='global', N=7, K=2, cpc={'tol': 0.3})
    W = replay_inputs(spec, 1)
    W2 = W.copy()
    W2[:, spec.cpc_off:] += 1.0
    tw = make_twin(spec)
    a, b = tw.replay(W, 4), tw.replay(W2, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    zo, eo, _ = replay_oracle.replay(spec, W[0], 4)
    assert max(rel_dev(a[0][0], zo), rel_dev(a[1][0], eo)) <= PARITY_TOL


def test_solved_point_mass_trajectory():
    ''' the point-mass solution of test_ipm_point_mass_converges_to_kkt_point: twin and oracle report
    the same four errors (their size is recorded in DESIGN, not bounded here) '''
    from aircraft_trajectory_optimization_amd.solver.ipm import InteriorPointSolver, IPMOptions
    spec = product_spec(track='race', model='point', use_quat=False, N=10, K=3)
    ev = HostEvaluator(spec)
    res = InteriorPointSolver(ev, spec.lbw, spec.ubw, ev.lbg, ev.ubg, IPMOptions(max_iter=200)).solve(spec.w0)
    assert res.status == 'optimal', res.status
    zs, er, _ = make_twin(spec).replay(res.x[None], 16)
    zo, eo, _ = replay_oracle.replay(spec, res.x, 16)
    print('replay of the solved point-mass raceline (oracle): max position error '
          f'{eo[:, 0].max():.3e} m, velocity error {eo[:, 2].max():.3e} m/s')
    assert rel_dev(er[0], eo) <= PARITY_TOL and rel_dev(zs[0], zo) <= PARITY_TOL
    assert np.all(er[0][:, [1, 3]] == 0)
