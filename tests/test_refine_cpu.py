'''
Refinement on the CPU: the solved point-mass raceline (racetrack, parametric, N = 10, K = 3) transferred
by the twin to refined_spec(spec, 2) and warm-solved there by the host solver replays better than the
coarse solution; refined_spec carries the closure branch and refuses what it cannot rebuild.

Measured (host IPM, oracle replay, 16 substeps): coarse optimal in 44 iterations, replay 3.97 m; refined
optimal in 62 iterations, replay 1.02 m.
'''
import numpy as np
import pytest

from tests import replay_oracle
from tests.helpers import HostEvaluator, product_spec
from tests.remesh_helpers import RemeshTwin


def test_warm_resolve_on_the_refined_mesh_replays_better():
    from aircraft_trajectory_optimization_amd.raceline.refine import refined_spec
    from aircraft_trajectory_optimization_amd.solver.ipm import InteriorPointSolver, IPMOptions
    spec = product_spec(track='race', model='point', use_quat=False, N=10, K=3)
    ev = HostEvaluator(spec)
    coarse = InteriorPointSolver(ev, spec.lbw, spec.ubw, ev.lbg, ev.ubg, IPMOptions(max_iter=200)).solve(spec.w0)
    assert coarse.status == 'optimal', coarse.status
    fine = refined_spec(spec, 2)
    assert (fine.N, fine.K) == (20, 3)
    w0 = RemeshTwin(spec, fine).remesh(coarse.x[None])[0]
    lbw, ubw = fine.lbw.copy(), fine.ubw.copy()
    lbw[:fine.N], ubw[:fine.N] = w0[:fine.N] / 100, w0[:fine.N] * 10
    fev = HostEvaluator(fine)
    res = InteriorPointSolver(fev, lbw, ubw, fev.lbg, fev.ubg, IPMOptions(max_iter=200)).solve(w0)
    before = replay_oracle.replay(spec, coarse.x, 16)[1][:, 0].max()
    after = replay_oracle.replay(fine, res.x, 16)[1][:, 0].max()
    print(f'coarse: {coarse.status}, {coarse.iters} it, replay {before:.3e} m; refined: {res.status}, '
          f'{res.iters} it, replay {after:.3e} m')
    assert res.status == 'optimal', res.status
    assert after < before


def test_refined_spec_carries_the_closure_branch():
    from aircraft_trajectory_optimization_amd.raceline.refine import refined_spec
    q = product_spec(track='race', N=4, K=2, quat_flip=True)
    fq = refined_spec(q, 3, K=4)
    assert (fq.N, fq.K, fq.quat_flip, fq.euler_wraps) == (12, 4, True, 0.0)
    assert fq.line is q.line and fq.vehicle is q.vehicle and fq.frame == q.frame
    assert q.N == 4 and q.config.N == 4                    # the source spec and its config are left alone
    e = product_spec(track='race', N=4, K=2, use_quat=False, euler_wraps=-1.0)
    fe = refined_spec(e)
    assert (fe.N, fe.K, fe.quat_flip, fe.euler_wraps) == (8, 2, False, -1.0)
    assert fe.native_spec()['euler_wraps'] == -1.0 and fq.native_spec()['quat_flip']
    g = refined_spec(product_spec(track='race', model='point', use_quat=False, frame='global', N=3, K=2), 2)
    assert g.N == 14                                       # the global frame had rounded 3 up to its 7 gate phases


def test_refined_spec_refuses_what_it_cannot_rebuild():
    from aircraft_trajectory_optimization_amd.raceline.refine import refined_spec
    plain = product_spec(track='race', model='point', use_quat=False, N=4, K=2)
    obstacle = product_spec(track='race', model='point', use_quat=False, N=4, K=2,
                            spheres=np.tile([0.0, 0.0, 1.0], (plain.P, 1)))
    with pytest.raises(NotImplementedError, match='depend on N'):
        refined_spec(obstacle)
    cpc = product_spec(track='race', model='point', use_quat=False, frame='global', N=7, K=2,
                       cpc={'waypoints': None, 'tol': 0.3})
    with pytest.raises(NotImplementedError, match='CPC'):
        refined_spec(cpc)
    rk4 = product_spec(track='race', N=7, K=2, rk4=True)
    with pytest.raises(NotImplementedError, match='RK4'):
        refined_spec(rk4)
    with pytest.raises(ValueError):
        refined_spec(plain, 0)
