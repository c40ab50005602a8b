'''
Clearance of collocation solutions from an obstacle mesh on the device (ato_clearance: k_clearance_pos,
k_mesh_sdist_tiles): the cases of tests/test_clearance_cpu.py through BatchedNLP.clearance against the numpy
oracle and the CPU twin at the CPU constants, batches that cross a wave in both layouts, batch invariance, the
three distance paths on the same points, optional outputs, the weight re-upload, the error codes,
clearance_solutions and the solver classes' clearance().
'''
import functools

import numpy as np
import pytest

from aircraft_trajectory_optimization_amd import native
from tests import clearance_oracle
from tests.clearance_helpers import CASES, DIST_TOL, IL, IM, POS_TOL, SAMPLES, ClearanceTwin, MeshTwin, case_id, \
    case_inputs, case_spec, coherent_batch, mesh, oracle_distance, random_points, rel_dev
from tests.helpers import product_spec
from tests.replay_helpers import replay_inputs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def batched(spec, B, layout=IL):
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    return BatchedNLP(spec, B, layout=layout, buffers=False)


@functools.lru_cache(maxsize=None)
def device_mesh(name):
    from aircraft_trajectory_optimization_amd.obstacles.mesh_obstacle import MeshObstacle
    return MeshObstacle() if name == 'arena' else MeshObstacle.from_arrays(*mesh(name))


def host(pos, dist, layout):
    ''' -> pos (B, N, S1, 3), dist (B, N, S1) host arrays '''
    torch.cuda.synchronize()
    p = None if pos is None else pos.cpu().numpy()
    d = None if dist is None else dist.cpu().numpy()
    if layout == IL:
        p = None if p is None else np.ascontiguousarray(np.moveaxis(p, (0, 3), (3, 0)))
        d = None if d is None else np.ascontiguousarray(np.moveaxis(d, 2, 0))
    return p, d


def check_positions(spec, W, samples, layouts=(IL, IM), nlps=None):
    ''' device against oracle and twin at POS_TOL; returns whether device and twin agree bit for bit '''
    twin = ClearanceTwin(spec)
    exact = True
    for layout in layouts:
        nlp = nlps[layout] if nlps else batched(spec, W.shape[0], layout)
        for S in samples:
            p, d = host(*nlp.clearance(None, W, samples=S), layout)
            assert d is None
            t = twin.positions(W, S, layout)
            dev = max(rel_dev(p, clearance_oracle.positions(spec, W, S)), rel_dev(p, t))
            assert dev <= POS_TOL, (layout, S, dev)
            exact = exact and np.array_equal(p, t)
    return exact


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_device_positions_match_oracle_and_twin(case):
    spec = case_spec(*case)
    nlps = {layout: batched(spec, 3, layout) for layout in (IL, IM)}
    exact = all([check_positions(spec, W, SAMPLES, nlps=nlps) for W in case_inputs(*case)])
    print(f'clearance device vs twin {case_id(case)}: bit for bit {exact}')


@pytest.mark.parametrize('B', (65, 130))
@pytest.mark.parametrize('case', [('race', 'point', 'parametric', 2), ('obstacles', 'dcm', 'relative', 9),
                                  ('race', 'esp', 'global', 1)], ids=case_id)
def test_device_positions_across_a_wave(case, B):
    ''' B = 65 / 130 in both layouts: more than one wave per (interval, sample), B no multiple of the block '''
    spec = case_spec(*case)
    check_positions(spec, replay_inputs(spec, B, 4), (0, 5))


def test_batch_invariance():
    ''' column b of a B = 65 call equals its B = 1 call bit for bit, positions and distances '''
    spec, W, _ = coherent_batch(65, 5)
    m = device_mesh('lattice')
    p, d = host(*batched(spec, 65).clearance(m, W, samples=5), IL)
    one = batched(spec, 1)
    for b in range(65):
        p1, d1 = host(*one.clearance(m, W[b:b + 1], samples=5), IL)
        assert np.array_equal(p1[0], p[b]) and np.array_equal(d1[0], d[b]), b


def three_ways(m, X):
    ''' X (n, 3) host points -> the old kernel's, the strided cull = 0 and cull = 1 distances, as [n][3] and as
    [3][n]; asserts the strided four agree bit for bit '''
    n = len(X)
    X = np.array(X, np.float64)
    old = m.signed_distance(X)
    rows = torch.as_tensor(np.ascontiguousarray(X), device=m.device)
    cols = torch.as_tensor(np.ascontiguousarray(X.T), device=m.device)
    outs = [m.signed_distance_strided(rows, n, 3, 1, cull=c).cpu().numpy() for c in (False, True)] + \
           [m.signed_distance_strided(cols, n, 1, n, cull=c).cpu().numpy() for c in (False, True)]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0], equal_nan=True)
    return old, outs[0]


@pytest.mark.parametrize('name', ('box', 'lattice', 'lattice63'))
def test_three_distance_paths_agree_on_the_synthetic_meshes(name):
    m, twin = device_mesh(name), MeshTwin(*mesh(name))
    sets = [(random_points(name, n, seed), oracle_distance(name, n, seed)) for n, seed in ((65, 1), (130, 2))]
    if name != 'box':
        pos = coherent_batch()[2]
        X = np.ascontiguousarray(pos.reshape(3, -1).T)
        sets.append((X, clearance_oracle.signed_distance(X, *mesh(name))))
    for X, do in sets:
        old, new = three_ways(m, X)
        dev = max(rel_dev(old, do), rel_dev(new, do), rel_dev(new, twin.sdist(X)), rel_dev(new, old))
        print(f'clearance distance {name} n={len(X)}: dev {dev:.3e}, strided == old kernel bit for bit '
              f'{np.array_equal(old, new)}, == twin {np.array_equal(new, twin.sdist(X))}')
        assert np.array_equal(np.sign(new), np.sign(do)) and dev <= DIST_TOL, dev


def test_three_distance_paths_agree_on_the_arena():
    ''' 198 points along the obstacle track (the oracle is Python) '''
    spec = case_spec('obstacles', 'point', 'parametric', 2)
    W = replay_inputs(spec, 11, 7)
    pos = ClearanceTwin(spec).raw(W, 5, IL)[1]
    X = np.ascontiguousarray(pos.reshape(3, -1).T)
    assert len(X) == 198
    m = device_mesh('arena')
    old, new = three_ways(m, X)
    do = clearance_oracle.signed_distance(X, m.vertices, m.faces)
    dev = max(rel_dev(old, do), rel_dev(new, do), rel_dev(new, old))
    print(f'clearance distance arena: dev {dev:.3e}, strided == old kernel bit for bit {np.array_equal(old, new)}')
    assert (np.abs(do) >= 1e-6).all()                           # no sign depends on rounding
    assert np.array_equal(np.sign(new), np.sign(do)) and np.array_equal(np.sign(old), np.sign(do))
    assert dev <= DIST_TOL, dev


@pytest.mark.parametrize('name', ('box', 'lattice63'))
def test_non_finite_and_far_points_on_the_device(name):
    ''' the point sets of the CPU test: a non-finite first point of a wave, far and absurd points '''
    from tests.test_clearance_cpu import _odd_points
    m, twin = device_mesh(name), MeshTwin(*mesh(name))
    for first in ((np.inf, 0.5, 0.5), (np.nan, 0.5, 0.5), (1e160, 0.5, 0.5), (1e8, -3e7, 2e7)):
        X = _odd_points(name, first)
        old, new = three_ways(m, X)
        assert np.array_equal(old, new, equal_nan=True)
        sane = np.isfinite(X).all(axis=1) & (np.abs(X).max(axis=1) < 1e100)
        assert rel_dev(new[sane], twin.sdist(X)[sane]) <= DIST_TOL


def test_outputs_are_optional_and_samples_may_change():
    spec, W, _ = coherent_batch(65, 5)
    m, twin = device_mesh('lattice63'), ClearanceTwin(spec)
    nlp = batched(spec, 65)
    p5, d5 = nlp.clearance(m, W, samples=5)
    pn, dn = nlp.clearance(None, W, samples=5)                    # mesh = NULL: positions only
    assert dn is None and torch.equal(pn, p5)
    p0, d0 = nlp.clearance(m, W, samples=5, positions=False)      # pos = NULL: the same distances
    assert p0 is None and torch.equal(d0, d5)
    for cull in (False, True):
        assert torch.equal(nlp.clearance(m, W, samples=5, cull=cull)[1], d5)
    # another sample count on the same handle re-uploads the weights, and back again
    for S in (0, 16, 5, 1):
        p, _ = host(*nlp.clearance(None, W, samples=S), IL)
        assert rel_dev(p, twin.positions(W, S)) <= POS_TOL, S
    assert torch.equal(nlp.clearance(m, W, samples=5, positions=False)[1], d5)
    # the resident w of a batch with buffers
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    res = BatchedNLP(spec, 65)
    res.set_w(W)
    assert torch.equal(res.clearance(m, samples=5)[1], d5)


def test_error_codes_launch_nothing():
    rk4 = product_spec(track='race', N=7, K=2, rk4=True)
    par = case_spec('race', 'esp', 'parametric', 2)
    m = device_mesh('box')

    def call(nlp, S, batch=1, layout=IL, set_line=True):
        sp_ = nlp.spec
        if set_line and sp_.param and not sp_.rk4:
            nlp.problem.clearance_set_line(sp_.line_table())
        S1 = sp_.K1 if S <= 0 else min(S, 64) + 1
        w = torch.as_tensor(np.array(sp_.w0)[:, None].copy(), device=nlp.device)
        pos = torch.full((3 * sp_.N * S1,), -7.0, dtype=torch.float64, device=nlp.device)
        dist = torch.full((sp_.N * S1,), -7.0, dtype=torch.float64, device=nlp.device)
        rc = nlp.problem.clearance_rc(batch, w.data_ptr(), S, pos.data_ptr(), dist.data_ptr(), m.handle, 1, layout)
        torch.cuda.synchronize()
        return rc, bool((pos == -7.0).all() and (dist == -7.0).all())

    for spec, kw, code in ((rk4, dict(S=4), native.ATO_ERR_UNSUPPORTED),
                           (par, dict(S=4, set_line=False), native.ATO_ERR_STATE),
                           (par, dict(S=-1), native.ATO_ERR_ARG), (par, dict(S=65), native.ATO_ERR_ARG),
                           (par, dict(S=4, batch=0), native.ATO_ERR_ARG), (par, dict(S=4, layout=7), native.ATO_ERR_ARG)):
        nlp = batched(spec, 1)
        rc, untouched = call(nlp, **kw)
        assert rc == code, (kw, rc, nlp.problem.lib.ato_last_error())
        assert nlp.problem.lib.ato_last_error() and untouched
    with pytest.raises(NotImplementedError, match='not supported'):
        batched(rk4, 1).clearance(None, np.array(rk4.w0)[None], samples=4)
    for S in (0, 64):
        rc, untouched = call(batched(par, 1), S)
        assert rc == native.ATO_OK and not untouched


def test_clearance_solutions_on_host_and_device_inputs():
    from aircraft_trajectory_optimization_amd.raceline.clearance import clearance_solutions
    spec, W, pos = coherent_batch(65, 5)
    m = device_mesh('lattice')
    r = clearance_solutions(spec, W, m, samples=5)
    rd = clearance_solutions(spec, torch.as_tensor(np.ascontiguousarray(W.T), device=m.device), m, samples=5)
    for name in ('pos', 'dist', 'd_min', 'where', 'gap', 'passed', 'certified'):
        assert torch.equal(getattr(r, name), getattr(rd, name)), name
    assert r.pos.shape == (3, 3, 6, 65) and r.dist.shape == (3, 6, 65) and r.where.shape == (65, 2)
    assert r.collision_radius == spec.vehicle.collision_radius
    p, d = r.pos.cpu().numpy(), r.dist.cpu().numpy()
    assert rel_dev(p, pos) <= POS_TOL
    assert np.array_equal(r.d_min.cpu().numpy(), d.reshape(-1, 65).min(0))
    wh = r.where.cpu().numpy()
    assert np.array_equal(d[wh[:, 0], wh[:, 1], np.arange(65)], d.reshape(-1, 65).min(0))
    gap = np.linalg.norm(np.diff(p, axis=2), axis=0).reshape(-1, 65).max(0)
    assert rel_dev(r.gap.cpu().numpy(), gap) <= 1e-14
    rc = spec.vehicle.collision_radius
    assert np.array_equal(r.passed.cpu().numpy(), r.d_min.cpu().numpy() >= rc)
    assert np.array_equal(r.certified.cpu().numpy(), (r.d_min - r.gap / 2).cpu().numpy() >= rc)
    assert not bool(r.passed.all()) and bool(clearance_solutions(spec, W, m, samples=5, collision_radius=-10.0).certified.all())
    # one vector, and the nodes only
    one = clearance_solutions(spec, W[0], m, samples=0)
    assert one.dist.shape == (3, 3, 1) and torch.equal(one.pos[..., 0], clearance_solutions(spec, W, m, samples=0).pos[..., 0])


def test_flown_trajectory_against_the_old_kernel():
    from aircraft_trajectory_optimization_amd.raceline.clearance import clearance_solutions
    spec, W, _ = coherent_batch(65, 5)
    m = device_mesh('lattice')
    r = clearance_solutions(spec, W, m, samples=4, flown=True)
    traj = batched(spec, 65).replay(W, substeps=4, trajectory=True)[2]           # (N, 4, nz, B)
    torch.cuda.synchronize()
    X = traj.cpu().numpy()[:, :, :3, :]                                          # (N, 4, 3, B)
    assert r.flown and r.pos.shape == (3, 3, 4, 65) and np.array_equal(r.pos.cpu().numpy(), np.moveaxis(X, 2, 0))
    old = m.signed_distance(np.ascontiguousarray(np.moveaxis(X, 2, 3)).reshape(-1, 3)).reshape(3, 4, 65)
    assert rel_dev(r.dist.cpu().numpy(), old) <= DIST_TOL
    assert np.array_equal(r.d_min.cpu().numpy(), r.dist.cpu().numpy().reshape(-1, 65).min(0))
    with pytest.raises(ValueError):
        clearance_solutions(spec, W, m, samples=0, flown=True)


def test_solver_class_clearance():
    ''' clearance() of an obstacle raceline class at B = 1: clearance_solutions, and _unpack's node distances '''
    from aircraft_trajectory_optimization_amd.pytypes import PointConfig
    from aircraft_trajectory_optimization_amd.raceline.clearance import clearance_solutions
    from aircraft_trajectory_optimization_amd.raceline.config import ParametricRacelineConfig
    from aircraft_trajectory_optimization_amd.raceline.solvers import ParametricObstaclePointRaceline
    from aircraft_trajectory_optimization_amd.tracks import make_line
    line = make_line('obstacles')
    line.config.gate_s = None
    cfg = ParametricRacelineConfig(verbose=False, N=6, K=3)
    cfg.closed = True
    cfg.fixed_gates = []
    m = device_mesh('arena')
    solver = ParametricObstaclePointRaceline(line, cfg, PointConfig(global_r=True, collision_radius=0.4), m)
    x = np.array(solver.spec.w0)
    states = solver.get_ws().states                                   # _unpack stores state.d at the nodes
    nodes = solver.clearance(x, samples=0)
    d_nodes = np.array([st.d for st in states]).reshape(6, 4)
    # the two node positions agree to POS_TOL and the distance is 1-Lipschitz in the position
    assert rel_dev(nodes.dist.cpu().numpy()[..., 0], d_nodes) <= DIST_TOL + POS_TOL * max(1.0, np.abs(x).max())
    assert nodes.collision_radius == 0.4 and bool(nodes.passed[0]) == bool(d_nodes.min() >= 0.4)
    dense = solver.clearance(x)
    ref = clearance_solutions(solver.spec, x[None], m, samples=16, collision_radius=0.4)
    for name in ('pos', 'dist', 'd_min', 'where', 'gap', 'passed', 'certified'):
        assert torch.equal(getattr(dense, name), getattr(ref, name)), name
    assert dense.dist.shape == (6, 17, 1) and torch.equal(dense.dist[:, 0], nodes.dist[:, 0])    # sample 0 is node 0
