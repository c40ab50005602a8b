'''
Whole-interval extrema on the device (ato_extrema: k_extrema, k_ext_combine) against a long-double oracle: the
candidates {0, 1} and the real roots of the derivative in (0, 1) (numpy polyroots of the power form, two Newton
steps in long double), random decision vectors over degrees, frames and layouts, planted cases, batch invariance,
extrema_solutions and the rejections.

TOL: csrc/ato_extrema.hpp derives slack < 2^-42 scale for a finished search, scale = max(1, max_i sum_j |T[i][j]|
|V_j|) (for s': 2 K scale / h_n); a reported extremum is an attained value and the true one lies within slack of
it, so |device - oracle| <= 2^-42 scale = 2.27e-13 scale is the derived bound the test holds. Measured on an MI355X:
at most 2.6e-14 scale (profiles/extrema/oracle_diff.txt), so the bound is 8.8 times the measured figure. The
slack assertion keeps the issue's 2^-40, against this scale and against the largest |root coefficient|.
'''
import numpy as np
import pytest

from aircraft_trajectory_optimization_amd import native
from tests.replay_helpers import FRAMES, MODELS
from tests.helpers import product_spec

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
LD = np.longdouble
IL, IM = native.ATO_LAYOUT_INTERLEAVED, native.ATO_LAYOUT_INSTANCE_MAJOR
TOL = 2.0 ** -42
SLACK = 2.0 ** -40


def spec_of(model, frame, K):
    return product_spec(track='race', K=K, **{**MODELS[model], **FRAMES[frame]})


def lagrange_power(tau, V):
    ''' power-form coefficients (ascending, long double) of the interpolant of V over tau '''
    tau, out = np.asarray(tau, LD), np.zeros(len(tau), LD)
    for j, vj in enumerate(V):
        c = np.array([LD(vj)])
        for r in range(len(tau)):
            if r != j:
                c = (np.append(LD(0), c) - np.append(c * tau[r], LD(0))) / (tau[j] - tau[r])
        out += c
    return out


def horner(c, x):
    acc = LD(0)
    for a in c[::-1]:
        acc = acc * x + a
    return acc


def lagrange_value(tau, V, x):
    tau, acc = np.asarray(tau, LD), LD(0)
    for j in range(len(tau)):
        lj = LD(1)
        for r in range(len(tau)):
            if r != j:
                lj *= (LD(x) - tau[r]) / (tau[j] - tau[r])
        acc += lj * LD(V[j])
    return acc


def oracle(tau, V, deriv=False, h=1.0):
    ''' (min, max) over [0, 1] of the interpolant of V (deriv: of its derivative / h), long double '''
    c = lagrange_power(tau, V)
    der = lambda q: q[1:] * np.arange(1, len(q), dtype=LD)      # noqa: E731
    if deriv:
        c = der(c) / LD(h)
    d1 = der(c)
    cand = [LD(0), LD(1)]
    if len(d1) > 1 and np.any(d1[1:] != 0):
        for r in np.polynomial.polynomial.polyroots(d1.astype(np.float64)):
            if abs(r.imag) < 1e-6:
                x = LD(r.real)
                for _ in range(2):
                    s = horner(der(d1), x)
                    x = x - horner(d1, x) / s if s != 0 else x
                if 0 < x < 1:
                    cand.append(x)
    vals = [horner(c, x) if deriv else lagrange_value(tau, V, x) for x in cand]
    return min(vals), max(vals)


def device(spec, W, layout=IL, intervals=True):
    ''' -> val (8, NVX, B), ival (NVX, N, 2, B) host arrays '''
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    val, ival = BatchedNLP(spec, len(W), layout=layout, buffers=False).extrema(W, intervals=intervals)
    torch.cuda.synchronize()
    val, ival = val.cpu().numpy(), None if ival is None else ival.cpu().numpy()
    if layout == IM:
        val, ival = val.transpose(2, 1, 0), None if ival is None else ival.transpose(1, 2, 3, 0)
    return val, ival


def nodes(spec, W):
    ''' h (B, N) and V (B, N, K1, nv) views of host decision vectors '''
    return W[:, :spec.N], W[:, spec.N:].reshape(len(W), spec.N, spec.K1, spec.nv)


def random_w(spec, B, seed):
    W = np.random.default_rng(seed).normal(size=(B, spec.nw)) * 3.0
    W[:, :spec.N] = 0.05 + 0.1 * np.abs(W[:, :spec.N])
    return W


@pytest.mark.parametrize('layout', (IL, IM))
@pytest.mark.parametrize('frame', ('global', 'parametric'))
@pytest.mark.parametrize('K', (1, 2, 4, 9))
def test_random_vectors_against_the_oracle(K, frame, layout):
    spec = spec_of('point', frame, K)
    W = random_w(spec, 5, 100 + K)
    h, V = nodes(spec, W)
    val, ival = device(spec, W, layout)
    Tc = native.extrema_table(spec.tau)
    T = np.abs(Tc)
    nvx = spec.nv + (1 if spec.param else 0)
    assert val.shape == (8, nvx, 5)
    worst = 0.0
    for b in range(5):
        for v in range(nvx):
            dv = v == spec.nv
            Vn = V[b, :, :, 0 if dv else v]
            A = (T @ np.abs(Vn).T).max(axis=0)                                   # (N,)
            scale = max(1.0, (2 * K * A / h[b]).max() if dv else A.max())
            ref = [oracle(spec.tau, Vn[n], dv, h[b, n]) for n in range(spec.N)]
            omin, omax = min(r[0] for r in ref), max(r[1] for r in ref)
            mn, mx, slack = (LD(val[c, v, b]) for c in (0, 3, 6))
            assert val[7, v, b] == 0.0
            assert omax <= mx + slack and omin >= mn - slack, (v, b)
            assert 0.0 <= slack <= SLACK * scale, (v, b, float(slack), scale)
            if not dv:      # the issue's own scale too: the largest |root coefficient|
                assert slack <= SLACK * max(1.0, np.abs(Tc @ Vn.T).max()), (v, b, float(slack))
            dev = float(max(abs(mx - omax), abs(mn - omin))) / scale
            worst = max(worst, dev)
            assert dev <= TOL, (v, b, dev)
            if not dv:
                assert mx >= Vn.max() - TOL * scale and mn <= Vn.min() + TOL * scale
                for c in (0, 3):
                    n, x = int(val[c + 1, v, b]), val[c + 2, v, b]
                    assert abs(lagrange_value(spec.tau, Vn[n], x) - val[c, v, b]) <= TOL * scale
            assert ival[v, :, 0, b].min() == val[0, v, b] and ival[v, :, 1, b].max() == val[3, v, b]
    print(f'extrema vs oracle K={K} {frame} layout={layout}: worst |dev - oracle| / scale = {worst:.3e}')


@pytest.fixture(scope='module')
def planted():
    ''' the point mass, parametric, K = 2, N = 3: a base line of constants and its extrema '''
    spec = spec_of('point', 'parametric', 2)
    W = np.tile(np.arange(1.0, spec.nw + 1.0) % 7.0 - 3.0, (3, 1))
    W[:, :spec.N] = 0.1
    _, V = nodes(spec, W)
    V[:] = V[:, :1, :1, :]                                   # every component constant over the lap
    return spec, W, device(spec, W)[0]


def parabola(spec, sign, xs):
    return sign * (1.0 - (np.asarray(spec.tau) - xs) ** 2)


@pytest.mark.parametrize('case', ('constant', 'linear', 'vertex_max', 'vertex_min', 'tie', 'nan', 'h_zero'))
def test_planted_cases(planted, case):
    spec, W0, base = planted
    W = W0.copy()
    h, V = nodes(spec, W)
    tau, N, v = np.asarray(spec.tau), spec.N, 4
    xs = 0.5 * (tau[1] + tau[2])
    if case == 'linear':
        V[:, :, :, v] = np.arange(N)[:, None] + tau[None, :]
    elif case in ('vertex_max', 'vertex_min'):
        sign = 1.0 if case == 'vertex_max' else -1.0
        V[:, :, :, v] = -5.0 * sign
        V[:, 1, :, v] = parabola(spec, sign, xs)
    elif case == 'tie':
        V[:, :, :, v] = -5.0
        V[:, 0, :, v] = V[:, 2, :, v] = parabola(spec, 1.0, xs)
    elif case == 'nan':
        V[2, 1, 1, v] = np.nan
    elif case == 'h_zero':
        h[1, 1] = 0.0
    val = device(spec, W, intervals=False)[0]
    rec = val[:, v, 0]
    if case == 'constant':
        assert np.array_equal(val[[1, 2, 4, 5, 6, 7], :spec.nv], np.zeros((6, spec.nv, 3)))
        assert np.array_equal(val[0, :spec.nv], V[:, 0, 0, :].T) and np.array_equal(val[3], val[0])
    elif case == 'linear':
        assert tuple(rec[[1, 2, 4, 5]]) == (0.0, 0.0, N - 1.0, 1.0) and rec[0] == 0.0
        assert abs(rec[3] - N) <= TOL * N
    elif case in ('vertex_max', 'vertex_min'):
        c = 3 if case == 'vertex_max' else 0
        assert rec[c + 1] == 1.0 and abs(rec[c + 2] - xs) < 1e-6 and abs(abs(rec[c]) - 1.0) <= SLACK
        assert tau[1] < rec[c + 2] < tau[2]
    elif case == 'tie':
        assert rec[4] == 0.0 and abs(rec[5] - xs) < 1e-6
    else:
        hit = np.zeros(val.shape[1:], bool)
        hit[(v, 2) if case == 'nan' else (spec.nv, 1)] = True
        assert np.isnan(val[7][hit]).all() and np.array_equal(val[:, ~hit], base[:, ~hit])
        assert not np.isnan(val[[0, 3]][:, hit]).any()


@pytest.mark.parametrize('B,col', ((5, 3), (70, 67)))
def test_batch_invariance(B, col):
    spec = spec_of('esp', 'parametric', 4)
    W = random_w(spec, B, 7)
    many, one = device(spec, W), device(spec, W[col:col + 1])
    assert np.array_equal(many[0][:, :, col], one[0][:, :, 0]) and np.array_equal(many[1][..., col], one[1][..., 0])


def test_extrema_solutions_finds_an_overshoot_between_nodes():
    from aircraft_trajectory_optimization_amd.raceline.audit import audit_solutions, extrema_solutions, path_bounds
    spec = spec_of('esp', 'global', 4)
    lb, ub = path_bounds(spec, varying='outer')
    lo, hi = np.isfinite(lb), np.isfinite(ub)
    mid = np.zeros(spec.nv)
    mid[lo & hi] = 0.5 * (lb[lo & hi] + ub[lo & hi])
    mid[lo & ~hi], mid[hi & ~lo] = lb[lo & ~hi] + 1.0, ub[hi & ~lo] - 1.0
    X = np.concatenate([np.full(spec.N, 0.1), np.tile(mid, spec.P)])[None].repeat(2, axis=0)
    _, V = nodes(spec, X)
    tau, u = np.asarray(spec.tau), spec.nz
    xs, d = 0.5 * (tau[2] + tau[3]), 0.5 * (tau[3] - tau[2])
    V[1, 2, :, u] = ub[u] + 0.5 * d * d - (tau - xs) ** 2        # every node below ub, the vertex 0.5 d^2 above it
    assert (V[1, 2, :, u] < ub[u]).all()
    over = float(oracle(tau, V[1, 2, :, u])[1] - LD(ub[u]))
    assert abs(over - 0.5 * d * d) < 1e-12
    big = np.full(spec.nw, np.inf)
    lbw, ubw = (np.concatenate([s * big[:spec.N], np.tile(b, spec.P)]) for s, b in ((-1.0, lb), (1.0, ub)))
    assert bool(audit_solutions(spec, X, samples=0, LBW=lbw, UBW=ubw).passed.all())
    res = extrema_solutions(spec, X, lb=lb, ub=ub)
    assert res.passed.tolist() == [True, False] and res.certified.tolist() == [True, False]
    m = res.margin[1].cpu().numpy()
    assert m[4] < -1e-6 and (np.delete(m, 4) >= 0.0).all()
    o = res.overshoot.cpu().numpy()
    scale = max(1.0, (np.abs(native.extrema_table(tau)) @ np.abs(V[1, 2, :, u])).max())
    assert abs(o[u, 1] - over) <= TOL * scale and np.count_nonzero(o) == 1


def test_rejections_leave_val_untouched():
    par, rk4 = spec_of('esp', 'parametric', 2), product_spec(track='race', N=7, K=2, rk4=True)
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    val = torch.full((8 * 64,), -7.0, dtype=torch.float64, device='cuda')

    def call(spec, batch=1, layout=IL, w=True):
        nlp = BatchedNLP(spec, 1, layout=IL, buffers=False)
        W = torch.as_tensor(np.array(spec.w0), device='cuda')
        rc = nlp.problem.extrema_rc(batch, W.data_ptr() if w else 0, val.data_ptr(), layout=layout)
        torch.cuda.synchronize()
        return rc

    for spec, kw, code in ((rk4, {}, native.ATO_ERR_UNSUPPORTED), (par, dict(batch=0), native.ATO_ERR_ARG),
                           (par, dict(layout=7), native.ATO_ERR_ARG), (par, dict(w=False), native.ATO_ERR_ARG)):
        assert call(spec, **kw) == code, kw
        assert bool((val == -7.0).all())
    assert call(par) == native.ATO_OK and not bool((val[:8 * (par.nv + 1)] == -7.0).any())
    with pytest.raises(NotImplementedError, match='RK4'):
        BatchedNLP(rk4, 1, buffers=False).extrema(np.array(rk4.w0)[None])
