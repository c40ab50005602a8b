'''
ORACLE (test infrastructure only) of the gate-passage check, in numpy, written from the definition in
include/ato.h and independent of csrc/ato_gatecheck.hpp (it calls no twin): positions by a vectorised Lagrange sum
and the product's own line.p2x (as tests/clearance_oracle.py), the crossings of a gate's plane
  - in the global frame from the roots of a(x), a degree-K polynomial per interval, through its monomial
    coefficients (numpy.roots), each root then polished inside the first bracket of +-POLISH (x 10, x 100) around
    it that holds a sign change (the monomial basis of K = 9 loses digits the comparison needs),
  - in the parametric frame from the sign changes of a grid FINE x finer than the kernel's,
every bracket refined by a bracketing root finder on the Lagrange form (bisection, all brackets of a call at once
so that the centreline is evaluated by one p2x per step; the root is the midpoint of the last bracket), and the
margins by plain numpy formulas. It also reports the conditions the tests ask of their inputs.
'''
import numpy as np

NCH = 9
FINE = 16
POLISH = 1e-6
HALVINGS = 64
CIRCLE, SQUARE = 0, 1


def lagrange(tau, xs):
    ''' [len(xs)][K + 1] l_j(x) '''
    tau, xs = np.asarray(tau, float), np.atleast_1d(np.asarray(xs, float))
    out = np.ones((len(xs), len(tau)))
    for j in range(len(tau)):
        for r in range(len(tau)):
            if r != j:
                out[:, j] *= (xs - tau[r]) / (tau[j] - tau[r])
    return out


def nodes3(spec, W):
    ''' (B, N, K1, 3): the first three state components of every node '''
    W = np.atleast_2d(np.asarray(W, float))
    return W[:, spec.N:spec.N + spec.P * spec.nv].reshape(W.shape[0], spec.N, spec.K1, spec.nv)[..., :3]


def lift(spec, q):
    ''' (..., 3) (s, y, n) -> global positions; the global frame's are positions already '''
    if not spec.param:
        return q
    flat = q.reshape(-1, 3)
    return spec.line.p2x(flat[:, 0], flat[:, 1], flat[:, 2]).T.reshape(q.shape)


def grid_positions(spec, W, xs):
    ''' global positions (B, N, len(xs), 3) of every interval at the abscissae xs '''
    return lift(spec, np.einsum('ij,bnjc->bnic', lagrange(spec.tau, xs), nodes3(spec, W)))


def coords(planes, X):
    ''' (a, p2, p3) (G, ..., 3) of global positions X (..., 3) in every gate's frame '''
    c, R = np.asarray(planes['centre'], float), np.asarray(planes['R'], float)
    return np.stack([(X - c[g]) @ R[g] for g in range(len(c))])


def margin(planes, g, p2, p3):
    if int(planes['shape'][g]) == CIRCLE:
        return planes['d_max'][g] - np.sqrt(p2 ** 2 + p3 ** 2)
    return planes['d_max'][g] - np.maximum(np.abs(p2), np.abs(p3))


def point_coords(spec, planes, Z, g, b, n, x):
    ''' (a, p2, p3) (M, 3) at abscissa x[m] of interval n[m] of instance b[m] in gate g[m]'s frame '''
    q = lift(spec, np.einsum('mj,mjc->mc', lagrange(spec.tau, x), Z[b, n]))
    c, R = np.asarray(planes['centre'], float), np.asarray(planes['R'], float)
    return np.einsum('mc,mci->mi', q - c[g], R[g])


def brackets(spec, planes, W, samples):
    ''' (g, b, n, lo, hi) arrays: one bracket around every root of a inside an interval the coarse search finds '''
    Z = nodes3(spec, W)
    B, N, G = Z.shape[0], spec.N, len(planes['d_max'])
    if spec.param:
        xs = np.arange(FINE * samples + 1) / (FINE * samples)
        av = coords(planes, grid_positions(spec, W, xs))[..., 0]                 # (G, B, N, F + 1)
        g, b, n, i = np.nonzero((av[..., :-1] >= 0) != (av[..., 1:] >= 0))
        return g, b, n, xs[i], xs[i + 1]
    out = []
    tau = np.asarray(spec.tau, float)
    Vinv = np.linalg.inv(np.vander(tau, increasing=True))
    an = coords(planes, Z)[..., 0]                                                # (G, B, N, K1)
    for g in range(G):
        for b in range(B):
            for n in range(N):
                mono = Vinv @ an[g, b, n]
                if not np.any(mono[1:] != 0):
                    continue
                r = np.roots(mono[::-1])
                last = -1.0
                for x in np.sort(r[np.abs(r.imag) < 1e-7].real):
                    if not 0.0 < x < 1.0:
                        continue
                    for widen in (1, 10, 100):
                        lo, hi = max(x - widen * POLISH, 0.0), min(x + widen * POLISH, 1.0)
                        e = lagrange(tau, [lo, hi]) @ an[g, b, n]
                        if (e[0] >= 0) != (e[1] >= 0):
                            if lo > last:
                                out.append((g, b, n, lo, hi))
                                last = hi
                            break
    arr = np.array(out, float).reshape(-1, 5)
    return arr[:, 0].astype(int), arr[:, 1].astype(int), arr[:, 2].astype(int), arr[:, 3], arr[:, 4]


def roots(spec, planes, W, samples):
    ''' (g, b, n, x, slope): every root of a inside an interval and |da/dx| there '''
    Z = nodes3(spec, W)
    g, b, n, lo, hi = brackets(spec, planes, W, samples)
    if len(g) == 0:
        return g, b, n, lo, lo
    slo = point_coords(spec, planes, Z, g, b, n, lo)[:, 0] >= 0
    for _ in range(HALVINGS):
        mid = 0.5 * (lo + hi)
        same = (point_coords(spec, planes, Z, g, b, n, mid)[:, 0] >= 0) == slo
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    x = 0.5 * (lo + hi)
    d = 1e-6
    up, dn = np.minimum(x + d, 1.0), np.maximum(x - d, 0.0)
    slope = np.abs(point_coords(spec, planes, Z, g, b, n, up)[:, 0] -
                   point_coords(spec, planes, Z, g, b, n, dn)[:, 0]) / (up - dn)
    return g, b, n, x, slope


def gatecheck(spec, planes, W, samples, axial_tol=1e-6):
    '''
    W (B, nw) -> (val (NCH, G, B), conditions): the crossings by the definition -- the junction before every
    interval (the wrap on closed problems), the roots of a inside every sample step, the first and last point of
    an open line within axial_tol -- and the best of them per (gate, instance). conditions: 'slope' the smallest
    |da/dx| at a root, 'sample' the smallest |a| at a sample, 'pairs' the number of sample steps that hold more
    than one root, 'odd' those of them that hold an odd number (a step with an even number shows no sign change
    and is, by the definition, no crossing; of an odd number the check finds one and the definition does not say
    which).
    '''
    W = np.atleast_2d(np.asarray(W, float))
    S, N, closed = int(samples), spec.N, bool(spec.config.closed)
    B, G = W.shape[0], len(planes['d_max'])
    Z = nodes3(spec, W)
    A = coords(planes, grid_positions(spec, W, np.arange(S + 1) / S))            # (G, B, N, S + 1, 3)
    rg, rb, rn, rx, rs = roots(spec, planes, W, S)
    rat = point_coords(spec, planes, Z, rg, rb, rn, rx) if len(rg) else np.zeros((0, 3))
    step = np.minimum(np.floor(rx * S).astype(int), S - 1)
    cond = {'slope': float(np.min(rs, initial=np.inf)), 'sample': float(np.min(np.abs(A[..., 0]))), 'pairs': 0, 'odd': 0}
    val = np.zeros((NCH, G, B))
    for g in range(G):
        for b in range(B):
            h = W[b, :N]
            mine = np.nonzero((rg == g) & (rb == b))[0]
            events = []         # (n, x, (a, p2, p3), direction)
            for n in range(N):
                a = A[g, b, n]
                if n > 0 or closed:
                    prev = A[g, b, n - 1, S]
                    if (prev[0] >= 0) != (a[0, 0] >= 0):
                        events.append((n, 0.0, a[0], 1.0 if a[0, 0] >= 0 else -1.0))
                elif abs(a[0, 0]) <= axial_tol:
                    events.append((0, 0.0, a[0], 1.0 if a[1, 0] - a[0, 0] >= 0 else -1.0))
                here_n = mine[rn[mine] == n]
                for i in range(S):
                    here = here_n[step[here_n] == i]
                    cond['pairs'] += int(len(here) > 1)
                    cond['odd'] += int(len(here) > 1 and len(here) % 2 == 1)
                    if (a[i, 0] >= 0) == (a[i + 1, 0] >= 0):
                        continue
                    if len(here):
                        events.append((n, rx[here[0]], rat[here[0]], -1.0 if a[i, 0] >= 0 else 1.0))
                    else:       # a sign change the root search did not resolve: shows in the comparison
                        events.append((n, np.nan, np.full(3, np.nan), np.nan))
                if n == N - 1 and not closed and abs(a[S, 0]) <= axial_tol:
                    events.append((n, 1.0, a[S], 1.0 if a[S, 0] - a[S - 1, 0] >= 0 else -1.0))
            out = np.full(NCH, np.nan)
            out[0], out[1], out[2], out[8] = len(events), -np.inf, -1.0, 0.0
            for n, x, at, direction in events:
                m = float(margin(planes, g, at[1], at[2]))
                if m > out[1]:
                    out[1:9] = [m, n, x, h[:n].sum() + x * h[n], at[1], at[2], np.hypot(at[1], at[2]), direction]
            if not np.all(np.isfinite(h) & (h > 0)) or not np.all(np.isfinite(A[g, b, ..., 0])):
                out[8] = np.nan
            val[:, g, b] = out
    return val, cond
