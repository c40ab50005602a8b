'''
Synthetic structures and operands for the tests of the interior-point column kernels
(tests/test_ipm_column_oracle_cpu.py pins tests/ipm_column_oracle.py against the solver's torch formulation
on the CPU, tests/test_gpu_ipm_columns.py compares the HIP kernels with the oracle).

Every structure is generated once at the widest batch (WMAX columns); a test at width W uses the first W
columns, so the oracle's results at WMAX serve every width (columns never interact). The columns in
PLANT_COLS are the last column of each tested width and the columns around the 64-column block boundary;
edge values are planted there.

Structures (n, mi, meq), with the reduction geometry they reach (chunks of CH = 32 elements per part; the
folds split the NC chunks of a step into FG = 8 or EG = 32 contiguous ranges):
  S0 (5, 0, 0)        m = 0: parts of length 0, NC < FG, null iin / ieq
  S1 (1, 0, 1)        one element per part, most fold ranges empty
  S2 (32, 32, 32)     every part an exact multiple of CH
  S3 (33, 31, 1)      one over and one under a chunk; also an all-unbounded and an all-two-sided column
  S4 (257, 300, 0)    meq = 0; errors NC = 29 < EG; direction NC = 19
  S5 (2100, 300, 900) errors NC = 143 > EG; measures NC = 105 and direction NC = 76: fold ranges of 9-14
                      chunks, one batch of 8 loads plus a remainder
iin / ieq are an interleaved partition of range(m) (the equality rows evenly spread), not two runs.

Operand classes:
  interior   iterates strictly inside their bounds, multipliers in (0, 2) (also where no bound is present: the
             masks must ignore them), mu in [1e-9, 0.1] log-uniform, g, y, gf, jty, dx, ds of either sign
             with magnitudes 1e-6 .. 1e6 log-uniform; in the even columns g is within 1e-9 of that draw from
             s / c_rhs (nearly feasible), so that E_mu is du / s_d there and depends on the sums. f has the sign of -lg (the log-barrier sum), so phi
             does not cancel and a relative bound on it means something.
  boundary   the interior operands with, in PLANT_COLS, some in the last chunk of a part: x == xL exactly
             (with dx < 0: the step size is 0), x below xL with zl = 0 (a negative multiplier step from 0),
             s == dU, dx = 0.0 and -0.0, mu = 0 in one column, and dw = -Ss in one entry (Ds = 0).
  nonfinite  the interior operands with NaN, +inf and -inf planted in x, g, y, zl, dx, mu, tau and dw, each
             value of each operand in a column of its own (NONFINITE_COLS); every other column is untouched.
The operands of a later step that an earlier step produces (gx, gs; dzl .. dvu; Sx, Ss) are the ORACLE's,
so every kernel is judged on its own.
'''
import functools

import numpy as np

from tests.ipm_column_oracle import ColumnOracle

STRUCTURES = {'S0': (5, 0, 0), 'S1': (1, 0, 1), 'S2': (32, 32, 32), 'S3': (33, 31, 1), 'S4': (257, 300, 0),
              'S5': (2100, 300, 900)}
WIDTHS = (1, 63, 64, 65, 130, 257)
WMAX = max(WIDTHS)
PLANT_COLS = (0, 62, 63, 64, 129, 256)              # W - 1 of every width; 62 | 63 | 64: the block boundary
CLASSES = ('interior', 'boundary', 'nonfinite')
UNBOUNDED_COL, TWO_SIDED_COL = 5, 64                # S3 only
KAPPA_D, KAPPA_SIGMA, S_MAX = 1e-5, 1e10, 100.0     # IPOPT's defaults (solver/ipm.py IPMOptions)
# nonfinite: operand i gets NaN, +inf, -inf in columns NONFINITE_COLS[3 i : 3 i + 3]
NONFINITE_OPS = ('x', 'g', 'y', 'zl', 'dx', 'mu', 'tau', 'dw')
NONFINITE_COLS = (0, 2, 8, 11, 20, 33, 47, 60, 61, 62, 63, 64, 66, 70, 100, 127, 128, 129, 131, 200, 254, 255,
                  256, 130)
NONFINITE_VALUES = (np.nan, np.inf, -np.inf)


def partition(mi, meq):
    ''' (iin, ieq): the equality rows evenly spread over range(mi + meq), both ascending '''
    m = mi + meq
    ieq = np.floor((np.arange(meq) + 0.5) * m / max(meq, 1)).astype(np.int64)
    assert len(set(ieq.tolist())) == meq
    iin = np.setdiff1d(np.arange(m), ieq)
    if mi and meq:
        assert not np.array_equal(iin, np.arange(mi)) and not np.array_equal(iin, np.arange(meq, m)), 'two runs'
    return iin, ieq


def _plant_sites(n, mi):
    ''' (part, row, column, what) of the boundary class; rows in the first and the last chunk of a part '''
    sites = [('x', n - 1, 63, 'on_lower'), ('x', n - 1, 0, 'on_lower'), ('x', 0, 64, 'below_lower'),
             ('x', 0, 256, 'below_lower'), ('x', n // 2, 129, 'below_lower')]
    if mi:
        sites += [('s', mi - 1, 62, 'on_upper'), ('s', mi - 1, 129, 'on_upper'), ('s', 0, 0, 'on_upper')]
    return sites


@functools.lru_cache(maxsize=None)
def structure(sid):
    ''' dims, iin, ieq and the bounds [rows][WMAX] of structure sid: every (element, column) draws one of
    none / lower / upper / both; the boundary class's sites have both bounds '''
    n, mi, meq = STRUCTURES[sid]
    rng = np.random.default_rng(1000 + int(sid[1:]))
    iin, ieq = partition(mi, meq)

    def draw(rows, part):
        kind = rng.integers(0, 4, size=(rows, WMAX))
        if sid == 'S3':
            kind[:, UNBOUNDED_COL] = 0
            kind[:, TWO_SIDED_COL] = 3
        for p, r, c, _ in _plant_sites(n, mi):
            if p == part:
                kind[r, c] = 3
        lo = rng.uniform(-5.0, 5.0, size=(rows, WMAX))
        hi = lo + rng.uniform(0.5, 4.0, size=(rows, WMAX))
        L = np.where((kind == 1) | (kind == 3), lo, -np.inf)
        Uq = np.where((kind == 2) | (kind == 3), hi, np.inf)
        return np.ascontiguousarray(L), np.ascontiguousarray(Uq)
    xL, xU = draw(n, 'x')
    dL, dU = draw(mi, 's')
    if sid == 'S3':
        assert not np.isfinite(xL[:, UNBOUNDED_COL]).any() and np.isfinite(xU[:, TWO_SIDED_COL]).all()
    return dict(sid=sid, dims=(n, mi, meq), iin=iin, ieq=ieq, xL=xL, xU=xU, dL=dL, dU=dU)


def oracle_of(st, cols=slice(None)):
    return ColumnOracle(st['dims'], st['iin'], st['ieq'], *(st[k][:, cols] for k in ('xL', 'xU', 'dL', 'dU')))


def _inside(rng, L, Uq):
    t = rng.uniform(0.01, 0.99, size=L.shape)
    hl, hu = np.isfinite(L), np.isfinite(Uq)
    L0, U0 = np.where(hl, L, 0.0), np.where(hu, Uq, 0.0)
    v = np.where(hl & hu, L0 + t * (U0 - L0), np.where(hl, L0 + 3.0 * t, np.where(hu, U0 - 3.0 * t, 2.0 * t - 1.0)))
    assert (v > L).all() and (v < Uq).all()
    return v


def _interior(st):
    n, mi, meq = st['dims']
    m = mi + meq
    rng = np.random.default_rng(2000 + int(st['sid'][1:]))

    def wide(*shape):                      # either sign, magnitudes 1e-6 .. 1e6
        return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-6.0, 6.0, size=shape)
    t = dict(x=_inside(rng, st['xL'], st['xU']), s=_inside(rng, st['dL'], st['dU']), g=wide(m, WMAX),
             c_rhs=rng.uniform(-1.0, 1.0, size=(meq, WMAX)), sg=10.0 ** rng.uniform(-3.0, 0.0, size=(m, WMAX)),
             y=wide(m, WMAX), gf=wide(n, WMAX), jty=wide(n, WMAX), dx=wide(n, WMAX), ds=wide(mi, WMAX),
             zl=rng.uniform(0.0, 2.0, size=(n, WMAX)), zu=rng.uniform(0.0, 2.0, size=(n, WMAX)),
             vl=rng.uniform(0.0, 2.0, size=(mi, WMAX)), vu=rng.uniform(0.0, 2.0, size=(mi, WMAX)),
             mu=10.0 ** rng.uniform(-9.0, -1.0, size=WMAX), tau=rng.uniform(0.9, 0.99, size=WMAX),
             az=rng.uniform(0.0, 1.0, size=WMAX),
             dw=np.where(rng.random(WMAX) < 0.5, 0.0, 10.0 ** rng.uniform(-8.0, 0.0, size=WMAX)),
             dc=np.where(rng.random(WMAX) < 0.5, 0.0, 10.0 ** rng.uniform(-10.0, -6.0, size=WMAX)))
    # the even columns are nearly feasible (g within 1e-9 of the wide draw from s / c_rhs): there the primal
    # infeasibility does not dominate E_mu, which then is du / s_d and so sensitive to the summed |y|, |z|
    near = np.arange(WMAX) % 2 == 0
    target = np.empty((m, WMAX))
    target[st['iin']], target[st['ieq']] = t['s'], t['c_rhs']
    t['g'] = np.where(near[None, :], target + 1e-9 * t['g'], t['g'])
    lg = oracle_of(st).measures(t['x'], t['s'], t['g'], t['c_rhs'], np.zeros(WMAX), t['mu'], KAPPA_D)[1]['lg'].S
    t['f'] = np.where(lg > 0, -1.0, 1.0) * rng.uniform(0.1, 1.0, size=WMAX)
    return t


def _boundary(st, t):
    n, mi, _ = st['dims']
    for part, r, c, what in _plant_sites(n, mi):
        if what == 'on_lower':             # slack exactly 0, and a step towards the bound
            t['x'][r, c] = st['xL'][r, c]
            t['dx'][r, c] = -abs(t['dx'][r, c])
        elif what == 'below_lower':        # negative slack; zl = 0 there: dzl = mu / slack < 0 from z = 0
            t['x'][r, c] = st['xL'][r, c] - 0.25
            t['zl'][r, c] = 0.0
        elif what == 'on_upper':
            t['s'][r, c] = st['dU'][r, c]
    t['dx'][n // 2, 256] = 0.0
    t['dx'][n // 2, 63] = -0.0
    t['dx'][0, 62] = -0.0
    t['dx'][n - 1, 64] = 0.0
    t['mu'][62] = 0.0
    t['mu'][256] = 0.0


def _nonfinite(st, t):
    n, mi, meq = st['dims']
    for i, name in enumerate(NONFINITE_OPS):
        for v, val in enumerate(NONFINITE_VALUES):
            c = NONFINITE_COLS[3 * i + v]
            a = t[name]
            if a.ndim == 1:
                a[c] = val
            elif a.shape[0]:
                a[(a.shape[0] - 1) if v != 1 else 0, c] = val      # last chunk of the part (NaN, -inf), first (+inf)


@functools.lru_cache(maxsize=None)
def case(sid, cls):
    ''' (structure, operands at WMAX, reference): reference[step] = the oracle's outputs, reference['sums'] its
    sums, for errors at mu ('errors') and at mu = 0 ('errors0'), rhs, direction, measures, multipliers and
    kkt_diag. Shared by every test and never modified (the arrays are read-only) '''
    st = structure(sid)
    t = _interior(st)
    if cls == 'boundary':
        _boundary(st, t)
    elif cls == 'nonfinite':
        _nonfinite(st, t)
    else:
        assert cls == 'interior'
    orc = oracle_of(st)
    with np.errstate(all='ignore'):
        t['dual_x'] = ((t['gf'] + t['jty']) - t['zl']) + t['zu']
    t['n_bounds'] = orc.n_bounds()
    ref, sums = {}, {}
    for key, mu in (('errors', t['mu']), ('errors0', np.zeros(WMAX))):
        ref[key], sums[key] = orc.errors(t['x'], t['s'], t['g'], t['c_rhs'], t['sg'], t['y'], t['zl'], t['zu'],
                                         t['vl'], t['vu'], t['dual_x'], mu, t['n_bounds'], S_MAX)
    ref['rhs'] = orc.rhs(t['x'], t['s'], t['g'], t['c_rhs'], t['gf'], t['jty'], t['y'], t['zl'], t['zu'], t['vl'],
                         t['vu'], t['mu'], KAPPA_D)
    t['Sx'], t['Ss'], t['gx'], t['gs'] = ref['rhs'][:4]
    if cls == 'boundary' and st['dims'][1]:          # Ss + dw = 0 in one entry of the last chunk, column 63
        t['dw'][63] = -t['Ss'][st['dims'][1] - 1, 63]
    ref['direction'], sums['direction'] = orc.direction(t['x'], t['s'], t['dx'], t['ds'], t['zl'], t['zu'], t['vl'],
                                                        t['vu'], t['gx'], t['gs'], t['mu'], t['tau'])
    t['dzl'], t['dzu'], t['dvl'], t['dvu'] = ref['direction'][:4]
    ref['measures'], sums['measures'] = orc.measures(t['x'], t['s'], t['g'], t['c_rhs'], t['f'], t['mu'], KAPPA_D)
    ref['multipliers'] = orc.multipliers(t['x'], t['s'], t['mu'], t['az'], KAPPA_SIGMA, t['zl'], t['zu'], t['vl'],
                                         t['vu'], t['dzl'], t['dzu'], t['dvl'], t['dvu'])
    ref['kkt_diag'] = orc.kkt_diag(t['Sx'], t['Ss'], t['dw'], t['dc'])
    ref['sums'] = sums
    for a in list(t.values()) + [v for k in ref if k != 'sums' for v in ref[k]]:
        a.setflags(write=False)
    return st, t, ref


def planted_columns(cls):
    ''' the columns of a class that differ from the interior operands '''
    if cls == 'nonfinite':
        return sorted(set(NONFINITE_COLS))
    return sorted(set(PLANT_COLS)) if cls == 'boundary' else []


def positive_slacks():
    ''' every positive bound slack of every structure and class (what the log-barrier sum takes the log of) '''
    out = []
    for sid in STRUCTURES:
        for cls in CLASSES:
            st, t, _ = case(sid, cls)
            for sl in oracle_of(st).slacks(t['x'], t['s']):
                sl = sl[np.isfinite(sl) & (sl > 0)]
                out.append(sl[sl != 1.0])
    return np.unique(np.concatenate(out))
