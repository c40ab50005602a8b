'''
Host oracle of the six element-by-column steps of the interior-point iteration (include/ato_ipm.h:
ato_ipm_errors, _rhs, _direction, _measures, _multipliers, _kkt_diag; solver/ipm_device.py
DeviceIPMKernels): a plain fp64 restatement on numpy [element][W] arrays, written from IPOPT's formulas as
the docstrings of BatchedInteriorPoint and include/ato_ipm.h give them. It imports nothing of the solver.

Conventions. A bound is present where it is finite; the slack of an absent bound is 1 and every term it
would feed is masked out. The slack of inequality row iin[k] is s[k]; c_rhs[k] belongs to equality row
ieq[k]. Every method returns the tuple the DeviceIPMKernels method of the same name returns; the three
steps that reduce over elements also return their sums (below).

Arithmetic.
  * Elementwise results are evaluated in the operation order of the kernels' source comments, one numpy
    operation per IEEE operation (no fused multiply-add can arise). fp64 + - * / are correctly rounded on
    the host and on the device (the library is built without contraction and without fast-math), so these
    results are compared BIT FOR BIT (assert_same: equal NaN masks, equal values, equal sign bits).
  * Maxima and minima are exact in any order and propagate NaN (numpy's max / min / maximum / minimum do,
    like torch.maximum / amax); the step sizes are clamped to 1 with the NaN kept. Also bit for bit.
  * Sums are computed exactly (math.fsum, one rounding) and come with S_abs = sum |term| and the number of
    terms T that are not masked out: |zl|, |zu|, |vl|, |vu|, |y| (errors); theta, the log-barrier sum and
    the one-sided linear damping sum (measures); gx.dx + gs.ds (direction). A column whose terms are not
    all finite has no rounding question: its sum is +-inf or NaN in any order, and is compared exactly.

Tolerances of the summed outputs (u = 2^-53; derived, not tuned).
  Any summation order of T terms, every partial sum rounded, errs by at most
  (T - 1) u / (1 - (T - 1) u) * S_abs [Higham, Accuracy and Stability of Numerical Algorithms, eq. (4.4)];
  adding a masked-out 0 or an empty chunk's 0 is exact. With the one rounding of the exact sum on this side
  the two sides differ by at most  sum_bound = (T + 2) u S_abs.
  * theta and the |z|, |y| sums have no cancellation (S_abs = S): a relative bound (T + 2) u.
  * E_mu = max(du / s_d, pr, co / s_c): du, pr, co are exact; s_d = max((S_y + S_z) / max(m + nz, 1),
    s_max) / s_max is fed by the T = 2 n + 2 mi + m terms of S_y + S_z summed in some order (relative error
    (T - 1) u), one division, a maximum (exact), one division, and du / s_d one more: (T + 2) u on the device
    side, 5 roundings on this side (the exact sums are each rounded, then added), second-order terms below
    1 u: relative (T + 8) u. s_c is fed by fewer terms; max is monotone and 1-Lipschitz, so
    |E - E'| <= (T + 8) u |E| = errors_rtol(...).
  * gphi_d: the products gx dx, gs ds are rounded identically on both sides; the absolute bound is
    (T + 2) u (sum |gx dx| + sum |gs ds|), T = n + mi.
  * phi = (f - mu lg) + (kd mu) lin. The damping sum lin errs by d_lin = (T_lin + 2) u S_abs_lin. The log
    sum lg errs by its summation, (T_lg + 2) u S_abs_lg, and by the logarithms themselves: a device log and
    a host log differ by at most LOG_ULP + 1 units in the last place (the measured distance plus one for
    the host's own log), and ulp(t) <= 2 u |t|: d_lg = (T_lg + 2) u S_abs_lg + (LOG_ULP + 1) 2 u S_abs_lg.
    To first order through the four roundings of the expression (each at most u of its result on either
    side, every result at most |f| + |mu lg| + |kd mu lin|):
        phi_bound = |mu| d_lg + |kd mu| d_lin + 8 u (|f| + |mu lg| + |kd mu lin|).
    On finite interior operands the tests also hold phi to the project's earlier ceiling of 1e-12 relative.

The device logarithm. The ROCm documentation installed with the toolchain states no fp64 accuracy for log
(no document under its share/ directory mentions one), so DEVICE_LOG_ULP is measured: the largest distance,
in units in the last place of the host value, between torch.log on the MI355X and numpy's log on the host
over every positive slack of tests/ipm_column_cases.py (all structures, all operand classes).
tests/test_gpu_ipm_columns.py::test_device_log_distance repeats the measurement and fails if the distance
ever exceeds the constant. HOST_TORCH_LOG_ULP bounds the same distance for torch.log on the CPU (the
vectorised SLEEF log, documented to 1.0 ulp, against a host log below 1 ulp: at most 2), used when the
oracle is pinned against the solver's torch formulation without a GPU.
'''
import math

import numpy as np

U = 2.0 ** -53
DEVICE_LOG_ULP = 1          # measured on the MI355X (see above): 21962 of the 795253 slacks differ, none by more than 1 ulp
HOST_TORCH_LOG_ULP = 2


# ---------------------------------------------------------------------------------------------- comparisons
def assert_same(got, want, what=''):
    ''' bitwise equality up to the NaN payload: equal shapes, equal NaN masks, equal values, equal sign bits
    (the rule of tests/test_gpu_resto_kernels.py _assert_same) '''
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f'{what}: {got.shape} {got.dtype} / {want.shape}'
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), f'{what}: NaN masks differ at {np.argwhere(ng != nw)[:4].tolist()}'
    g0, w0 = np.where(ng, 0.0, got), np.where(nw, 0.0, want)
    bad = g0 != w0
    assert not bad.any(), f'{what}: values differ at {np.argwhere(bad)[:4].tolist()}: {g0[bad][:4]} / {w0[bad][:4]}'
    sg = np.signbit(g0) != np.signbit(w0)
    assert not sg.any(), f'{what}: signs differ at {np.argwhere(sg)[:4].tolist()}'


def assert_sum_close(got, want, bound, what=''):
    ''' a summed output [W]: exactly the oracle's where that is not finite, within bound [W] elsewhere '''
    got, want, bound = np.asarray(got), np.asarray(want), np.asarray(bound)
    assert got.shape == want.shape == bound.shape, what
    fin = np.isfinite(want)
    assert_same(got[~fin], want[~fin], what + ' (non-finite columns)')
    with np.errstate(all='ignore'):
        err = np.abs(got[fin] - want[fin])
    ok = err <= bound[fin]
    assert ok.all(), (f'{what}: columns {np.flatnonzero(fin)[~ok][:4].tolist()} err {err[~ok][:4]} '
                      f'bound {bound[fin][~ok][:4]}')


def ulp_distance(got, want):
    ''' |got - want| in units in the last place of want (finite, nonzero want) '''
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


# ---------------------------------------------------------------------------------------------------- sums
class Sum:
    ''' exact column sums S [W] of terms [T][W] (masked-out terms are 0 and not counted), S_abs = sum
    |term| [W], T [W] the number of counted terms '''

    def __init__(self, terms, counted=None):
        terms = np.asarray(terms, np.float64)
        rows, W = terms.shape
        self.S, self.S_abs = np.zeros(W), np.zeros(W)
        self.T = np.full(W, rows, np.int64) if counted is None else np.asarray(counted).sum(0).astype(np.int64)
        fin = np.isfinite(terms).all(0) if rows else np.ones(W, bool)
        with np.errstate(all='ignore'):
            mag = np.abs(terms)
            for b in range(W):
                if fin[b]:
                    self.S[b] = math.fsum(terms[:, b].tolist())
                    self.S_abs[b] = math.fsum(mag[:, b].tolist())
                else:                      # +-inf or NaN in any order
                    self.S[b] = terms[:, b].sum()
                    self.S_abs[b] = mag[:, b].sum()

    def bound(self):
        ''' (T + 2) u S_abs '''
        return (self.T + 2) * U * self.S_abs

    def first(self, W):
        ''' the same sums of the first W columns '''
        s = object.__new__(Sum)
        s.S, s.S_abs, s.T = self.S[:W], self.S_abs[:W], self.T[:W]
        return s


def errors_rtol(n, mi, meq):
    ''' relative bound of E_mu: (T + 8) u, T = 2 n + 2 mi + m the terms that feed s_d '''
    return (2 * n + 2 * mi + (mi + meq) + 8) * U


def phi_bound(sums, f, mu, kappa_d, log_ulp):
    ''' first-order bound of phi = (f - mu lg) + (kd mu) lin (derivation above); sums: measures()'s '''
    lg, lin = sums['lg'], sums['lin']
    with np.errstate(all='ignore'):
        d_lg = lg.bound() + (log_ulp + 1) * 2 * U * lg.S_abs
        d_lin = lin.bound()
        km = np.abs(kappa_d * mu)
        return np.abs(mu) * d_lg + km * d_lin + 8 * U * (np.abs(f) + np.abs(mu * lg.S) + np.abs(km * lin.S))


# -------------------------------------------------------------------------------------------------- oracle
def _cmax(a):
    ''' NaN-propagating column maximum of non-negative terms, 0 for no terms '''
    return np.max(a, axis=0, initial=0.0)


def _nmax(a, b):
    ''' the kernels' two-operand maximum as their source states it: NaN if either is, else a > b ? a : b. Only
    the sign of a tie between +0 and -0 depends on that (IEEE 754 leaves it open and torch.maximum leaves it to
    the backend): it is the second operand's. In these steps such a tie needs mu = 0 in the multiplier
    safeguard, which the solver never passes (mu >= mu_min > 0 there; mu = 0 only enters errors, whose
    maxima are over absolute values) '''
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a > b, a, b))


def _nmin(a, b):
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a < b, a, b))


class ColumnOracle:
    def __init__(self, dims, iin, ieq, xL, xU, dL, dU):
        self.n, self.mi, self.meq = (int(v) for v in dims)
        self.m = self.mi + self.meq
        self.iin, self.ieq = np.asarray(iin, np.int64), np.asarray(ieq, np.int64)
        assert len(self.iin) == self.mi and len(self.ieq) == self.meq
        assert sorted(np.concatenate([self.iin, self.ieq]).tolist()) == list(range(self.m))
        self.xL, self.xU, self.dL, self.dU = (np.asarray(v, np.float64) for v in (xL, xU, dL, dU))
        self.hxl, self.hxu = np.isfinite(self.xL), np.isfinite(self.xU)
        self.hsl, self.hsu = np.isfinite(self.dL), np.isfinite(self.dU)
        # one-sided bounds: the ones IPOPT damps linearly (kappa_d)
        self.dxl, self.dxu = self.hxl & ~self.hxu, self.hxu & ~self.hxl
        self.dsl, self.dsu = self.hsl & ~self.hsu, self.hsu & ~self.hsl
        self.W = self.xL.shape[1]

    def n_bounds(self):
        return (self.hxl.sum(0) + self.hxu.sum(0) + self.hsl.sum(0) + self.hsu.sum(0)).astype(np.float64)

    # ---- pieces
    def slacks(self, x, s):
        ''' (x - xL, xU - x, s - dL, dU - s), 1 where the bound is absent '''
        with np.errstate(all='ignore'):
            return (np.where(self.hxl, x - self.xL, 1.0), np.where(self.hxu, self.xU - x, 1.0),
                    np.where(self.hsl, s - self.dL, 1.0), np.where(self.hsu, self.dU - s, 1.0))

    def resid(self, g, s, c_rhs):
        ''' constraint residual [m][W]: g - s on the slack rows, g - c_rhs on the equality rows '''
        r = np.empty_like(g)
        with np.errstate(all='ignore'):
            r[self.iin] = g[self.iin] - s
            r[self.ieq] = g[self.ieq] - c_rhs
        return r

    def _sides(self, x, s):
        a, b, c, d = self.slacks(x, s)
        return ((a, self.hxl), (b, self.hxu), (c, self.hsl), (d, self.hsu))

    # ---- the six steps
    def errors(self, x, s, g, c_rhs, sg, y, zl, zu, vl, vu, dual_x, mu, n_bounds, s_max):
        ''' ((E_mu, dual inf, primal inf, complementarity inf, max |r / sg|), sums) '''
        with np.errstate(all='ignore'):
            r = self.resid(g, s, c_rhs)
            dual_s = (-y[self.iin] - vl) + vu
            du = np.maximum(_cmax(np.abs(dual_x)), _cmax(np.abs(dual_s)))
            pr = _cmax(np.abs(r))
            pr_uns = _cmax(np.abs(r / sg))
            co = np.zeros(self.W)
            for (sl, msk), z in zip(self._sides(x, s), (zl, zu, vl, vu)):
                co = np.maximum(co, _cmax(np.where(msk, np.abs(sl * z - mu), 0.0)))
            sums = {k: Sum(np.abs(v)) for k, v in (('zl', zl), ('zu', zu), ('vl', vl), ('vu', vu), ('y', y))}
            zsum = ((sums['zl'].S + sums['zu'].S) + sums['vl'].S) + sums['vu'].S
            s_d = np.maximum((sums['y'].S + zsum) / np.maximum(self.m + n_bounds, 1.0), s_max) / s_max
            s_c = np.maximum(zsum / np.maximum(n_bounds, 1.0), s_max) / s_max
            E = np.maximum(np.maximum(du / s_d, pr), co / s_c)
        return (E, du, pr, co, pr_uns), sums

    def rhs(self, x, s, g, c_rhs, gf, jty, y, zl, zu, vl, vu, mu, kappa_d):
        ''' (Sx, Ss, gx, gs, rhs_x, rhs_s, rhs_y) '''
        with np.errstate(all='ignore'):
            a, b, c, d = self.slacks(x, s)
            Sx = np.where(self.hxl, zl / a, 0.0) + np.where(self.hxu, zu / b, 0.0)
            Ss = np.where(self.hsl, vl / c, 0.0) + np.where(self.hsu, vu / d, 0.0)
            km = kappa_d * mu
            gx = (gf - mu * np.where(self.hxl, 1.0 / a, 0.0)) + mu * np.where(self.hxu, 1.0 / b, 0.0)
            gx = gx + km * (self.dxl.astype(np.float64) - self.dxu.astype(np.float64))
            gs = (-mu) * np.where(self.hsl, 1.0 / c, 0.0) + mu * np.where(self.hsu, 1.0 / d, 0.0)
            gs = gs + km * (self.dsl.astype(np.float64) - self.dsu.astype(np.float64))
            return Sx, Ss, gx, gs, -(gx + jty), -(gs - y[self.iin]), -self.resid(g, s, c_rhs)

    @staticmethod
    def _ftb(v, dv, mask, ntau):
        ''' fraction-to-the-boundary candidates: (-tau v) / dv where the bound is present and dv < 0 '''
        sel = mask & (dv < 0.0)
        return np.where(sel, (ntau * v) / np.where(sel, dv, -1.0), np.inf)

    def direction(self, x, s, dx, ds, zl, zu, vl, vu, gx, gs, mu, tau):
        ''' ((dzl, dzu, dvl, dvu, alpha_max, alpha_z, gphi_d), sums) '''
        with np.errstate(all='ignore'):
            a, b, c, d = self.slacks(x, s)
            dzl = np.where(self.hxl, ((mu / a) - zl) - ((zl / a) * dx), 0.0)
            dzu = np.where(self.hxu, ((mu / b) - zu) + ((zu / b) * dx), 0.0)
            dvl = np.where(self.hsl, ((mu / c) - vl) - ((vl / c) * ds), 0.0)
            dvu = np.where(self.hsu, ((mu / d) - vu) + ((vu / d) * ds), 0.0)
            nt = -tau
            f = self._ftb
            cand = np.concatenate([f(a, dx, self.hxl, nt), f(b, -dx, self.hxu, nt), f(c, ds, self.hsl, nt),
                                   f(d, -ds, self.hsu, nt)])
            candz = np.concatenate([f(zl, dzl, self.hxl, nt), f(zu, dzu, self.hxu, nt), f(vl, dvl, self.hsl, nt),
                                    f(vu, dvu, self.hsu, nt)])
            alpha_max = np.minimum(np.min(cand, axis=0, initial=np.inf), 1.0)
            alpha_z = np.minimum(np.min(candz, axis=0, initial=np.inf), 1.0)
            gd = Sum(np.concatenate([gx * dx, gs * ds]))
        return (dzl, dzu, dvl, dvu, alpha_max, alpha_z, gd.S), {'gphi_d': gd}

    def measures(self, x, s, g, c_rhs, f, mu, kappa_d):
        ''' ((theta, phi), sums) '''
        with np.errstate(all='ignore'):
            sides = self._sides(x, s)
            th = Sum(np.abs(self.resid(g, s, c_rhs)))
            lg = Sum(np.concatenate([np.where(msk, np.log(sl), 0.0) for sl, msk in sides]),
                     np.concatenate([msk for _, msk in sides]))
            one = (self.dxl, self.dxu, self.dsl, self.dsu)
            lin = Sum(np.concatenate([np.where(msk, sl, 0.0) for (sl, _), msk in zip(sides, one)]),
                      np.concatenate(one))
            phi = (f - mu * lg.S) + (kappa_d * mu) * lin.S
        return (th.S, phi), {'theta': th, 'lg': lg, 'lin': lin}

    def multipliers(self, x, s, mu, az, kappa_sigma, zl, zu, vl, vu, dzl, dzu, dvl, dvu):
        ''' the accepted bound multipliers (zl, zu, vl, vu): z + az dz, kept within kappa_sigma of mu / slack '''
        out = []
        ks = kappa_sigma
        with np.errstate(all='ignore'):
            for (sl, msk), z, dz in zip(self._sides(x, s), (zl, zu, vl, vu), (dzl, dzu, dvl, dvu)):
                zn = z + az * dz
                out.append(np.where(msk, _nmin(_nmax(zn, mu / (ks * sl)), (ks * mu) / sl), 0.0))
        return tuple(out)

    def kkt_diag(self, Sx, Ss, dw, dc):
        ''' (dx, dr, Ds): Sx + dw, -dc on the equality rows and -dc - 1 / Ds on the slack rows, Ss + dw '''
        with np.errstate(all='ignore'):
            Ds = Ss + dw
            dr = np.full((self.m, self.W), np.nan)       # every row is written below: the rows are a partition
            dr[self.ieq] = np.broadcast_to(-dc, (self.meq, self.W))
            dr[self.iin] = -dc - 1.0 / Ds
            return Sx + dw, dr, Ds
