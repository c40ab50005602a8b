// ato_gatecheck.hpp -- where, when and how far inside its opening a collocation solution goes through each gate.
//
// A gate row of the NLP is a point constraint: it holds at one abscissa of one interval (node Z[interval, 0] in
// the global frame; the Lagrange point d of the interval that contains the gate's nominal s in the parametric
// frame, placed through a frame FROZEN at the gate's s). This check asks the continuous trajectory instead. For a
// gate plane with centre c, axes e1, e2, e3 (columns of R), half-opening d_max and a shape, a point with global
// position x has
//   a = e1 . (x - c),   p2 = e2 . (x - c),   p3 = e3 . (x - c)
// (dot3 of the sampling layer: fused multiply-adds in a fixed order). The points of a lap are (n, i), i = 0 .. S,
// n = 0 .. N - 1, at the abscissae i / S of the clearance (S = samples in [1, 64]); closed problems follow the last
// point of interval N - 1 by (0, 0). With sg(p) = (a_p >= 0) there is a crossing between consecutive points iff
// their sg differ:
//   - both in one interval: bisection on [x_i, x_i+1], the polynomial re-evaluated (and lifted through the
//     centreline at the point's own s) at every midpoint; the crossing abscissa x* is the right end of the last
//     bracket. GATE_BISECT = 53 halvings: a bracket of width 1 (S = 1) ends below 2^-52, one ulp of the abscissa;
//     the loop leaves early once the midpoint rounds onto an end, after which no halving changes the bracket.
//   - a junction between two intervals, or the closed wrap: the later point, unrefined (the jump is the solver's
//     continuity residual).
//   - open lines: the first point and the last point are crossings too when |a| <= axial_tol (their gates sit on
//     them and a may have either sign of rounding); their direction is that of a over the adjacent sample step.
//     An end point within axial_tol on the arriving side whose adjacent step also changes sign is counted twice,
//     as the end point and as the bisected crossing of that step: n_cross is then one more than the passages
//     ("found exactly once" holds for sign changes; the end-point rule adds to them, it does not replace them).
// Margin of a crossing: d_max - sqrt(p2^2 + p3^2) (circle), d_max - max(|p2|, |p3|) (square). The best crossing of
// a (gate, instance) has the largest margin, ties to the earliest (n, x*). A non-finite a or margin never becomes
// the best crossing and turns the flag channel into NaN, as does a step size h_n that is not finite and positive
// (the passage time would mean nothing); a NaN a compares as "not >= 0", so no read depends on it.
//
// Positions are the clearance's: clearance_point at the sample abscissae (the handle's weight table), and at any
// other abscissa the same sum with lagrange_weight in place of the table (gate_point) -- at i / S the two are the
// same products in the same order.
//
// Three launches: the clearance's positions into the handle's position buffer; k_gate_cross, one thread per
// (gate, interval, instance), which writes a partial record; k_gate_reduce, one thread per (gate, instance), which
// combines the records in ascending n, sums h and writes the GATE_NCH channels. Partial records: GATE_PART doubles
// per (gate, interval, instance), [G][N][GATE_PART][B], in a buffer on the handle of G N GATE_PART B doubles,
// grown only when a call needs more (64 gates x 50 intervals x 512 instances: 92 MB; the race track's 7 gates:
// 10 MB). No atomics, no device-wide synchronisation: results are bitwise repeatable and do not depend on the batch.
//
// Everything ATO_HD here is shared by the HIP kernels (ato_gatecheck.hip) and the CPU twin
// (tests/native/gatecheck_hostcheck.cpp).
#pragma once
#include "ato_clearance.hpp"

namespace ato {

constexpr int GATE_NCH = ATO_GATECHECK_NCH;
constexpr int GATE_MAX = 64;       // gates per call
constexpr int GATE_BISECT = 53;    // halvings of a bracket: 2^-53 < ulp(1) = 2^-52, the widest bracket being [0, 1]
// partial record of one (gate, interval, instance)
enum { GP_COUNT = 0, GP_MARGIN, GP_X, GP_P2, GP_P3, GP_DIR, GP_BAD, GATE_PART };

// gate-check arguments (kernel argument)
struct GateD {
    ClearD c;                      // the positions' arguments: N, K1, NV, S1 = S + 1, param, nw, weights, line
    int32_t G, closed;
    double axial_tol;
    const double* tau;             // [K1] behind a pointer: an indexed array in the kernel argument would be copied
    const ato_gate_plane* planes;  // [G]
};

// 0 (ATO_OK) or the error code of an ato_gatecheck call with these arguments; *msg gets the reason
inline int gatecheck_check(const ProbD& p, bool has_line, int n_gates, int batch, int layout, int samples,
                           double axial_tol, const char** msg) {
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (int rc = check_layout(layout, msg)) return rc;
    if (samples < 1 || samples > SAMPLE_SMAX) {
        *msg = "samples must be in [1, 64] (the node rule leaves the tail of an interval without a bracket)";
        return ATO_ERR_ARG;
    }
    if (!(axial_tol >= 0.0)) { *msg = "axial_tol must be >= 0"; return ATO_ERR_ARG; }
    if (n_gates > GATE_MAX) { *msg = "more than 64 gates"; return ATO_ERR_ARG; }
    if (int rc = check_collocation(p, "gate passage of RK4-transcribed problems (K = 0) is not supported", msg)) return rc;
    if (int rc = check_line(p, has_line, "parametric gate passage needs the centreline table (ato_clearance_set_line)",
                            msg))
        return rc;
    if (n_gates < 1) { *msg = "the problem has no gates and none are set (ato_gatecheck_set_gates)"; return ATO_ERR_STATE; }
    return ATO_OK;
}

// the planes of a problem's own gates
inline std::vector<ato_gate_plane> gate_planes_of(const std::vector<ato_gate>& gates) {
    std::vector<ato_gate_plane> out;
    for (const ato_gate& g : gates) {
        ato_gate_plane q{};
        for (int a = 0; a < 3; ++a) q.centre[a] = g.gate_x[a];
        for (int a = 0; a < 9; ++a) q.R[a] = g.R[a];
        q.d_max = g.d_max;
        q.shape = g.shape;
        out.push_back(q);
    }
    return out;
}

inline GateD gatecheck_args(const ProbD& p, int samples, const double* wt, const LineD& line, const double* tau,
                            const ato_gate_plane* planes, int G, double axial_tol) {
    return GateD{clearance_args(p, samples, wt, line), G, p.closed, axial_tol, tau, planes};
}

// clearance_point at any abscissa x of interval n: the same sums with l_j(x) = lagrange_weight
ATO_HD void gate_point(const GateD& a, int n, double x, const double* __restrict__ w, long ws, double* out) {
    const ClearD& c = a.c;
    const double* z = w + ((long)c.N + (long)n * c.K1 * c.NV) * ws;
    const double l0 = lagrange_weight(a.tau, c.K1, x, 0);
#pragma unroll
    for (int q = 0; q < 3; ++q) out[q] = l0 * z[(long)q * ws];
    for (int j = 1; j < c.K1; ++j) {
        const double lj = lagrange_weight(a.tau, c.K1, x, j);
#pragma unroll
        for (int q = 0; q < 3; ++q) out[q] = fma(lj, z[((long)j * c.NV + q) * ws], out[q]);
    }
    if (c.param) clearance_lift(c.line, out);
}

// axial and lateral coordinates of a global position in a gate's frame: apl = (a, p2, p3)
ATO_HD void gate_coords(const ato_gate_plane& g, const double* x, double* apl) {
    const double d[3] = {x[0] - g.centre[0], x[1] - g.centre[1], x[2] - g.centre[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double e[3] = {g.R[i], g.R[3 + i], g.R[6 + i]};
        apl[i] = dot3(e, d);
    }
}

ATO_HD double gate_margin(const ato_gate_plane& g, double p2, double p3) {
    if (g.shape == ATO_GATE_CIRCLE) return g.d_max - sqrt(fma(p3, p3, p2 * p2));
    return g.d_max - fmax(fabs(p2), fabs(p3));      // fmax drops a NaN operand: gate_offer looks at p2, p3 themselves
}

ATO_HD bool gate_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }      // false for NaN

// the partial record in registers: named scalars and selects only, so that no element is reached through a pointer
// the compiler has to keep in memory
struct GateRec {
    double count, margin, x, p2, p3, dir, bad;
};

// offer the crossing at abscissa x with coordinates apl and direction dir to the record
ATO_HD void gate_offer(const ato_gate_plane& g, double x, const double* apl, double dir, GateRec& r) {
    const double m = gate_margin(g, apl[1], apl[2]);
    const bool ok = gate_finite(apl[0]) && gate_finite(m) && gate_finite(apl[1]) && gate_finite(apl[2]);
    const bool take = ok && m > r.margin;
    r.count += 1.0;
    r.bad = ok ? r.bad : 1.0;
    r.margin = take ? m : r.margin;
    r.x = take ? x : r.x;
    r.p2 = take ? apl[1] : r.p2;
    r.p3 = take ? apl[2] : r.p3;
    r.dir = take ? dir : r.dir;
}

// One (gate gi, interval n, instance b): the junction before the interval's first point, its S sample steps and,
// on open lines, the first and the last point of the lap. pos: the positions' buffer on the grid sg; w points at
// the instance's element 0 of the decision vector, element stride ws; out [GATE_PART].
ATO_HD void gate_interval(const GateD& a, const SampleGrid& sg, int gi, int n, int b, const double* __restrict__ pos,
                          const double* __restrict__ w, long ws, double* out) {
    const ato_gate_plane& g = a.planes[gi];
    const int S = a.c.S1 - 1, N = a.c.N;
    GateRec rec{0.0, -ATO_INF, 0.0, 0.0, 0.0, 0.0, 0.0};
    double x[3], cur[3], prev[3];
    sg.load<3>(pos, n, 0, b, x);
    gate_coords(g, x, cur);
    if (!gate_finite(cur[0])) rec.bad = 1.0;
    if (n > 0 || a.closed) {
        // the junction (or the wrap): the later point, unrefined
        sg.load<3>(pos, n > 0 ? n - 1 : N - 1, S, b, x);
        gate_coords(g, x, prev);
        if (!gate_finite(prev[0])) rec.bad = 1.0;
        if ((prev[0] >= 0.0) != (cur[0] >= 0.0)) gate_offer(g, 0.0, cur, cur[0] >= 0.0 ? 1.0 : -1.0, rec);
    }
    // Scan the S sample steps first and only note which of them change sign (bit i: step [x_i, x_i+1]; S <= 64),
    // then bisect the noted steps in ascending order: the lanes of a wave that have a crossing refine their first
    // ones together, whichever steps they lie in, instead of one step's lanes at a time.
    const double first_a = cur[0];
    const bool first_tol = n == 0 && !a.closed && fabs(cur[0]) <= a.axial_tol;
    const double first[3] = {cur[0], cur[1], cur[2]};
    unsigned long long change = 0ULL, nonneg = 0ULL;
    for (int i = 0; i < S; ++i) {
#pragma unroll
        for (int q = 0; q < 3; ++q) prev[q] = cur[q];
        sg.load<3>(pos, n, i + 1, b, x);
        gate_coords(g, x, cur);
        if (!gate_finite(cur[0])) rec.bad = 1.0;
        if (i == 0 && first_tol) gate_offer(g, 0.0, first, cur[0] - first_a >= 0.0 ? 1.0 : -1.0, rec);
        const bool slo = prev[0] >= 0.0;
        nonneg |= (unsigned long long)slo << i;
        change |= (unsigned long long)(slo != (cur[0] >= 0.0)) << i;
    }
    while (change != 0ULL) {
        const int i = __builtin_ctzll(change);
        change &= change - 1ULL;
        const bool slo = (nonneg >> i) & 1ULL;
        double lo = (double)i / (double)S, hi = (double)(i + 1) / (double)S;
        double at[3];
        sg.load<3>(pos, n, i + 1, b, x);
        gate_coords(g, x, at);
        for (int it = 0; it < GATE_BISECT; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) break;
            double xm[3], am[3];
            gate_point(a, n, mid, w, ws, xm);
            gate_coords(g, xm, am);
            if (!gate_finite(am[0])) rec.bad = 1.0;
            if ((am[0] >= 0.0) == slo) {
                lo = mid;
            } else {
                hi = mid;
#pragma unroll
                for (int q = 0; q < 3; ++q) at[q] = am[q];
            }
        }
        gate_offer(g, hi, at, slo ? -1.0 : 1.0, rec);
    }
    if (n == N - 1 && !a.closed && fabs(cur[0]) <= a.axial_tol)
        gate_offer(g, 1.0, cur, cur[0] - prev[0] >= 0.0 ? 1.0 : -1.0, rec);
    out[GP_COUNT] = rec.count;
    out[GP_MARGIN] = rec.margin;
    out[GP_X] = rec.x;
    out[GP_P2] = rec.p2;
    out[GP_P3] = rec.p3;
    out[GP_DIR] = rec.dir;
    out[GP_BAD] = rec.bad;
}

// the partial record of (gate gi, interval n, instance b) in the handle's buffer: component c at part_at(...) + c B
ATO_HD long part_at(int N, int B, int gi, int n, int b) { return ((long)gi * N + n) * GATE_PART * B + b; }

// One (gate gi, instance b): the records in ascending n into the GATE_NCH channels out; w, ws as above (h_n is
// element n of the decision vector)
ATO_HD void gate_reduce(const GateD& a, int gi, int b, int B, const double* __restrict__ part,
                        const double* __restrict__ w, long ws, double* out) {
    const int N = a.c.N;
    const double nan = __builtin_nan("");
    double count = 0.0, best = -ATO_INF, run = 0.0, bad = 0.0;
    double bn = -1.0, bx = nan, bt = nan, b2 = nan, b3 = nan, bd = 0.0;
    for (int n = 0; n < N; ++n) {
        const double* r = part + part_at(N, B, gi, n, b);
        const double hn = w[(long)n * ws];
        count += r[(long)GP_COUNT * B];
        if (r[(long)GP_BAD * B] != 0.0) bad = 1.0;
        if (!(hn > 0.0 && gate_finite(hn))) bad = 1.0;      // no passage time without finite positive steps
        const double m = r[(long)GP_MARGIN * B];
        if (m > best) {
            best = m;
            bn = (double)n;
            bx = r[(long)GP_X * B];
            bt = fma(bx, hn, run);
            b2 = r[(long)GP_P2 * B];
            b3 = r[(long)GP_P3 * B];
            bd = r[(long)GP_DIR * B];
        }
        run += hn;
    }
    out[0] = count;
    out[1] = best;
    out[2] = bn;
    out[3] = bx;
    out[4] = bt;
    out[5] = b2;
    out[6] = b3;
    out[7] = sqrt(fma(b3, b3, b2 * b2));
    out[8] = bad != 0.0 ? nan : bd;
}

// val: channel c of (gate gi, instance b) at [(c G + gi) B + b] (interleaved) or [(b G + gi) GATE_NCH + c]
ATO_HD void gate_store(double* val, bool il, int G, int B, int gi, int b, const double* out) {
#pragma unroll
    for (int c = 0; c < GATE_NCH; ++c) {
        if (il) val[((long)c * G + gi) * B + b] = out[c];
        else val[((long)b * G + gi) * GATE_NCH + c] = out[c];
    }
}

#ifdef __HIPCC__
// the two kernels and their launcher (after launch_clearance_pos into pos): ato_gatecheck.hip. which: bit 0 the
// crossings, bit 1 the reduction
hipError_t launch_gatecheck(const GateD& a, int B, int layout, const double* w, const double* pos, double* part,
                            double* val, hipStream_t st, int which);
#endif  // __HIPCC__

}  // namespace ato
