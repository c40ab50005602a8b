// ato_extrema.hpp -- the minimum and maximum of every node-vector component over WHOLE intervals, with a rigorous
// enclosure: what the audit's channels 0-6 leave open between two samples.
//
// Between nodes every component v of the node vector is a polynomial of degree K in the interval's abscissa,
//   p_{n,v}(x) = sum_j l_j(x) V[n, j, v],   x in [0, 1],
// and in parametric problems channel NV is p_{n,0}'(x) / h_n (the audit's sdot). Per (channel v, instance b) the
// check reports ATO_EXTREMA_NCH = 8 doubles: min, its interval and abscissa, max, its interval and abscissa, a
// slack >= 0 with  true min >= min - slack  and  true max <= max + slack, and a flag (0; 1: the visit cap was hit;
// NaN: a non-finite value, or for sdot an h_n that is not finite and positive).
//
// Method, per (v, n, b):
//   1. c_i = sum_j T[i][j] V_j, j ascending, fused multiply-adds: the Bernstein coefficients of p on [0, 1]. T is
//      made on the host in long double (extrema_table: the product of the linear factors of l_j in Bernstein
//      form) and rounded to fp64. The same loop forms A_i = sum_j |T[i][j]| |V_j|. K1 bit-equal node values are
//      the constant polynomial exactly: c_i = V_0 and no rounding term. The derivative channel takes the
//      degree-(K - 1) coefficients d_i = K (c_{i+1} - c_i) / h_n.
//   2. Branch and bound over dyadic boxes [k 2^-d, (k + 1) 2^-d]. The coefficients of a box bound p on it (convex
//      hull) and its two end coefficients are values of p. A box is dropped when its largest coefficient is at
//      most (best attained maximum + stop) and its smallest at least (best attained minimum - stop), else halved
//      (de Casteljau at 1/2: averages only). stop = 2^-44 max(1, max_i |c_i|). No stack: the traversal keeps
//      (k, d) and re-derives a box's coefficients from the interval's root coefficients along the bits of k, the
//      most significant first; a right half is the left half of the reversed polynomial, so every lane of a wave
//      runs the same instructions whatever its k. Depth is capped at EXT_DMAX = 48 (k 2^-d stays exact) and the
//      visits at EXT_CAP = 4096; at the cap the root box's bounds stand in for what was not visited and flag = 1.
//   3. The two winning abscissae are re-evaluated through the Lagrange form (lagrange_weight / lagrange_dweight,
//      the products and the sum in the order of gate_point and audit_point): the reported min and max are values
//      the audit would report at those abscissae.
//
// Slack. Let U be the largest coefficient of any dropped or finished box (at the cap: of the root box) and L the
// smallest. Exact coefficients of a box bound p on it, so with e the distance between a computed and an exact box
// coefficient, p <= U + e and p >= L - e everywhere on the interval, and
//   slack = max(U - max, min - L, 0) + e
// with the REPORTED (re-evaluated) min and max: their own rounding is inside the first term, not assumed small.
// e = e_conv + e_sub, u = 2^-53:
//   e_conv: T[i][j] carries one rounding (u |T| |V|), the K1-term multiply-add chain at most K1 more:
//           |c_i - exact| <= (K1 + 1) u A_i; the header takes (K1 + 3) u max_i A_i, the two spare units covering
//           the rounding of this bound's own arithmetic.
//   e_sub:  a halving is D levels of averages, each rounds once (the 0.5 is exact) and averages do not amplify:
//           at most D u max|c| per halving, at most EXT_DMAX halvings: e_sub = 48 D u max_i |c_i| <= 432 u max|c|,
//           i.e. about 5 K^2 ulp of the coefficient scale.
//   sdot:   d_i = K (c_{i+1} - c_i) / h_n: e_conv' = 2 K e_conv / h_n + 4 u max|d| (difference, product, quotient
//           and one spare), e_sub' = 48 (K - 1) u max|d|.
// With the stop width 2^-44 scale, scale = max(1, max_i A_i) >= max(1, max|c|) (for sdot: 2 K scale / h_n), a
// finished search has slack <= (2^-44 + 432 u + (K1 + 3) u) scale + the re-evaluation's rounding < 2^-42 scale.
//
// Work split: a block is 64 instances x 4 waves; its lanes share (v, n-range) and differ in b, so decision-vector
// reads of the interleaved layout are contiguous. The four waves take the intervals of the block's n-range
// round-robin, T and tau are staged in LDS once per block, the waves' records are combined through LDS. Grid
// (ceil(B / 64), NVX, nsplit): nsplit in [1, 16] splits the lap so that small batches still fill the device
// (extrema_nsplit); with nsplit > 1 the records go to a buffer on the handle [nsplit][NCH][NVX][B] and k_ext_combine
// folds them per (v, b). The combine rule (ext_combine) is a total order -- better value, ties to the earliest
// (n, x); slack by max; flag by or / NaN -- so any combination order gives the same bits: no atomics, no
// device-wide synchronisation, results do not depend on the batch. No matrix instructions: the only dense
// product is the K1 x K1 conversion and its fixed order is what keeps device, host builds and oracles comparable.
//
// Everything ATO_HD here is shared by the kernels (ato_extrema.hip) and host builds. No input value moves a read:
// every index is n, j, v or b. CPC progress variables are not read and no centreline is needed.
#pragma once
#include "ato_sample.hpp"

namespace ato {

constexpr int EXT_NCH = ATO_EXTREMA_NCH;
constexpr int EXT_DMAX = 48;           // deepest box: k 2^-d exact in fp64, e_sub's factor
constexpr int EXT_CAP = 4096;          // visits per (v, n, b)
constexpr int EXT_SPLIT_MAX = 16;
constexpr int EXT_LANES = 64, EXT_WAVES = 4;
constexpr double EXT_U = 1.1102230246251565404e-16;        // 2^-53
constexpr double EXT_STOP = 5.6843418860808014870e-14;     // 2^-44

// extrema arguments (kernel argument)
struct ExtD {
    int32_t N, K1, NV, NVX, nw, nsplit;
    const double* tab;      // [K1][K1] T, then tau [K1] (ato_create)
};

// [K1][K1] T[i][j]: Bernstein coefficient i (degree K = K1 - 1, on [0, 1]) of l_j over tau_0 .. tau_K. Host side,
// long double: l_j is built as a product of linear factors in Bernstein form, (x - t) = (-t, 1 - t) of degree 1, a
// degree-m polynomial a times a linear b being c_i = ((m + 1 - i) a_i b_0 + i a_{i-1} b_1) / (m + 1); rounded once.
inline void extrema_table(const double* tau, int K1, double* T) {
    for (int j = 0; j < K1; ++j) {
        long double a[ATO_KMAX + 2] = {1.0L}, c[ATO_KMAX + 2];
        int m = 0;
        for (int r = 0; r < K1; ++r) {
            if (r == j) continue;
            const long double den = (long double)tau[j] - (long double)tau[r];
            const long double b0 = -(long double)tau[r] / den, b1 = (1.0L - (long double)tau[r]) / den;
            for (int i = 0; i <= m + 1; ++i) {
                const long double lo = i <= m ? (long double)(m + 1 - i) * a[i] * b0 : 0.0L;
                const long double hi = i >= 1 ? (long double)i * a[i - 1] * b1 : 0.0L;
                c[i] = (lo + hi) / (long double)(m + 1);
            }
            ++m;
            for (int i = 0; i <= m; ++i) a[i] = c[i];
        }
        for (int i = 0; i < K1; ++i) T[i * K1 + j] = (double)a[i];
    }
}

// 0 (ATO_OK) or the error code of an ato_extrema call with these arguments; *msg gets the reason
inline int extrema_check(const ProbD& p, int batch, int layout, bool has_w, bool has_val, const char** msg) {
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (int rc = check_layout(layout, msg)) return rc;
    if (!has_w || !has_val) { *msg = "null buffer"; return ATO_ERR_ARG; }
    // nothing is lifted, so there is no check_line: no centreline table is needed
    return check_collocation(p, "extrema of RK4-transcribed problems (K = 0) are not supported", msg);
}

inline int extrema_nvx(const ProbD& p) { return p.frame != GLOBAL ? p.NV + 1 : p.NV; }

// the lap's split: the fewest parts in [1, 16] that give about two blocks per compute unit (256 of them), every
// wave of a block keeping at least one interval
inline int extrema_nsplit(int N, int NVX, int B) {
    const long blocks = (((long)B + EXT_LANES - 1) / EXT_LANES) * NVX;
    long s = (512 + blocks - 1) / blocks;
    const long most = (N + EXT_WAVES - 1) / EXT_WAVES;
    if (s > most) s = most;
    if (s > EXT_SPLIT_MAX) s = EXT_SPLIT_MAX;
    return s < 1 ? 1 : (int)s;
}

inline ExtD extrema_args(const ProbD& p, int nsplit, const double* tab) {
    return ExtD{p.N, p.K1, p.NV, extrema_nvx(p), p.nw, nsplit, tab};
}

ATO_HD bool ext_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }      // false for NaN

// l_j'(x): lagrange_drow's sum for one j (m and r ascending)
ATO_HD double lagrange_dweight(const double* tau, int K1, double x, int j) {
    double acc = 0.0;
    for (int m = 0; m < K1; ++m) {
        if (m == j) continue;
        double v = 1.0 / (tau[j] - tau[m]);
        for (int r = 0; r < K1; ++r) {
            if (r == j || r == m) continue;
            v *= (x - tau[r]) / (tau[j] - tau[r]);
        }
        acc += v;
    }
    return acc;
}

// the record of one (v, b), of a part of it, or of one interval: the eight channels as named scalars
struct ExtRec {
    double mn, mn_n, mn_x, mx, mx_n, mx_x, slack, flag;
};

ATO_HD ExtRec ext_empty() {
    const double nan = __builtin_nan("");
    return ExtRec{ATO_INF, -1.0, nan, -ATO_INF, -1.0, nan, 0.0, 0.0};
}

// fold b into a: a total order, so the result does not depend on the order of the folds
ATO_HD void ext_combine(ExtRec& a, const ExtRec& b) {
    const bool lo = b.mn < a.mn || (b.mn == a.mn && (b.mn_n < a.mn_n || (b.mn_n == a.mn_n && b.mn_x < a.mn_x)));
    const bool hi = b.mx > a.mx || (b.mx == a.mx && (b.mx_n < a.mx_n || (b.mx_n == a.mx_n && b.mx_x < a.mx_x)));
    const bool take_lo = lo && b.mn_n >= 0.0, take_hi = hi && b.mx_n >= 0.0;
    a.mn = take_lo ? b.mn : a.mn;
    a.mn_n = take_lo ? b.mn_n : a.mn_n;
    a.mn_x = take_lo ? b.mn_x : a.mn_x;
    a.mx = take_hi ? b.mx : a.mx;
    a.mx_n = take_hi ? b.mx_n : a.mx_n;
    a.mx_x = take_hi ? b.mx_x : a.mx_x;
    a.slack = b.slack > a.slack ? b.slack : a.slack;
    a.flag = (a.flag != a.flag || b.flag != b.flag) ? __builtin_nan("") : (b.flag > a.flag ? b.flag : a.flag);
}

// the left (right: the right) half of the box with coefficients c[0 .. D]: de Casteljau at 1/2, in place. The
// right half is the reversed left half of the reversed polynomial: the same averages, one instruction stream.
template <int D>
ATO_HD void ext_halve(double* c, bool right) {
#pragma unroll
    for (int i = 0; i < (D + 1) / 2; ++i) {
        const double lo = c[i], hi = c[D - i];
        c[i] = right ? hi : lo;
        c[D - i] = right ? lo : hi;
    }
#pragma unroll
    for (int r = 1; r <= D; ++r)
#pragma unroll
        for (int i = D; i >= r; --i) c[i] = 0.5 * (c[i - 1] + c[i]);
#pragma unroll
    for (int i = 0; i < (D + 1) / 2; ++i) {
        const double lo = c[i], hi = c[D - i];
        c[i] = right ? hi : lo;
        c[D - i] = right ? lo : hi;
    }
}

// what a search leaves: the best attained coefficient values and their abscissae, the bounds U, L of the dropped
// and finished boxes, and whether the visit cap was hit
struct ExtHit {
    double mn, mn_x, mx, mx_x, U, L;
    bool capped;
};

ATO_HD void ext_offer(ExtHit& h, double v, double x) {
    const bool lo = v < h.mn || (v == h.mn && x < h.mn_x), hi = v > h.mx || (v == h.mx && x < h.mx_x);
    h.mn = lo ? v : h.mn;
    h.mn_x = lo ? x : h.mn_x;
    h.mx = hi ? v : h.mx;
    h.mx_x = hi ? x : h.mx_x;
}

// branch and bound on the finite root coefficients root[0 .. D] of one interval
template <int D>
ATO_HD void ext_search(const double* root, double stop, ExtHit& h) {
    double rlo = root[0], rhi = root[0];
#pragma unroll
    for (int i = 1; i <= D; ++i) {
        rlo = root[i] < rlo ? root[i] : rlo;
        rhi = root[i] > rhi ? root[i] : rhi;
    }
    h = ExtHit{root[0], 0.0, root[0], 0.0, -ATO_INF, ATO_INF, false};
    ext_offer(h, root[D], 1.0);
    unsigned long long k = 0ULL;
    int d = 0, visits = 0;
    for (;;) {
        double c[D + 1];
#pragma unroll
        for (int i = 0; i <= D; ++i) c[i] = root[i];
        for (int lev = d - 1; lev >= 0; --lev) ext_halve<D>(c, (k >> lev) & 1ULL);
        double lo = c[0], hi = c[0];
#pragma unroll
        for (int i = 1; i <= D; ++i) {
            lo = c[i] < lo ? c[i] : lo;
            hi = c[i] > hi ? c[i] : hi;
        }
        ext_offer(h, c[0], ldexp((double)k, -d));
        ext_offer(h, c[D], ldexp((double)(k + 1ULL), -d));
        ++visits;
        const bool open = hi > h.mx + stop || lo < h.mn - stop;
        if (open && d < EXT_DMAX) {
            if (visits >= EXT_CAP) {
                h.capped = true;
                h.U = rhi;
                h.L = rlo;
                return;
            }
            k <<= 1;
            ++d;
            continue;
        }
        h.U = hi > h.U ? hi : h.U;
        h.L = lo < h.L ? lo : h.L;
        while (d > 0 && (k & 1ULL)) {
            k >>= 1;
            --d;
        }
        if (d == 0) return;
        k += 1ULL;
    }
}

// p(x) (deriv: p'(x) / h) of the node values z[j zs], j = 0 .. K1 - 1, through the Lagrange form, as gate_point and
// audit_point sum it. K1 is a run-time value here and the node values are read again: rolled loops, nothing of the
// re-evaluation is live during the search
ATO_HD double ext_value(const double* tau, int K1, const double* __restrict__ z, long zs, double x, bool deriv,
                        double h) {
    double acc = (deriv ? lagrange_dweight(tau, K1, x, 0) : lagrange_weight(tau, K1, x, 0)) * z[0];
#pragma unroll 1
    for (int j = 1; j < K1; ++j)
        acc = fma(deriv ? lagrange_dweight(tau, K1, x, j) : lagrange_weight(tau, K1, x, j), z[(long)j * zs], acc);
    return deriv ? acc / h : acc;
}

// search, re-evaluation and slack of one polynomial with root coefficients c[0 .. D]; e: the conversion's bound
template <int D>
ATO_HD void ext_finish(const double* tau, int K1, const double* __restrict__ z, long zs, const double* c, double e,
                       bool same, bool deriv, double h, int n, ExtRec& r) {
    double cmax = fabs(c[0]);
#pragma unroll
    for (int i = 1; i <= D; ++i) cmax = fabs(c[i]) > cmax ? fabs(c[i]) : cmax;
    ExtHit hit;
    ext_search<D>(c, EXT_STOP * (cmax > 1.0 ? cmax : 1.0), hit);
    const double mn = ext_value(tau, K1, z, zs, hit.mn_x, deriv, h), mx = ext_value(tau, K1, z, zs, hit.mx_x, deriv, h);
    const double err = same ? 0.0 : e + (double)(EXT_DMAX * D) * EXT_U * cmax;
    double gap = hit.U - mx;
    gap = mn - hit.L > gap ? mn - hit.L : gap;
    gap = gap > 0.0 ? gap : 0.0;
    const bool ok = ext_finite(mn) && ext_finite(mx);
    const double nan = __builtin_nan("");
    r = ExtRec{mn, (double)n, hit.mn_x, mx, (double)n, hit.mx_x, gap + err, hit.capped ? 1.0 : 0.0};
    if (!ok) {
        r = ext_empty();
        r.flag = nan;
    }
}

// One (channel v, interval n) of one instance: w points at the instance's element 0 of the decision vector,
// element stride ws; tab: T then tau (LDS in the kernel).
template <int K1>
ATO_HD void ext_interval(const ExtD& a, const double* tab, int v, int n, const double* __restrict__ w, long ws,
                         ExtRec& r) {
    constexpr int K = K1 - 1;
    const double* tau = tab + K1 * K1;
    const bool deriv = v == a.NV;
    const double* z = w + ((long)a.N + (long)n * K1 * a.NV + (deriv ? 0 : v)) * ws;
    const long zs = (long)a.NV * ws;
    // j is the rolled outer loop (one node value live at a time), i the unrolled inner one: every c_i still sums in
    // ascending j
    double c[K1], ab[K1];
    const double V0 = z[0];
    bool same = true;
#pragma unroll
    for (int i = 0; i < K1; ++i) {
        c[i] = tab[i * K1] * V0;
        ab[i] = fabs(tab[i * K1]) * fabs(V0);
    }
#pragma unroll 1
    for (int j = 1; j < a.K1; ++j) {
        const double Vj = z[(long)j * zs];
        same = same && Vj == V0;
#pragma unroll
        for (int i = 0; i < K1; ++i) {
            c[i] = fma(tab[i * K1 + j], Vj, c[i]);
            ab[i] = fma(fabs(tab[i * K1 + j]), fabs(Vj), ab[i]);
        }
    }
    double A = 0.0, Asum = 0.0;
#pragma unroll
    for (int i = 0; i < K1; ++i) {
        c[i] = same ? V0 : c[i];
        A = ab[i] > A ? ab[i] : A;
        Asum += ab[i];
    }
    const double nan = __builtin_nan("");
    r = ext_empty();
    r.flag = nan;
    if (!ext_finite(Asum)) return;
    const double e = (double)(K1 + 3) * EXT_U * A;
    if (!deriv) {
        ext_finish<K>(tau, a.K1, z, zs, c, e, same, false, 1.0, n, r);
        return;
    }
    const double h = w[(long)n * ws];
    if (!(h > 0.0 && ext_finite(h))) return;
    double dc[K > 1 ? K : 1], dsum = 0.0, dmax = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        dc[i] = (double)K * (c[i + 1] - c[i]) / h;
        dsum += fabs(dc[i]);
        dmax = fabs(dc[i]) > dmax ? fabs(dc[i]) : dmax;
    }
    const double ed = 2.0 * (double)K * e / h + 4.0 * EXT_U * dmax;
    if (!ext_finite(dsum) || !ext_finite(ed)) return;
    ext_finish<K - 1>(tau, a.K1, z, zs, dc, ed, same, true, h, n, r);
}

// channel c of (v, b): val [(c NVX + v) B + b] (interleaved) or [(b NVX + v) NCH + c]
ATO_HD void ext_store(double* val, bool il, int NVX, int B, int v, int b, const ExtRec& r) {
    const double o[EXT_NCH] = {r.mn, r.mn_n, r.mn_x, r.mx, r.mx_n, r.mx_x, r.slack, r.flag};
#pragma unroll
    for (int c = 0; c < EXT_NCH; ++c) {
        if (il) val[((long)c * NVX + v) * B + b] = o[c];
        else val[((long)b * NVX + v) * EXT_NCH + c] = o[c];
    }
}

// the partial record of (part s, v, b): component c at ext_part_at(...) + c NVX B
ATO_HD long ext_part_at(int NVX, int B, int s, int v, int b) { return ((long)s * EXT_NCH * NVX + v) * B + b; }

#ifdef __HIPCC__
// the two kernels and their launcher (ato_extrema.hip); part: [nsplit][NCH][NVX][B] when a.nsplit > 1
hipError_t launch_extrema(const ExtD& a, int B, int layout, const double* w, double* part, double* val, double* ival,
                          hipStream_t st);
#endif  // __HIPCC__

}  // namespace ato
