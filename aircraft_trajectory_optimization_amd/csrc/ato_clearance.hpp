// ato_clearance.hpp -- dense global positions of a batch of collocation solutions.
//
// One work item = (instance b, interval n, sample i): the first three state components of the interval's
// collocation polynomial at abscissa x_i,
//   q = sum_j l_j(x_i) Z[n, j, 0..2],
// x_i = i / S for samples = S >= 1 (S + 1 points, both ends), or the nodes tau_0 .. tau_K themselves for
// samples = 0 (identity weights: the reference's own collision test, base_raceline.py:1312-1327). In the
// global frame q is the position. In the parametric frame (global_r or the relative attitude: the position
// does not depend on the attitude) q = (s, y, n) and the position is
//   x_c(s) + y e_y(s) + n e_n(s)
// with the centreline evaluated at the sample's own interpolated s: s is free at interior nodes, so a
// per-boundary table (the replay's) does not reach them. (Bounds, s' >= 0 and the ODE defects at the same samples:
// ato_audit.hpp.) The centreline is the two piecewise cubics of
// SplineCenterline (_xc and _ry, linear extrapolation pieces included; piece = number of knots <= s) and
// the frame is frame_from_terms: e_s = x_c' / |x_c'|, e_y = normalise(r_y - e_s (e_s . r_y)),
// e_n = e_s x e_y. CPC variables sit after the node block and are not read.
//
// Shared by the HIP kernel (k_clearance_pos, ato_clearance.hip) and the CPU twin
// (tests/native/clearance_hostcheck.cpp): clearance_point() is ATO_HD. Sums, Horner steps, dot and cross
// products are explicit fused multiply-adds in a fixed order, so the twin and the device round alike
// whatever the compilers would contract; l_j(tau_k) is exactly delta_jk, so sample 0 is node 0 bit for bit.
#pragma once
#include <cmath>
#include "ato_program.hpp"

namespace ato {

constexpr int CLEAR_SMAX = 64;      // samples per interval

// the centreline as the kernel reads it: knots kx [nx], coefficients cx [nx + 1][4][3] (piece, power, axis)
// of x_c; kr [nr], cr [nr + 1][4][3] of r_y. Piece 0 is left of the first knot, piece nk right of the last.
struct LineD {
    int32_t nx, nr;
    const double *kx, *cx, *kr, *cr;
};

// clearance arguments (kernel argument): only what the kernel reads
struct ClearD {
    int32_t N, K1, NV, S1, param;
    int32_t nw;
    const double* wt;      // [S1][K1] Lagrange weights l_j(x_i)
    LineD line;
};

inline int clearance_points(int K1, int samples) { return samples == 0 ? K1 : samples + 1; }

// l_j(x_i) by the product formula of replay_weights: over r != j (ascending) of (x - tau_r) / (tau_j - tau_r);
// host side, fp64: the one table the kernel, the twin and the test oracle use
inline void clearance_weights(const double* tau, int K1, int samples, double* wt) {
    const int S1 = clearance_points(K1, samples);
    for (int i = 0; i < S1; ++i) {
        const double x = samples == 0 ? tau[i] : (double)i / (double)samples;
        for (int j = 0; j < K1; ++j) {
            double v = 1.0;
            for (int r = 0; r < K1; ++r) {
                if (r == j) continue;
                v *= (x - tau[r]) / (tau[j] - tau[r]);
            }
            wt[i * K1 + j] = v;
        }
    }
}

// 0 (ATO_OK) or the error code of an ato_clearance call with these arguments; *msg gets the reason
inline int clearance_check(const ProbD& p, bool has_line, int batch, int layout, int samples, const char** msg) {
    *msg = "";
    if (batch < 1) { *msg = "batch must be >= 1"; return ATO_ERR_ARG; }
    if (layout != ATO_LAYOUT_INTERLEAVED && layout != ATO_LAYOUT_INSTANCE_MAJOR) {
        *msg = "unknown layout";
        return ATO_ERR_ARG;
    }
    if (samples < 0 || samples > CLEAR_SMAX) { *msg = "samples must be in [0, 64]"; return ATO_ERR_ARG; }
    if (p.trans != ATO_TRANS_COLLOCATION) {
        *msg = "clearance of RK4-transcribed problems (K = 0) is not supported";
        return ATO_ERR_UNSUPPORTED;
    }
    if (p.frame != GLOBAL && !has_line) {
        *msg = "parametric clearance needs the centreline table (ato_clearance_set_line)";
        return ATO_ERR_STATE;
    }
    return ATO_OK;
}

inline ClearD clearance_args(const ProbD& p, int samples, const double* wt, const LineD& line) {
    return ClearD{p.N, p.K1, p.NV, clearance_points(p.K1, samples), p.frame != GLOBAL ? 1 : 0, p.nw, wt, line};
}

// number of knots <= s (numpy.searchsorted(knots, s, side='right'))
ATO_HD int clearance_piece(const double* __restrict__ k, int nk, double s) {
    int lo = 0, hi = nk;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (k[mid] <= s) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// value (and first derivative, if d) of a piecewise cubic at s: Horner in fused multiply-adds
ATO_HD void clearance_cubic(const double* __restrict__ k, const double* __restrict__ c, int nk, double s, double* v,
                            double* d) {
    const int pc = clearance_piece(k, nk, s);
    const double x = s - k[pc > 0 ? pc - 1 : 0];
    const double* q = c + (long)pc * 12;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c0 = q[a], c1 = q[3 + a], c2 = q[6 + a], c3 = q[9 + a];
        v[a] = fma(fma(fma(c3, x, c2), x, c1), x, c0);
        if (d) d[a] = fma(fma(3.0 * c3, x, 2.0 * c2), x, c1);
    }
}

ATO_HD double clearance_dot(const double* a, const double* b) { return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0])); }

// (s, y, n) -> x_c(s) + y e_y(s) + n e_n(s)
ATO_HD void clearance_lift(const LineD& L, double* q) {
    const double y = q[1], n = q[2];
    double xc[3], xs[3], ry[3], es[3], ey[3], en[3];
    clearance_cubic(L.kx, L.cx, L.nx, q[0], xc, xs);
    clearance_cubic(L.kr, L.cr, L.nr, q[0], ry, nullptr);
    const double mag = sqrt(clearance_dot(xs, xs));
#pragma unroll
    for (int a = 0; a < 3; ++a) es[a] = xs[a] / mag;
    const double pr = clearance_dot(es, ry);
#pragma unroll
    for (int a = 0; a < 3; ++a) ey[a] = fma(-es[a], pr, ry[a]);
    const double my = sqrt(clearance_dot(ey, ey));
#pragma unroll
    for (int a = 0; a < 3; ++a) ey[a] = ey[a] / my;
    en[0] = fma(es[1], ey[2], -(es[2] * ey[1]));
    en[1] = fma(es[2], ey[0], -(es[0] * ey[2]));
    en[2] = fma(es[0], ey[1], -(es[1] * ey[0]));
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = fma(n, en[a], fma(y, ey[a], xc[a]));
}

// One (instance, interval n, sample i). w points at the instance's element 0 of the decision vector, element
// stride ws; out[c] receives component c of the global position.
ATO_HD void clearance_point(const ClearD& a, int n, int i, const double* __restrict__ w, long ws, double* out) {
    const double* l = a.wt + (long)i * a.K1;
    const double* z = w + ((long)a.N + (long)n * a.K1 * a.NV) * ws;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = l[0] * z[(long)c * ws];
    for (int j = 1; j < a.K1; ++j) {
        const double lj = l[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = fma(lj, z[((long)j * a.NV + c) * ws], out[c]);
    }
    if (a.param) clearance_lift(a.line, out);
}

#ifdef __HIPCC__
// the kernel and its launcher: ato_clearance.hip
hipError_t launch_clearance_pos(const ClearD& a, int B, int layout, const double* w, double* pos, hipStream_t st);
#endif  // __HIPCC__

}  // namespace ato
