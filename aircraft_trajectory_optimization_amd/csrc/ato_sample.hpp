// ato_sample.hpp -- the sampling layer the post-solve checks share (replay, mesh transfer, clearance, audit,
// gate passage).
//
// Each of them evaluates an interval's collocation polynomial away from its nodes and, in parametric problems,
// places the result through the centreline. What they have in common lives here, once:
//   - the Lagrange basis l_j(x) over tau_0 .. tau_K and its derivative, as host-side fp64 row functions, and the
//     sample abscissae of the clearance and the audit (clearance_points, clearance_weights);
//   - the centreline as the kernels read it (LineD), its packing from an ato_line_table, the piece search, the
//     cubic evaluator and the frame e_s, e_y, e_n of frame_from_terms;
//   - the (interval, sample) x instance grid of the clearance and the audit: where an instance's decision vector
//     starts, its element stride, and the two output layouts;
//   - the argument checks every call starts with, and the zero-curvature NodeGeom of the global models.
// A new post-solve check starts from this header and keeps only its own arithmetic.
//
// Everything ATO_HD is shared by the HIP kernels and their CPU twins (tests/native/*_hostcheck.cpp). Horner steps,
// dot and cross products are explicit fused multiply-adds in a fixed order, so the twins and the device round
// alike whatever the compilers would contract. The weight tables are plain multiplications and divisions:
// l_j(tau_k) is exactly delta_jk.
#pragma once
#include <cmath>
#include <vector>
#include "ato_program.hpp"

namespace ato {

// the largest substep count of the replay and sample count of the clearance and the audit: one limit, the
// device weight tables of a handle are sized by it and the messages below name it
constexpr int SAMPLE_SMAX = 64;

// ---------------------------------------------------------------- Lagrange basis (host side, fp64)
// l_j(x): the product over r != j (ascending) of (x - tau_r) / (tau_j - tau_r). ATO_HD: the gate check evaluates
// it on the device at bisection midpoints, one weight at a time (no row array in registers)
ATO_HD double lagrange_weight(const double* tau, int K1, double x, int j) {
    double v = 1.0;
    for (int r = 0; r < K1; ++r) {
        if (r == j) continue;
        v *= (x - tau[r]) / (tau[j] - tau[r]);
    }
    return v;
}

// l_j(x), j = 0 .. K1 - 1
ATO_HD void lagrange_row(const double* tau, int K1, double x, double* l) {
    for (int j = 0; j < K1; ++j) l[j] = lagrange_weight(tau, K1, x, j);
}

// l_j'(x) = sum_{m != j} 1 / (tau_j - tau_m) prod_{r != j, m} (x - tau_r) / (tau_j - tau_r), m and r ascending
inline void lagrange_drow(const double* tau, int K1, double x, double* dl) {
    for (int j = 0; j < K1; ++j) {
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
        dl[j] = acc;
    }
}

// points per interval: i / samples, i = 0 .. samples (both ends), or the nodes tau_0 .. tau_K for samples = 0
inline int clearance_points(int K1, int samples) { return samples == 0 ? K1 : samples + 1; }
inline double sample_abscissa(const double* tau, int samples, int i) {
    return samples == 0 ? tau[i] : (double)i / (double)samples;
}

// [S1][K1] l_j(x_i): the one table the kernels, the twins and the test oracles use (the clearance's name: the
// audit takes the clearance's samples)
inline void clearance_weights(const double* tau, int K1, int samples, double* wt) {
    const int S1 = clearance_points(K1, samples);
    for (int i = 0; i < S1; ++i) lagrange_row(tau, K1, sample_abscissa(tau, samples, i), wt + (long)i * K1);
}

// ---------------------------------------------------------------- argument checks
// Each returns 0 (ATO_OK) or the error code and sets *msg; a *_check calls them in the order it reports.
inline int check_batch(int batch, const char** msg) {
    if (batch < 1) { *msg = "batch must be >= 1"; return ATO_ERR_ARG; }
    return ATO_OK;
}
inline int check_layout(int layout, const char** msg) {
    if (layout != ATO_LAYOUT_INTERLEAVED && layout != ATO_LAYOUT_INSTANCE_MAJOR) {
        *msg = "unknown layout";
        return ATO_ERR_ARG;
    }
    return ATO_OK;
}
inline int check_samples(int samples, const char** msg) {
    if (samples < 0 || samples > SAMPLE_SMAX) { *msg = "samples must be in [0, 64]"; return ATO_ERR_ARG; }
    return ATO_OK;
}
// collocation only; `unsupported` is the caller's own sentence
inline int check_collocation(const ProbD& p, const char* unsupported, const char** msg) {
    if (p.trans != ATO_TRANS_COLLOCATION) { *msg = unsupported; return ATO_ERR_UNSUPPORTED; }
    return ATO_OK;
}
// parametric problems need the centreline table; `missing` is the caller's own sentence
inline int check_line(const ProbD& p, bool has_line, const char* missing, const char** msg) {
    if (p.frame != GLOBAL && !has_line) { *msg = missing; return ATO_ERR_STATE; }
    return ATO_OK;
}

// ---------------------------------------------------------------- the centreline
// The centreline as the kernels read it: knots kx [nx], coefficients cx [nx + 1][4][3] (piece, power, axis) of x_c;
// kr [nr], cr [nr + 1][4][3] of r_y. Piece 0 is left of the first knot, piece nk right of the last. These are the
// two piecewise cubics of SplineCenterline (_xc and _ry, linear extrapolation pieces included).
struct LineD {
    int32_t nx, nr;
    const double *kx, *cx, *kr, *cr;
};

// an ato_line_table in one buffer: knots and coefficients back to back, in the order of LineD's pointers
inline std::vector<double> line_pack(const ato_line_table& t) {
    const size_t nx = (size_t)t.n_xc, nr = (size_t)t.n_ry;
    std::vector<double> buf;
    buf.insert(buf.end(), t.xc_knots, t.xc_knots + nx);
    buf.insert(buf.end(), t.xc_coef, t.xc_coef + (nx + 1) * 12);
    buf.insert(buf.end(), t.ry_knots, t.ry_knots + nr);
    buf.insert(buf.end(), t.ry_coef, t.ry_coef + (nr + 1) * 12);
    return buf;
}

// the view of a line_pack() buffer (or of its device copy) at d
inline LineD line_view(const ato_line_table& t, const double* d) {
    const size_t nx = (size_t)t.n_xc, nr = (size_t)t.n_ry;
    return LineD{t.n_xc, t.n_ry, d, d + nx, d + nx + (nx + 1) * 12, d + nx + (nx + 1) * 12 + nr};
}

// number of knots <= s (numpy.searchsorted(knots, s, side='right')): in [0, nk] for any s, NaN (piece 0) and
// +-inf included, so no input value can move a read outside the tables
ATO_HD int line_piece(const double* __restrict__ k, int nk, double s) {
    int lo = 0, hi = nk;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (k[mid] <= s) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// value, first and second derivative (d, dd may be NULL) of a piecewise cubic at s: Horner in fused multiply-adds.
// The extrapolation pieces carry no quadratic or cubic coefficient, so their second derivative is zero.
ATO_HD void line_cubic(const double* __restrict__ k, const double* __restrict__ c, int nk, double s, double* v,
                       double* d, double* dd) {
    const int pc = line_piece(k, nk, s);
    const double x = s - k[pc > 0 ? pc - 1 : 0];
    const double* q = c + (long)pc * 12;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c0 = q[a], c1 = q[3 + a], c2 = q[6 + a], c3 = q[9 + a];
        v[a] = fma(fma(fma(c3, x, c2), x, c1), x, c0);
        if (d) d[a] = fma(fma(3.0 * c3, x, 2.0 * c2), x, c1);
        if (dd) dd[a] = fma(6.0 * c3, x, 2.0 * c2);
    }
}

ATO_HD double dot3(const double* a, const double* b) { return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0])); }

ATO_HD void cross3(const double* a, const double* b, double* o) {
    o[0] = fma(a[1], b[2], -(a[2] * b[1]));
    o[1] = fma(a[2], b[0], -(a[0] * b[2]));
    o[2] = fma(a[0], b[1], -(a[1] * b[0]));
}

// frame_from_terms (centerlines/base_centerline.py) at s: e_s = x_c' / |x_c'|, e_y = normalise(r_y - e_s (e_s . r_y)),
// e_n = e_s x e_y
struct LineFrame {
    double xc[3], xs[3], ry[3];     // x_c, x_c', r_y
    double es[3], ey[3], en[3];
    double mag;                     // |x_c'|
};

// xss, rys (may be NULL): x_c'' and r_y', the curvature terms of the audit
ATO_HD void line_frame(const LineD& L, double s, LineFrame& F, double* xss, double* rys) {
    line_cubic(L.kx, L.cx, L.nx, s, F.xc, F.xs, xss);
    line_cubic(L.kr, L.cr, L.nr, s, F.ry, rys, nullptr);
    F.mag = sqrt(dot3(F.xs, F.xs));
#pragma unroll
    for (int a = 0; a < 3; ++a) F.es[a] = F.xs[a] / F.mag;
    const double pr = dot3(F.es, F.ry);
#pragma unroll
    for (int a = 0; a < 3; ++a) F.ey[a] = fma(-F.es[a], pr, F.ry[a]);
    const double my = sqrt(dot3(F.ey, F.ey));
#pragma unroll
    for (int a = 0; a < 3; ++a) F.ey[a] = F.ey[a] / my;
    cross3(F.es, F.ey, F.en);
}

// the node geometry the global models are given: they read none of it
ATO_HD NodeGeom<double> flat_geom() {
    NodeGeom<double> G;
#pragma unroll
    for (int i = 0; i < 9; ++i) G.Rp[i] = 0.0;
    G.ks = G.ky = G.kn = 0.0;
    G.mag = 1.0;
    return G;
}

// ---------------------------------------------------------------- the (interval, sample) x instance grid
// One work item = (interval n of N, sample i of S1, instance b of B). Decision vectors and outputs are interleaved
// ([element][instance]) or instance-major; an output has NCH channels per item:
//   interleaved:     out[c N S1 B + (n S1 + i) B + b]
//   instance-major:  out[((b N + n) S1 + i) NCH + c]
struct SampleGrid {
    int N, S1, B;
    bool il;
    // element 0 of instance b's decision vector (length nw) and its element stride
    ATO_HD const double* input(const double* w, int b, int nw) const { return w + (il ? (long)b : (long)b * nw); }
    ATO_HD long stride() const { return il ? (long)B : 1L; }
    // the NCH channels of item (n, i, b) of a buffer a store<NCH> filled
    template <int NCH>
    ATO_HD void load(const double* in, int n, int i, int b, double* v) const {
        if (il) {
            const long plane = (long)N * S1 * B, p = (long)(n * S1 + i) * B + b;
#pragma unroll
            for (int c = 0; c < NCH; ++c) v[c] = in[c * plane + p];
        } else {
            const long p = ((long)b * N + n) * S1 + i;
#pragma unroll
            for (int c = 0; c < NCH; ++c) v[c] = in[p * NCH + c];
        }
    }
    template <int NCH>
    ATO_HD void store(double* out, int n, int i, int b, const double* v) const {
        if (il) {
            const long plane = (long)N * S1 * B, p = (long)(n * S1 + i) * B + b;
#pragma unroll
            for (int c = 0; c < NCH; ++c) out[c * plane + p] = v[c];
        } else {
            const long p = ((long)b * N + n) * S1 + i;
#pragma unroll
            for (int c = 0; c < NCH; ++c) out[p * NCH + c] = v[c];
        }
    }
};

#ifdef __HIPCC__
// the launch grid of a kernel over a SampleGrid: blockIdx.x is the (interval, sample) pair, blockIdx.y the block
// of `block` instances
inline hipError_t sample_grid_dims(int N, int S1, int B, int block, dim3* grid) {
    const long gx = (long)N * S1, gy = ((long)B + block - 1) / block;
    if (gx > 0x7fffffffL || gy > 65535) return hipErrorInvalidValue;
    *grid = dim3((unsigned)gx, (unsigned)gy);
    return hipSuccess;
}
#endif  // __HIPCC__

}  // namespace ato
