// ato_audit.hpp -- what the NLP constrains at a node, evaluated anywhere on an interval.
//
// One work item = (instance b, interval n, sample i). The whole node vector v = (z, u, du) of the interval's
// collocation polynomial is interpolated at abscissa x_i,
//   v = sum_j l_j(x_i) V[n, j, .],        zp = sum_j l_j'(x_i) Z[n, j, .] / h_n,
// x_i = i / S for samples = S >= 1 (S + 1 points, both ends) or the nodes tau_0 .. tau_K for samples = 0 (the
// clearance's abscissae: clearance_points, ato_sample.hpp). At the nodes l_j(tau_k) is exactly delta_jk and the
// derivative weights are the problem's own C table (dw[k][j] = C[j][k]), so the node audit evaluates the NLP's
// own polynomial derivative. In parametric problems the node geometry (R_p, k_s, k_y, k_n, |x_c'|) is
// frame_from_terms of the centreline's two piecewise cubics (ato_clearance_set_line) AT THE SAMPLE'S OWN
// interpolated s; the NLP freezes it at the node's nominal s, so at an interior node whose s has moved the
// defects below show what that freezing costs.
//
// Output: ATO_AUDIT_NCH = 14 doubles per item. Margins (0-8) are ">= 0 means satisfied" and +inf where the
// quantity does not exist; defects and deviations (9-13) are >= 0, and 0 where the group does not exist.
//    0 pos    min over components [0, 3) of min(v_c - lb_c, ub_c - v_c)    (parametric: s and the corridor y, n)
//    1 att    the same over the attitude [IR, IR + NR)
//    2 vel    over [IV, IV + 3)
//    3 rate   over [IW, IW + 3)                                              (drone)
//    4 u      over the inputs
//    5 du     over the input rates
//    6 sdot   zp[0]                          (parametric: the expression of seg_sdot, whose row is >= 0)
//    7 reg    gamma - (k_n y - k_y n) at the sample's own curvatures (parametric): with force_reg (the default of the
//             Python configuration) at EVERY sample, without it where k_y^2 + k_n^2 > 0.1 at the sample, else +inf.
//             The NLP carries the row only with force_reg and only at nodes whose NOMINAL curvature passes that
//             test, so under the default a failed channel 7 may be a constraint the solve never had.
//    8 stage  1 - u.u / T_max^2              (point mass, seg_stage)
//    9 d_pos  max over rows [0, 3) of |f_i(z, u; G) - zp_i|, f = M::rows of the problem's own model variant
//   10 d_att  the same over the attitude rows
//   11 d_vel  over the velocity rows
//   12 d_rate over the body-rate rows                                        (drone)
//   13 att_dev  quaternion: |q.q - 1|; DCM: Frobenius norm of R^T R - I; Euler angles and point mass: 0
// lb / ub are per component of the node vector: [NV] shared, or per instance in the call's layout (interleaved
// [NV][B], instance-major [B][NV]); NULL gives +inf in channels 0-5, an infinite bound contributes +inf.
//
// NOT covered: the obstacle-tube sphere rows (a per-node table with no definition between nodes; the clearance
// answers that on the mesh itself), gates (ato_gatecheck.hpp) and closure rows (point constraints), CPC progress variables (not
// read), the dU rows (a degree-K interpolant that matches another's derivative at K + 1 points is that
// derivative everywhere) and RK4 transcriptions. The audit bounds nothing about the arc between two samples.
//
// Shared by the HIP kernel (k_audit, ato_audit.hip) and the CPU twin (tests/native/audit_hostcheck.cpp):
// audit_point() is ATO_HD. Interpolation sums, Horner steps, dot and cross products are explicit fused
// multiply-adds in a fixed order. Every table read is indexed by n, i, j or by line_piece()'s result,
// which lies in [0, n_knots] for any s (NaN and +-inf included): no input value can move a read outside its
// table. Nothing renormalises or clips; outputs may be NaN or inf.
#pragma once
#include "ato_sample.hpp"

namespace ato {

constexpr int AUDIT_NCH = ATO_AUDIT_NCH;
constexpr int AUDIT_NMARGIN = 9;

// audit arguments (kernel argument): only what the kernel reads
struct AuditD {
    int32_t N, K1, NV, S1, nw, force_reg, bounds_per_instance;
    double gamma;
    Vehicle veh;
    const double* wt;      // [S1][K1] l_j(x_i)   (clearance_weights)
    const double* dw;      // [S1][K1] l_j'(x_i)  (audit_dweights)
    const double *lb, *ub; // NULL: no bounds
    LineD line;
};

// [S1][K1] l_j'(x_i) (lagrange_drow); with samples = 0 the problem's own table, dw[k][j] = C[j][k]. Host side, fp64.
inline void audit_dweights(const double* tau, const double* C, int K1, int samples, double* dw) {
    const int S1 = clearance_points(K1, samples);
    for (int i = 0; i < S1; ++i) {
        if (samples == 0) {
            for (int j = 0; j < K1; ++j) dw[i * K1 + j] = C[j * K1 + i];
        } else {
            lagrange_drow(tau, K1, sample_abscissa(tau, samples, i), dw + (long)i * K1);
        }
    }
}

// 0 (ATO_OK) or the error code of an ato_audit call with these arguments; *msg gets the reason
inline int audit_check(const ProbD& p, bool has_line, int batch, int layout, int samples, bool has_lb, bool has_ub,
                       const char** msg) {
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (int rc = check_layout(layout, msg)) return rc;
    if (int rc = check_samples(samples, msg)) return rc;
    if (has_lb != has_ub) { *msg = "lb and ub must both be given or both be NULL"; return ATO_ERR_ARG; }
    if (int rc = check_collocation(p, "audit of RK4-transcribed problems (K = 0) is not supported", msg)) return rc;
    return check_line(p, has_line, "parametric audit needs the centreline table (ato_clearance_set_line)", msg);
}

inline AuditD audit_args(const ProbD& p, int samples, const double* wt, const double* dw, const LineD& line,
                         const double* lb, const double* ub, int bounds_per_instance) {
    return AuditD{p.N, p.K1, p.NV, clearance_points(p.K1, samples), p.nw, p.force_reg, bounds_per_instance ? 1 : 0,
                  p.gamma, p.veh, wt, dw, lb, ub, line};
}

// frame_from_terms (centerlines/base_centerline.py) at s: Rp = [e_s e_y e_n] row-major, k_s, k_y, k_n, |x_c'|:
// the frame of the sampling layer and the curvatures from x_c'' and r_y'
ATO_HD void audit_geom(const LineD& L, double s, NodeGeom<double>& G) {
    LineFrame F;
    double xss[3], rys[3], cr[3];
    line_frame(L, s, F, xss, rys);
    const double mag = F.mag;
    const double a_ = dot3(F.xs, F.es), b_ = dot3(F.xs, F.ey);
    const double c_ = dot3(F.ry, F.es), d_ = dot3(F.ry, F.ey);
    const double r0 = dot3(xss, F.en), r1 = dot3(rys, F.en);
    const double det = fma(a_, d_, -(b_ * c_));
    const double kyks0 = fma(d_, r0, -(b_ * r1)) / det / mag;
    const double kyks1 = fma(a_, r1, -(c_ * r0)) / det / mag;
    cross3(xss, F.xs, cr);
    G.kn = -dot3(cr, F.en) / (mag * mag * mag);
    G.ks = kyks1;
    G.ky = -kyks0;
    G.mag = mag;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        G.Rp[a * 3 + 0] = F.es[a];
        G.Rp[a * 3 + 1] = F.ey[a];
        G.Rp[a * 3 + 2] = F.en[a];
    }
}

// the smaller of m and x; NaN if either is (fmin would drop it: a NaN margin must fail)
ATO_HD double audit_min(double m, double x) { return (x < m || x != x) ? x : m; }
// the larger of m and |x|; NaN likewise
ATO_HD double audit_amax(double m, double x) {
    const double a = fabs(x);
    return (a > m || a != a) ? a : m;
}

// One (instance b of B, interval n, sample i). w points at the instance's element 0 of the decision vector,
// element stride ws; out[c] receives channel c.
template <class M>
ATO_HD void audit_point(const AuditD& a, int n, int i, int b, int B, bool il, const double* __restrict__ w, long ws,
                        double* out) {
    constexpr int NZ = M::NZ, NU = M::NU, NV = NZ + 2 * NU;
    const double inf = ATO_INF;
    const int K1 = a.K1;
    const double* l = a.wt + (long)i * K1;
    const double* dl = a.dw + (long)i * K1;
    const double* zn = w + ((long)a.N + (long)n * K1 * NV) * ws;
    double v[NV], zp[NZ];
    {
        const double l0 = l[0], d0 = dl[0];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const double x = zn[(long)c * ws];
            v[c] = l0 * x;
            if (c < NZ) zp[c] = d0 * x;
        }
    }
    for (int j = 1; j < K1; ++j) {
        const double lj = l[j], dj = dl[j];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const double x = zn[((long)j * NV + c) * ws];
            v[c] = fma(lj, x, v[c]);
            if (c < NZ) zp[c] = fma(dj, x, zp[c]);
        }
    }
    const double h = w[(long)n * ws];
#pragma unroll
    for (int c = 0; c < NZ; ++c) zp[c] = zp[c] / h;

    // ---- variable bounds, channels 0-5
    {
        double m[6] = {inf, inf, inf, inf, inf, inf};
        if (a.lb) {
            const long bs = a.bounds_per_instance ? (il ? (long)B : 1L) : 1L;
            const long b0 = a.bounds_per_instance ? (il ? (long)b : (long)b * NV) : 0L;
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const int g = c < 3 ? 0 : c < M::IV ? 1 : c < M::IV + 3 ? 2 : c < NZ ? 3 : c < NZ + NU ? 4 : 5;
                const double lo = v[c] - a.lb[b0 + c * bs], hi = a.ub[b0 + c * bs] - v[c];
                m[g] = audit_min(audit_min(m[g], lo), hi);
            }
        }
#pragma unroll
        for (int g = 0; g < 6; ++g) out[g] = m[g];
    }

    // ---- geometry at the sample's own s; s-dot, regularity, stage
    NodeGeom<double> G;
    if constexpr (M::PARAM) {
        audit_geom(a.line, v[0], G);
        out[6] = zp[0];
        const bool reg = fma(G.ky, G.ky, G.kn * G.kn) > 0.1 || a.force_reg;
        out[7] = reg ? a.gamma - fma(G.kn, v[1], -(G.ky * v[2])) : inf;
    } else {
        G = flat_geom();
        out[6] = inf;
        out[7] = inf;
    }
    if constexpr (!M::IS_DRONE) {
        double uu = v[NZ] * v[NZ];
#pragma unroll
        for (int c = 1; c < NU; ++c) uu = fma(v[NZ + c], v[NZ + c], uu);
        out[8] = 1.0 - uu / a.veh.Tmax / a.veh.Tmax;
    } else {
        out[8] = inf;
    }

    // ---- ODE defects |f_i - zp_i| by row group (a value-only emitter: the Jacobian arguments are dropped)
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    auto emit = [&](int r, double fi, const double*, const double*) {
        const int g = r < 3 ? 0 : r < M::IV ? 1 : r < M::IV + 3 ? 2 : 3;
        d[g] = audit_amax(d[g], fi - zp[r]);
    };
    if constexpr (ode_split<M>() < NZ) {
        // the evaluator's two row groups (ode_split): the position and attitude rows do not stay live over
        // the force rows
        M::template rows<0, ode_split<M>()>(v, v + NZ, G, a.veh, emit);
        M::template rows<ode_split<M>(), NZ>(v, v + NZ, G, a.veh, emit);
    } else {
        M::template rows<0, NZ>(v, v + NZ, G, a.veh, emit);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) out[9 + g] = d[g];

    // ---- attitude deviation
    if constexpr (M::HAS_QUAT) {
        const double* q = v + M::IR;
        out[13] = fabs(fma(q[3], q[3], fma(q[2], q[2], fma(q[1], q[1], q[0] * q[0]))) - 1.0);
    } else if constexpr (M::HAS_DCM) {
        const double* R = v + M::IR;
        double f2 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double e = fma(R[6 + r], R[6 + c], fma(R[3 + r], R[3 + c], R[r] * R[c])) - (r == c ? 1.0 : 0.0);
                f2 = fma(e, e, f2);
            }
        out[13] = sqrt(f2);
    } else {
        out[13] = 0.0;
    }
}

#ifdef __HIPCC__
// explicitly instantiated per model variant in ato_audit.hip
template <class M>
hipError_t launch_audit(const AuditD& a, int B, int layout, const double* w, double* val, hipStream_t st);
#endif  // __HIPCC__

}  // namespace ato
