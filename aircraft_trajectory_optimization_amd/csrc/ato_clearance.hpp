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
// ato_audit.hpp.) The weight table, the centreline's two piecewise cubics and the frame e_s, e_y, e_n are those
// of the sampling layer (ato_sample.hpp). CPC variables sit after the node block and are not read.
//
// Shared by the HIP kernel (k_clearance_pos, ato_clearance.hip) and the CPU twin
// (tests/native/clearance_hostcheck.cpp): clearance_point() is ATO_HD. The sums are explicit fused multiply-adds
// in a fixed order, as everything in the sampling layer, so the twin and the device round alike whatever the
// compilers would contract; l_j(tau_k) is exactly delta_jk, so sample 0 is node 0 bit for bit.
#pragma once
#include "ato_sample.hpp"

namespace ato {

// clearance arguments (kernel argument): only what the kernel reads
struct ClearD {
    int32_t N, K1, NV, S1, param;
    int32_t nw;
    const double* wt;      // [S1][K1] Lagrange weights l_j(x_i) (clearance_weights)
    LineD line;
};

// 0 (ATO_OK) or the error code of an ato_clearance call with these arguments; *msg gets the reason
inline int clearance_check(const ProbD& p, bool has_line, int batch, int layout, int samples, const char** msg) {
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (int rc = check_layout(layout, msg)) return rc;
    if (int rc = check_samples(samples, msg)) return rc;
    if (int rc = check_collocation(p, "clearance of RK4-transcribed problems (K = 0) is not supported", msg)) return rc;
    return check_line(p, has_line, "parametric clearance needs the centreline table (ato_clearance_set_line)", msg);
}

inline ClearD clearance_args(const ProbD& p, int samples, const double* wt, const LineD& line) {
    return ClearD{p.N, p.K1, p.NV, clearance_points(p.K1, samples), p.frame != GLOBAL ? 1 : 0, p.nw, wt, line};
}

// (s, y, n) -> x_c(s) + y e_y(s) + n e_n(s)
ATO_HD void clearance_lift(const LineD& L, double* q) {
    const double y = q[1], n = q[2];
    LineFrame F;
    line_frame(L, q[0], F, nullptr, nullptr);
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = fma(n, F.en[a], fma(y, F.ey[a], F.xc[a]));
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
