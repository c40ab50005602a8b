// ato_remesh.hpp -- transfer of collocation decision vectors between two discretisations.
//
// Source: N intervals of degree K; destination: N' = r N intervals of degree K' (r >= 1 an integer,
// K' >= 1 any degree) of the same model variant. Per instance
//   h'[n r + j]     = h[n] / r
//   v'[n r + j, k'] = sum_m l_m((j + tau'_k') / r) v[n, m]        for every per-node variable v
// (the NZ states, the NU inputs and the NU input rates: everything Cols<M> addresses per node), with
// l_m the Lagrange basis over the source nodes tau_0 = 0, tau_1 .. tau_K (ato_sample.hpp): the interpolant of
// interpolate_collocation and of the replay's input. Nothing is renormalised or clipped.
//
// One work item = (instance, source interval n, per-node variable v), v == NV being the interval's h:
// it holds the K + 1 source values and writes the r (K' + 1) results. Nothing depends on the model but
// the per-node width NV, a runtime value. Shared by the HIP kernel (k_remesh, ato_remesh.hip) and the CPU twin
// (tests/native/remesh_hostcheck.cpp): remesh_item() is ATO_HD. The sum runs in ascending m as
// explicit fused multiply-adds, so the twin and the device round alike whatever the compilers would
// contract; l_m(tau_k) is exactly delta_mk, so the identity transfer (r = 1, K' = K) is bitwise for
// finite inputs.
#pragma once
#include "ato_sample.hpp"

namespace ato {

// remesh arguments next to the two ProbD (kernel argument): only what the kernel reads
struct RemeshD {
    int32_t N, K1s, K1d, NV, r;     // source intervals, nodes per interval (source, destination), node width, factor
    int32_t nws, nwd;               // decision-vector lengths
    const double* wt;               // [r][K1d][K1s] weights l_m((j + tau'_k') / r)
};

// l_m((j + tau'_k') / r) over the source nodes (lagrange_row): the one table the kernel, the twin and the test
// oracle use
inline void remesh_weights(const double* tau_s, int K1s, const double* tau_d, int K1d, int r, double* wt) {
    for (int j = 0; j < r; ++j)
        for (int k = 0; k < K1d; ++k)
            lagrange_row(tau_s, K1s, ((double)j + tau_d[k]) / (double)r, wt + ((long)j * K1d + k) * K1s);
}

// 0 (ATO_OK) or the error code of an ato_remesh call with these arguments; *msg gets the reason
inline int remesh_check(const ProbD& s, const ProbD& d, int batch_src, int batch_dst, bool has_cols, int layout,
                        const char** msg) {
    const char* const rk4 = "transfer of RK4-transcribed problems (K = 0) is not supported";
    *msg = "";
    if (int rc = check_batch(batch_src < batch_dst ? batch_src : batch_dst, msg)) return rc;
    if (!has_cols && batch_src != batch_dst) {
        *msg = "without a column map the two batches must be equal";
        return ATO_ERR_ARG;
    }
    if (int rc = check_layout(layout, msg)) return rc;
    if (s.model != d.model || s.att != d.att || s.frame != d.frame || s.NV != d.NV) {
        *msg = "source and destination must have the same model variant (model, attitude, frame)";
        return ATO_ERR_ARG;
    }
    if (int rc = check_collocation(s, rk4, msg)) return rc;
    if (int rc = check_collocation(d, rk4, msg)) return rc;
    if (s.cpc_m > 0 || d.cpc_m > 0) {
        *msg = "transfer of CPC progress variables is not supported";
        return ATO_ERR_UNSUPPORTED;
    }
    if (d.N < s.N || d.N % s.N != 0) {
        *msg = "the destination's N must be a multiple of the source's";
        return ATO_ERR_ARG;
    }
    return ATO_OK;
}

inline RemeshD remesh_args(const ProbD& s, const ProbD& d, const double* wt) {
    return RemeshD{s.N, s.K1, d.K1, s.NV, d.N / s.N, s.nw, d.nw, wt};
}

// One (instance, source interval n, variable v). ws / wd point at the instance's element 0 of the source
// and destination decision vectors, element strides ss / sd.
ATO_HD void remesh_item(const RemeshD& a, int n, int v, const double* __restrict__ ws, long ss,
                        double* __restrict__ wd, long sd) {
    const int r = a.r;
    if (v == a.NV) {
        const double h = ws[(long)n * ss] / (double)r;
        for (int j = 0; j < r; ++j) wd[((long)n * r + j) * sd] = h;
        return;
    }
    const int K1s = a.K1s, K1d = a.K1d;
    double x[ATO_KMAX + 1];
#pragma unroll
    for (int m = 0; m <= ATO_KMAX; ++m)
        x[m] = m < K1s ? ws[((long)a.N + ((long)n * K1s + m) * a.NV + v) * ss] : 0.0;
    const double* l = a.wt;
    const long Nd = (long)a.N * r;
    for (int j = 0; j < r; ++j)
        for (int k = 0; k < K1d; ++k, l += K1s) {
            double acc = l[0] * x[0];
#pragma unroll
            for (int m = 1; m <= ATO_KMAX; ++m)
                if (m < K1s) acc = fma(l[m], x[m], acc);
            wd[(Nd + (((long)n * r + j) * K1d + k) * a.NV + v) * sd] = acc;
        }
}

#ifdef __HIPCC__
// the kernel and its launcher: ato_remesh.hip
hipError_t launch_remesh(const RemeshD& a, int Bs, int Bd, int layout, const double* w_src, const int32_t* cols,
                         double* w_dst, hipStream_t st);
#endif  // __HIPCC__

}  // namespace ato
