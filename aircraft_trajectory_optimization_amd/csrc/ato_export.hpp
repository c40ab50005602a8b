// ato_export.hpp -- solved racelines as global-frame state tables on a time grid.
//
// A solve returns step sizes h_0 .. h_{N-1} and collocation nodes X[n, k] = (z, u, du) in the problem's own frame
// and attitude parameterisation. For a list of times shared by all instances the export evaluates, per (time j,
// instance b), the reference's z_interp / u_interp / du_interp (utils/discretization_utils.interpolate_collocation)
// and lifts the result to one table of ATO_EXPORT_NCH channels that does not depend on the model variant.
//
// Conventions (pinned by the tests against the Python interpolant):
//   t_start   t_start[0] = 0, t_start[n + 1] = t_start[n] + h_n: one fp64 addition per interval, ascending, which is
//             numpy.cumsum bit for bit (export_tstart; no tree or pairwise scan). T_b = t_start[N].
//   t         times[j] (seconds), or times[j] * T_b with `relative` (one multiplication).
//   interval  n = (number of t_start[0..N] <= t) - 1, searchsorted(side = 'right') - 1 (export_interval, the loop
//             of line_piece: its result lies in [-1, N] for any t and any column, NaN, +-inf and a non-monotone
//             t_start from a non-positive h included, so no input value moves a read outside the tables).
//   n = -1    (t < 0) the first node X[0, 0] is held, x = 0.
//   n = N     (t >= T_b) the end value sum_k D_k X[N - 1, k] is held, D the problem's own table (the replay's end
//             value, not l_k(1) recomputed), x = 1.
//   else      x = (t - t_start[n]) / h_n and every component is sum_k l_k(x) X[n, k], k ascending, l_k(x) by
//             lagrange_weight (the product formula), one weight at a time.
//   NaN t     NaN in every channel of both outputs.
// nodes: the NV components (z, u, du) as interpolated. state: the channels below; what a problem does not have is
// NaN.
//    0      t used (seconds)            1  interval n (-1, 0 .. N - 1, N)           2  abscissa x
//    3-5    global position: the identity, or x_c(s) + y e_y(s) + n e_n(s) at the sample's own s (line_frame)
//    6-9    body -> global quaternion (qi, qj, qk, qr): r as interpolated, unnormalised, for the ESP pose with a
//           global attitude (the global frame and global_r); in every other drone case ws_quat of the rotation
//           nearest to R (export_polar: an interpolated quaternion or DCM gives an R that is not orthonormal, and
//           zu2state's Rotation.from_matrix orthogonalises such a matrix, U V^T of its SVD, before it converts
//           it); its sign is made continuous along the samples in the order of `times` by the chain below
//    10-12  global velocity R vb, R = R(r) (AttSel), left-multiplied by [e_s e_y e_n](s) for the relative
//           attitude; nothing is renormalised before R is formed. Point mass: its own velocity components.
//    13-15  body velocity, 16-18 body rates (drone)
//    19-22  inputs (drone: 4 rotor thrusts; point mass: 3 thrust components), 23-26 input rates
//    27-29  (s, y, n) of a parametric problem
// The sign chain: q_0 is kept; q_j is negated when its dot product with the already-signed q_{j-1} is negative.
// Whether sample j is negated depends on j - 1 only through "j - 1 was negated", so sample j is a map of that bit
// (two bits: the output for either input) that depends on the raw q_j and q_{j-1} alone, and the pass is the
// composition of the maps: the sample axis is cut into G segments (export_segments), every segment composes its
// own maps (export_segment_map), a segment's entry state is the fold of the maps before it, and a second walk negates in
// place (export_segment_apply). The pattern of k_ws_chain (ato_warmstart.hpp). A NaN dot product negates nothing.
//
// Not covered: RK4 transcriptions, the closed line's wrap of t beyond the lap (values are held, as in the
// reference), per-instance time arrays, fp32, CPC progress variables (not read), the trajectory as flown (the
// replay's traj). The export certifies nothing; replay, audit, clearance and gate check are the judges.
//
// Everything ATO_HD here is shared by the HIP kernels (ato_export.hip) and the CPU twin
// (tests/native/export_hostcheck.cpp). Sums, dot products and the frame are explicit fused multiply-adds in a
// fixed order; R(r) is the models' own (plain products, which host and device compilers may contract differently).
#pragma once
#include "ato_sample.hpp"

namespace ato {

constexpr int EXPORT_NCH = ATO_EXPORT_NCH;
constexpr int EXPORT_GMAX = 16;        // segments of the sign chain at the most = waves of a k_export_qchain workgroup
constexpr int EXPORT_SEG_MIN = 8;      // samples per segment at the least: a shorter walk does not pay for its extra read
constexpr int EXPORT_WAVES = 1024;     // waves the sign pass wants in flight (4 on each of 256 compute units)
constexpr int EXPORT_POLAR_MAX = 32;   // Newton steps of export_polar at the most (5 reach fp64 from 0.2 off)
enum { EX_T = 0, EX_N = 1, EX_X = 2, EX_POS = 3, EX_Q = 6, EX_VG = 10, EX_VB = 13, EX_WB = 16, EX_U = 19, EX_DU = 23,
       EX_SYN = 27 };

// export arguments (kernel argument): only what the kernels read
struct ExportD {
    int32_t N, K1, nw, n_times, relative;
    const double* tau;         // [K1] behind pointers: an indexed array in the kernel argument would be copied
    const double* D;           // [K1]
    const double* times;       // [n_times]
    double* ts;                // [N + 1][B] interval start times (scratch of the handle)
    LineD line;
};

// 0 (ATO_OK) or the error code of an ato_export call with these arguments; *msg gets the reason
inline int export_check(const ProbD& p, bool has_line, int batch, int layout, int n_times, bool has_w, bool has_times,
                        bool has_nodes, bool has_state, const char** msg) {
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (int rc = check_layout(layout, msg)) return rc;
    if (n_times < 1) { *msg = "n_times must be >= 1"; return ATO_ERR_ARG; }
    if (!has_w || !has_times) { *msg = "null buffer"; return ATO_ERR_ARG; }
    if (!has_nodes && !has_state) { *msg = "nothing to export: nodes and state are both NULL"; return ATO_ERR_ARG; }
    if (int rc = check_collocation(p, "export of RK4-transcribed problems (K = 0) is not supported", msg)) return rc;
    return check_line(p, has_line, "parametric export needs the centreline table (ato_clearance_set_line)", msg);
}

inline ExportD export_args(const ProbD& p, int n_times, int relative, const double* tau, const double* D,
                           const double* times, double* ts, const LineD& line) {
    return ExportD{p.N, p.K1, p.nw, n_times, relative ? 1 : 0, tau, D, times, ts, line};
}

// the frame of a model variant (the relative attitude multiplies R by the centreline's frame)
template <class M>
struct ExportFrame;
template <int ATT, int FRAME>
struct ExportFrame<DroneModel<ATT, FRAME>> { static constexpr int value = FRAME; };
template <int FRAME>
struct ExportFrame<PointModel<FRAME>> { static constexpr int value = FRAME; };

// One instance: t_start[0 .. N] at ts[n B] from the step sizes w[n ws]. N dependent additions, ascending.
ATO_HD void export_tstart(int N, const double* __restrict__ w, long ws, double* __restrict__ ts, long B) {
    double run = 0.0;
    ts[0] = run;
    for (int n = 0; n < N; ++n) {
        run += w[(long)n * ws];
        ts[(long)(n + 1) * B] = run;
    }
}

// (number of ts[0 B], ts[1 B], .. ts[N B] <= t) - 1, in [-1, N] for any t and any column
ATO_HD int export_interval(const double* __restrict__ ts, long B, int N, double t) {
    int lo = 0, hi = N + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ts[(long)mid * B] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// One (time tj, instance): the node vector v [NV] at the time and head = (t, n, x). ts points at the instance's
// t_start[0] (stride B), w at element 0 of its decision vector (stride ws).
template <int NV>
ATO_HD void export_interp(const ExportD& a, double tj, const double* __restrict__ ts, long B,
                          const double* __restrict__ w, long ws, double* v, double* head) {
    const int N = a.N, K1 = a.K1;
    const double t = a.relative ? tj * ts[(long)N * B] : tj;
    const int n = export_interval(ts, B, N, t);
    const bool before = n < 0, after = n >= N;
    const int ni = before ? 0 : (after ? N - 1 : n);
    double x = before ? 0.0 : 1.0;
    if (!before && !after) x = (t - ts[(long)n * B]) / w[(long)n * ws];
    const double* z = w + ((long)N + (long)ni * K1 * NV) * ws;
    const double l0 = before ? 1.0 : (after ? a.D[0] : lagrange_weight(a.tau, K1, x, 0));
#pragma unroll
    for (int c = 0; c < NV; ++c) v[c] = l0 * z[(long)c * ws];
    const int kn = before ? 1 : K1;        // the held first node is X[0, 0] itself
    for (int k = 1; k < kn; ++k) {
        const double lk = after ? a.D[k] : lagrange_weight(a.tau, K1, x, k);
#pragma unroll
        for (int c = 0; c < NV; ++c) v[c] = fma(lk, z[((long)k * NV + c) * ws], v[c]);
    }
    head[EX_T] = t;
    head[EX_N] = (double)n;
    head[EX_X] = x;
    if (t != t) {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int c = 0; c < NV; ++c) v[c] = nan;
        head[EX_N] = head[EX_X] = nan;
    }
}

// The rotation nearest to R (row-major, det > 0) in place: the orthogonal polar factor, U V^T of the SVD, by Newton's
// iteration Q <- (Q + Q^-T) / 2 with Q^-T = cof(Q) / det(Q), the rows of cof(Q) being the cross products of Q's
// rows. Quadratic: it stops once no entry moves by more than 1e-15 (an orthonormal R after one step). A matrix
// with no nearest rotation (det <= 0, NaN or inf entries; SciPy raises there) becomes NaN, and so does its quaternion.
ATO_HD void export_polar(double* R) {
    for (int it = 0; it < EXPORT_POLAR_MAX; ++it) {
        double cof[9];
        cross3(R + 3, R + 6, cof);
        cross3(R + 6, R, cof + 3);
        cross3(R, R + 3, cof + 6);
        const double det = dot3(R, cof);
        if (!(det > 0.0) || det - det != 0.0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = __builtin_nan("");
            return;
        }
        double delta = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double q = 0.5 * (R[i] + cof[i] / det), d = fabs(q - R[i]);
            delta = (d > delta || d != d) ? d : delta;
            R[i] = q;
        }
        if (!(delta > 1e-15)) break;
    }
}

// The channels EX_POS .. of out [EXPORT_NCH] from the node vector v of model variant M; the quaternion is unsigned.
template <class M>
ATO_HD void export_lift(const LineD& L, const double* v, double* out) {
    constexpr int NZ = M::NZ, NU = M::NU, FRAME = ExportFrame<M>::value;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int c = EX_POS; c < EXPORT_NCH; ++c) out[c] = nan;
    double Rp[9];                          // [e_s e_y e_n] row-major (the relative attitude's left factor)
    if constexpr (M::PARAM) {
        LineFrame F;
        line_frame(L, v[0], F, nullptr, nullptr);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            out[EX_POS + i] = fma(v[2], F.en[i], fma(v[1], F.ey[i], F.xc[i]));
            out[EX_SYN + i] = v[i];
            Rp[i * 3] = F.es[i];
            Rp[i * 3 + 1] = F.ey[i];
            Rp[i * 3 + 2] = F.en[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) out[EX_POS + i] = v[i];
    }
    if constexpr (M::IS_DRONE) {
        double R[9];
        M::A::R(v + M::IR, R);
        if constexpr (FRAME == PARAM_REL) {
            double Q[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    Q[i * 3 + j] = fma(Rp[i * 3 + 2], R[6 + j], fma(Rp[i * 3 + 1], R[3 + j], Rp[i * 3] * R[j]));
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = Q[i];
        }
        if constexpr (M::HAS_QUAT && FRAME != PARAM_REL) {
#pragma unroll
            for (int i = 0; i < 4; ++i) out[EX_Q + i] = v[M::IR + i];
        } else {
            double Q[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) Q[i] = R[i];
            export_polar(Q);
            ws_quat(Q, out + EX_Q);
        }
        const double* vb = v + M::IV;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            out[EX_VG + i] = fma(R[i * 3 + 2], vb[2], fma(R[i * 3 + 1], vb[1], R[i * 3] * vb[0]));
            out[EX_VB + i] = vb[i];
            out[EX_WB + i] = v[M::IW + i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) out[EX_VG + i] = v[3 + i];
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        out[EX_U + i] = v[NZ + i];
        out[EX_DU + i] = v[NZ + NU + i];
    }
}

// ---------------------------------------------------------------- the sign chain
// channel c of item (j, b) of a state table
ATO_HD long export_at(bool il, int n_times, long B, int j, long b, int c) {
    return il ? ((long)c * n_times + j) * B + b : ((long)b * n_times + j) * EXPORT_NCH + c;
}

// A map of the chain's state (1: the sample before was negated): bit s holds the state after for the state s before.
constexpr unsigned EX_MAP_ID = 2u;
ATO_HD unsigned export_map_at(unsigned m, unsigned s) { return (m >> s) & 1u; }
// first `a`, then `b`
ATO_HD unsigned export_map_then(unsigned a, unsigned b) {
    return export_map_at(b, export_map_at(a, 0)) | export_map_at(b, export_map_at(a, 1)) << 1;
}
// the map of one sample from its raw quaternion r and the raw quaternion l of the sample before: -l . r = -(l . r)
ATO_HD unsigned export_sample_map(const double* r, const double* l) {
    const double d = fma(r[3], l[3], fma(r[2], l[2], fma(r[1], l[1], r[0] * l[0])));
    return (unsigned)(d < 0.0) | (unsigned)(-d < 0.0) << 1;
}

ATO_HD void export_load_q(const double* state, bool il, int n_times, long B, int j, long b, double* q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = state[export_at(il, n_times, B, j, b, EX_Q + i)];
}

// The number G of segments the sample axis of a call is cut into, 1 .. EXPORT_GMAX. The maps compose associatively,
// so the table does not depend on G; G only sets how the two walks are spread: as many segments as fill the device
// with the call's ceil(B / 64) workgroups (few instances, many segments; from 256 workgroups on, four), but none
// shorter than EXPORT_SEG_MIN samples.
inline int export_segments(int n_times, long B) {
    const long blocks = (B + 63) / 64;
    long G = (EXPORT_WAVES + blocks - 1) / blocks;
    G = G < 4 ? 4 : (G > EXPORT_GMAX ? EXPORT_GMAX : G);
    const long fit = ((long)n_times + EXPORT_SEG_MIN - 1) / EXPORT_SEG_MIN;
    return (int)(G < fit ? G : (fit < 1 ? 1 : fit));
}

// samples [p0, p1) of segment g of G (empty when p0 >= p1)
ATO_HD void export_segment(int n_times, int G, int g, int* p0, int* p1) {
    const int len = (n_times + G - 1) / G;
    *p0 = g * len < n_times ? g * len : n_times;
    *p1 = n_times - *p0 < len ? n_times : *p0 + len;
}

// First walk of segment g of instance b: the composition of its samples' maps; prev receives the raw quaternion
// of the sample before the segment (the second walk of the segment before may negate it in place).
ATO_HD unsigned export_segment_map(const double* state, bool il, int n_times, long B, long b, int G, int g,
                                   double* prev) {
    int p0, p1;
    export_segment(n_times, G, g, &p0, &p1);
    unsigned m = EX_MAP_ID;
    if (p0 >= p1) return m;
    double l[4], r[4];
    export_load_q(state, il, n_times, B, p0 > 0 ? p0 - 1 : 0, b, l);
#pragma unroll
    for (int i = 0; i < 4; ++i) prev[i] = l[i];
    for (int p = p0 > 0 ? p0 : 1; p < p1; ++p) {
        export_load_q(state, il, n_times, B, p, b, r);
        m = export_map_then(m, export_sample_map(r, l));
#pragma unroll
        for (int i = 0; i < 4; ++i) l[i] = r[i];
    }
    return m;
}

// Second walk of segment g from its entry state s: the negation in place
ATO_HD void export_segment_apply(double* state, bool il, int n_times, long B, long b, int G, int g, unsigned s,
                                 const double* prev) {
    int p0, p1;
    export_segment(n_times, G, g, &p0, &p1);
    double l[4], r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) l[i] = prev[i];
    for (int p = p0; p < p1; ++p) {
        export_load_q(state, il, n_times, B, p, b, r);
        if (p > 0) s = export_map_at(export_sample_map(r, l), s);
#pragma unroll
        for (int i = 0; i < 4; ++i) l[i] = r[i];
        if (s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) state[export_at(il, n_times, B, p, b, EX_Q + i)] = -r[i];
        }
    }
}

#ifdef __HIPCC__
// the kernels and their launcher, explicitly instantiated per model variant in ato_export.hip
template <class M>
hipError_t launch_export(const ExportD& a, int B, int layout, const double* w, double* nodes, double* state,
                         hipStream_t st);
#endif  // __HIPCC__

}  // namespace ato
