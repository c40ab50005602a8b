// ato_warmstart.hpp -- lift of point-mass racelines into drone warm starts (raceline/warmstart.py: drone_guess,
// the reference's use_ws path, drone_raceline.py:158-274).
//
// A point-mass problem and a drone problem over the same N, K (both collocation). Per instance, every node
// p = n K1 + k of the point-mass decision vector gives the node of the drone decision vector:
//   T = Rw up, vg = Rw zp[3:6], dT = Rw dup      Rw = the point problem's Rp at the node (relative attitude), else I
//   closed line:  R = [e1 e2 e3], e3 = T / |T|, e1 = vg / |vg| made orthogonal to e3 and renormalised, e2 = e3 x e1
//   open line:    R = I + [v]x + [v]x^2 (1 - c) / s^2, t = T / |T|, v = -(t x ez), s = |v|, c = t . ez
//   R <- Rp^T R                                   Rp = the drone problem's, when its attitude is the relative one
//   attitude r:   DCM  R row-major
//                 ESP  (qi, qj, qk, qr) of R, see ws_quat()
//                 YPR  (atan2(R10, R00), -asin(R20), atan2(R21, R22)); |R20| >= 1 - 1e-12 flags the node
//   vb = R^T vg, wb = R^T (T x dT) / |T|^2, every rotor thrust |T| / 4, thrust rates 0
//   h_n as the point-mass h_n, its bounds h_n / 100 and 10 h_n
// in the operation order of drone_guess_batch. A zero or non-finite |T|, |vg|, |e1| (closed) or s (open) flags
// the node; what the arithmetic gives is written all the same, NaN included. Nothing is clipped.
//
// Pass 1 (ws_node, one work item per (node, instance) of the SampleGrid with S1 = K1) writes the raw attitude.
// Pass 2 (quaternion and Euler poses) restores continuity along the lap, the one serial part:
//   ESP  node p is negated when |r_p - r_{p-1}| >= 1, r_{p-1} as already fixed
//   YPR  when |r_p - r_{p-1}| > 1 the yaw moves by -+2 pi towards r_{p-1}; still > 1: continuity failed
// What node p does depends on p - 1 only through a small state: "p - 1 was negated" (2 values), or the yaw
// offset of p - 1, one of 0, +2 pi, -2 pi, or "failed" (4 values; the offset does not accumulate: the raw yaw is
// in [-pi, pi] and a node moves by at most one turn). So node p is a map state -> state that depends on the raw
// values of p and p - 1 alone, the lap is the composition of the maps, and composition is associative: the lap
// is cut into WS_G segments, every segment composes its own maps (ws_segment_map), the entry state of a segment
// is the fold of the maps before it, and a second walk applies the change in place (ws_segment_apply). A map is
// a byte: two bits of output per input state.
//
// Shared by the HIP kernels (ato_warmstart.hip) and the CPU twin (tests/native/warmstart_hostcheck.cpp):
// everything below the argument check is ATO_HD. Dot and cross products are the sampling layer's explicit fused
// multiply-adds, so the twin and the device round alike up to sqrt, atan2 and asin.
#pragma once
#include "ato_sample.hpp"

namespace ato {

constexpr int WS_G = 4;               // segments of the chain = waves of a pass-2 workgroup
constexpr int WS_POINT_NV = 12;       // point-mass node: z (6), u (3), du (3)
constexpr double WS_TWO_PI = 6.283185307179586, WS_PI = 3.141592653589793;
enum { WS_INFO_STATUS = 0, WS_INFO_QUAT_FLIP = 1, WS_INFO_EULER_WRAPS = 2 };

// warm-start arguments (kernel argument): only what the kernels read
struct WarmD {
    int32_t N, K1, P;
    int32_t nvd, nr;            // drone node width, attitude width (4, 3, 9)
    int32_t nwp, nwd;           // decision-vector lengths
    int32_t closed;
    const double* geom_p;       // the point problem's node geometry [P][ATO_GEOM_WIDTH] when Rw = Rp, else NULL
    const double* geom_d;       // the drone problem's when R <- Rp^T R, else NULL
};

// 0 (ATO_OK) or the error code of an ato_warmstart call with these problems; *msg gets the reason
inline int warmstart_check(const ProbD& pt, const ProbD& dr, int batch, int layout, const char** msg) {
    const char* const rk4 = "warm starts of RK4-transcribed problems (K = 0) are not supported";
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (int rc = check_layout(layout, msg)) return rc;
    if (pt.model != ATO_MODEL_POINT) { *msg = "the first problem must be a point mass"; return ATO_ERR_ARG; }
    if (dr.model != ATO_MODEL_DRONE) { *msg = "the second problem must be a drone"; return ATO_ERR_ARG; }
    if (int rc = check_collocation(pt, rk4, msg)) return rc;
    if (int rc = check_collocation(dr, rk4, msg)) return rc;
    if (dr.cpc_m > 0) {
        *msg = "warm starts of CPC progress variables are not supported";
        return ATO_ERR_UNSUPPORTED;
    }
    if (pt.N != dr.N || pt.K != dr.K) { *msg = "warm start needs the same discretisation"; return ATO_ERR_ARG; }
    return ATO_OK;
}

// geom_p / geom_d: the two problems' geometry tables as the caller holds them (host or device)
inline WarmD warmstart_args(const ProbD& pt, const ProbD& dr, const double* geom_p, const double* geom_d) {
    return WarmD{dr.N, dr.K1, dr.P, dr.NV, dr.NZ - 9, pt.nw, dr.nw, dr.closed,
                 pt.frame == PARAM_REL ? geom_p : nullptr, dr.frame == PARAM_REL ? geom_d : nullptr};
}

ATO_HD bool ws_bad(double x) { return !(x > 0.0 && x <= 1.79769313486231570815e308); }

// ws_quat(): rotation matrix -> unit quaternion, in the sampling layer (ato_sample.hpp; the export shares it)

// Pass 1: node p of one instance. wp / wd point at the instance's element 0 of the point-mass and the drone
// decision vector, element strides sp / sd. Returns whether the node is degenerate (status 2).
template <int ATT, bool CLOSED>
ATO_HD bool ws_node(const WarmD& a, int p, const double* __restrict__ wp, long sp, double* __restrict__ wd,
                    long sd) {
    constexpr int NR = ATT == ATO_ATT_ESP ? 4 : (ATT == ATO_ATT_DCM ? 9 : 3);
    const double* zp = wp + ((long)a.N + (long)p * WS_POINT_NV) * sp;
    double pos[3], v[3], up[3], dup[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pos[i] = zp[i * sp];
        v[i] = zp[(3 + i) * sp];
        up[i] = zp[(6 + i) * sp];
        dup[i] = zp[(9 + i) * sp];
    }
    double T[3], vg[3], dT[3];
    if (a.geom_p) {
        const double* Rw = a.geom_p + (long)p * ATO_GEOM_WIDTH;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            T[i] = dot3(up, Rw + 3 * i);
            vg[i] = dot3(v, Rw + 3 * i);
            dT[i] = dot3(dup, Rw + 3 * i);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            T[i] = up[i];
            vg[i] = v[i];
            dT[i] = dup[i];
        }
    }
    const double Tn = sqrt(dot3(T, T));
    bool bad = ws_bad(Tn);
    double R[9];
    if constexpr (CLOSED) {
        const double vn = sqrt(dot3(vg, vg));
        double e1[3], e2[3], e3[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            e1[i] = vg[i] / vn;
            e3[i] = T[i] / Tn;
        }
        const double pr = dot3(e1, e3);
#pragma unroll
        for (int i = 0; i < 3; ++i) e1[i] = fma(-e3[i], pr, e1[i]);
        const double n1 = sqrt(dot3(e1, e1));
#pragma unroll
        for (int i = 0; i < 3; ++i) e1[i] = e1[i] / n1;
        cross3(e3, e1, e2);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            R[i * 3] = e1[i];
            R[i * 3 + 1] = e2[i];
            R[i * 3 + 2] = e3[i];
        }
        bad = bad || ws_bad(vn) || ws_bad(n1);
    } else {
        // v = -(t x ez) = (-t1, t0, 0): [v]x has the entries (0,2) = v1, (1,2) = -v0, (2,0) = -v1, (2,1) = v0
        const double v0 = -(T[1] / Tn), v1 = T[0] / Tn, c = T[2] / Tn;
        const double s = sqrt(fma(v1, v1, v0 * v0));
        const double f = (1.0 - c) / (s * s);
        R[0] = fma(-(v1 * v1), f, 1.0);
        R[1] = (v0 * v1) * f;
        R[2] = v1;
        R[3] = (v0 * v1) * f;
        R[4] = fma(-(v0 * v0), f, 1.0);
        R[5] = -v0;
        R[6] = -v1;
        R[7] = v0;
        R[8] = fma(-fma(v0, v0, v1 * v1), f, 1.0);
        bad = bad || ws_bad(s);
    }
    if (a.geom_d) {
        const double* Rp = a.geom_d + (long)p * ATO_GEOM_WIDTH;
        double Q[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Q[i * 3 + j] = fma(Rp[6 + i], R[6 + j], fma(Rp[3 + i], R[3 + j], Rp[i] * R[j]));
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Q[i];
    }
    double* zd = wd + ((long)a.N + (long)p * a.nvd) * sd;
#pragma unroll
    for (int i = 0; i < 3; ++i) zd[i * sd] = pos[i];
    if constexpr (ATT == ATO_ATT_DCM) {
#pragma unroll
        for (int i = 0; i < 9; ++i) zd[(3 + i) * sd] = R[i];
    } else if constexpr (ATT == ATO_ATT_ESP) {
        double q[4];
        ws_quat(R, q);
#pragma unroll
        for (int i = 0; i < 4; ++i) zd[(3 + i) * sd] = q[i];
    } else {
        zd[3 * sd] = atan2(R[3], R[0]);
        zd[4 * sd] = -asin(R[6]);
        zd[5 * sd] = atan2(R[7], R[8]);
        bad = bad || !(fabs(R[6]) < 1.0 - 1e-12);
    }
    double tw[3];
    cross3(T, dT, tw);
    const double T2 = Tn * Tn, thr = Tn / 4.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        zd[(3 + NR + i) * sd] = fma(R[6 + i], vg[2], fma(R[3 + i], vg[1], R[i] * vg[0]));
        zd[(6 + NR + i) * sd] = fma(R[6 + i], tw[2], fma(R[3 + i], tw[1], R[i] * tw[0])) / T2;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        zd[(9 + NR + i) * sd] = thr;
        zd[(13 + NR + i) * sd] = 0.0;
    }
    return bad;
}

// h_n and its bounds (the k = 0 item of interval n); hlb / hub: the instance's element 0 of [N x B], or NULL
ATO_HD void ws_step(int n, const double* __restrict__ wp, long sp, double* __restrict__ wd, long sd, double* hlb,
                    double* hub) {
    const double h = wp[(long)n * sp];
    wd[(long)n * sd] = h;
    if (hlb) hlb[(long)n * sd] = h / 100.0;
    if (hub) hub[(long)n * sd] = h * 10.0;
}

// ---------------------------------------------------------------- the chain
// A map of the chain's state: bits [2 s, 2 s + 1] hold the state after the node(s) for the state s before.
// ESP: s = 1 when the previous node was negated. YPR: 0 no offset, 1 +2 pi, 2 -2 pi, 3 failed (absorbing).
constexpr unsigned WS_MAP_ID = 0x24;       // 0 -> 0, 1 -> 1, 2 -> 2
ATO_HD unsigned ws_map_at(unsigned m, unsigned s) { return s == 3 ? 3u : (m >> (2 * s)) & 3u; }
// first `a`, then `b`
ATO_HD unsigned ws_map_then(unsigned a, unsigned b) {
    return ws_map_at(b, ws_map_at(a, 0)) | ws_map_at(b, ws_map_at(a, 1)) << 2 | ws_map_at(b, ws_map_at(a, 2)) << 4;
}
ATO_HD double ws_yaw_offset(unsigned s) { return s == 1 ? WS_TWO_PI : (s == 2 ? -WS_TWO_PI : 0.0); }

// the map of one node from its raw attitude r and the raw attitude l of the node before
template <int ATT>
ATO_HD unsigned ws_node_map(const double* r, const double* l) {
    if constexpr (ATT == ATO_ATT_ESP) {
        double d[4], e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            d[i] = r[i] - l[i];
            e[i] = r[i] + l[i];
        }
        const unsigned fa = sqrt(fma(d[3], d[3], fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])))) >= 1.0;
        const unsigned fb = sqrt(fma(e[3], e[3], fma(e[2], e[2], fma(e[1], e[1], e[0] * e[0])))) >= 1.0;
        return fa | fb << 2 | 2u << 4;
    } else {
        unsigned m = 0;
#pragma unroll
        for (unsigned s = 0; s < 3; ++s) {
            double d[3] = {r[0] - (l[0] + ws_yaw_offset(s)), r[1] - l[1], r[2] - l[2]};
            unsigned o = 0;
            if (sqrt(dot3(d, d)) > 1.0) {
                if (d[0] > WS_PI) o = 2;
                else if (d[0] <= -WS_PI) o = 1;
                d[0] = (r[0] + ws_yaw_offset(o)) - (l[0] + ws_yaw_offset(s));
                if (sqrt(dot3(d, d)) > 1.0) o = 3;
            }
            m |= o << (2 * s);
        }
        return m;
    }
}

// the attitude of node p of an instance's drone vector (element 0 at wd, stride sd)
template <int NR>
ATO_HD void ws_load_att(const WarmD& a, int p, const double* wd, long sd, double* r) {
    const double* z = wd + ((long)a.N + (long)p * a.nvd + 3) * sd;
#pragma unroll
    for (int i = 0; i < NR; ++i) r[i] = z[i * sd];
}

// nodes [p0, p1) of segment g (empty when p0 >= p1)
ATO_HD void ws_segment(const WarmD& a, int g, int* p0, int* p1) {
    const int len = (a.P + WS_G - 1) / WS_G;
    *p0 = g * len;
    *p1 = *p0 + len < a.P ? *p0 + len : a.P;
}

// First walk of segment g: the composition of its nodes' maps; prev receives the raw attitude of the node before
// the segment (the second walk needs it after the segment before has changed that node in place).
template <int ATT>
ATO_HD unsigned ws_segment_map(const WarmD& a, int g, const double* wd, long sd, double* prev) {
    constexpr int NR = ATT == ATO_ATT_ESP ? 4 : 3;
    int p0, p1;
    ws_segment(a, g, &p0, &p1);
    unsigned m = WS_MAP_ID;
    if (p0 >= p1) return m;
    double l[NR], r[NR];
    if (p0 > 0) ws_load_att<NR>(a, p0 - 1, wd, sd, l);
    else ws_load_att<NR>(a, 0, wd, sd, l);
#pragma unroll
    for (int i = 0; i < NR; ++i) prev[i] = l[i];
    for (int p = p0 > 0 ? p0 : 1; p < p1; ++p) {
        ws_load_att<NR>(a, p, wd, sd, r);
        m = ws_map_then(m, ws_node_map<ATT>(r, l));
#pragma unroll
        for (int i = 0; i < NR; ++i) l[i] = r[i];
    }
    return m;
}

// Second walk of segment g from its entry state s: the change in place. The segment that holds the last node
// also writes the instance's info (element 0 at info, stride si); status 2 of pass 1 stays.
template <int ATT>
ATO_HD void ws_segment_apply(const WarmD& a, int g, unsigned s, const double* prev, double* wd, long sd,
                             double* info, long si) {
    constexpr int NR = ATT == ATO_ATT_ESP ? 4 : 3;
    int p0, p1;
    ws_segment(a, g, &p0, &p1);
    if (p0 >= p1) return;
    double l[NR], r[NR], last[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) last[i] = l[i] = prev[i];
    for (int p = p0; p < p1; ++p) {
        ws_load_att<NR>(a, p, wd, sd, r);
        if (p > 0) s = ws_map_at(ws_node_map<ATT>(r, l), s);
        double* z = wd + ((long)a.N + (long)p * a.nvd + 3) * sd;
#pragma unroll
        for (int i = 0; i < NR; ++i) last[i] = l[i] = r[i];
        if constexpr (ATT == ATO_ATT_ESP) {
            if (s == 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) z[i * sd] = last[i] = -r[i];
            }
        } else {
            if (s == 1 || s == 2) z[0] = last[0] = r[0] + ws_yaw_offset(s);
        }
    }
    if (p1 != a.P) return;
    double first[NR];
    ws_load_att<NR>(a, 0, wd, sd, first);     // node 0 is never changed
    double flip = 0.0, wraps = 0.0;
    if (a.closed) {
        if constexpr (ATT == ATO_ATT_ESP) {
            double d[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = first[i] - last[i];
            flip = sqrt(fma(d[3], d[3], fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])))) > 1.0 ? 1.0 : 0.0;
        } else {
            wraps = rint((last[0] - first[0]) / 2.0 / WS_PI);
        }
    }
    if (s == 3 && info[WS_INFO_STATUS * si] != 2.0) info[WS_INFO_STATUS * si] = 1.0;
    info[WS_INFO_QUAT_FLIP * si] = flip;
    info[WS_INFO_EULER_WRAPS * si] = wraps;
}

#ifdef __HIPCC__
// the kernels and their launcher: ato_warmstart.hip
hipError_t launch_warmstart(const WarmD& a, int att, int B, int layout, const double* w_point, double* w_drone,
                            double* hlb, double* hub, double* info, hipStream_t st);
#endif  // __HIPCC__

}  // namespace ato
