// ato_replay.hpp -- replay of a collocation solution through the vehicle ODE.
//
// One work item = (instance b, interval n): the interval's start state Z[n,0] is lifted to the
// global model and integrated over h_n with S classical RK4 substeps under the solution's own
// inputs u(tau) = sum_j l_j(tau) U[n,j]; the result is compared with the collocation polynomial's
// own end value sum_k D_k Z[n,k], lifted at boundary n + 1. The number that comes out does not
// depend on the NLP rows: it says whether the trajectory flies, not whether it is optimal or
// feasible (the replay uses the solution's h and u as they are).
//
// The dynamics are the GLOBAL variant of the problem's model (DroneModel<ATT, GLOBAL> /
// PointModel<GLOBAL>) through the same rows() the evaluation kernels run, with an emitter that
// drops the Jacobian arguments. Parametric problems (global_r) are lifted by
//   p = x_c(s_n) + y e_y(s_n) + n e_n(s_n)          (ato_gate::xc / ey / en carry the same terms)
// from a per-boundary table [N+1][12] = xc(3), Rp(9, layout of node_geom); attitude, body velocity
// and body rates are global already (ato_models.hpp: with global_r the attitude state is the global
// rotation; the point mass's velocity is global too).
//
// Shared by the HIP kernel (k_replay below) and the CPU twin (tests/native/replay_hostcheck.cpp):
// replay_interval() is ATO_HD. Nothing renormalises the quaternion or the DCM on the way: the drift
// is part of what is reported.
#pragma once
#include "ato_sample.hpp"

namespace ato {

constexpr int REPLAY_LIFT_W = 12;     // doubles per boundary in the lift table

// replay arguments next to ProbD (kernel argument)
struct ReplayD {
    int32_t S;             // RK4 substeps per interval
    int32_t has_traj;
    const double* lw;      // [2 S + 1][K1] Lagrange weights l_j(i / (2 S))
    const double* lift;    // [N + 1][REPLAY_LIFT_W]; NULL: global-frame problem
};

// l_j(i / (2 S)), i = 0 .. 2 S (lagrange_row): the one table the kernel, the twin and the test oracle all use
inline void replay_weights(const double* tau, int K1, int S, double* lw) {
    for (int i = 0; i <= 2 * S; ++i) lagrange_row(tau, K1, (double)i / (double)(2 * S), lw + (long)i * K1);
}

// 0 (ATO_OK) or the error code of an ato_replay call with these arguments; *msg gets the reason
inline int replay_check(const ProbD& p, bool has_lift, int batch, int layout, int substeps, const char** msg) {
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (int rc = check_layout(layout, msg)) return rc;
    if (substeps < 1 || substeps > SAMPLE_SMAX) { *msg = "substeps must be in [1, 64]"; return ATO_ERR_ARG; }
    if (int rc = check_collocation(p, "replay of RK4-transcribed problems (K = 0) is not supported", msg)) return rc;
    if (p.frame == PARAM_REL) {
        *msg = "replay of parametric problems with the relative attitude (global_r = 0) is not supported";
        return ATO_ERR_UNSUPPORTED;
    }
    if (p.frame == PARAM_GR && !has_lift) {
        *msg = "parametric replay needs the lift table (ato_replay_set_lift)";
        return ATO_ERR_STATE;
    }
    return ATO_OK;
}

template <class M>
struct GlobalOf;
template <int ATT, int FRAME>
struct GlobalOf<DroneModel<ATT, FRAME>> {
    using type = DroneModel<ATT, GLOBAL>;
    static constexpr bool relative = FRAME == PARAM_REL;
};
template <int FRAME>
struct GlobalOf<PointModel<FRAME>> {
    using type = PointModel<GLOBAL>;
    static constexpr bool relative = FRAME == PARAM_REL;
};

// position of a problem-frame state at interval boundary nb (identity for global-frame problems)
template <class M>
ATO_HD void replay_lift(const ReplayD& r, int nb, double* z) {
    if constexpr (M::PARAM) {
        const double* t = r.lift + (long)nb * REPLAY_LIFT_W;
        const double y = z[1], n = z[2];
#pragma unroll
        for (int a = 0; a < 3; ++a) z[a] = t[a] + y * t[3 + a * 3 + 1] + n * t[3 + a * 3 + 2];
    }
}

// rotation angle of R(ra)^T R(rb): atan2(|vee(E - E^T)| / 2, (tr E - 1) / 2)
template <class G>
ATO_HD double replay_att_angle(const double* ra, const double* rb) {
    if constexpr (G::IS_DRONE) {
        using A = typename G::A;
        double Ra[9], Rb[9], E[9];
        A::R(ra, Ra);
        A::R(rb, Rb);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) E[i * 3 + j] = Ra[i] * Rb[j] + Ra[3 + i] * Rb[3 + j] + Ra[6 + i] * Rb[6 + j];
        const double v0 = E[7] - E[5], v1 = E[2] - E[6], v2 = E[3] - E[1];
        return atan2(0.5 * sqrt(v0 * v0 + v1 * v1 + v2 * v2), 0.5 * (E[0] + E[4] + E[8] - 1.0));
    } else {
        return 0.0;
    }
}

// One (instance, interval). w: decision-vector accessor of the instance (w(col)); zs / er / tj point
// at the instance's element 0 of zsim / err / traj with element stride st (tj may be NULL):
//   zsim[(n NZ + i) st], err[(n 4 + c) st], traj[((n S + s) NZ + i) st]
template <class M, class W>
ATO_HD void replay_interval(const ProbD& p, const ReplayD& r, int n, const W& w, double* zs, double* er,
                            double* tj, long st) {
    using G = typename GlobalOf<M>::type;
    constexpr int NZ = M::NZ, NU = M::NU;
    const int K1 = p.K1, S = r.S;
    const Cols<M> c{p.N, K1};
    const double h = w(n), hs = h / (double)S;

    double z[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) z[i] = w(c.z(n, 0, i));
    replay_lift<M>(r, n, z);

    // u at abscissa i / (2 S); the nodes are re-read (L2) so they hold no registers over the stages
    auto input = [&](int i, double* u) {
        const double* l = r.lw + (long)i * K1;
#pragma unroll
        for (int m = 0; m < NU; ++m) u[m] = 0.0;
        for (int j = 0; j < K1; ++j) {
            const double lj = l[j];
#pragma unroll
            for (int m = 0; m < NU; ++m) u[m] += lj * w(c.u(n, j, m));
        }
    };

    const NodeGeom<double> geo = flat_geom();

    double ua[NU], um[NU], ub[NU];
    input(0, ua);
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        input(2 * s + 1, um);
        input(2 * s + 2, ub);
        double k[NZ], acc[NZ], zz[NZ], us[NU];
#pragma unroll
        for (int i = 0; i < NZ; ++i) {
            k[i] = 0.0;
            acc[i] = 0.0;
        }
        // one model instance in a rolled loop over the four stages (as rk4_phi)
#pragma unroll 1
        for (int sg = 0; sg < 4; ++sg) {
            const double cs = sg == 0 ? 0.0 : (sg == 3 ? hs : 0.5 * hs);
#pragma unroll
            for (int i = 0; i < NZ; ++i) zz[i] = z[i] + cs * k[i];
#pragma unroll
            for (int m = 0; m < NU; ++m) us[m] = sg == 0 ? ua[m] : (sg == 3 ? ub[m] : um[m]);
            G::template rows<0, NZ>(zz, us, geo, p.veh,
                                    [&](int i, double fi, const double*, const double*) { k[i] = fi; });
            const double wt = (sg == 0 || sg == 3) ? 1.0 : 2.0;
#pragma unroll
            for (int i = 0; i < NZ; ++i) acc[i] += wt * k[i];
        }
        const double h6 = hs / 6.0;
#pragma unroll
        for (int i = 0; i < NZ; ++i) z[i] += h6 * acc[i];
#pragma unroll
        for (int m = 0; m < NU; ++m) ua[m] = ub[m];
        if (tj) {
#pragma unroll
            for (int i = 0; i < NZ; ++i) tj[(((long)n * S + s) * NZ + i) * st] = z[i];
        }
    }
#pragma unroll
    for (int i = 0; i < NZ; ++i) zs[((long)n * NZ + i) * st] = z[i];

    // the collocation polynomial's own end value, lifted at boundary n + 1
    double zr[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) zr[i] = 0.0;
    for (int j = 0; j < K1; ++j) {
        const double dj = p.D[j];
#pragma unroll
        for (int i = 0; i < NZ; ++i) zr[i] += dj * w(c.z(n, j, i));
    }
    replay_lift<M>(r, n + 1, zr);

    auto dist3 = [&](int i0) {
        const double a = z[i0] - zr[i0], b = z[i0 + 1] - zr[i0 + 1], d = z[i0 + 2] - zr[i0 + 2];
        return sqrt(a * a + b * b + d * d);
    };
    double* e = er + (long)n * 4 * st;
    e[0] = dist3(0);
    e[st] = replay_att_angle<G>(z + M::IR, zr + M::IR);
    e[2 * st] = dist3(M::IV);
    if constexpr (M::IS_DRONE) e[3 * st] = dist3(M::IW);
    else e[3 * st] = 0.0;
}

#ifdef __HIPCC__
constexpr int REPLAY_BLOCK = 64;

// decision-vector reads of one instance, element stride ws
struct ReplayW {
    const double* __restrict__ w;
    long ws;
    __device__ __forceinline__ double operator()(int col) const { return w[(long)col * ws]; }
};

// One thread per (b, n), b fastest: with the interleaved layout a wave's loads and stores of one
// element are contiguous over its instances.
template <class M>
__global__ __launch_bounds__(REPLAY_BLOCK) void k_replay(ProbD p, ReplayD r, int B, int layout,
                                                         const double* __restrict__ w, double* __restrict__ zsim,
                                                         double* __restrict__ err, double* __restrict__ traj) {
    const long t = (long)blockIdx.x * REPLAY_BLOCK + threadIdx.x;
    if (t >= (long)p.N * B) return;
    const int n = (int)(t / B), b = (int)(t % B);
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    const long st = il ? B : 1;
    const ReplayW W{w + (il ? (long)b : (long)b * p.nw), st};
    double* zs = zsim + (il ? (long)b : (long)b * p.N * p.NZ);
    double* er = err + (il ? (long)b : (long)b * p.N * 4);
    double* tj = r.has_traj ? traj + (il ? (long)b : (long)b * p.N * r.S * p.NZ) : nullptr;
    replay_interval<M>(p, r, n, W, zs, er, tj, st);
}

// explicitly instantiated per model variant in ato_replay.hip
template <class M>
hipError_t launch_replay(const ProbD& p, const ReplayD& r, int B, int layout, const double* w, double* zsim,
                         double* err, double* traj, hipStream_t st);

#ifdef ATO_DEFINE_REPLAY_LAUNCHER
template <class M>
hipError_t launch_replay(const ProbD& p, const ReplayD& r, int B, int layout, const double* w, double* zsim,
                         double* err, double* traj, hipStream_t st) {
    if constexpr (GlobalOf<M>::relative) {
        // the relative attitude: rejected by replay_check before any launch
        return hipErrorInvalidValue;
    } else {
        const long items = (long)p.N * B;
        const dim3 grid((unsigned)((items + REPLAY_BLOCK - 1) / REPLAY_BLOCK)), block(REPLAY_BLOCK);
        hipLaunchKernelGGL((k_replay<M>), grid, block, 0, st, p, r, B, layout, w, zsim, err, traj);
        return hipGetLastError();
    }
}
#endif
#endif  // __HIPCC__

}  // namespace ato
