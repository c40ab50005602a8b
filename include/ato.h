/*
 * ato.h -- C ABI of the MI355X raceline NLP evaluation library (libato.so).
 *
 * What it replaces. The reference builds its collocation NLP as CasADi SX
 * expressions and hands them to IPOPT:
 *     ca.nlpsol('solver', 'ipopt', {'x': w, 'f': J, 'g': g}, opts)
 *         drone3d/raceline/base_raceline.py:752-799
 *     solver(x0=..., lbx=..., ubx=..., lbg=..., ubg=...)
 *         drone3d/raceline/base_raceline.py:157-191
 * Inside that call IPOPT evaluates CasADi's generated functions nlp_g, nlp_jac_g
 * (fixed sparsity), nlp_f and nlp_grad_f on every iterate. This library is the
 * drop-in for those evaluations, for a BATCH of independent problem instances
 * that share one structure (same track, N, K, model), on one HIP device.
 *
 *   ato_create        <- building w, g, J and the nlpsol structure
 *                        (base_raceline.py:218-239, 625-717)
 *   ato_sizes         <- w.numel(), g.numel(), jac_g sparsity nnz
 *   ato_sparsity      <- nlp_jac_g sparsity_out (CSR here; CasADi keeps CCS)
 *   ato_bounds        <- lbg / ubg lists built next to g (base_raceline.py:245-247)
 *   ato_eval          <- nlp_g + nlp_jac_g + nlp_f + nlp_grad_f for B instances
 *   ato_destroy, ato_last_error
 *
 * Conventions: all pointers to ato_eval are DEVICE pointers; tables in
 * ato_problem_desc are HOST pointers copied at ato_create. Every function
 * returns ATO_OK (0) or a negative error code, and ato_last_error() holds the
 * message for the calling thread. A handle belongs to the device that was
 * current when it was created; it is not shared between threads concurrently.
 */
#ifndef ATO_H
#define ATO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATO_ABI_VERSION 3
#define ATO_KMAX 9            /* highest collocation degree supported */
#define ATO_GEOM_WIDTH 16     /* doubles per node in the geometry table */

enum { ATO_OK = 0, ATO_ERR_ARG = -1, ATO_ERR_UNSUPPORTED = -2, ATO_ERR_HIP = -3,
       ATO_ERR_STATE = -4 };

enum { ATO_MODEL_DRONE = 0, ATO_MODEL_POINT = 1 };
enum { ATO_ATT_ESP = 0, ATO_ATT_YPR = 1, ATO_ATT_DCM = 2 };  /* quaternion / yaw-pitch-roll / direction-cosine
                                                              matrix (build-side, config 5) */
enum { ATO_FRAME_GLOBAL = 0, ATO_FRAME_PARAMETRIC = 1 };
enum { ATO_TRANS_COLLOCATION = 0, ATO_TRANS_RK4 = 1 };
enum { ATO_GATE_CIRCLE = 0, ATO_GATE_SQUARE = 1 };
#define ATO_CPC_MAX 16
/* Batch layout of w, g, jac, grad_f on the device.
 * INTERLEAVED:      element e of instance b at [e * B + b]  (coalesced; default)
 * INSTANCE_MAJOR:   element e of instance b at [b * n + e]  (n = nw, ng or nnz) */
enum { ATO_LAYOUT_INTERLEAVED = 0, ATO_LAYOUT_INSTANCE_MAJOR = 1 };

/* One gate constraint (base_raceline.py:545-595, parametric placement
 * :986-1032, global placement :907-918). */
typedef struct ato_gate {
    int32_t interval;     /* interval n whose nodes interpolate the gate state   */
    int32_t shape;        /* ATO_GATE_CIRCLE / ATO_GATE_SQUARE                    */
    int32_t fix_center;   /* 1: x - gate_x == 0 (3 rows)                         */
    int32_t axial;        /* 1: axial equality row (global frame)                */
    int32_t at_end;       /* 1: state is z_F of the last interval                */
    int32_t n_coef;       /* weights in coef, on the consecutive nodes starting at   *
                           * node (interval, 0): K+1 (collocation), 1 (global frame:  *
                           * Z[interval, 0] itself), 2 (RK4: Z[n], Z[n+1] interpolated)*/
    double coef[ATO_KMAX + 1];  /* Lagrange weights l_k(d) on Z[interval, k]     */
    double gate_x[3];     /* gate centre                                          */
    double R[9];          /* gate orientation (row-major, columns e1 e2 e3)       */
    double xc[3], ey[3], en[3];  /* centreline point and frame at gate s (param.) */
    double d_max;         /* gate_ri - collision_radius                           */
} ato_gate;

typedef struct ato_problem_desc {
    int32_t abi_version;       /* ATO_ABI_VERSION */
    int32_t model;             /* ATO_MODEL_*  */
    int32_t attitude;          /* ATO_ATT_*    (drone only) */
    int32_t frame;             /* ATO_FRAME_*  */
    int32_t global_r;          /* 1: attitude relative to the global frame */
    int32_t transcription;     /* ATO_TRANS_*  */
    int32_t N, K;              /* intervals, collocation degree (0 for RK4) */
    int32_t closed;            /* periodic raceline */
    int32_t cleanly_closed;    /* centreline frame continuous at s_max -> s_min */
    int32_t quat_flip;         /* closure uses qF + q0 instead of qF - q0 */
    int32_t force_regularity;  /* curvature regularity rows */
    int32_t n_gates;
    int32_t phase_len;         /* global frame: intervals per gate phase (0: none) */
    int32_t has_spheres;       /* obstacle tube rows, one per node */
    int32_t pad0;
    double euler_wraps;        /* YPR closure offset count (2 pi * wraps) */
    double gamma;              /* regularity bound */
    /* vehicle (pytypes.py:357-402) */
    double m, g, b[3], I[3], bw[3], l, kt, T_max;
    double Rcost[16], dRcost[16];   /* input / input-rate cost matrices, nu x nu row-major */
    /* collocation coefficients (discretization_utils.py:8-34) */
    double tau[ATO_KMAX + 1], Bq[ATO_KMAX + 1];
    double C[(ATO_KMAX + 1) * (ATO_KMAX + 1)];   /* C[j * (K+1) + r] */
    double D[ATO_KMAX + 1];
    /* closure for parametric point mass on skew-closed lines (base_raceline.py:1209-1222) */
    double A_skew[4];
    /* host tables, copied at ato_create */
    const double* node_geom;   /* [P][ATO_GEOM_WIDTH]: Rp(9) ks ky kn |xc'| reg_active . . . */
    const double* node_s;      /* [P] fixed s of every node (parametric) */
    const double* interval_s;  /* [N+1] s at interval starts (parametric) */
    const ato_gate* gates;     /* [n_gates] */
    const double* spheres;     /* [P][3]: dy, dn, available radius (obstacle tube) */
    /* CPC gate progress (config 5; Foehn et al. 2021 time-optimal planning; build-side, the reference
     * only displays a CPC trajectory, cpc_utils.py:14-101). cpc_m > 0 (global frame, no gate rows):
     * per node q three blocks of cpc_m variables after the node variables -- progress lambda, its
     * decrease mu, tolerance nu -- and the rows, node by node after the obstacle rows:
     *   mu_j (|p_q - w_j|^2 - nu_j) = 0      (cpc_m complementarity rows)
     *   lambda_j - lambda_{j+1} <= 0        (cpc_m - 1 order rows)
     *   lambda_{q+1,j} - lambda_{q,j} + mu_{q,j} = 0   (cpc_m progress rows, not at the last node) */
    int32_t cpc_m;             /* waypoints (<= ATO_CPC_MAX); 0: no CPC */
    int32_t pad1;
    double cpc_wp[ATO_CPC_MAX * 3];   /* waypoint positions w_j */
} ato_problem_desc;

typedef struct ato_handle ato_handle;

int ato_create(const ato_problem_desc* desc, ato_handle** out);
int ato_destroy(ato_handle* h);

/* nw decision variables, ng constraint rows, nnz structural Jacobian entries. */
int ato_sizes(const ato_handle* h, int32_t* nw, int32_t* ng, int32_t* nnz);

/* CSR pattern of dg/dw in reference row order: row_ptr[ng+1], col[nnz] (host arrays
 * owned by the handle; valid until ato_destroy). Columns are ascending per row. */
int ato_sparsity(const ato_handle* h, const int32_t** row_ptr, const int32_t** col);

/* lbg / ubg (host arrays of ng doubles, caller owned). */
int ato_bounds(const ato_handle* h, double* lbg, double* ubg);

/* Structural nonzeros of grad f: idx (host, caller owned, may be NULL to query nnz) gets the
 * ascending indices of h_n and of every node's inputs u and input rates du -- the only variables
 * in the cost J = sum h_n B_k (u'Ru + du'dR du + 1) (base_raceline.py:601-623); the states'
 * entries are structural zeros. */
int ato_gradf_sparsity(const ato_handle* h, int32_t* nnz, int32_t* idx);

/* sparse != 0: ato_eval / ato_eval_f32 write only the ato_gradf_sparsity entries of grad_f and
 * leave the others untouched (the caller zero-fills its buffer once); 0 (default): every entry. */
int ato_gradf_mode(ato_handle* h, int32_t sparse);

/* Reserve device scratch for batches up to max_batch (call before graph capture). */
int ato_reserve(ato_handle* h, int32_t max_batch);

/* Evaluate g, J (values in ato_sparsity order), f and grad_f for `batch` instances.
 * w: [nw x batch] in `layout`; any of g / jac / f / grad_f may be NULL to skip it.
 * f is [batch]. stream is a hipStream_t (NULL = default stream). Asynchronous. */
int ato_eval(ato_handle* h, int32_t batch, int32_t layout, const double* w,
             double* g, double* jac, double* f, double* grad_f, void* stream);

/* Same evaluation in fp32 (w, outputs float). */
int ato_eval_f32(ato_handle* h, int32_t batch, int32_t layout, const float* w,
                 float* g, float* jac, float* f, float* grad_f, void* stream);

/* Hessian of the Lagrangian  sigma * grad^2 f + sum_i lam_i * grad^2 g_i  (IPOPT's nlp_hess_l,
 * base_raceline.py:752-799). Structure: lower triangle (col <= row) CSR with ascending columns
 * (host arrays owned by the handle). The first call analyses the structure and colours the
 * columns; n_colors seeded passes make up one evaluation. */
int ato_hess_sparsity(ato_handle* h, int32_t* nnz, const int32_t** row_ptr, const int32_t** col,
                      int32_t* n_colors);

/* hess [nnz_h x batch] (layout) for w [nw x batch], lam [ng x batch], sigma [batch] (fp64).
 * Asynchronous on stream; allocates its scratch on the first call for a larger batch
 * (ato_reserve after ato_hess_sparsity pre-allocates it). */
int ato_hess_eval(ato_handle* h, int32_t batch, int32_t layout, const double* w, const double* lam,
                  const double* sigma, double* hess, void* stream);

/* Per-instance obstacle-tube sphere centres (config 4's perturbed tubes; the reference builds one
 * ObstacleFreeTube per solve, mesh_obstacle.py:219-237, so a batch of perturbed tubes is a batch of
 * problems that differ only in these constants). centres: DEVICE array [P][2][stride] of doubles,
 * (dy, dn) of node p for instance b at index (2 p + c) * stride + b; it must stay valid while
 * evaluations use it. Applies to ato_eval / ato_eval_f32 / ato_hess_eval until replaced; NULL
 * returns to the descriptor's shared table. The rows' upper bounds (available radius^2) then
 * differ per instance and are the caller's (ato_sphere_rows gives their row indices). Requires a
 * problem with sphere rows (has_spheres). */
int ato_set_instance_spheres(ato_handle* h, const double* centres, int64_t stride);

/* Row index of each node's sphere row, rows[P] (-1: no sphere row at that node). */
int ato_sphere_rows(const ato_handle* h, int32_t* rows);

/* Triangle mesh of an obstacle environment (MeshObstacle, drone3d/obstacles/mesh_obstacle.py:18-161;
 * replaces trimesh.proximity.signed_distance / closest_point). vertices [nv][3], faces [nf][3]
 * (0-based triangles), host arrays copied at creation. */
typedef struct ato_mesh ato_mesh;
int ato_mesh_create(const double* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                    ato_mesh** out);
int ato_mesh_destroy(ato_mesh* mesh);

/* Signed distance of n points (device [n][3]) to the mesh into dist (device [n]): positive
 * outside, negative inside (ray-crossing parity). closest (device [n][3], may be NULL) gets the
 * closest surface point. Asynchronous on stream. */
int ato_mesh_signed_distance(ato_mesh* mesh, int32_t n, const double* points, double* dist, double* closest,
                             void* stream);

/* The same distance for points of any regular layout: component c of point p at
 * points[p * stride_point + c * stride_comp] (device), dist (device [n]). It walks a second copy of the
 * triangles, sorted at ato_mesh_create by the Morton code of their centroids and cut into tiles with
 * axis-aligned boxes; one wave is 64 consecutive points, so it is meant for coherent point sets
 * (consecutive points close together). cull = 0 visits every tile; cull = 1 skips a tile's distance
 * pass when no point of the wave can be nearer to its box than the point's best so far, and its
 * crossing pass when no point's ray meets the box. Both give the distances of ato_mesh_signed_distance.
 * Asynchronous on stream. */
int ato_mesh_signed_distance_strided(ato_mesh* mesh, int64_t n, const double* points, int64_t stride_point,
                                     int64_t stride_comp, double* dist, int32_t cull, void* stream);

/* Replay of collocation solutions through the vehicle ODE (csrc/ato_replay.hpp): per (instance,
 * interval) the start state Z[n,0], lifted to the global model, is integrated over h_n with
 * `substeps` classical RK4 steps under the solution's own inputs u(tau) = sum_j l_j(tau) U[n,j] and
 * compared with the collocation polynomial's end value sum_k D_k Z[n,k]. The dynamics are the global
 * variant of the problem's model; nothing renormalises the attitude on the way. It certifies the
 * dynamics of w, not optimality or constraints. Collocation problems in the global frame or
 * parametric with global_r; the RK4 transcription and the relative attitude return
 * ATO_ERR_UNSUPPORTED.
 *
 * Lift table for parametric problems: host [N+1][12] = xc(3), Rp(9, layout of node_geom) at interval_s[0..N];
 * copied. Not needed (ignored) for global-frame problems. */
int ato_replay_set_lift(ato_handle* h, const double* lift);
/* zsim [N*NZ x batch], err [N*4 x batch], traj [N*S*NZ x batch] or NULL; substeps in [1, 64].
 * zsim: simulated global-model state at the end of every interval; err per interval: position error
 * (m), attitude error (rotation angle of R(r_sim)^T R(r_ref), rad; 0 for the point mass), body /
 * global velocity error (m/s), body-rate error (rad/s; 0 for the point mass); traj: the state after
 * every substep. Element e of instance b at [e * batch + b] (interleaved) or [b * n + e].
 * Asynchronous on stream; no device-wide synchronisation; the weight table is uploaded on the
 * stream when substeps changes (calls with different substeps on different streams are the caller's
 * to order). A parametric problem without a lift table returns ATO_ERR_STATE. */
int ato_replay(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t substeps,
               double* zsim, double* err, double* traj, void* stream);

/* Transfer of decision vectors between two discretisations of one scenario (csrc/ato_remesh.hpp). src has
 * N intervals of degree K, dst N' = r N intervals of degree K' (r >= 1 an integer; K' >= 1, possibly below
 * K), both collocation transcriptions of the same model variant (model, attitude, frame). Per instance
 *   h'[n r + j]     = h[n] / r
 *   v'[n r + j, k'] = sum_m l_m((j + tau'_k') / r) v[n, m]     for every per-node variable (states, inputs,
 *                                                              input rates)
 * with l_m the Lagrange basis over the source nodes tau_0 = 0, tau_1 .. tau_K (the interpolant of the replay's
 * input), evaluated by the product formula of the replay's weights, summed in ascending m. For K' >= K the
 * piecewise polynomial as a function of time is unchanged; r = 1, K' = K copies finite inputs bit for bit.
 * Nothing is renormalised or clipped, multipliers are not transferred, and feasibility on the new mesh is not
 * preserved: the result is a start for a warm solve.
 *
 * w_src [nw x batch_src], w_dst [nw' x batch_dst], both in `layout`. cols: device array [batch_dst], the source
 * column of every destination column, or NULL for the identity (then batch_dst == batch_src). A destination
 * column whose entry is outside [0, batch_src) is left unwritten. Asynchronous on stream; no device-wide
 * synchronisation. The weight table [r][K'+1][K+1] lives on dst, one per source discretisation: the first call
 * with a new one allocates it and uploads it on that call's stream (calls on other streams are the caller's
 * to order after it); no other call allocates.
 * ATO_ERR_ARG: N' not a multiple of N or below it, batch < 1, unknown layout, different model variant;
 * ATO_ERR_UNSUPPORTED: an RK4-transcribed problem, or one that carries CPC progress variables. */
int ato_remesh(ato_handle* src, ato_handle* dst, int32_t batch_src, int32_t batch_dst, int32_t layout,
               const double* w_src, const int32_t* cols, double* w_dst, void* stream);

/* Clearance of collocation solutions from an obstacle mesh (csrc/ato_clearance.hpp): per (instance, interval,
 * sample) the global position of the interval's own polynomial, sum_j l_j(x_i) Z[n, j, 0..2], and its signed
 * distance to the mesh. samples = S in [1, 64]: S + 1 points per interval at x_i = i / S, both ends; samples = 0:
 * the K + 1 collocation nodes (the reference's collision test, base_raceline.py:1312-1327). S1 is that count.
 * Parametric problems (global_r or the relative attitude) are placed by x_c(s) + y e_y(s) + n e_n(s) at the
 * sample's own interpolated s, from the centreline's two piecewise cubics: knots [n] and coefficients
 * [n + 1][4][3] (piece, power 0..3, axis) of x_c and of r_y, piece 0 left of the first knot and piece n right of
 * the last (linear extrapolation), the piece of s being the number of knots <= s. Host arrays, copied; not needed
 * (ignored) for global-frame problems. It certifies positions against the mesh, nothing about the arc between
 * samples; variable bounds and s' >= 0 between the nodes are ato_audit's, gate openings ato_gatecheck's. */
typedef struct ato_line_table {
    int32_t n_xc, n_ry;
    const double *xc_knots, *xc_coef, *ry_knots, *ry_coef;
} ato_line_table;
int ato_clearance_set_line(ato_handle* h, const ato_line_table* line);
/* w [nw x batch] in `layout`. pos: point p, component c at [c * N*S1*batch + p] with p = (n S1 + i) batch + b
 * (interleaved) or at [p * 3 + c] with p = (b N + n) S1 + i (instance-major); dist [N*S1*batch] by the same p
 * (ato_mesh_signed_distance_strided with `cull`). mesh and dist may be NULL: positions only. pos may be NULL
 * when dist is wanted: a buffer on the handle, grown only when a call needs more. Asynchronous on stream; no
 * device-wide synchronisation; the weight table is uploaded on the stream when samples changes.
 * ATO_ERR_UNSUPPORTED: RK4 transcription; ATO_ERR_STATE: a parametric problem without its centreline table;
 * ATO_ERR_ARG: samples outside [0, 64], batch < 1, unknown layout; nothing is launched or written then. */
int ato_clearance(ato_handle* h, ato_mesh* mesh, int32_t batch, int32_t layout, const double* w, int32_t samples,
                  double* pos, double* dist, int32_t cull, void* stream);

/* Audit of collocation solutions between their nodes (csrc/ato_audit.hpp): per (instance, interval, sample), with
 * the samples of ato_clearance, the whole node vector (z, u, du) of the interval's own polynomial and its state
 * derivative are evaluated and held against everything the NLP constrains at a node. Channels, ATO_AUDIT_NCH
 * doubles per item; margins are ">= 0 means satisfied" and +inf where the quantity does not exist, defects are
 * >= 0 and 0 where the group does not exist:
 *   0-5   min(v - lb, ub - v) over position / attitude / velocity / body rates / inputs / input rates
 *   6     s-dot (parametric)
 *   7     gamma - (k_n y - k_y n) (parametric): with force_regularity (the configuration's default) at EVERY
 *         sample, although the NLP then carries the row only at nodes whose nominal curvature has
 *         k_y^2 + k_n^2 > 0.1, so a failed channel 7 may be a constraint the solve never had; without
 *         force_regularity only where k_y^2 + k_n^2 > 0.1 at the sample's own s, +inf elsewhere
 *   8     1 - u.u / T_max^2 (point mass)
 *   9-12  max |f_i(z, u) - z'_i| over the position / attitude / velocity / body-rate rows of the problem's own
 *         model variant, parametric geometry taken at the sample's own s (table of ato_clearance_set_line)
 *   13    |q.q - 1| (quaternion), Frobenius norm of R^T R - I (DCM), else 0
 * lb, ub: device bounds per component of the node vector, [NV], or with bounds_per_instance [NV x batch] in
 * `layout`; both NULL: +inf in channels 0-5. val: item p, channel c at [c * N*S1*batch + p] with
 * p = (n S1 + i) batch + b (interleaved) or at [p * ATO_AUDIT_NCH + c] with p = (b N + n) S1 + i
 * (instance-major). Not covered: obstacle-tube sphere rows, gates (ato_gatecheck), closure rows, CPC variables, the dU rows,
 * RK4 transcriptions, and the arc between two samples. Asynchronous on stream; no device-wide synchronisation;
 * both weight tables are uploaded on the stream when samples changes. The tables are per-handle state: use ONE
 * stream per handle for ato_audit (and likewise for ato_clearance and ato_replay), or synchronise between calls
 * on different streams: a call on another stream does not wait for an upload queued on the first, and a call with
 * another sample count overwrites the table a kernel of the first may still read. ATO_ERR_UNSUPPORTED: RK4 transcription;
 * ATO_ERR_STATE: a parametric problem without its centreline table; ATO_ERR_ARG: samples outside [0, 64],
 * batch < 1, unknown layout, exactly one of lb / ub NULL; nothing is launched or written then. */
#define ATO_AUDIT_NCH 14
int ato_audit(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t samples, const double* lb,
              const double* ub, int32_t bounds_per_instance, double* val, void* stream);

/* Gate passage of collocation solutions (csrc/ato_gatecheck.hpp): does the continuous trajectory go through each
 * gate's opening, where and when. A gate plane has a centre c, axes e1 e2 e3 (the columns of R, row-major as in
 * ato_gate), a half-opening d_max and a shape; a point at global position x has a = e1.(x - c), p2 = e2.(x - c),
 * p3 = e3.(x - c). The points of a lap are the samples of ato_clearance, (n, i) at abscissa i / S, i = 0 .. S,
 * n = 0 .. N - 1 (samples = S in [1, 64]; the node rule samples = 0 is rejected: it leaves the tail (tau_K, 1]
 * without a bracket), parametric problems placed through the centreline at the point's own s; closed problems wrap
 * to (0, 0). A crossing lies between consecutive points whose (a >= 0) differ: inside one interval it is refined by
 * 53 bisections of the polynomial itself and reported at the right end of the last bracket; across an interval
 * junction or the wrap it is the later point, unrefined. On open lines the first and the last point are crossings
 * too when |a| <= axial_tol (metres; their gates sit on them). The margin of a crossing is d_max - sqrt(p2^2 + p3^2)
 * (circle) or d_max - max(|p2|, |p3|) (square), fix_center gates included (their exact row is channel 7). The
 * direction of a crossing is recorded, not required. Per (gate, instance) ATO_GATECHECK_NCH doubles:
 *   0  n_cross   crossings found
 *   1  margin    of the best crossing (the largest margin, ties to the earliest (n, x)); -inf if there is none
 *   2  interval  n of the best crossing (-1: none)
 *   3  x         its abscissa in [0, 1]
 *   4  t         sum_{m < n} h_m + x h_n, the passage time
 *   5, 6  p2, p3 lateral offsets there
 *   7  off       sqrt(p2^2 + p3^2)
 *   8  flag      +1 / -1: direction of the best crossing along e1; 0: none; NaN: some evaluated a or margin of
 *                this (gate, instance) was not finite (a non-finite value never becomes the best crossing), or
 *                some step size h_n is not finite and positive
 * Channels 3-7 are NaN without a crossing. val: channel c of gate g, instance b at [(c G + g) batch + b]
 * (interleaved) or [(b G + g) ATO_GATECHECK_NCH + c] (instance-major). The gates are the problem's own (centre, R,
 * d_max, shape of desc.gates, in their order) unless ato_gatecheck_set_gates replaced them: planes is a host array
 * of n <= 64 planes, copied (tighter openings, CPC waypoints as circular gates); n = 0 returns to the problem's
 * own. It reads the first three state components only: any model, any attitude, the three frames. Not covered: the
 * trajectory as flown (ato_replay), RK4 transcriptions, closure rows, the gate's frame as an obstacle, gate order
 * (t is reported). Three launches on the stream (positions, crossings per interval, reduction per gate); no
 * device-wide synchronisation, no atomics: bitwise repeatable, independent of the batch. The partial records live
 * in a buffer on the handle, grown only when a call needs more. The weight table and the position buffer are
 * per-handle state shared with ato_clearance: use ONE stream per handle for ato_gatecheck, ato_clearance, ato_audit
 * and ato_replay, or synchronise between calls on different streams. ATO_ERR_UNSUPPORTED: RK4 transcription;
 * ATO_ERR_STATE: a parametric problem without its centreline table (ato_clearance_set_line), or no gates (a CPC
 * problem or a parametric line without gate_s, and none set); ATO_ERR_ARG: samples outside [1, 64], batch < 1,
 * unknown layout, axial_tol negative or NaN, more than 64 gates; nothing is launched or written then. */
#define ATO_GATECHECK_NCH 9
typedef struct ato_gate_plane {
    double centre[3];
    double R[9];          /* row-major, columns e1 e2 e3 */
    double d_max;
    int32_t shape;        /* ATO_GATE_CIRCLE / ATO_GATE_SQUARE */
    int32_t pad;
} ato_gate_plane;
/* ato_gatecheck_set_gates synchronises the whole device before it replaces the planes (a queued check may still read
 * the old ones), as ato_clearance_set_line does: it is a set-up call, not one for a hot path. */
int ato_gatecheck_set_gates(ato_handle* h, const ato_gate_plane* planes, int32_t n);
int ato_gatecheck(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t samples, double axial_tol,
                  double* val, void* stream);
/* Profiling aid: the same call with only the launches of a bit mask (1 positions, 2 crossings, 4 reduction; 7 is
 * ato_gatecheck). A launch left out reads what the last whole call left in the handle's buffers, so a subset is
 * accepted only after a whole call of the same batch, layout, samples and gates on this handle (ATO_ERR_STATE
 * otherwise). Not part of the check's interface: tools/bench_gatecheck.py is its only user. */
int ato_gatecheck_launches(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t samples,
                           double axial_tol, double* val, void* stream, int32_t launches);

/* Per-kernel timing with HIP events recorded on the evaluation stream. ato_timing(h, n)
 * allocates n event slots and starts recording (n = 0 stops); while on, each ato_eval
 * records events around its Jacobian kernel and its cost-reduction kernel. ato_timing_read
 * waits for the recorded events and returns the summed durations (ms) and the call count. */
int ato_timing(ato_handle* h, int32_t max_calls);
int ato_timing_read(ato_handle* h, double* eval_ms, double* reduce_ms, int32_t* calls);
/* Sample the timing: while on, only every stride-th ato_eval (counted from the last ato_timing
 * call) records its events (stride 1, the default: every call). Each recorded call puts three
 * event packets into the stream, about 10 us of gaps at the benchmark size; sampling keeps the
 * kernel durations measured inside a timed loop without slowing the loop itself. */
int ato_timing_stride(ato_handle* h, int32_t stride);

const char* ato_last_error(void);

/* Library version string, e.g. "ato 1 gfx950". */
const char* ato_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ATO_H */
