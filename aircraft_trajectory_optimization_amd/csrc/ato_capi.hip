// ato_capi.hip -- the C ABI of libato.so (include/ato.h): handle lifetime, sparsity, bounds,
// and dispatch of ato_eval to the per-model launchers (ato_inst.hip).
#include <hip/hip_runtime.h>
#include <string>
#include <exception>
#include <new>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include "ato_kernels.hpp"

#include "ato_handle.hpp"

static thread_local std::string g_last_error;

static int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

void ato_internal_set_error(const std::string& msg) { g_last_error = msg; }

#define ATO_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) return fail(ATO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class V>
static int upload(const std::vector<V>& host, V** dev) {
    *dev = nullptr;
    if (host.empty()) return ATO_OK;
    ATO_HIP(hipMalloc((void**)dev, host.size() * sizeof(V)));
    ATO_HIP(hipMemcpy(*dev, host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice));
    return ATO_OK;
}

static void release(ato_handle* h) {
    if (!h) return;
    (void)hipFree(h->d_geom);
    (void)hipFree(h->d_node_s);
    (void)hipFree(h->d_interval_s);
    (void)hipFree(h->d_spheres);
    (void)hipFree(h->d_cpc_wp);
    (void)hipFree(h->d_gates);
    (void)hipFree(h->d_seg);
    (void)hipFree(h->d_tail);
    (void)hipFree(h->d_units);
    (void)hipFree(h->d_units_lf);
    (void)hipFree(h->d_fpart);
    for (int32_t* d : {h->d_color, h->d_take_e, h->d_take_r, h->d_tk_ptr, h->d_tk_ent, h->d_tk_row, h->d_tkf_ptr,
                       h->d_tkf_ent, h->d_tkf_row, h->d_take_off})
        (void)hipFree(d);
    (void)hipFree(h->d_amask);
    (void)hipFree(h->d_dJ);
    (void)hipFree(h->d_dgf);
    (void)hipFree(h->d_lift);
    for (auto& kv : h->remesh_tabs) (void)hipFree(kv.second.dev);
    (void)hipFree(h->d_line);
    (void)hipFree(h->d_clear_pos);
    (void)hipFree(h->d_gate_tau);       // the planes follow tau in the same allocation
    (void)hipFree(h->d_gate_part);
    for (ato_weight_cache* c : {&h->replay_w, &h->clear_w, &h->audit_w}) (void)hipFree(c->dev);
    h->remesh_tabs.clear();
    for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
    h->events.clear();
}

extern "C" {

const char* ato_last_error(void) { return g_last_error.c_str(); }

const char* ato_version(void) { return "ato 2 gfx950"; }

static int create_impl(const ato_problem_desc* desc, ato_handle** out);

// C++ exceptions (std::bad_alloc, std::length_error of the host layout / Hessian analysis) must not
// cross the C ABI: they would end the host process in std::terminate (SIGABRT)
#define ATO_NOEXCEPT_BODY(expr)                                                                   \
    try {                                                                                        \
        return (expr);                                                                           \
    } catch (const std::exception& e_) {                                                         \
        return fail(ATO_ERR_ARG, std::string("host exception: ") + e_.what());                   \
    } catch (...) {                                                                              \
        return fail(ATO_ERR_ARG, "host exception");                                              \
    }

int ato_create(const ato_problem_desc* desc, ato_handle** out) { ATO_NOEXCEPT_BODY(create_impl(desc, out)) }

static int create_impl(const ato_problem_desc* desc, ato_handle** out) {
    if (!desc || !out) return fail(ATO_ERR_ARG, "null argument");
    *out = nullptr;
    ato_handle* h = new (std::nothrow) ato_handle();
    if (!h) return fail(ATO_ERR_ARG, "out of host memory");
    std::string err = h->L.build(*desc);
    if (!err.empty()) {
        delete h;
        return fail(err.find("not supported") != std::string::npos ? ATO_ERR_UNSUPPORTED : ATO_ERR_ARG, err);
    }
    // Debug / profiling aid: ATO_DEBUG_UNITS=<digits> keeps only the listed unit kinds
    // (0 tail, 1 ODE_A, 2 ODE_B, 3 node, 4 interval). Outputs are then incomplete.
    if (const char* filt = std::getenv("ATO_DEBUG_UNITS")) {
        std::vector<int32_t> kept;
        int cnt[3] = {0, 0, 0};
        for (int c = 0; c < 3; ++c)   // keep the class ordering of the table
            for (size_t u = 0; u + 3 < h->L.units.size(); u += 4) {
                const int kind = h->L.units[u];
                const int cl = kind == ato::UNIT_TAIL ? 0 : (kind <= ato::UNIT_ODE_B ? 1 : 2);
                if (cl == c && std::strchr(filt, '0' + kind)) {
                    kept.insert(kept.end(), &h->L.units[u], &h->L.units[u] + 4);
                    ++cnt[c];
                }
            }
        h->L.units = kept;
        h->L.units_lf = kept;
        h->L.p.cls_off[0] = 0;
        h->L.p.cls_off[1] = cnt[0];
        h->L.p.cls_off[2] = cnt[0] + cnt[1];
        h->L.p.cls_off[3] = cnt[0] + cnt[1] + cnt[2];
        h->L.rebind();
    }
    int rc;
    if (hipGetDevice(&h->device) != hipSuccess) {
        delete h;
        return fail(ATO_ERR_HIP, "no HIP device");
    }
    if ((rc = upload(h->L.geom, &h->d_geom)) || (rc = upload(h->L.node_s, &h->d_node_s)) ||
        (rc = upload(h->L.interval_s, &h->d_interval_s)) || (rc = upload(h->L.spheres, &h->d_spheres)) ||
        (rc = upload(h->L.gates, &h->d_gates)) || (rc = upload(h->L.seg, &h->d_seg)) ||
        (rc = upload(h->L.tail, &h->d_tail)) || (rc = upload(h->L.units, &h->d_units)) ||
        (rc = upload(h->L.units_lf, &h->d_units_lf)) || (rc = upload(h->L.cpc_wp, &h->d_cpc_wp))) {
        release(h);
        delete h;
        return rc;
    }
    // the weight tables of the replay, the clearance and the audit (value and derivative), sized for the largest
    // substep / sample count: the calls themselves allocate nothing
    const size_t row = (ATO_KMAX + 1) * sizeof(double);
    const struct {
        ato_weight_cache* cache;
        size_t rows;
        const char* what;
    } caches[] = {{&h->replay_w, 2 * ato::SAMPLE_SMAX + 1, "replay weight table: out of device memory"},
                  {&h->clear_w, ato::SAMPLE_SMAX + 1, "clearance weight table: out of device memory"},
                  {&h->audit_w, 2 * (ato::SAMPLE_SMAX + 1), "audit weight tables: out of device memory"}};
    for (const auto& c : caches)
        if (hipMalloc((void**)&c.cache->dev, c.rows * row) != hipSuccess) {
            release(h);
            delete h;
            return fail(ATO_ERR_HIP, c.what);
        }
    // gate passage: tau and room for GATE_MAX planes, the problem's own gates uploaded (a problem with more than
    // GATE_MAX keeps its count, which ato_gatecheck rejects)
    {
        const size_t tau_bytes = (ATO_KMAX + 1) * sizeof(double);
        if (hipMalloc((void**)&h->d_gate_tau, tau_bytes + ato::GATE_MAX * sizeof(ato_gate_plane)) != hipSuccess) {
            release(h);
            delete h;
            return fail(ATO_ERR_HIP, "gate planes: out of device memory");
        }
        h->d_gate_planes = (ato_gate_plane*)(h->d_gate_tau + ATO_KMAX + 1);
        const std::vector<ato_gate_plane> own = ato::gate_planes_of(h->L.gates);
        h->n_gate_planes = (int32_t)own.size();
        hipError_t e = hipMemcpy(h->d_gate_tau, h->L.p.tau, tau_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess && !own.empty() && own.size() <= (size_t)ato::GATE_MAX)
            e = hipMemcpy(h->d_gate_planes, own.data(), own.size() * sizeof(ato_gate_plane), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            release(h);
            delete h;
            return fail(ATO_ERR_HIP, "gate planes: upload failed");
        }
    }
    h->pd = h->L.p;
    h->pd.geom = h->d_geom;
    h->pd.node_s = h->d_node_s;
    h->pd.interval_s = h->d_interval_s;
    h->pd.spheres = h->d_spheres;
    h->pd.cpc_wp = h->d_cpc_wp;
    h->pd.gates = h->d_gates;
    h->pd.seg = h->d_seg;
    h->pd.tail = h->d_tail;
    h->pd.units = h->d_units;
    h->pd_lf = h->pd;
    h->pd_lf.units = h->d_units_lf;
    if (const char* e = std::getenv("ATO_LONGFIRST_MAX_B")) h->lf_max_batch = std::atoi(e);
    if (const char* e = std::getenv("ATO_EVAL_TILE")) h->eval_tile = std::atoi(e);
    if (const char* e = std::getenv("ATO_EVAL_TILE_LF")) h->tile_lf = std::atoi(e) != 0;
    if (const char* e = std::getenv("ATO_HESS_MASK")) h->hess_mask = std::atoi(e) != 0;
    *out = h;
    return ATO_OK;
}

int ato_destroy(ato_handle* h) {
    if (!h) return ATO_OK;
    release(h);
    delete h;
    return ATO_OK;
}

int ato_sizes(const ato_handle* h, int32_t* nw, int32_t* ng, int32_t* nnz) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    if (nw) *nw = h->L.p.nw;
    if (ng) *ng = h->L.p.ng;
    if (nnz) *nnz = h->L.p.nnz;
    return ATO_OK;
}

int ato_sparsity(const ato_handle* h, const int32_t** row_ptr, const int32_t** col) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    if (row_ptr) *row_ptr = h->L.row_ptr.data();
    if (col) *col = h->L.col.data();
    return ATO_OK;
}

int ato_set_instance_spheres(ato_handle* h, const double* centres, int64_t stride) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    if (centres && !h->L.p.has_spheres) return fail(ATO_ERR_ARG, "per-instance spheres need a problem with sphere rows");
    if (centres && stride < 1) return fail(ATO_ERR_ARG, "bad sphere table stride");
    for (ato::ProbD* p : {&h->pd, &h->pd_lf}) {
        p->isph = centres;
        p->isph_stride = centres ? stride : 0;
    }
    return ATO_OK;
}

int ato_sphere_rows(const ato_handle* h, int32_t* rows) {
    if (!h || !rows) return fail(ATO_ERR_ARG, "null argument");
    for (int q = 0; q < h->L.p.P; ++q) rows[q] = h->L.seg[((size_t)q * ato::NSEG + ato::SEG_SPHERE) * 2];
    return ATO_OK;
}

int ato_gradf_mode(ato_handle* h, int32_t sparse) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    for (ato::ProbD* p : {&h->pd, &h->pd_lf}) p->gf_sparse = sparse ? 1 : 0;
    return ATO_OK;
}

int ato_gradf_sparsity(const ato_handle* h, int32_t* nnz, int32_t* idx) {
    if (!h || !nnz) return fail(ATO_ERR_ARG, "null argument");
    // the entries the gradient passes write with a value (Layout units: interval n writes h_n, node
    // (n, k) its inputs u and input rates du); everything else is a structural zero of grad f
    const ato::ProbD& p = h->L.p;
    const int N = p.N, NZ = p.NZ, NU = p.NU, NV = p.NV;
    const int per_interval = p.K1;          // (RK4: K = 0, one node per interval)
    int32_t c = 0;
    for (int n = 0; n < N; ++n) {
        if (idx) idx[c] = n;
        ++c;
    }
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < per_interval; ++k)
            for (int i = 0; i < 2 * NU; ++i) {
                if (idx) idx[c] = N + (n * per_interval + k) * NV + NZ + i;
                ++c;
            }
    *nnz = c;
    return ATO_OK;
}

int ato_bounds(const ato_handle* h, double* lbg, double* ubg) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    for (size_t i = 0; i < h->L.lbg.size(); ++i) {
        if (lbg) lbg[i] = h->L.lbg[i];
        if (ubg) ubg[i] = h->L.ubg[i];
    }
    return ATO_OK;
}

// colours whose seeded passes share one launch: their scratch is held at once, within a byte budget
// (ATO_HESS_GROUP_BYTES, default 2 GiB) -- at B = 512 on the racetrack nine colours, at restoration widths
// all of them
static size_t hess_group_bytes() {
    static const size_t v = [] {
        const char* e = std::getenv("ATO_HESS_GROUP_BYTES");
        const long long b = e ? std::atoll(e) : (2LL << 30);
        return (size_t)(b > 0 ? b : 0);
    }();
    return v;
}

static int hess_reserve(ato_handle* h, int32_t max_batch) {
    if (max_batch <= h->hess_reserved) return ATO_OK;
    // the old scratch may still be read by kernels queued on any stream: drain before freeing
    if (h->d_dJ || h->d_dgf) ATO_HIP(hipDeviceSynchronize());
    (void)hipFree(h->d_dJ);
    (void)hipFree(h->d_dgf);
    h->d_dJ = h->d_dgf = nullptr;
    h->hess_reserved = 0;
    h->hess_colors = 0;
    const size_t per = ((size_t)std::max(h->L.p.nnz, 1) + (size_t)h->L.p.nw) * (size_t)max_batch * sizeof(double);
    const int nc = std::max(h->HL.n_colors, 1);
    const int g = (int)std::max<size_t>(1, std::min<size_t>((size_t)nc, hess_group_bytes() / std::max<size_t>(per, 1)));
    ATO_HIP(hipMalloc(&h->d_dJ, (size_t)g * std::max(h->L.p.nnz, 1) * max_batch * sizeof(double)));
    if (hipMalloc(&h->d_dgf, (size_t)g * h->L.p.nw * max_batch * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(h->d_dJ);
        h->d_dJ = nullptr;
        return fail(ATO_ERR_HIP, "hessian scratch: out of device memory");
    }
    h->hess_reserved = max_batch;
    h->hess_colors = g;
    return ATO_OK;
}

int ato_reserve(ato_handle* h, int32_t max_batch) {
    if (!h || max_batch < 1) return fail(ATO_ERR_ARG, "bad reserve arguments");
    if (h->hess_ready) {
        int rc = hess_reserve(h, max_batch);
        if (rc) return rc;
    }
    if (max_batch <= h->reserved) return ATO_OK;
    if (h->d_fpart) {
        ATO_HIP(hipDeviceSynchronize());        // queued evaluations may still write the old partials
        ATO_HIP(hipFree(h->d_fpart));
    }
    h->d_fpart = nullptr;
    h->reserved = 0;
    ATO_HIP(hipMalloc(&h->d_fpart, (size_t)h->L.p.N * max_batch * sizeof(double)));
    h->reserved = max_batch;
    return ATO_OK;
}

}  // extern "C"

template <class T>
static int eval_impl(ato_handle* h, int32_t batch, int32_t layout, const T* w, T* g, T* jac, T* f,
                     T* grad_f, void* stream) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    if (batch < 1) return fail(ATO_ERR_ARG, "batch must be >= 1");
    if (layout != ATO_LAYOUT_INTERLEAVED && layout != ATO_LAYOUT_INSTANCE_MAJOR)
        return fail(ATO_ERR_ARG, "unknown layout");
    if (!w) return fail(ATO_ERR_ARG, "w is null");
    const bool wf = f || grad_f;
    if (wf && !(f && grad_f)) return fail(ATO_ERR_ARG, "f and grad_f must be requested together");
    if (wf && batch > h->reserved) {
        int rc = ato_reserve(h, batch);
        if (rc) return rc;
    }
    // small batches run the long-first unit order (see Layout::build_units); larger ones run in
    // instance tiles of eval_tile chunks (long-first inside a tile when tile_lf)
    const bool tiled = batch > h->lf_max_batch && h->eval_tile > 0;
    const ato::ProbD& p = batch <= h->lf_max_batch || (tiled && h->tile_lf) ? h->pd_lf : h->pd;
    hipError_t e = hipSuccess;
    ato::with_model(p, [&]<class M>() {
        hipEvent_t* ev = nullptr;
        const bool sample = h->timing_stride <= 1 || h->timing_seen % h->timing_stride == 0;
        if (!h->events.empty()) ++h->timing_seen;
        if (sample && (size_t)(h->timed_calls + 1) * 3 <= h->events.size())
            ev = &h->events[(size_t)h->timed_calls++ * 3];
        e = ato::launch_eval<M, T>(p, batch, layout, w, g, jac, grad_f, f, (T*)h->d_fpart, (hipStream_t)stream,
                                   ev, tiled ? h->eval_tile : 0);
    });
    if (e != hipSuccess) return fail(ATO_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return ATO_OK;
}

extern "C" int ato_timing(ato_handle* h, int32_t max_calls) {
    if (!h || max_calls < 0) return fail(ATO_ERR_ARG, "bad timing arguments");
    for (hipEvent_t e : h->events) ATO_HIP(hipEventDestroy(e));
    h->events.clear();
    h->timed_calls = 0;
    h->timing_seen = 0;
    for (int i = 0; i < 3 * max_calls; ++i) {
        hipEvent_t e;
        // timing only: without the system-scope release the stop stamp is not delayed by the
        // write-back of the L2s the kernel's ~250 MB of stores stream through (hipExtLaunchKernel
        // stamps with default events read 52.4 us where rocprof's trace of the same launches
        // averaged 46.7 us, gpurun_out/r03i)
        ATO_HIP(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
        h->events.push_back(e);
    }
    return ATO_OK;
}

extern "C" int ato_timing_stride(ato_handle* h, int32_t stride) {
    if (!h || stride < 1) return fail(ATO_ERR_ARG, "bad timing stride");
    h->timing_stride = stride;
    return ATO_OK;
}

extern "C" int ato_timing_read(ato_handle* h, double* eval_ms, double* reduce_ms, int32_t* calls) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    double se = 0.0, sr = 0.0;
    for (int32_t c = 0; c < h->timed_calls; ++c) {
        hipEvent_t* ev = &h->events[(size_t)c * 3];
        ATO_HIP(hipEventSynchronize(ev[2]));
        float a = 0.f, b = 0.f;
        ATO_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
        ATO_HIP(hipEventElapsedTime(&b, ev[1], ev[2]));
        se += a;
        sr += b;
    }
    if (eval_ms) *eval_ms = se;
    if (reduce_ms) *reduce_ms = sr;
    if (calls) *calls = h->timed_calls;
    return ATO_OK;
}

// Hessian structure, colouring and recovery tables (host analysis + upload), once per handle
static int ensure_hess_impl(ato_handle* h);
static int ensure_hess(ato_handle* h) { ATO_NOEXCEPT_BODY(ensure_hess_impl(h)) }
static int ensure_hess_impl(ato_handle* h) {
    if (h->hess_ready) return ATO_OK;
    std::string err = h->HL.build(h->L);
    if (!err.empty()) return fail(ATO_ERR_UNSUPPORTED, err);
    int rc;
    if ((rc = upload(h->HL.color, &h->d_color)) || (rc = upload(h->HL.take_e, &h->d_take_e)) ||
        (rc = upload(h->HL.take_r, &h->d_take_r)) || (rc = upload(h->HL.tk_ptr, &h->d_tk_ptr)) ||
        (rc = upload(h->HL.tk_ent, &h->d_tk_ent)) || (rc = upload(h->HL.tk_row, &h->d_tk_row)) ||
        (rc = upload(h->HL.tkf_ptr, &h->d_tkf_ptr)) || (rc = upload(h->HL.tkf_ent, &h->d_tkf_ent)) ||
        (rc = upload(h->HL.tkf_row, &h->d_tkf_row)) || (rc = upload(h->HL.amask, &h->d_amask)) ||
        (rc = upload(h->HL.take_off, &h->d_take_off)))
        return rc;
    h->hess_ready = true;
    return ATO_OK;
}

extern "C" int ato_hess_sparsity(ato_handle* h, int32_t* nnz, const int32_t** row_ptr, const int32_t** col,
                                 int32_t* n_colors) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    int rc = ensure_hess(h);
    if (rc) return rc;
    if (nnz) *nnz = h->HL.nnz();
    if (row_ptr) *row_ptr = h->HL.row_ptr.data();
    if (col) *col = h->HL.col.data();
    if (n_colors) *n_colors = h->HL.n_colors;
    return ATO_OK;
}

extern "C" int ato_hess_eval(ato_handle* h, int32_t batch, int32_t layout, const double* w, const double* lam,
                             const double* sigma, double* hess, void* stream) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    if (batch < 1) return fail(ATO_ERR_ARG, "batch must be >= 1");
    if (layout != ATO_LAYOUT_INTERLEAVED && layout != ATO_LAYOUT_INSTANCE_MAJOR)
        return fail(ATO_ERR_ARG, "unknown layout");
    if (!w || !lam || !sigma || !hess) return fail(ATO_ERR_ARG, "null buffer");
    int rc = ensure_hess(h);
    if (rc) return rc;
    if ((rc = hess_reserve(h, batch))) return rc;
    const bool mk = h->hess_mask;
    const ato::HessDev hd{h->d_color, h->d_take_e, h->d_take_r, mk ? h->d_tk_ptr : h->d_tkf_ptr,
                          mk ? h->d_tk_ent : h->d_tkf_ent, mk ? h->d_tk_row : h->d_tkf_row,
                          mk ? h->d_amask : nullptr, h->HL.mask_words,
                          h->HL.take_off.data(), h->HL.n_colors, h->HL.nnz(), h->d_take_off,
                          // colours per launch at this batch: as many as the scratch holds
                          (int)std::max<long long>(1, std::min<long long>(h->HL.n_colors,
                              (long long)h->hess_colors * h->hess_reserved / batch))};
    hipError_t e = hipSuccess;
    ato::ProbD p = batch <= h->lf_max_batch ? h->pd_lf : h->pd;   // unit order as in ato_eval
    p.gf_sparse = 0;    // the seeded passes' grad f tangents fill a scratch buffer: every entry is written
    ato::with_model(p, [&]<class M>() {
        e = ato::launch_hess<M>(p, hd, batch, layout, w, lam, sigma, hess, h->d_dJ, h->d_dgf,
                                (hipStream_t)stream);
    });
    if (e != hipSuccess) return fail(ATO_ERR_HIP, std::string("hessian launch: ") + hipGetErrorString(e));
    return ATO_OK;
}

extern "C" int ato_replay_set_lift(ato_handle* h, const double* lift) {
    if (!h || !lift) return fail(ATO_ERR_ARG, "null argument");
    if (h->L.p.frame == ato::GLOBAL) return ATO_OK;      // not needed: ignored
    const size_t bytes = (size_t)(h->L.p.N + 1) * ato::REPLAY_LIFT_W * sizeof(double);
    if (!h->d_lift) ATO_HIP(hipMalloc((void**)&h->d_lift, bytes));
    ATO_HIP(hipMemcpy(h->d_lift, lift, bytes, hipMemcpyHostToDevice));
    return ATO_OK;
}

static int replay_impl(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t substeps,
                       double* zsim, double* err, double* traj, void* stream) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    const ato::ProbD& p = h->pd;
    const char* msg = "";
    if (int rc = ato::replay_check(p, h->d_lift != nullptr, batch, layout, substeps, &msg)) return fail(rc, msg);
    if (!w || !zsim || !err) return fail(ATO_ERR_ARG, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    ATO_HIP(h->replay_w.use(substeps, (size_t)(2 * substeps + 1) * p.K1,
                            [&](double* lw) { ato::replay_weights(p.tau, p.K1, substeps, lw); }, st));
    const ato::ReplayD r{substeps, traj ? 1 : 0, h->replay_w.dev, p.frame == ato::GLOBAL ? nullptr : h->d_lift};
    hipError_t e = hipSuccess;
    ato::with_model(p, [&]<class M>() { e = ato::launch_replay<M>(p, r, batch, layout, w, zsim, err, traj, st); });
    if (e != hipSuccess) return fail(ATO_ERR_HIP, std::string("replay launch: ") + hipGetErrorString(e));
    return ATO_OK;
}

extern "C" int ato_replay(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t substeps,
                          double* zsim, double* err, double* traj, void* stream) {
    ATO_NOEXCEPT_BODY(replay_impl(h, batch, layout, w, substeps, zsim, err, traj, stream))
}

static int remesh_impl(ato_handle* src, ato_handle* dst, int32_t batch_src, int32_t batch_dst, int32_t layout,
                       const double* w_src, const int32_t* cols, double* w_dst, void* stream) {
    if (!src || !dst) return fail(ATO_ERR_ARG, "null handle");
    const ato::ProbD &ps = src->pd, &pd = dst->pd;
    const char* msg = "";
    if (int rc = ato::remesh_check(ps, pd, batch_src, batch_dst, cols != nullptr, layout, &msg)) return fail(rc, msg);
    if (!w_src || !w_dst) return fail(ATO_ERR_ARG, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    const int r = pd.N / ps.N;
    std::vector<double> key{(double)r};
    key.insert(key.end(), ps.tau, ps.tau + ps.K1);
    ato_handle::RemeshTable& tab = dst->remesh_tabs[key];
    if (!tab.dev) {
        tab.host.resize((size_t)r * pd.K1 * ps.K1);
        ato::remesh_weights(ps.tau, ps.K1, pd.tau, pd.K1, r, tab.host.data());
        const size_t bytes = tab.host.size() * sizeof(double);
        if (hipMalloc((void**)&tab.dev, bytes) != hipSuccess) {
            tab.dev = nullptr;
            return fail(ATO_ERR_HIP, "remesh weight table: out of device memory");
        }
        if (hipMemcpyAsync(tab.dev, tab.host.data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
            (void)hipFree(tab.dev);
            tab.dev = nullptr;
            return fail(ATO_ERR_HIP, "remesh weight table: upload failed");
        }
    }
    const ato::RemeshD a = ato::remesh_args(ps, pd, tab.dev);
    const hipError_t e = ato::launch_remesh(a, batch_src, batch_dst, layout, w_src, cols, w_dst, st);
    if (e != hipSuccess) return fail(ATO_ERR_HIP, std::string("remesh launch: ") + hipGetErrorString(e));
    return ATO_OK;
}

extern "C" int ato_remesh(ato_handle* src, ato_handle* dst, int32_t batch_src, int32_t batch_dst, int32_t layout,
                          const double* w_src, const int32_t* cols, double* w_dst, void* stream) {
    ATO_NOEXCEPT_BODY(remesh_impl(src, dst, batch_src, batch_dst, layout, w_src, cols, w_dst, stream))
}

static int clearance_set_line_impl(ato_handle* h, const ato_line_table* t) {
    if (!h || !t) return fail(ATO_ERR_ARG, "null argument");
    if (h->L.p.frame == ato::GLOBAL) return ATO_OK;      // not needed: ignored
    if (t->n_xc < 2 || t->n_ry < 2 || !t->xc_knots || !t->xc_coef || !t->ry_knots || !t->ry_coef)
        return fail(ATO_ERR_ARG, "bad centreline table");
    const std::vector<double> buf = ato::line_pack(*t);
    double* d = nullptr;
    ATO_HIP(hipMalloc((void**)&d, buf.size() * sizeof(double)));
    if (hipMemcpy(d, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return fail(ATO_ERR_HIP, "centreline table: upload failed");
    }
    if (hipDeviceSynchronize() != hipSuccess) {      // a queued clearance may still read the table this one replaces
        (void)hipFree(d);
        return fail(ATO_ERR_HIP, "centreline table: device synchronisation failed");
    }
    (void)hipFree(h->d_line);
    h->d_line = d;
    h->line = ato::line_view(*t, d);
    return ATO_OK;
}

extern "C" int ato_clearance_set_line(ato_handle* h, const ato_line_table* t) {
    ATO_NOEXCEPT_BODY(clearance_set_line_impl(h, t))
}

static int clearance_impl(ato_handle* h, ato_mesh* mesh, int32_t batch, int32_t layout, const double* w,
                          int32_t samples, double* pos, double* dist, int32_t cull, void* stream) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    const ato::ProbD& p = h->pd;
    const char* msg = "";
    if (int rc = ato::clearance_check(p, h->d_line != nullptr, batch, layout, samples, &msg)) return fail(rc, msg);
    if (!w || (!pos && !dist)) return fail(ATO_ERR_ARG, "null buffer");
    if (dist && !mesh) return fail(ATO_ERR_ARG, "distances need a mesh");
    if (cull != 0 && cull != 1) return fail(ATO_ERR_ARG, "cull must be 0 or 1");
    hipStream_t st = (hipStream_t)stream;
    const int S1 = ato::clearance_points(p.K1, samples);
    const size_t npts = (size_t)p.N * S1 * batch;
    if (!pos) {
        if (h->clear_pos_len < 3 * npts) {
            // the one allocation of this call path: hipFree waits for the work that still reads the old buffer
            (void)hipFree(h->d_clear_pos);
            h->d_clear_pos = nullptr;
            h->clear_pos_len = 0;
            ATO_HIP(hipMalloc((void**)&h->d_clear_pos, 3 * npts * sizeof(double)));
            h->clear_pos_len = 3 * npts;
        }
        pos = h->d_clear_pos;
    }
    ATO_HIP(h->clear_w.use(samples, (size_t)S1 * p.K1,
                           [&](double* wt) { ato::clearance_weights(p.tau, p.K1, samples, wt); }, st));
    const ato::ClearD a = ato::clearance_args(p, samples, h->clear_w.dev, h->line);
    const hipError_t e = ato::launch_clearance_pos(a, batch, layout, w, pos, st);
    if (e != hipSuccess) return fail(ATO_ERR_HIP, std::string("clearance launch: ") + hipGetErrorString(e));
    if (!dist) return ATO_OK;
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    return ato_mesh_signed_distance_strided(mesh, (int64_t)npts, pos, il ? 1 : 3, il ? (int64_t)npts : 1, dist, cull,
                                            stream);
}

extern "C" int ato_clearance(ato_handle* h, ato_mesh* mesh, int32_t batch, int32_t layout, const double* w,
                             int32_t samples, double* pos, double* dist, int32_t cull, void* stream) {
    ATO_NOEXCEPT_BODY(clearance_impl(h, mesh, batch, layout, w, samples, pos, dist, cull, stream))
}

static int audit_impl(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t samples,
                      const double* lb, const double* ub, int32_t bounds_per_instance, double* val, void* stream) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    const ato::ProbD& p = h->pd;
    const char* msg = "";
    if (int rc = ato::audit_check(p, h->d_line != nullptr, batch, layout, samples, lb != nullptr, ub != nullptr, &msg))
        return fail(rc, msg);
    if (!w || !val) return fail(ATO_ERR_ARG, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    const size_t len = (size_t)ato::clearance_points(p.K1, samples) * p.K1;
    ATO_HIP(h->audit_w.use(samples, 2 * len, [&](double* tab) {
        ato::clearance_weights(p.tau, p.K1, samples, tab);
        ato::audit_dweights(p.tau, p.C, p.K1, samples, tab + len);
    }, st));
    const ato::AuditD a =
        ato::audit_args(p, samples, h->audit_w.dev, h->audit_w.dev + len, h->line, lb, ub, bounds_per_instance);
    hipError_t e = hipErrorInvalidValue;
    ato::with_model(p, [&]<class M>() { e = ato::launch_audit<M>(a, batch, layout, w, val, st); });
    if (e != hipSuccess) return fail(ATO_ERR_HIP, std::string("audit launch: ") + hipGetErrorString(e));
    return ATO_OK;
}

extern "C" int ato_audit(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t samples,
                         const double* lb, const double* ub, int32_t bounds_per_instance, double* val, void* stream) {
    ATO_NOEXCEPT_BODY(audit_impl(h, batch, layout, w, samples, lb, ub, bounds_per_instance, val, stream))
}

static int gatecheck_set_gates_impl(ato_handle* h, const ato_gate_plane* planes, int32_t n) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    if (n < 0 || n > ato::GATE_MAX) return fail(ATO_ERR_ARG, "gate planes: n must be in [0, 64]");
    if (n > 0 && !planes) return fail(ATO_ERR_ARG, "null argument");
    std::vector<ato_gate_plane> use = n > 0 ? std::vector<ato_gate_plane>(planes, planes + n)
                                            : ato::gate_planes_of(h->L.gates);
    for (const ato_gate_plane& g : use)
        if (g.shape != ATO_GATE_CIRCLE && g.shape != ATO_GATE_SQUARE) return fail(ATO_ERR_ARG, "bad gate shape");
    ATO_HIP(hipDeviceSynchronize());      // a queued gate check may still read the planes these replace
    if (!use.empty() && use.size() <= (size_t)ato::GATE_MAX)
        ATO_HIP(hipMemcpy(h->d_gate_planes, use.data(), use.size() * sizeof(ato_gate_plane), hipMemcpyHostToDevice));
    h->n_gate_planes = (int32_t)use.size();
    h->gate_last[0] = -1;      // the records on the handle belong to other planes
    return ATO_OK;
}

extern "C" int ato_gatecheck_set_gates(ato_handle* h, const ato_gate_plane* planes, int32_t n) {
    ATO_NOEXCEPT_BODY(gatecheck_set_gates_impl(h, planes, n))
}

// grow a buffer of the handle to len doubles; hipFree waits for the work that still reads the old one
static int grow(double** buf, size_t* have, size_t len, const char* what) {
    if (*have >= len) return ATO_OK;
    (void)hipFree(*buf);
    *buf = nullptr;
    *have = 0;
    if (hipMalloc((void**)buf, len * sizeof(double)) != hipSuccess) return fail(ATO_ERR_HIP, what);
    *have = len;
    return ATO_OK;
}

static int gatecheck_impl(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t samples,
                          double axial_tol, double* val, void* stream, int32_t launches) {
    if (!h) return fail(ATO_ERR_ARG, "null handle");
    const ato::ProbD& p = h->pd;
    const char* msg = "";
    if (int rc = ato::gatecheck_check(p, h->d_line != nullptr, h->n_gate_planes, batch, layout, samples, axial_tol,
                                      &msg))
        return fail(rc, msg);
    if (!w || !val) return fail(ATO_ERR_ARG, "null buffer");
    if (launches < 1 || launches > 7) return fail(ATO_ERR_ARG, "launches must be in [1, 7]");
    hipStream_t st = (hipStream_t)stream;
    const int G = h->n_gate_planes, S1 = samples + 1;
    // a subset of the launches reads what a whole call left in the handle's buffers: only after one of this shape
    const int64_t shape[4] = {batch, layout, samples, G};
    if (launches != 7 && !std::equal(shape, shape + 4, h->gate_last))
        return fail(ATO_ERR_STATE, "a subset of the launches needs a whole ato_gatecheck call of the same shape before it");
    if (int rc = grow(&h->d_clear_pos, &h->clear_pos_len, (size_t)3 * p.N * S1 * batch,
                      "gate passage positions: out of device memory"))
        return rc;
    if (int rc = grow(&h->d_gate_part, &h->gate_part_len, (size_t)G * p.N * ato::GATE_PART * batch,
                      "gate passage records: out of device memory"))
        return rc;
    ATO_HIP(h->clear_w.use(samples, (size_t)S1 * p.K1,
                           [&](double* wt) { ato::clearance_weights(p.tau, p.K1, samples, wt); }, st));
    const ato::GateD a =
        ato::gatecheck_args(p, samples, h->clear_w.dev, h->line, h->d_gate_tau, h->d_gate_planes, G, axial_tol);
    hipError_t e = hipSuccess;
    if (launches & 1) e = ato::launch_clearance_pos(a.c, batch, layout, w, h->d_clear_pos, st);
    if (e == hipSuccess && (launches & 6))
        e = ato::launch_gatecheck(a, batch, layout, w, h->d_clear_pos, h->d_gate_part, val, st, launches >> 1);
    if (e != hipSuccess) return fail(ATO_ERR_HIP, std::string("gate passage launch: ") + hipGetErrorString(e));
    if (launches == 7) std::copy(shape, shape + 4, h->gate_last);
    return ATO_OK;
}

extern "C" int ato_gatecheck(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t samples,
                             double axial_tol, double* val, void* stream) {
    ATO_NOEXCEPT_BODY(gatecheck_impl(h, batch, layout, w, samples, axial_tol, val, stream, 7))
}

extern "C" int ato_gatecheck_launches(ato_handle* h, int32_t batch, int32_t layout, const double* w, int32_t samples,
                                      double axial_tol, double* val, void* stream, int32_t launches) {
    ATO_NOEXCEPT_BODY(gatecheck_impl(h, batch, layout, w, samples, axial_tol, val, stream, launches))
}

extern "C" int ato_eval(ato_handle* h, int32_t batch, int32_t layout, const double* w, double* g,
                        double* jac, double* f, double* grad_f, void* stream) {
    return eval_impl<double>(h, batch, layout, w, g, jac, f, grad_f, stream);
}

extern "C" int ato_eval_f32(ato_handle* h, int32_t batch, int32_t layout, const float* w, float* g,
                            float* jac, float* f, float* grad_f, void* stream) {
    return eval_impl<float>(h, batch, layout, w, g, jac, f, grad_f, stream);
}
