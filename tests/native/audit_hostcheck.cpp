// audit_hostcheck.cpp -- TEST-ONLY CPU twin of the between-node audit kernel.
//
// Compiles csrc/ato_audit.hpp with g++ (no HIP) and runs the same audit_point() the kernel runs, one (instance,
// interval, sample) at a time, with the same argument checks and weight tables. It is never loaded by the
// product package.
#include <string>
#include <vector>
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_layout.hpp"
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_audit.hpp"

namespace {
thread_local std::string last_err;
}  // namespace

struct atoa_handle {
    ato::Layout L;
    std::vector<double> line;
    ato::LineD ld{};
};

extern "C" {

const char* atoa_last_error() { return last_err.c_str(); }

int atoa_create(const ato_problem_desc* d, atoa_handle** out) {
    auto* h = new atoa_handle();
    std::string e = h->L.build(*d);
    if (!e.empty()) {
        last_err = e;
        delete h;
        return ATO_ERR_ARG;
    }
    *out = h;
    return ATO_OK;
}

void atoa_destroy(atoa_handle* h) { delete h; }

int atoa_set_line(atoa_handle* h, const ato_line_table* t) {
    if (h->L.p.frame == ato::GLOBAL) return ATO_OK;
    const size_t nx = (size_t)t->n_xc, nr = (size_t)t->n_ry;
    std::vector<double>& b = h->line;
    b.clear();
    b.insert(b.end(), t->xc_knots, t->xc_knots + nx);
    b.insert(b.end(), t->xc_coef, t->xc_coef + (nx + 1) * 12);
    b.insert(b.end(), t->ry_knots, t->ry_knots + nr);
    b.insert(b.end(), t->ry_coef, t->ry_coef + (nr + 1) * 12);
    const double* d = b.data();
    h->ld = ato::LineD{t->n_xc, t->n_ry, d, d + nx, d + nx + (nx + 1) * 12, d + nx + (nx + 1) * 12 + nr};
    return ATO_OK;
}

// the two weight tables of ato_audit for this problem: wt, dw [S1][K + 1]
void atoa_weights(const atoa_handle* h, int samples, double* wt, double* dw) {
    ato::clearance_weights(h->L.p.tau, h->L.p.K1, samples, wt);
    ato::audit_dweights(h->L.p.tau, h->L.p.C, h->L.p.K1, samples, dw);
}

// first row in g of every node's segment of `kind` (ato::SegKind; -1: none)
void atoa_seg_rows(const atoa_handle* h, int kind, int32_t* rows) {
    for (int q = 0; q < h->L.p.P; ++q) rows[q] = h->L.seg[((size_t)q * ato::NSEG + kind) * 2];
}

// the node geometry of audit_geom at s[0..n): out [n][13] = Rp (9), ks, ky, kn, mag
void atoa_geom(const atoa_handle* h, int n, const double* s, double* out) {
    for (int i = 0; i < n; ++i) {
        ato::NodeGeom<double> G;
        ato::audit_geom(h->ld, s[i], G);
        for (int c = 0; c < 9; ++c) out[i * 13 + c] = G.Rp[c];
        out[i * 13 + 9] = G.ks;
        out[i * 13 + 10] = G.ky;
        out[i * 13 + 11] = G.kn;
        out[i * 13 + 12] = G.mag;
    }
}

// ato_audit on host arrays (same layouts, same return codes)
int atoa_audit(const atoa_handle* h, int B, int layout, const double* w, int samples, const double* lb,
               const double* ub, int bounds_per_instance, double* val) {
    const ato::ProbD& p = h->L.p;
    const char* msg = "";
    if (int rc = ato::audit_check(p, !h->line.empty(), B, layout, samples, lb != nullptr, ub != nullptr, &msg)) {
        last_err = msg;
        return rc;
    }
    const int S1 = ato::clearance_points(p.K1, samples);
    std::vector<double> wt((size_t)S1 * p.K1), dw((size_t)S1 * p.K1);
    ato::clearance_weights(p.tau, p.K1, samples, wt.data());
    ato::audit_dweights(p.tau, p.C, p.K1, samples, dw.data());
    const ato::AuditD a = ato::audit_args(p, samples, wt.data(), dw.data(), h->ld, lb, ub, bounds_per_instance);
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    const long plane = (long)a.N * S1 * B;
    ato::with_model(p, [&]<class M>() {
        for (int n = 0; n < a.N; ++n)
            for (int i = 0; i < S1; ++i)
                for (int b = 0; b < B; ++b) {
                    double out[ato::AUDIT_NCH];
                    ato::audit_point<M>(a, n, i, b, B, il, w + (il ? (long)b : (long)b * a.nw), il ? (long)B : 1L, out);
                    for (int c = 0; c < ato::AUDIT_NCH; ++c) {
                        if (il) val[c * plane + ((long)n * S1 + i) * B + b] = out[c];
                        else val[(((long)b * a.N + n) * S1 + i) * ato::AUDIT_NCH + c] = out[c];
                    }
                }
    });
    return ATO_OK;
}

}  // extern "C"
