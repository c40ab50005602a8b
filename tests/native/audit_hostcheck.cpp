// audit_hostcheck.cpp -- TEST-ONLY CPU twin of the between-node audit kernel.
//
// Compiles csrc/ato_audit.hpp with g++ (no HIP) and runs the same audit_point() the kernel runs, one (instance,
// interval, sample) of the kernel's own SampleGrid (csrc/ato_sample.hpp) at a time, with the same argument checks
// and weight tables. It is never loaded by the
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
    h->line = ato::line_pack(*t);
    h->ld = ato::line_view(*t, h->line.data());
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
    const size_t len = (size_t)ato::clearance_points(p.K1, samples) * p.K1;
    std::vector<double> wt(len), dw(len);
    ato::clearance_weights(p.tau, p.K1, samples, wt.data());
    ato::audit_dweights(p.tau, p.C, p.K1, samples, dw.data());
    const ato::AuditD a = ato::audit_args(p, samples, wt.data(), dw.data(), h->ld, lb, ub, bounds_per_instance);
    const ato::SampleGrid g{a.N, a.S1, B, layout == ATO_LAYOUT_INTERLEAVED};
    ato::with_model(p, [&]<class M>() {
        for (int n = 0; n < a.N; ++n)
            for (int i = 0; i < a.S1; ++i)
                for (int b = 0; b < B; ++b) {
                    double out[ato::AUDIT_NCH];
                    ato::audit_point<M>(a, n, i, b, B, g.il, g.input(w, b, a.nw), g.stride(), out);
                    g.store<ato::AUDIT_NCH>(val, n, i, b, out);
                }
    });
    return ATO_OK;
}

}  // extern "C"
