// gatecheck_hostcheck.cpp -- TEST-ONLY CPU twin of the gate-passage kernels.
//
// Compiles csrc/ato_gatecheck.hpp with g++ (no HIP) and runs the same clearance_point(), gate_interval() and
// gate_reduce() the three launches run, one work item at a time in the kernels' own layouts, with the same
// argument checks, weight table and partial records. It is never loaded by the product package.
#include <string>
#include <vector>
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_layout.hpp"
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_gatecheck.hpp"

namespace {
thread_local std::string last_err;
}  // namespace

struct atog_handle {
    ato::Layout L;
    std::vector<double> line;
    ato::LineD ld{};
    std::vector<ato_gate_plane> planes;
};

extern "C" {

const char* atog_last_error() { return last_err.c_str(); }

int atog_create(const ato_problem_desc* d, atog_handle** out) {
    auto* h = new atog_handle();
    std::string e = h->L.build(*d);
    if (!e.empty()) {
        last_err = e;
        delete h;
        return ATO_ERR_ARG;
    }
    h->planes = ato::gate_planes_of(h->L.gates);
    *out = h;
    return ATO_OK;
}

void atog_destroy(atog_handle* h) { delete h; }

int atog_set_line(atog_handle* h, const ato_line_table* t) {
    if (h->L.p.frame == ato::GLOBAL) return ATO_OK;
    h->line = ato::line_pack(*t);
    h->ld = ato::line_view(*t, h->line.data());
    return ATO_OK;
}

// ato_gatecheck_set_gates (n = 0: the problem's own); n beyond 64 is kept so that the check can be reached
int atog_set_gates(atog_handle* h, const ato_gate_plane* planes, int n) {
    if (n < 0 || (n > 0 && !planes)) return ATO_ERR_ARG;
    h->planes = n > 0 ? std::vector<ato_gate_plane>(planes, planes + n) : ato::gate_planes_of(h->L.gates);
    return ATO_OK;
}

int atog_n_gates(const atog_handle* h) { return (int)h->planes.size(); }

// the planes in use: out [n_gates]
void atog_gates(const atog_handle* h, ato_gate_plane* out) {
    for (size_t i = 0; i < h->planes.size(); ++i) out[i] = h->planes[i];
}

// first row in g of every gate of the problem: rows [n_gates of the problem]
void atog_gate_rows(const atog_handle* h, int32_t* rows) {
    for (size_t t = 0; t + 3 < h->L.tail.size(); t += 4)
        if (h->L.tail[t] == ato::TAIL_GATE) rows[h->L.tail[t + 1]] = h->L.tail[t + 2];
}

// ato_gatecheck on host arrays (same layouts, same return codes)
int atog_gatecheck(const atog_handle* h, int B, int layout, const double* w, int samples, double axial_tol,
                   double* val) {
    const ato::ProbD& p = h->L.p;
    const char* msg = "";
    const int G = (int)h->planes.size();
    if (int rc = ato::gatecheck_check(p, !h->line.empty(), G, B, layout, samples, axial_tol, &msg)) {
        last_err = msg;
        return rc;
    }
    const int S1 = samples + 1;
    // exact sizes: an index past an end is a heap overflow a sanitizer sees
    std::vector<double> wt((size_t)S1 * p.K1), tau(p.tau, p.tau + p.K1);
    std::vector<double> pos((size_t)3 * p.N * S1 * B), part((size_t)G * p.N * ato::GATE_PART * B);
    ato::clearance_weights(p.tau, p.K1, samples, wt.data());
    const ato::GateD a = ato::gatecheck_args(p, samples, wt.data(), h->ld, tau.data(), h->planes.data(), G, axial_tol);
    const ato::SampleGrid g{p.N, S1, B, layout == ATO_LAYOUT_INTERLEAVED};
    for (int n = 0; n < p.N; ++n)
        for (int i = 0; i < S1; ++i)
            for (int b = 0; b < B; ++b) {
                double out[3];
                ato::clearance_point(a.c, n, i, g.input(w, b, p.nw), g.stride(), out);
                g.store<3>(pos.data(), n, i, b, out);
            }
    for (int gi = 0; gi < G; ++gi)
        for (int n = 0; n < p.N; ++n)
            for (int b = 0; b < B; ++b) {
                double rec[ato::GATE_PART];
                ato::gate_interval(a, g, gi, n, b, pos.data(), g.input(w, b, p.nw), g.stride(), rec);
                double* out = part.data() + ato::part_at(p.N, B, gi, n, b);
                for (int c = 0; c < ato::GATE_PART; ++c) out[(long)c * B] = rec[c];
            }
    for (int gi = 0; gi < G; ++gi)
        for (int b = 0; b < B; ++b) {
            double out[ato::GATE_NCH];
            ato::gate_reduce(a, gi, b, B, part.data(), g.input(w, b, p.nw), g.stride(), out);
            ato::gate_store(val, g.il, G, B, gi, b, out);
        }
    return ATO_OK;
}

}  // extern "C"
