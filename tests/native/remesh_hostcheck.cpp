// remesh_hostcheck.cpp -- TEST-ONLY CPU twin of the mesh-transfer kernel.
//
// Compiles csrc/ato_remesh.hpp with g++ (no HIP) and runs the same remesh_item() the device kernel
// runs, one (instance, interval, variable) at a time, with the same argument checks and the same
// weight table. It is never loaded by the product package.
#include <string>
#include <vector>
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_layout.hpp"
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_remesh.hpp"

namespace {
thread_local std::string last_err;
}  // namespace

struct atom_handle {
    ato::Layout L;
};

extern "C" {

const char* atom_last_error() { return last_err.c_str(); }

int atom_create(const ato_problem_desc* d, atom_handle** out) {
    auto* h = new atom_handle();
    std::string e = h->L.build(*d);
    if (!e.empty()) {
        last_err = e;
        delete h;
        return ATO_ERR_ARG;
    }
    *out = h;
    return ATO_OK;
}

void atom_destroy(atom_handle* h) { delete h; }

// the weight table of ato_remesh(src, dst): wt [r][K' + 1][K + 1], r = N' / N (the caller checked the pair)
void atom_weights(const atom_handle* src, const atom_handle* dst, double* wt) {
    const ato::ProbD &s = src->L.p, &d = dst->L.p;
    ato::remesh_weights(s.tau, s.K1, d.tau, d.K1, d.N / s.N, wt);
}

// ato_remesh on host arrays (same layouts, same column map, same return codes)
int atom_remesh(const atom_handle* src, const atom_handle* dst, int Bs, int Bd, int layout, const double* w_src,
                const int32_t* cols, double* w_dst) {
    const ato::ProbD &s = src->L.p, &d = dst->L.p;
    const char* msg = "";
    if (int rc = ato::remesh_check(s, d, Bs, Bd, cols != nullptr, layout, &msg)) {
        last_err = msg;
        return rc;
    }
    const int r = d.N / s.N;
    std::vector<double> wt((size_t)r * d.K1 * s.K1);
    ato::remesh_weights(s.tau, s.K1, d.tau, d.K1, r, wt.data());
    const ato::RemeshD a = ato::remesh_args(s, d, wt.data());
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    for (int b = 0; b < Bd; ++b) {
        const int bs = cols ? cols[b] : b;
        if (bs < 0 || bs >= Bs) continue;
        const double* ws = w_src + (il ? (long)bs : (long)bs * a.nws);
        double* wd = w_dst + (il ? (long)b : (long)b * a.nwd);
        for (int n = 0; n < a.N; ++n)
            for (int v = 0; v <= a.NV; ++v) ato::remesh_item(a, n, v, ws, il ? (long)Bs : 1L, wd, il ? (long)Bd : 1L);
    }
    return ATO_OK;
}

}  // extern "C"
