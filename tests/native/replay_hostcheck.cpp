// replay_hostcheck.cpp -- TEST-ONLY CPU twin of the replay kernel.
//
// Compiles csrc/ato_replay.hpp with g++ (no HIP) and runs the same replay_interval() the device
// kernel runs, one (instance, interval) at a time, with the same argument checks and the same
// weight table. It is never loaded by the product package.
#include <string>
#include <vector>
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_layout.hpp"
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_replay.hpp"

namespace {

struct HostW {
    const double* w;
    long ws;
    double operator()(int col) const { return w[(long)col * ws]; }
};

thread_local std::string last_err;

}  // namespace

struct ator_handle {
    ato::Layout L;
    std::vector<double> lift;
};

extern "C" {

const char* ator_last_error() { return last_err.c_str(); }

int ator_create(const ato_problem_desc* d, ator_handle** out) {
    auto* h = new ator_handle();
    std::string e = h->L.build(*d);
    if (!e.empty()) {
        last_err = e;
        delete h;
        return ATO_ERR_ARG;
    }
    *out = h;
    return ATO_OK;
}

void ator_destroy(ator_handle* h) { delete h; }

int ator_set_lift(ator_handle* h, const double* lift) {
    if (h->L.p.frame == ato::GLOBAL) return ATO_OK;
    h->lift.assign(lift, lift + (size_t)(h->L.p.N + 1) * ato::REPLAY_LIFT_W);
    return ATO_OK;
}

// the weight table of ato_replay for this problem: lw [2 S + 1][K + 1]
void ator_weights(const ator_handle* h, int S, double* lw) { ato::replay_weights(h->L.p.tau, h->L.p.K1, S, lw); }

// ato_replay on host arrays (same layouts, same return codes)
int ator_replay(const ator_handle* h, int B, int layout, const double* w, int S, double* zsim, double* err,
                double* traj) {
    const ato::ProbD& p = h->L.p;
    const char* msg = "";
    if (int rc = ato::replay_check(p, !h->lift.empty(), B, layout, S, &msg)) {
        last_err = msg;
        return rc;
    }
    std::vector<double> lw((size_t)(2 * S + 1) * p.K1);
    ato::replay_weights(p.tau, p.K1, S, lw.data());
    const ato::ReplayD r{S, traj ? 1 : 0, lw.data(), h->lift.empty() ? nullptr : h->lift.data()};
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    const long st = il ? B : 1;
    ato::with_model(p, [&]<class M>() {
        if constexpr (!ato::GlobalOf<M>::relative) {
            for (int n = 0; n < p.N; ++n)
                for (int b = 0; b < B; ++b) {
                    const HostW W{w + (il ? (long)b : (long)b * p.nw), st};
                    double* zs = zsim + (il ? (long)b : (long)b * p.N * p.NZ);
                    double* er = err + (il ? (long)b : (long)b * p.N * 4);
                    double* tj = traj ? traj + (il ? (long)b : (long)b * p.N * S * p.NZ) : nullptr;
                    ato::replay_interval<M>(p, r, n, W, zs, er, tj, st);
                }
        }
    });
    return ATO_OK;
}

}  // extern "C"
