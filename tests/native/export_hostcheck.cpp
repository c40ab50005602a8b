// export_hostcheck.cpp -- TEST-ONLY CPU twin of the export kernels: csrc/ato_export.hpp compiled with g++ (no HIP),
// the same ATO_HD functions and argument check the three launches run, one work item at a time in the kernels' own
// layouts; every first walk of an instance comes before its second walks, as the barrier orders them. Never loaded
// by the product package. With -DEXPORT_MAIN a stand-alone program over hand-made problems (the sanitizer build).
#include <vector>
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_layout.hpp"
#include "../../aircraft_trajectory_optimization_amd/csrc/ato_export.hpp"

struct atoe_handle {
    ato::Layout L;
    std::vector<double> line;
    ato::LineD ld{};
};

extern "C" {

int atoe_create(const ato_problem_desc* d, atoe_handle** out) {
    *out = new atoe_handle();
    return (*out)->L.build(*d).empty() ? ATO_OK : ATO_ERR_ARG;
}

void atoe_set_line(atoe_handle* h, const ato_line_table* t) {
    h->line = ato::line_pack(*t);
    h->ld = ato::line_view(*t, h->line.data());
}

// ato_export on host arrays (same layouts, same return codes)
int atoe_export(const atoe_handle* h, int B, int layout, const double* w, int n_times, const double* times,
                int relative, double* nodes, double* state) {
    const ato::ProbD& p = h->L.p;
    const char* msg = "";
    if (int rc = ato::export_check(p, !h->line.empty(), B, layout, n_times, w != nullptr, times != nullptr,
                                   nodes != nullptr, state != nullptr, &msg))
        return rc;
    // exact sizes: an index past an end is a heap overflow a sanitizer sees
    std::vector<double> ts((size_t)(p.N + 1) * B), tau(p.tau, p.tau + p.K1), D(p.D, p.D + p.K1);
    const ato::ExportD a = ato::export_args(p, n_times, relative, tau.data(), D.data(), times, ts.data(), h->ld);
    const ato::SampleGrid g{n_times, 1, B, layout == ATO_LAYOUT_INTERLEAVED};
    for (int b = 0; b < B; ++b) ato::export_tstart(p.N, g.input(w, b, p.nw), g.stride(), ts.data() + b, B);
    ato::with_model(p, [&]<class M>() {
        constexpr int NV = M::NZ + 2 * M::NU;
        for (int j = 0; j < n_times; ++j)
            for (int b = 0; b < B; ++b) {
                double v[NV], out[ato::EXPORT_NCH];
                ato::export_interp<NV>(a, times[j], ts.data() + b, B, g.input(w, b, p.nw), g.stride(), v, out);
                if (nodes) g.store<NV>(nodes, j, 0, b, v);
                if (!state) continue;
                ato::export_lift<M>(a.line, v, out);
                g.store<ato::EXPORT_NCH>(state, j, 0, b, out);
            }
        if (!M::IS_DRONE || !state) return;
        const int G = ato::export_segments(n_times, B);
        for (int b = 0; b < B; ++b) {
            unsigned maps[ato::EXPORT_GMAX], s = 0;
            double prev[ato::EXPORT_GMAX][4] = {};
            for (int q = 0; q < G; ++q) maps[q] = ato::export_segment_map(state, g.il, n_times, B, b, G, q, prev[q]);
            for (int q = 0; q < G; ++q) {
                ato::export_segment_apply(state, g.il, n_times, B, b, G, q, s, prev[q]);
                s = ato::export_map_at(maps[q], s);
            }
        }
    });
    return ATO_OK;
}

}  // extern "C"

#ifdef EXPORT_MAIN
// The three poses and the point mass in the global frame, both layouts, B = 67 across a wave, 131 times (sixteen
// segments, the last one empty) before, inside and after the lap, one of them NaN; nodes in one layout only.
#include <cmath>
#include <cstdio>

int main() {
    const int N = 3, K = 2, B = 67, T = 131;
    for (int v = 0; v < 8; ++v) {
        ato_problem_desc d{};
        d.abi_version = ATO_ABI_VERSION;
        d.model = v < 6 ? ATO_MODEL_DRONE : ATO_MODEL_POINT;
        d.attitude = v / 2 == 1 ? ATO_ATT_YPR : (v / 2 == 2 ? ATO_ATT_DCM : ATO_ATT_ESP);
        d.frame = ATO_FRAME_GLOBAL, d.global_r = 1, d.transcription = ATO_TRANS_COLLOCATION;
        d.N = N, d.K = K, d.closed = 1, d.cleanly_closed = 1;
        d.m = d.g = d.T_max = d.l = d.kt = 1.0;
        for (int i = 0; i < 3; ++i) d.b[i] = d.I[i] = d.bw[i] = 1.0;
        for (int k = 0; k <= K; ++k) d.tau[k] = (double)k / (K + 1), d.Bq[k] = d.D[k] = 1.0 / (K + 1);
        atoe_handle* h = nullptr;
        if (atoe_create(&d, &h)) return 1;
        std::vector<double> w((size_t)h->L.p.nw * B), times(T), nodes((size_t)h->L.p.NV * T * B),
            state((size_t)ato::EXPORT_NCH * T * B);
        for (size_t i = 0; i < w.size(); ++i) w[i] = 0.3 + std::fabs(std::sin(0.37 * (double)i));
        for (int j = 0; j < T; ++j) times[j] = j == 2 ? std::nan("") : -0.1 + 1.5 * j / T;
        const int rc = atoe_export(h, B, v % 2, w.data(), T, times.data(), 0, v % 2 ? nullptr : nodes.data(), state.data());
        double sum = 0.0;
        for (double x : state) sum += x == x ? x : 1.0;
        std::printf("variant %d layout %d: rc %d checksum %.17g\n", v / 2, v % 2, rc, sum);
        delete h;
        if (rc != 0) return 1;
    }
    return 0;
}
#endif
