// ato_handle.hpp -- the opaque ato_handle of include/ato.h (library-internal).
#pragma once
#include <map>
#include <vector>
#include <hip/hip_runtime.h>
#include "ato_kernels.hpp"
#include "ato_replay.hpp"
#include "ato_remesh.hpp"
#include "ato_clearance.hpp"
#include "ato_audit.hpp"
#include "ato_gatecheck.hpp"

// A Lagrange weight table on the device, keyed by a substep or sample count. dev is allocated once (ato_create,
// sized for the largest key) and holds the table of the key last uploaded; the host tables it is uploaded from
// are made on first use and never rewritten or dropped (an upload may still be queued on a stream).
struct ato_weight_cache {
    double* dev = nullptr;
    int32_t key = -1;
    std::map<int32_t, std::vector<double>> host;
    // make dev hold the table of `key`: len doubles, written by fill(double*) the first time the key is seen,
    // uploaded on st only when the key changes; a warm call does nothing
    template <class Fill>
    hipError_t use(int32_t k, size_t len, Fill&& fill, hipStream_t st) {
        if (key == k) return hipSuccess;
        std::vector<double>& tab = host[k];
        if (tab.empty()) {
            tab.resize(len);
            fill(tab.data());
        }
        const hipError_t e = hipMemcpyAsync(dev, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) key = k;
        return e;
    }
};

struct ato_handle {
    ato::Layout L;
    int device = 0;
    ato::ProbD pd{};            // device-pointer copy of L.p (interval-major unit table)
    ato::ProbD pd_lf{};         // the same with the long-first unit table (batches <= lf_max_batch)
    int32_t lf_max_batch = 2048;
    // batches above lf_max_batch: the workgroup order runs eval_tile 64-instance chunks through every
    // unit before the next chunks start (0 = one pass per unit over the whole batch); tile_lf picks
    // the long-first unit table inside the tiles
    int32_t eval_tile = 8;
    bool tile_lf = true;
    double* d_geom = nullptr;
    double* d_node_s = nullptr;
    double* d_interval_s = nullptr;
    double* d_spheres = nullptr;
    double* d_cpc_wp = nullptr;
    ato_gate* d_gates = nullptr;
    int32_t* d_seg = nullptr;
    int32_t* d_tail = nullptr;
    int32_t* d_units = nullptr;
    int32_t* d_units_lf = nullptr;
    void* d_fpart = nullptr;    // [N][reserved] cost partials (double; reused for float)
    int32_t reserved = 0;
    std::vector<hipEvent_t> events;   // 3 per timed call
    int32_t timed_calls = 0;
    int32_t timing_stride = 1;        // events on every timing_stride-th evaluation
    int64_t timing_seen = 0;          // evaluations since ato_timing
    // Hessian of the Lagrangian (built on first use)
    bool hess_ready = false;
    ato::HessLayout HL;
    int32_t *d_color = nullptr, *d_take_e = nullptr, *d_take_r = nullptr;
    int32_t *d_tk_ptr = nullptr, *d_tk_ent = nullptr, *d_tk_row = nullptr;
    int32_t *d_tkf_ptr = nullptr, *d_tkf_ent = nullptr, *d_tkf_row = nullptr;
    uint32_t* d_amask = nullptr;
    bool hess_mask = false;           // ATO_HESS_MASK=1: the masked colour passes (HessLayout::amask)
    int32_t* d_take_off = nullptr;    // device copy of HL.take_off (the colour of a take, grouped passes)
    // seeded-pass scratch for hess_colors colours at hess_reserved instances: [colour][nnz][B] / [colour][nw][B]
    // (a launch runs as many colours as fit at its batch: fewer, larger launches)
    double* d_dJ = nullptr;
    double* d_dgf = nullptr;
    int32_t hess_reserved = 0;
    int32_t hess_colors = 0;
    // replay (ato_replay.hpp): lift table [N+1][12] (parametric problems) and the weight table [2 S + 1][K + 1]
    // by substep count S
    double* d_lift = nullptr;
    ato_weight_cache replay_w;
    // mesh transfer INTO this problem (ato_remesh.hpp): one weight table [r][K' + 1][K + 1] per source
    // discretisation, keyed by (r, the source's tau_0 .. tau_K); allocated and uploaded by the first call
    // with that key, on that call's stream, and never rewritten or freed before the handle
    struct RemeshTable {
        std::vector<double> host;
        double* dev = nullptr;
    };
    std::map<std::vector<double>, RemeshTable> remesh_tabs;
    // clearance (ato_clearance.hpp): the centreline's two piecewise cubics (ato_clearance_set_line, one
    // allocation: line_pack), the weight table [S1][K + 1] by sample count and the position buffer of calls that
    // pass pos = NULL (grown only when a call needs more)
    double* d_line = nullptr;
    ato::LineD line{};
    ato_weight_cache clear_w;
    double* d_clear_pos = nullptr;
    size_t clear_pos_len = 0;
    // audit (ato_audit.hpp): value and derivative weight tables by sample count, back to back
    ato_weight_cache audit_w;
    // gate passage (ato_gatecheck.hpp): tau_0 .. tau_K and up to GATE_MAX planes in one allocation (ato_create),
    // the planes in use (the problem's own unless ato_gatecheck_set_gates replaced them) and the partial records
    // [G][N][GATE_PART][B] (grown only when a call needs more). Positions: d_clear_pos and clear_w above.
    double* d_gate_tau = nullptr;
    ato_gate_plane* d_gate_planes = nullptr;
    int32_t n_gate_planes = 0;
    double* d_gate_part = nullptr;
    size_t gate_part_len = 0;
    int64_t gate_last[4] = {-1, -1, -1, -1};   // batch, layout, samples, G of the last whole call (ato_gatecheck_launches)
};
