// ato_warmstart.hip -- the warm-start kernels (ato_warmstart.hpp): the poses and closed / open lines are template
// parameters, so a kernel carries no pose branch and holds only the live rotation matrix in registers.
#include <hip/hip_runtime.h>
#include "ato_warmstart.hpp"

namespace ato {

constexpr int WS_BLOCK = 256;      // pass 1: instances per workgroup
constexpr int WS_LANES = 64;       // pass 2: instances per workgroup, one wave per segment

// info [3 x B] = 0 before pass 1 flags into it (a kernel, not a memset node: the call may be captured in a graph)
__global__ __launch_bounds__(WS_BLOCK) void k_ws_clear(int B, double* __restrict__ info) {
    const long t = (long)blockIdx.x * WS_BLOCK + threadIdx.x;
    if (t < 3L * B) info[t] = 0.0;
}

// Pass 1. One thread per (node, instance) of the SampleGrid with S1 = K1: blockIdx.x is the node, blockIdx.y the
// block of instances, so the two geometry rows of a block sit behind uniform addresses (scalar loads) and, with the
// interleaved layout, a wave's loads of one point-mass element and its stores of one drone element are contiguous
// over its instances. No LDS. A degenerate node stores 2 into the instance's status: every such store of a call
// writes the same value, so their order does not matter.
template <int ATT, bool CLOSED>
__global__ __launch_bounds__(WS_BLOCK) void k_ws_nodes(WarmD a, int B, int layout, const double* __restrict__ w_point,
                                                       double* __restrict__ w_drone, double* __restrict__ hlb,
                                                       double* __restrict__ hub, double* __restrict__ info) {
    const int p = blockIdx.x, n = p / a.K1;
    const int b = blockIdx.y * WS_BLOCK + threadIdx.x;
    if (b >= B) return;
    const SampleGrid g{a.N, a.K1, B, layout == ATO_LAYOUT_INTERLEAVED};
    const double* wp = g.input(w_point, b, a.nwp);
    double* wd = w_drone + (g.il ? (long)b : (long)b * a.nwd);
    const long s = g.stride();
    if (p == n * a.K1) {
        const long hb = g.il ? (long)b : (long)b * a.N;
        ws_step(n, wp, s, wd, s, hlb ? hlb + hb : nullptr, hub ? hub + hb : nullptr);
    }
    if (ws_node<ATT, CLOSED>(a, p, wp, s, wd, s)) info[g.il ? (long)b : 3L * b] = 2.0;
}

// Pass 2. A workgroup is 64 instances x WS_G segments of the lap: threadIdx.x is the instance (adjacent lanes,
// adjacent instances), threadIdx.y the segment, one wave each. Every thread composes the maps of its segment,
// the WS_G x 64 maps of the workgroup meet in LDS (one byte each), every thread folds the maps before its own
// segment and walks its segment again to change it in place. The raw attitude before a segment is read before
// the barrier: after it, the segment before may already have changed that node. No atomics, nothing between
// workgroups.
template <int ATT>
__global__ __launch_bounds__(WS_LANES * WS_G) void k_ws_chain(WarmD a, int B, int layout,
                                                              double* __restrict__ w_drone,
                                                              double* __restrict__ info) {
    __shared__ unsigned char maps[WS_G][WS_LANES];
    const int lane = threadIdx.x, seg = threadIdx.y;
    const int b = blockIdx.x * WS_LANES + lane;
    const bool live = b < B;
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    double* wd = w_drone + (il ? (long)b : (long)b * a.nwd);
    const long s = il ? (long)B : 1L;
    double prev[4] = {0.0, 0.0, 0.0, 0.0};
    maps[seg][lane] = (unsigned char)(live ? ws_segment_map<ATT>(a, seg, wd, s, prev) : WS_MAP_ID);
    __syncthreads();
    if (!live) return;
    unsigned st = 0;
    for (int g = 0; g < seg; ++g) st = ws_map_at(maps[g][lane], st);
    ws_segment_apply<ATT>(a, seg, st, prev, wd, s, info + (il ? (long)b : 3L * b), il ? (long)B : 1L);
}

template <int ATT, bool CLOSED>
static hipError_t launch_nodes(const WarmD& a, int B, int layout, const double* w_point, double* w_drone,
                               double* hlb, double* hub, double* info, hipStream_t st) {
    dim3 grid;
    if (hipError_t e = sample_grid_dims(a.N, a.K1, B, WS_BLOCK, &grid)) return e;
    hipLaunchKernelGGL((k_ws_nodes<ATT, CLOSED>), grid, dim3(WS_BLOCK), 0, st, a, B, layout, w_point, w_drone, hlb,
                       hub, info);
    return hipGetLastError();
}

template <int ATT>
static hipError_t launch_pose(const WarmD& a, int B, int layout, const double* w_point, double* w_drone, double* hlb,
                              double* hub, double* info, hipStream_t st) {
    const hipError_t e = a.closed ? launch_nodes<ATT, true>(a, B, layout, w_point, w_drone, hlb, hub, info, st)
                                  : launch_nodes<ATT, false>(a, B, layout, w_point, w_drone, hlb, hub, info, st);
    if (e != hipSuccess) return e;
    if constexpr (ATT != ATO_ATT_DCM) {
        const long blocks = ((long)B + WS_LANES - 1) / WS_LANES;
        hipLaunchKernelGGL((k_ws_chain<ATT>), dim3((unsigned)blocks), dim3(WS_LANES, WS_G), 0, st, a, B, layout,
                           w_drone, info);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t launch_warmstart(const WarmD& a, int att, int B, int layout, const double* w_point, double* w_drone,
                            double* hlb, double* hub, double* info, hipStream_t st) {
    hipLaunchKernelGGL(k_ws_clear, dim3((unsigned)((3L * B + WS_BLOCK - 1) / WS_BLOCK)), dim3(WS_BLOCK), 0, st, B,
                       info);
    if (hipError_t e = hipGetLastError()) return e;
    if (att == ATO_ATT_ESP) return launch_pose<ATO_ATT_ESP>(a, B, layout, w_point, w_drone, hlb, hub, info, st);
    if (att == ATO_ATT_YPR) return launch_pose<ATO_ATT_YPR>(a, B, layout, w_point, w_drone, hlb, hub, info, st);
    if (att == ATO_ATT_DCM) return launch_pose<ATO_ATT_DCM>(a, B, layout, w_point, w_drone, hlb, hub, info, st);
    return hipErrorInvalidValue;
}

}  // namespace ato
