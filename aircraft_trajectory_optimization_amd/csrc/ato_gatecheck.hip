// ato_gatecheck.hip -- the gate-passage kernels (ato_gatecheck.hpp): one instantiation each, nothing depends on
// the model but the per-node width.
#include <hip/hip_runtime.h>
#include "ato_gatecheck.hpp"

namespace ato {

constexpr int GATE_BLOCK = 256;

// One thread per (gate, interval, instance): blockIdx.x is the (gate, interval) pair and blockIdx.y the block of
// instances, so the gate plane and tau sit behind uniform addresses (scalar loads) and, with the interleaved
// layout, a wave's loads of one position component and its stores of one record component are contiguous over
// its instances. The sample loop keeps two points in registers, not the interval's S + 1. Only lanes that see a
// sign change bisect: accepted divergence, few (gate, interval, instance) items have a crossing.
__global__ __launch_bounds__(GATE_BLOCK) void k_gate_cross(GateD a, int B, int layout, const double* __restrict__ w,
                                                           const double* __restrict__ pos,
                                                           double* __restrict__ part) {
    const int q = blockIdx.x, gi = q / a.c.N, n = q - gi * a.c.N;
    const int b = blockIdx.y * GATE_BLOCK + threadIdx.x;
    if (b >= B) return;
    const SampleGrid sg{a.c.N, a.c.S1, B, layout == ATO_LAYOUT_INTERLEAVED};
    double rec[GATE_PART];
    gate_interval(a, sg, gi, n, b, pos, sg.input(w, b, a.c.nw), sg.stride(), rec);
    double* out = part + part_at(a.c.N, B, gi, n, b);
#pragma unroll
    for (int c = 0; c < GATE_PART; ++c) out[(long)c * B] = rec[c];
}

// One thread per (gate, instance): blockIdx.x is the gate, blockIdx.y the block of instances.
__global__ __launch_bounds__(GATE_BLOCK) void k_gate_reduce(GateD a, int B, int layout, const double* __restrict__ w,
                                                            const double* __restrict__ part,
                                                            double* __restrict__ val) {
    const int gi = blockIdx.x;
    const int b = blockIdx.y * GATE_BLOCK + threadIdx.x;
    if (b >= B) return;
    const SampleGrid sg{a.c.N, a.c.S1, B, layout == ATO_LAYOUT_INTERLEAVED};
    double out[GATE_NCH];
    gate_reduce(a, gi, b, B, part, sg.input(w, b, a.c.nw), sg.stride(), out);
    gate_store(val, sg.il, a.G, B, gi, b, out);
}

// which: bit 0 the crossings, bit 1 the reduction (both in an ato_gatecheck call; one alone when a launch is timed)
hipError_t launch_gatecheck(const GateD& a, int B, int layout, const double* w, const double* pos, double* part,
                            double* val, hipStream_t st, int which) {
    dim3 grid;
    if (which & 1) {
        if (hipError_t e = sample_grid_dims(a.G, a.c.N, B, GATE_BLOCK, &grid)) return e;
        hipLaunchKernelGGL(k_gate_cross, grid, dim3(GATE_BLOCK), 0, st, a, B, layout, w, pos, part);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (which & 2) {
        if (hipError_t e = sample_grid_dims(a.G, 1, B, GATE_BLOCK, &grid)) return e;
        hipLaunchKernelGGL(k_gate_reduce, grid, dim3(GATE_BLOCK), 0, st, a, B, layout, w, part, val);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace ato
