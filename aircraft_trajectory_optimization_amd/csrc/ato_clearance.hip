// ato_clearance.hip -- the dense-position kernel (ato_clearance.hpp): one instantiation, nothing depends on
// the model but the per-node width.
#include <hip/hip_runtime.h>
#include "ato_clearance.hpp"

namespace ato {

constexpr int CLEAR_BLOCK = 256;

// One thread per (b, n, i) of the SampleGrid (ato_sample.hpp, which has the output layouts). blockIdx.x is the
// (interval, sample) pair and blockIdx.y the block of instances, so the weights of a block are one row of the
// table behind a uniform address (scalar loads) and, with the interleaved layout, a wave's loads of one source
// element and its stores of one component are contiguous over its instances. The spline pieces are gathered per
// lane: s is the instance's own.
__global__ __launch_bounds__(CLEAR_BLOCK) void k_clearance_pos(ClearD a, int B, int layout,
                                                              const double* __restrict__ w,
                                                              double* __restrict__ pos) {
    const int q = blockIdx.x, n = q / a.S1, i = q - n * a.S1;
    const int b = blockIdx.y * CLEAR_BLOCK + threadIdx.x;
    if (b >= B) return;
    const SampleGrid g{a.N, a.S1, B, layout == ATO_LAYOUT_INTERLEAVED};
    double out[3];
    clearance_point(a, n, i, g.input(w, b, a.nw), g.stride(), out);
    g.store<3>(pos, n, i, b, out);
}

hipError_t launch_clearance_pos(const ClearD& a, int B, int layout, const double* w, double* pos, hipStream_t st) {
    dim3 grid;
    if (hipError_t e = sample_grid_dims(a.N, a.S1, B, CLEAR_BLOCK, &grid)) return e;
    hipLaunchKernelGGL(k_clearance_pos, grid, dim3(CLEAR_BLOCK), 0, st, a, B, layout, w, pos);
    return hipGetLastError();
}

}  // namespace ato
