// ato_clearance.hip -- the dense-position kernel (ato_clearance.hpp): one instantiation, nothing depends on
// the model but the per-node width.
#include <hip/hip_runtime.h>
#include "ato_clearance.hpp"

namespace ato {

constexpr int CLEAR_BLOCK = 256;

// One thread per (b, n, i). blockIdx.x is the (interval, sample) pair and blockIdx.y the block of instances,
// so the weights of a block are one row of the table behind a uniform address (scalar loads) and, with the
// interleaved layout, a wave's loads of one source element and its stores of one component are contiguous
// over its instances. The spline pieces are gathered per lane: s is the instance's own.
//   interleaved:     pos[c N S1 B + (n S1 + i) B + b]
//   instance-major:  pos[((b N + n) S1 + i) 3 + c]
__global__ __launch_bounds__(CLEAR_BLOCK) void k_clearance_pos(ClearD a, int B, int layout,
                                                              const double* __restrict__ w,
                                                              double* __restrict__ pos) {
    const int q = blockIdx.x, n = q / a.S1, i = q - n * a.S1;
    const int b = blockIdx.y * CLEAR_BLOCK + threadIdx.x;
    if (b >= B) return;
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    double out[3];
    clearance_point(a, n, i, w + (il ? (long)b : (long)b * a.nw), il ? (long)B : 1L, out);
    if (il) {
        const long plane = (long)a.N * a.S1 * B, p = (long)q * B + b;
#pragma unroll
        for (int c = 0; c < 3; ++c) pos[c * plane + p] = out[c];
    } else {
        const long p = ((long)b * a.N + n) * a.S1 + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) pos[p * 3 + c] = out[c];
    }
}

hipError_t launch_clearance_pos(const ClearD& a, int B, int layout, const double* w, double* pos, hipStream_t st) {
    const long gx = (long)a.N * a.S1, gy = ((long)B + CLEAR_BLOCK - 1) / CLEAR_BLOCK;
    if (gx > 0x7fffffffL || gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_clearance_pos, dim3((unsigned)gx, (unsigned)gy), dim3(CLEAR_BLOCK), 0, st, a, B, layout, w,
                       pos);
    return hipGetLastError();
}

}  // namespace ato
