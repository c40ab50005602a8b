// ato_remesh.hip -- the mesh-transfer kernel (ato_remesh.hpp): one instantiation, nothing depends on the model.
#include <hip/hip_runtime.h>
#include "ato_remesh.hpp"

namespace ato {

constexpr int REMESH_BLOCK = 256;

// One thread per work item. Interleaved: the instance is fastest, so a wave's loads and stores of one
// element are contiguous over its instances. Instance-major: the variable is fastest, so they are
// contiguous over a node's variables. cols (or NULL: identity) maps a destination column to its source
// column; an entry outside [0, Bs) skips the column.
__global__ __launch_bounds__(REMESH_BLOCK) void k_remesh(RemeshD a, int Bs, int Bd, int layout,
                                                         const double* __restrict__ w_src,
                                                         const int32_t* __restrict__ cols,
                                                         double* __restrict__ w_dst) {
    const long per = (long)a.N * (a.NV + 1);
    const long t = (long)blockIdx.x * REMESH_BLOCK + threadIdx.x;
    if (t >= per * Bd) return;
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    const int b = (int)(il ? t % Bd : t / per);
    const int q = (int)(il ? t / Bd : t % per);
    const int n = q / (a.NV + 1), v = q % (a.NV + 1);
    const int bs = cols ? cols[b] : b;
    if (bs < 0 || bs >= Bs) return;
    const double* ws = w_src + (il ? (long)bs : (long)bs * a.nws);
    double* wd = w_dst + (il ? (long)b : (long)b * a.nwd);
    remesh_item(a, n, v, ws, il ? (long)Bs : 1L, wd, il ? (long)Bd : 1L);
}

hipError_t launch_remesh(const RemeshD& a, int Bs, int Bd, int layout, const double* w_src, const int32_t* cols,
                         double* w_dst, hipStream_t st) {
    const long items = (long)a.N * (a.NV + 1) * Bd;
    const long blocks = (items + REMESH_BLOCK - 1) / REMESH_BLOCK;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_remesh, dim3((unsigned)blocks), dim3(REMESH_BLOCK), 0, st, a, Bs, Bd, layout, w_src, cols,
                       w_dst);
    return hipGetLastError();
}

}  // namespace ato
