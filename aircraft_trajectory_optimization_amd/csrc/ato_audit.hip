// ato_audit.hip -- the between-node audit kernel (ato_audit.hpp), one instantiation per model variant.
#include <hip/hip_runtime.h>
#include "ato_audit.hpp"

namespace ato {

constexpr int AUDIT_BLOCK = 256;

// One thread per (b, n, i), the grid of k_clearance_pos: blockIdx.x is the (interval, sample) pair and
// blockIdx.y the block of instances, so both weight rows of a block sit behind a uniform address (scalar
// loads) and, with the interleaved layout, a wave's loads of one source element and its stores of one channel
// are contiguous over its instances. The spline pieces are gathered per lane: s is the instance's own.
//   interleaved:     val[c N S1 B + (n S1 + i) B + b]
//   instance-major:  val[(((b N + n) S1 + i) NCH + c]
// One wave per SIMD at 256 threads: the whole register file is the thread's (no scratch, no LDS; the listing
// is profiles/audit/kernel_resource_usage.txt).
template <class M>
__global__ __launch_bounds__(AUDIT_BLOCK) void k_audit(AuditD a, int B, int layout, const double* __restrict__ w,
                                                       double* __restrict__ val) {
    const int q = blockIdx.x, n = q / a.S1, i = q - n * a.S1;
    const int b = blockIdx.y * AUDIT_BLOCK + threadIdx.x;
    if (b >= B) return;
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    double out[AUDIT_NCH];
    audit_point<M>(a, n, i, b, B, il, w + (il ? (long)b : (long)b * a.nw), il ? (long)B : 1L, out);
    if (il) {
        const long plane = (long)a.N * a.S1 * B, p = (long)q * B + b;
#pragma unroll
        for (int c = 0; c < AUDIT_NCH; ++c) val[c * plane + p] = out[c];
    } else {
        const long p = ((long)b * a.N + n) * a.S1 + i;
#pragma unroll
        for (int c = 0; c < AUDIT_NCH; ++c) val[p * AUDIT_NCH + c] = out[c];
    }
}

template <class M>
hipError_t launch_audit(const AuditD& a, int B, int layout, const double* w, double* val, hipStream_t st) {
    const long gx = (long)a.N * a.S1, gy = ((long)B + AUDIT_BLOCK - 1) / AUDIT_BLOCK;
    if (gx > 0x7fffffffL || gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_audit<M>), dim3((unsigned)gx, (unsigned)gy), dim3(AUDIT_BLOCK), 0, st, a, B, layout, w,
                       val);
    return hipGetLastError();
}

#define ATO_AUDIT_INST(...) \
    template hipError_t launch_audit<__VA_ARGS__>(const AuditD&, int, int, const double*, double*, hipStream_t);
ATO_AUDIT_INST(DroneModel<ESP, GLOBAL>)
ATO_AUDIT_INST(DroneModel<ESP, PARAM_GR>)
ATO_AUDIT_INST(DroneModel<ESP, PARAM_REL>)
ATO_AUDIT_INST(DroneModel<YPR, GLOBAL>)
ATO_AUDIT_INST(DroneModel<YPR, PARAM_GR>)
ATO_AUDIT_INST(DroneModel<YPR, PARAM_REL>)
ATO_AUDIT_INST(DroneModel<DCM, GLOBAL>)
ATO_AUDIT_INST(DroneModel<DCM, PARAM_GR>)
ATO_AUDIT_INST(DroneModel<DCM, PARAM_REL>)
ATO_AUDIT_INST(PointModel<GLOBAL>)
ATO_AUDIT_INST(PointModel<PARAM_GR>)
ATO_AUDIT_INST(PointModel<PARAM_REL>)
#undef ATO_AUDIT_INST

}  // namespace ato
