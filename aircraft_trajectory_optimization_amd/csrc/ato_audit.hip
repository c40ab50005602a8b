// ato_audit.hip -- the between-node audit kernel (ato_audit.hpp), one instantiation per model variant.
#include <hip/hip_runtime.h>
#include "ato_audit.hpp"

namespace ato {

constexpr int AUDIT_BLOCK = 256;

// One thread per (b, n, i) of the SampleGrid (ato_sample.hpp, which has the output layouts), the grid of
// k_clearance_pos: blockIdx.x is the (interval, sample) pair and blockIdx.y the block of instances, so both weight
// rows of a block sit behind a uniform address (scalar loads) and, with the interleaved layout, a wave's loads of
// one source element and its stores of one channel are contiguous over its instances. The spline pieces are
// gathered per lane: s is the instance's own.
// One wave per SIMD at 256 threads: the whole register file is the thread's (no scratch, no LDS; the listing
// is profiles/sample_layer/kernel_resource_usage_head.txt).
template <class M>
__global__ __launch_bounds__(AUDIT_BLOCK) void k_audit(AuditD a, int B, int layout, const double* __restrict__ w,
                                                       double* __restrict__ val) {
    const int q = blockIdx.x, n = q / a.S1, i = q - n * a.S1;
    const int b = blockIdx.y * AUDIT_BLOCK + threadIdx.x;
    if (b >= B) return;
    const SampleGrid g{a.N, a.S1, B, layout == ATO_LAYOUT_INTERLEAVED};
    double out[AUDIT_NCH];
    audit_point<M>(a, n, i, b, B, g.il, g.input(w, b, a.nw), g.stride(), out);
    g.store<AUDIT_NCH>(val, n, i, b, out);
}

template <class M>
hipError_t launch_audit(const AuditD& a, int B, int layout, const double* w, double* val, hipStream_t st) {
    dim3 grid;
    if (hipError_t e = sample_grid_dims(a.N, a.S1, B, AUDIT_BLOCK, &grid)) return e;
    hipLaunchKernelGGL((k_audit<M>), grid, dim3(AUDIT_BLOCK), 0, st, a, B, layout, w, val);
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
