// ato_export.hip -- the export kernels (ato_export.hpp). The model variant is a template parameter of the sample
// kernel, so it carries no pose or frame branch and holds only the variant's node vector in registers.
#include <hip/hip_runtime.h>
#include "ato_export.hpp"

namespace ato {

constexpr int EX_BLOCK = 64;       // instances per workgroup: one wave

// One thread per instance, adjacent lanes adjacent instances: the sequential prefix sum of the step sizes into the
// handle's [N + 1][B] table. With the interleaved layout a wave's loads of h_n and its stores of t_start[n + 1]
// are contiguous; the N additions of a thread depend on each other, the instances do not.
__global__ __launch_bounds__(EX_BLOCK) void k_export_tstart(ExportD a, int B, int layout,
                                                            const double* __restrict__ w) {
    const int b = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (b >= B) return;
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    export_tstart(a.N, w + (il ? (long)b : (long)b * a.nw), il ? (long)B : 1L, a.ts + b, (long)B);
}

// One thread per (time j, instance b): blockIdx.x is the time, blockIdx.y the block of 64 instances, so times[j],
// tau and D sit behind uniform addresses (scalar loads) and, with the interleaved layout, a wave's loads of one
// t_start row or node element and its stores of one channel are contiguous over its instances. Each lane searches
// its own t_start column (log2(N + 1) dependent loads), forms the K + 1 weights one at a time (a hold needs none),
// accumulates the node vector in registers and lifts it; the spline pieces are gathered per lane, s is the
// instance's own. One wave per workgroup: up to 512 VGPRs, no LDS, no scratch
// (profiles/export/kernel_resource_usage.txt).
template <class M>
__global__ __launch_bounds__(EX_BLOCK) void k_export_sample(ExportD a, int B, int layout,
                                                            const double* __restrict__ w,
                                                            double* __restrict__ nodes, double* __restrict__ state) {
    constexpr int NV = M::NZ + 2 * M::NU;
    const int j = blockIdx.x;
    const int b = blockIdx.y * EX_BLOCK + threadIdx.x;
    if (b >= B) return;
    const SampleGrid g{a.n_times, 1, B, layout == ATO_LAYOUT_INTERLEAVED};
    double v[NV], out[EXPORT_NCH];
    export_interp<NV>(a, a.times[j], a.ts + b, (long)B, g.input(w, b, a.nw), g.stride(), v, out);
    if (nodes) g.store<NV>(nodes, j, 0, b, v);
    if (state) {
        export_lift<M>(a.line, v, out);
        g.store<EXPORT_NCH>(state, j, 0, b, out);
    }
}

// The sign pass. A workgroup is 64 instances x G segments of the sample axis, G = blockDim.y chosen per call by
// export_segments (1 .. EXPORT_GMAX: sixteen waves for the 8 workgroups of B = 512, four from B = 16384 on):
// threadIdx.x is the instance (adjacent lanes, adjacent instances), threadIdx.y the segment, one wave each. Every
// thread composes the maps of its segment, the G x 64 maps of the workgroup meet in LDS (one byte each), every
// thread folds the maps before its own segment (at most 15 LDS reads of its own lane's column, no bank conflict
// within a wave) and walks its segment again to negate in place. The raw quaternion before a segment is read before
// the barrier: after it, the segment before may already have negated that sample. No atomics, nothing between
// workgroups. 16 waves a workgroup leave 128 VGPRs a lane; the kernel needs far fewer.
__global__ __launch_bounds__(EX_BLOCK * EXPORT_GMAX) void k_export_qchain(int n_times, int B, int layout,
                                                                         double* __restrict__ state) {
    __shared__ unsigned char maps[EXPORT_GMAX][EX_BLOCK];
    const int lane = threadIdx.x, seg = threadIdx.y, G = blockDim.y;
    const int b = blockIdx.x * EX_BLOCK + lane;
    const bool live = b < B;
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    double prev[4] = {0.0, 0.0, 0.0, 0.0};
    maps[seg][lane] = (unsigned char)(live ? export_segment_map(state, il, n_times, B, b, G, seg, prev) : EX_MAP_ID);
    __syncthreads();
    if (!live) return;
    unsigned s = 0;
    for (int g = 0; g < seg; ++g) s = export_map_at(maps[g][lane], s);
    export_segment_apply(state, il, n_times, B, b, G, seg, s, prev);
}

template <class M>
hipError_t launch_export(const ExportD& a, int B, int layout, const double* w, double* nodes, double* state,
                         hipStream_t st) {
    const long blocks = ((long)B + EX_BLOCK - 1) / EX_BLOCK;
    if (blocks > 65535) return hipErrorInvalidValue;      // blockIdx.y of the sample kernel
    hipLaunchKernelGGL(k_export_tstart, dim3((unsigned)blocks), dim3(EX_BLOCK), 0, st, a, B, layout, w);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((k_export_sample<M>), dim3((unsigned)a.n_times, (unsigned)blocks), dim3(EX_BLOCK), 0, st, a, B,
                       layout, w, nodes, state);
    if (hipError_t e = hipGetLastError()) return e;
    if constexpr (M::IS_DRONE) {
        if (state) {
            const unsigned G = (unsigned)export_segments(a.n_times, B);
            hipLaunchKernelGGL(k_export_qchain, dim3((unsigned)blocks), dim3(EX_BLOCK, G), 0, st, a.n_times, B, layout,
                               state);
            return hipGetLastError();
        }
    }
    return hipSuccess;
}

#define ATO_EXPORT_INST(...)                                                                                  \
    template hipError_t launch_export<__VA_ARGS__>(const ExportD&, int, int, const double*, double*, double*, \
                                                   hipStream_t);
ATO_EXPORT_INST(DroneModel<ESP, GLOBAL>)
ATO_EXPORT_INST(DroneModel<ESP, PARAM_GR>)
ATO_EXPORT_INST(DroneModel<ESP, PARAM_REL>)
ATO_EXPORT_INST(DroneModel<YPR, GLOBAL>)
ATO_EXPORT_INST(DroneModel<YPR, PARAM_GR>)
ATO_EXPORT_INST(DroneModel<YPR, PARAM_REL>)
ATO_EXPORT_INST(DroneModel<DCM, GLOBAL>)
ATO_EXPORT_INST(DroneModel<DCM, PARAM_GR>)
ATO_EXPORT_INST(DroneModel<DCM, PARAM_REL>)
ATO_EXPORT_INST(PointModel<GLOBAL>)
ATO_EXPORT_INST(PointModel<PARAM_GR>)
ATO_EXPORT_INST(PointModel<PARAM_REL>)
#undef ATO_EXPORT_INST

}  // namespace ato
