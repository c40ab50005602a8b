// ato_compare.hip -- the comparison kernels (ato_compare.hpp): the position table, the pair kernel and the groups.
#include <hip/hip_runtime.h>
#include "ato_compare.hpp"

namespace ato {

constexpr int CMP_SBLOCK = 64;                                 // instances per workgroup of the sampling kernels
constexpr int CMP_SIDE = CMP_TILE / CMP_RB;                    // 16 x 16 threads own a 64 x 64 tile
constexpr int CMP_THREADS = CMP_SIDE * CMP_SIDE;
constexpr int CMP_STAGE = 3 * CMP_CHUNK * CMP_TILE;            // doubles of one operand's chunk
constexpr int CMP_PITCH = CMP_TILE + 1;                        // row pitch of the mirrored tile in LDS
static_assert(CMP_TILE == 64, "a tile row is one 64-bit adjacency word");
static_assert(CMP_TILE * CMP_PITCH <= 2 * CMP_STAGE, "the mirrored tile reuses the staging buffers");

// One thread per instance: the export's start times into the handle's [N + 1][B] table, and the lap time.
__global__ __launch_bounds__(CMP_SBLOCK) void k_compare_tstart(ExportD a, int B, int layout,
                                                               const double* __restrict__ w, double* __restrict__ lap) {
    const int b = blockIdx.x * CMP_SBLOCK + threadIdx.x;
    if (b >= B) return;
    const bool il = layout == ATO_LAYOUT_INTERLEAVED;
    export_tstart(a.N, w + (il ? (long)b : (long)b * a.nw), il ? (long)B : 1L, a.ts + b, (long)B);
    if (lap) lap[b] = a.ts[(long)a.N * B + b];
}

// One thread per (fraction j, instance b), the grid of k_export_sample: the export's interpolation and lift at
// t = f_j T_b, of which only the position leaves the thread (the rest of the lift is dead code here).
template <class M>
__global__ __launch_bounds__(CMP_SBLOCK) void k_compare_sample(ExportD a, int B, int layout,
                                                               const double* __restrict__ w, double* __restrict__ pos) {
    constexpr int NV = M::NZ + 2 * M::NU;
    const int j = blockIdx.x;
    const int b = blockIdx.y * CMP_SBLOCK + threadIdx.x;
    if (b >= B) return;
    const SampleGrid g{a.n_times, 1, B, layout == ATO_LAYOUT_INTERLEAVED};
    double v[NV], out[EXPORT_NCH];
    const double f = (double)j / (double)(a.n_times - 1);
    export_interp<NV>(a, f, a.ts + b, (long)B, g.input(w, b, a.nw), g.stride(), v, out);
    export_lift<M>(a.line, v, out);
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[((long)c * a.n_times + j) * B + b] = out[EX_POS + c];
}

// The pair kernel. blockIdx.y is the tile of 64 rows (instances a of px), blockIdx.x the tile of 64 columns
// (instances b of py); of a self-comparison only the tiles with column tile >= row tile run, the others leave at
// once. The 256 threads form 16 x 16; thread (tx, ty) owns rows ty 4 + i and columns tx + 16 k, i, k < 4: sixteen
// pairs whose sum, maximum and argmax stay in registers over the whole sample axis. The samples come through LDS
// in chunks of CMP_CHUNK: both operands' chunk (3 axes x 16 samples x 64 instances each) is loaded with the
// instance index fastest (a wave reads 64 consecutive doubles of one sample row), then per sample a thread reads
// 4 + 4 points -- its four rows are one address per quarter wave (broadcast), its four columns 16 consecutive
// doubles per read -- and updates 16 pairs: one LDS read of a point serves four pairs. Rows and columns past the
// batch are staged as zeros and never stored.
// Results: the tile's three channels go to val directly (16 lanes write 128 consecutive bytes); the mirror image
// of an off-diagonal tile of a self-comparison is transposed through LDS so that its stores run along a row too.
// The adjacency word of every tile row (and, mirrored, tile column) is put together in LDS by integer OR, which is
// order-independent, and stored whole by one thread: a word belongs to exactly one workgroup, so there are no
// global atomics and padding bits stay zero. No scratch (profiles/compare/kernel_resource_usage.txt).
__global__ __launch_bounds__(CMP_THREADS) void k_compare_pairs(int count, int bx, const double* __restrict__ px, int by,
                                                               const double* __restrict__ py, int self, int metric,
                                                               double eps, double* __restrict__ val,
                                                               unsigned long long* __restrict__ adj) {
    __shared__ double lds[2 * CMP_STAGE];
    __shared__ unsigned long long rowbits[CMP_TILE], colbits[CMP_TILE];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (self && ti > tj) return;
    const int tid = threadIdx.x, tx = tid % CMP_SIDE, ty = tid / CMP_SIDE;
    const int row0 = ti * CMP_TILE, col0 = tj * CMP_TILE;
    double* xs = lds;
    double* ys = lds + CMP_STAGE;
    if (tid < CMP_TILE) rowbits[tid] = colbits[tid] = 0ull;     // ordered before the ORs by the barriers of the loop

    ComparePair p[CMP_RB][CMP_RB];
#pragma unroll
    for (int i = 0; i < CMP_RB; ++i)
#pragma unroll
        for (int k = 0; k < CMP_RB; ++k) p[i][k] = ComparePair{0.0, -1.0, 0};

    for (int s0 = 0; s0 < count; s0 += CMP_CHUNK) {
        for (int e = tid; e < CMP_STAGE; e += CMP_THREADS) {
            const int r = e % CMP_TILE, s = (e / CMP_TILE) % CMP_CHUNK, c = e / (CMP_TILE * CMP_CHUNK);
            const int j = s0 + s;
            const long at = (long)c * count + j;
            xs[e] = (j < count && row0 + r < bx) ? px[at * bx + row0 + r] : 0.0;
            ys[e] = (j < count && col0 + r < by) ? py[at * by + col0 + r] : 0.0;
        }
        __syncthreads();
        const int n = count - s0 < CMP_CHUNK ? count - s0 : CMP_CHUNK;
        for (int s = 0; s < n; ++s) {
            double xa[CMP_RB][3], yb[CMP_RB][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int i = 0; i < CMP_RB; ++i) xa[i][c] = xs[(c * CMP_CHUNK + s) * CMP_TILE + ty * CMP_RB + i];
#pragma unroll
                for (int k = 0; k < CMP_RB; ++k) yb[k][c] = ys[(c * CMP_CHUNK + s) * CMP_TILE + tx + CMP_SIDE * k];
            }
#pragma unroll
            for (int i = 0; i < CMP_RB; ++i)
#pragma unroll
                for (int k = 0; k < CMP_RB; ++k)
                    compare_step(p[i][k], compare_d2(xa[i][0], xa[i][1], xa[i][2], yb[k][0], yb[k][1], yb[k][2]),
                                 s0 + s);
        }
        __syncthreads();
    }

    double o[CMP_RB][CMP_RB][CMP_NCH];
#pragma unroll
    for (int i = 0; i < CMP_RB; ++i)
#pragma unroll
        for (int k = 0; k < CMP_RB; ++k) compare_finish(p[i][k], count, o[i][k]);
    const bool mirror = self && ti != tj;

    if (adj) {
        unsigned long long cm[CMP_RB] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int i = 0; i < CMP_RB; ++i) {
            unsigned long long rm = 0ull;
#pragma unroll
            for (int k = 0; k < CMP_RB; ++k) {
                const int r = ty * CMP_RB + i, c = tx + CMP_SIDE * k;
                const double m = metric == CMP_METRIC_RMS ? o[i][k][CMP_RMS] : o[i][k][CMP_MAX];
                if (m <= eps && row0 + r < bx && col0 + c < by) {
                    rm |= 1ull << c;
                    cm[k] |= 1ull << r;
                }
            }
            if (rm) atomicOr(&rowbits[ty * CMP_RB + i], rm);
        }
        if (mirror) {
#pragma unroll
            for (int k = 0; k < CMP_RB; ++k)
                if (cm[k]) atomicOr(&colbits[tx + CMP_SIDE * k], cm[k]);
        }
        __syncthreads();
        const long W = ((long)by + 63) / 64;
        if (tid < CMP_TILE) {
            if (row0 + tid < bx) adj[(long)(row0 + tid) * W + tj] = rowbits[tid];
        } else if (mirror && tid < 2 * CMP_TILE) {
            const int c = tid - CMP_TILE;
            if (col0 + c < by) adj[(long)(col0 + c) * W + ti] = colbits[c];
        }
    }
    if (!val) return;

#pragma unroll
    for (int ch = 0; ch < CMP_NCH; ++ch) {
#pragma unroll
        for (int i = 0; i < CMP_RB; ++i)
#pragma unroll
            for (int k = 0; k < CMP_RB; ++k) {
                const int r = row0 + ty * CMP_RB + i, c = col0 + tx + CMP_SIDE * k;
                if (r < bx && c < by) val[((long)ch * bx + r) * by + c] = o[i][k][ch];
            }
        if (!mirror) continue;
        // the mirror image: element (c, r) of the square result is this tile's (r, c), transposed through LDS
        __syncthreads();
#pragma unroll
        for (int i = 0; i < CMP_RB; ++i)
#pragma unroll
            for (int k = 0; k < CMP_RB; ++k) lds[(ty * CMP_RB + i) * CMP_PITCH + tx + CMP_SIDE * k] = o[i][k][ch];
        __syncthreads();
        for (int e = tid; e < CMP_TILE * CMP_TILE; e += CMP_THREADS) {
            const int r = e % CMP_TILE, c = e / CMP_TILE;
            if (row0 + r < bx && col0 + c < by)
                val[((long)ch * bx + col0 + c) * by + row0 + r] = lds[r * CMP_PITCH + c];
        }
    }
}

// The groups kernel: one workgroup, labels in LDS behind the two flag words (ato_compare.hpp has the argument for
// the sweep bound and for the races). A thread takes one adjacency word at a time, consecutive threads consecutive
// words, so the matrix is read in whole lines once per sweep.
__global__ __launch_bounds__(CMP_GROUP_BLOCK) void k_compare_groups(int batch, const unsigned long long* __restrict__ adj,
                                                                    int* __restrict__ group, int* __restrict__ info) {
    extern __shared__ int group_lds[];
    int* flag = group_lds;             // [2]: "sweep s changed a label" at s & 1
    int* label = group_lds + 2;        // [batch]
    const int tid = threadIdx.x;
    const long W = ((long)batch + 63) / 64, words = (long)batch * W;
    for (int i = tid; i < batch; i += CMP_GROUP_BLOCK) label[i] = i;
    if (tid < 2) flag[tid] = 0;
    __syncthreads();
    int sweeps = 0, capped = 1;
    for (int s = 0; s < batch; ++s) {                   // at most `batch` sweeps, whatever the data
        int changed = 0;
        for (long e = tid; e < words; e += CMP_GROUP_BLOCK) {
            unsigned long long bits = adj[e];
            if (!bits) continue;
            const int i = (int)(e / W), base = (int)(e % W) * 64;
            const int before = label[i];
            int m = before;
            while (bits) {
                const int j = base + __builtin_ctzll(bits);
                bits &= bits - 1;
                if (j >= batch) break;                  // padding bits of a foreign matrix: never an index
                const int lj = label[j];
                if (lj < m) m = lj;
                else if (m < lj) changed |= atomicMin(&label[j], m) > m;
            }
            if (m < before) changed |= atomicMin(&label[i], m) > m;
        }
        __syncthreads();
        for (int i = tid; i < batch; i += CMP_GROUP_BLOCK) {
            const int l = label[i], ll = label[l];
            if (ll < l) { label[i] = ll; changed = 1; }
        }
        if (changed) flag[s & 1] = 1;
        if (tid == 0) flag[(s + 1) & 1] = 0;            // the next sweep sets it only after its own barrier above
        __syncthreads();
        sweeps = s + 1;
        if (!flag[s & 1]) { capped = 0; break; }
    }
    for (int i = tid; i < batch; i += CMP_GROUP_BLOCK) group[i] = label[i];
    if (tid == 0) {
        info[0] = sweeps;
        info[1] = capped;
    }
}

template <class M>
hipError_t launch_compare_sample(const ExportD& a, int B, int layout, const double* w, double* pos, double* lap,
                                 hipStream_t st) {
    const long blocks = ((long)B + CMP_SBLOCK - 1) / CMP_SBLOCK;
    if (blocks > 65535) return hipErrorInvalidValue;      // blockIdx.y of the sample kernel
    hipLaunchKernelGGL(k_compare_tstart, dim3((unsigned)blocks), dim3(CMP_SBLOCK), 0, st, a, B, layout, w, lap);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((k_compare_sample<M>), dim3((unsigned)a.n_times, (unsigned)blocks), dim3(CMP_SBLOCK), 0, st, a,
                       B, layout, w, pos);
    return hipGetLastError();
}

hipError_t launch_compare_pairs(int count, int bx, const double* px, int by, const double* py, int metric, double eps,
                                double* val, unsigned long long* adj, hipStream_t st) {
    const int self = py == nullptr;
    if (self) { by = bx; py = px; }
    const long tr = ((long)bx + CMP_TILE - 1) / CMP_TILE, tc = ((long)by + CMP_TILE - 1) / CMP_TILE;
    if (tr > 65535) return hipErrorInvalidValue;          // blockIdx.y
    hipLaunchKernelGGL(k_compare_pairs, dim3((unsigned)tc, (unsigned)tr), dim3(CMP_THREADS), 0, st, count, bx, px, by,
                       py, self, metric, eps, val, adj);
    return hipGetLastError();
}

hipError_t launch_compare_groups(int batch, const unsigned long long* adj, int* group, int* info, hipStream_t st) {
    hipLaunchKernelGGL(k_compare_groups, dim3(1), dim3(CMP_GROUP_BLOCK), (size_t)(batch + 2) * sizeof(int), st, batch,
                       adj, group, info);
    return hipGetLastError();
}

#define ATO_COMPARE_INST(...)                                                                                 \
    template hipError_t launch_compare_sample<__VA_ARGS__>(const ExportD&, int, int, const double*, double*, \
                                                           double*, hipStream_t);
ATO_COMPARE_INST(DroneModel<ESP, GLOBAL>)
ATO_COMPARE_INST(DroneModel<ESP, PARAM_GR>)
ATO_COMPARE_INST(DroneModel<ESP, PARAM_REL>)
ATO_COMPARE_INST(DroneModel<YPR, GLOBAL>)
ATO_COMPARE_INST(DroneModel<YPR, PARAM_GR>)
ATO_COMPARE_INST(DroneModel<YPR, PARAM_REL>)
ATO_COMPARE_INST(DroneModel<DCM, GLOBAL>)
ATO_COMPARE_INST(DroneModel<DCM, PARAM_GR>)
ATO_COMPARE_INST(DroneModel<DCM, PARAM_REL>)
ATO_COMPARE_INST(PointModel<GLOBAL>)
ATO_COMPARE_INST(PointModel<PARAM_GR>)
ATO_COMPARE_INST(PointModel<PARAM_REL>)
#undef ATO_COMPARE_INST

}  // namespace ato
