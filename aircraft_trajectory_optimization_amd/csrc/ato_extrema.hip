// ato_extrema.hip -- the interval-extrema kernels (ato_extrema.hpp): one instantiation per polynomial degree, so
// that every coefficient array is indexed by constants and lives in registers.
#include <hip/hip_runtime.h>
#include "ato_extrema.hpp"

namespace ato {

constexpr int EXT_BLOCK = EXT_LANES * EXT_WAVES;

// blockIdx.x: the block of 64 instances, blockIdx.y: the channel v, blockIdx.z: the part of the lap. Lane = instance,
// wave = the interval's residue mod 4 within the part. out: val (nsplit == 1, the call's layout) or the partial
// records; ival (or NULL): the per-interval min and max, [NVX][N][2][B] interleaved, [B][NVX][N][2] instance-major.
template <int K1>
__global__ __launch_bounds__(EXT_BLOCK) void k_extrema(ExtD a, int B, int layout, const double* __restrict__ w,
                                                        double* __restrict__ out, double* __restrict__ ival) {
    __shared__ double s_tab[K1 * K1 + K1];
    __shared__ double s_rec[EXT_WAVES - 1][EXT_NCH][EXT_LANES];
    for (int i = threadIdx.x; i < K1 * K1 + K1; i += EXT_BLOCK) s_tab[i] = a.tab[i];
    __syncthreads();
    const int lane = threadIdx.x & (EXT_LANES - 1), wave = threadIdx.x / EXT_LANES;
    const int b = blockIdx.x * EXT_LANES + lane, v = blockIdx.y, part = blockIdx.z;
    const bool live = b < B, il = layout == ATO_LAYOUT_INTERLEAVED;
    const int n0 = (int)((long)part * a.N / a.nsplit), n1 = (int)((long)(part + 1) * a.N / a.nsplit);
    ExtRec rec = ext_empty();
    if (live) {
        const double* wb = w + (il ? (long)b : (long)b * a.nw);
        const long ws = il ? (long)B : 1L;
        for (int n = n0 + wave; n < n1; n += EXT_WAVES) {
            ExtRec r;
            ext_interval<K1>(a, s_tab, v, n, wb, ws, r);
            if (ival) {
                const bool ok = r.mx_n >= 0.0;
                const double lo = ok ? r.mn : r.flag, hi = ok ? r.mx : r.flag;      // a rejected interval: NaN
                if (il) {
                    double* o = ival + (((long)v * a.N + n) * 2) * B + b;
                    o[0] = lo;
                    o[B] = hi;
                } else {
                    double* o = ival + (((long)b * a.NVX + v) * a.N + n) * 2;
                    o[0] = lo;
                    o[1] = hi;
                }
            }
            ext_combine(rec, r);
        }
    }
    if (wave > 0) {
        const double o[EXT_NCH] = {rec.mn, rec.mn_n, rec.mn_x, rec.mx, rec.mx_n, rec.mx_x, rec.slack, rec.flag};
#pragma unroll
        for (int c = 0; c < EXT_NCH; ++c) s_rec[wave - 1][c][lane] = o[c];
    }
    __syncthreads();
    if (wave > 0 || !live) return;
#pragma unroll
    for (int q = 0; q < EXT_WAVES - 1; ++q) {
        const ExtRec r{s_rec[q][0][lane], s_rec[q][1][lane], s_rec[q][2][lane], s_rec[q][3][lane],
                       s_rec[q][4][lane], s_rec[q][5][lane], s_rec[q][6][lane], s_rec[q][7][lane]};
        ext_combine(rec, r);
    }
    if (a.nsplit == 1) ext_store(out, il, a.NVX, B, v, b, rec);
    else ext_store(out + (long)part * EXT_NCH * a.NVX * B, true, a.NVX, B, v, b, rec);
}

// One thread per (v, b): the nsplit partial records into val
__global__ __launch_bounds__(EXT_BLOCK) void k_ext_combine(ExtD a, int B, int layout, const double* __restrict__ part,
                                                            double* __restrict__ val) {
    const int b = blockIdx.x * EXT_BLOCK + threadIdx.x, v = blockIdx.y;
    if (b >= B) return;
    const long cs = (long)a.NVX * B;
    ExtRec rec = ext_empty();
    for (int s = 0; s < a.nsplit; ++s) {
        const double* p = part + ext_part_at(a.NVX, B, s, v, b);
        const ExtRec r{p[0], p[cs], p[2 * cs], p[3 * cs], p[4 * cs], p[5 * cs], p[6 * cs], p[7 * cs]};
        ext_combine(rec, r);
    }
    ext_store(val, layout == ATO_LAYOUT_INTERLEAVED, a.NVX, B, v, b, rec);
}

template <int K1>
static void launch_k(const ExtD& a, int B, int layout, const double* w, double* out, double* ival, dim3 grid,
                     hipStream_t st) {
    hipLaunchKernelGGL(k_extrema<K1>, grid, dim3(EXT_BLOCK), 0, st, a, B, layout, w, out, ival);
}

hipError_t launch_extrema(const ExtD& a, int B, int layout, const double* w, double* part, double* val, double* ival,
                          hipStream_t st) {
    const long gx = ((long)B + EXT_LANES - 1) / EXT_LANES;
    if (gx > 0x7fffffffL || a.NVX > 65535 || a.nsplit < 1 || a.nsplit > EXT_SPLIT_MAX) return hipErrorInvalidValue;
    if (a.nsplit > 1 && !part) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)a.NVX, (unsigned)a.nsplit);
    double* out = a.nsplit == 1 ? val : part;
    switch (a.K1) {
        case 2: launch_k<2>(a, B, layout, w, out, ival, grid, st); break;
        case 3: launch_k<3>(a, B, layout, w, out, ival, grid, st); break;
        case 4: launch_k<4>(a, B, layout, w, out, ival, grid, st); break;
        case 5: launch_k<5>(a, B, layout, w, out, ival, grid, st); break;
        case 6: launch_k<6>(a, B, layout, w, out, ival, grid, st); break;
        case 7: launch_k<7>(a, B, layout, w, out, ival, grid, st); break;
        case 8: launch_k<8>(a, B, layout, w, out, ival, grid, st); break;
        case 9: launch_k<9>(a, B, layout, w, out, ival, grid, st); break;
        case 10: launch_k<10>(a, B, layout, w, out, ival, grid, st); break;
        default: return hipErrorInvalidValue;
    }
    if (hipError_t e = hipGetLastError()) return e;
    if (a.nsplit > 1) {
        const dim3 cgrid((unsigned)(((long)B + EXT_BLOCK - 1) / EXT_BLOCK), (unsigned)a.NVX);
        hipLaunchKernelGGL(k_ext_combine, cgrid, dim3(EXT_BLOCK), 0, st, a, B, layout, part, val);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace ato
