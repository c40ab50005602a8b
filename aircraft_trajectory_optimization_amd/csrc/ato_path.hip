// ato_path.hip -- the path-distance kernel (ato_path.hpp): directed point-to-polyline distances of every pair of
// columns of two position tables, both ways, in one launch.
#include <hip/hip_runtime.h>
#include "ato_path.hpp"

namespace ato {

constexpr int PATH_WAVE = 64;
constexpr int PATH_WAVES = 4;
constexpr int PATH_THREADS = PATH_WAVE * PATH_WAVES;
constexpr int PATH_SUB = PATH_WAVES * PATH_C;                   // segment-side instances of one sweep
constexpr int PATH_NSUB = PATH_TILE / PATH_SUB;
constexpr int PATH_STAGE = PATH_SUB * PATH_CHUNK * PATH_REC;    // doubles of a staged chunk of records
constexpr int PATH_PITCH = PATH_SUB + 1;                        // pitch of the result tile [4][64][16] in LDS
constexpr int PATH_OUT = 4 * PATH_TILE * PATH_PITCH;
constexpr int PATH_LDS = PATH_STAGE > PATH_OUT ? PATH_STAGE : PATH_OUT;
static_assert(PATH_TILE == PATH_WAVE, "a lane is a sample-side instance and a tile row is one adjacency word");
static_assert(PATH_NSUB * PATH_SUB == PATH_TILE, "the sweeps cover the tile");
static_assert(PATH_REC >= 7 && PATH_REC % 2 == 0, "a record is read in 16-byte pieces");

// blockIdx.y is the tile of 64 rows (instances a of px), blockIdx.x the tile of 64 columns (instances b of py).
// pass 0: P = px (samples), Q = py (segments); pass 1 the other way round. ato_path.hpp has the data flow.
__global__ __launch_bounds__(PATH_THREADS) void k_compare_path(int count, int bx, const double* __restrict__ px, int by,
                                                               const double* __restrict__ py, int self, int metric,
                                                               double eps, double* __restrict__ val,
                                                               unsigned long long* __restrict__ adj) {
    __shared__ __attribute__((aligned(16))) double lds[PATH_LDS];
    // per pass: "near" words by sample-side instance (bits over the segment side, LDS atomic OR) and by
    // segment-side instance (bits over the sample side, a ballot), and "finite" words by segment-side instance
    __shared__ unsigned long long bitS[2][PATH_TILE], bitG[2][PATH_TILE], okG[2][PATH_TILE];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (self && ti > tj) return;
    const int tid = threadIdx.x, lane = tid % PATH_WAVE, wave = tid / PATH_WAVE;
    const int row0 = ti * PATH_TILE, col0 = tj * PATH_TILE;
    const bool mirror = self && ti != tj;
    const int nseg = count - 1;
    if (tid < 2 * PATH_TILE) bitS[tid / PATH_TILE][tid % PATH_TILE] = 0ull;   // ordered before the ORs by the loop's barriers

#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const double* __restrict__ P = pass ? py : px;
        const double* __restrict__ Q = pass ? px : py;
        const int nP = pass ? by : bx, nQ = pass ? bx : by;
        const int p0 = pass ? col0 : row0, q0 = pass ? row0 : col0;
        const int inst = p0 + lane;
        const bool in_p = inst < nP;
#pragma unroll 1
        for (int sub = 0; sub < PATH_NSUB; ++sub) {
            const int g0 = sub * PATH_SUB;              // first segment-side instance of the sweep, within the tile
            PathFold f[PATH_C];
#pragma unroll
            for (int k = 0; k < PATH_C; ++k) f[k] = PathFold{0.0, -1.0, 0, 0};

            for (int i0 = 0; i0 < count; i0 += PATH_R) {
                double pt[PATH_R][3], best[PATH_R][PATH_C];
                int bseg[PATH_R][PATH_C];
#pragma unroll
                for (int j = 0; j < PATH_R; ++j) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        pt[j][c] = (in_p && i0 + j < count) ? P[((long)c * count + i0 + j) * nP + inst] : 0.0;
#pragma unroll
                    for (int k = 0; k < PATH_C; ++k) { best[j][k] = __builtin_inf(); bseg[j][k] = 0; }
                }
                for (int s0 = 0; s0 < nseg; s0 += PATH_CHUNK) {
                    __syncthreads();                    // the last chunk, or the result tile, has been read
                    for (int e = tid; e < PATH_SUB * PATH_CHUNK; e += PATH_THREADS) {
                        const int g = e % PATH_SUB, s = e / PATH_SUB, seg = s0 + s, gi = q0 + g0 + g;
                        PathSeg r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                        if (seg < nseg && gi < nQ) {
                            const double* a = Q + (long)seg * nQ + gi;
                            const long ch = (long)count * nQ;
                            r = path_segment(a[0], a[ch], a[2 * ch], a[nQ], a[ch + nQ], a[2 * ch + nQ]);
                        }
                        double* w = lds + (g * PATH_CHUNK + s) * PATH_REC;
                        w[0] = r.qx; w[1] = r.qy; w[2] = r.qz; w[3] = r.ex; w[4] = r.ey; w[5] = r.ez; w[6] = r.inv;
                    }
                    __syncthreads();
                    const int n = nseg - s0 < PATH_CHUNK ? nseg - s0 : PATH_CHUNK;
                    for (int s = 0; s < n; ++s) {
#pragma unroll
                        for (int k = 0; k < PATH_C; ++k) {
                            const double* w = lds + ((wave * PATH_C + k) * PATH_CHUNK + s) * PATH_REC;
                            const PathSeg r{w[0], w[1], w[2], w[3], w[4], w[5], w[6]};
#pragma unroll
                            for (int j = 0; j < PATH_R; ++j) {
                                const double d2 = path_d2(r, pt[j][0], pt[j][1], pt[j][2]);
                                if (d2 < best[j][k]) { best[j][k] = d2; bseg[j][k] = s0 + s; }
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < PATH_R; ++j)
                    if (i0 + j < count) {
#pragma unroll
                        for (int k = 0; k < PATH_C; ++k) path_step(f[k], best[j][k], i0 + j, bseg[j][k]);
                    }
            }

            // the sweep's 4 directed records of this thread: channels, finiteness, bits
            __syncthreads();                            // the last chunk has been read: the tile takes its place
#pragma unroll
            for (int k = 0; k < PATH_C; ++k) {
                const int g = g0 + wave * PATH_C + k, gi = q0 + g;
                const bool in = in_p && gi < nQ;
                double t = 0.0;
                if (val && in) {                        // t* of the winning sample on its nearest segment
                    const long ch = (long)count;
                    const double* a = Q + (long)f[k].seg * nQ + gi;
                    const double* p = P + (long)f[k].at * nP + inst;
                    const PathSeg r = path_segment(a[0], a[ch * nQ], a[2 * ch * nQ], a[nQ], a[ch * nQ + nQ],
                                                   a[2 * ch * nQ + nQ]);
                    t = path_t(r, p[0] - r.qx, p[ch * nP] - r.qy, p[2 * ch * nP] - r.qz);
                }
                double o[4];
                const bool ok = path_finish(f[k], count, t, o);
                const bool near = ok && in && (metric == CMP_METRIC_RMS ? o[PATH_CH_RMS] : o[PATH_CH_MAX]) <= eps;
                const unsigned long long okm = __ballot(ok), nearm = __ballot(near);
                if (lane == 0) { okG[pass][g] = okm; bitG[pass][g] = nearm; }
                if (near) atomicOr(&bitS[pass][lane], 1ull << g);
                // pass 1 knows both directions: okG[0][this column] has the rows' bits of pass 0
                const bool both = pass == 0 || ((okG[0][lane] >> g) & 1ull);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    lds[(c * PATH_TILE + lane) * PATH_PITCH + wave * PATH_C + k] = both ? o[c] : __builtin_nan("");
            }
            if (!val) continue;
            __syncthreads();
            // plane c of the pass-0 half at [sample side][segment side], plane 4 + c at [segment side][sample side]
            if (pass == 0 || mirror)
                for (int e = tid; e < 4 * PATH_TILE * PATH_SUB; e += PATH_THREADS) {
                    const int g = e % PATH_SUB, l = (e / PATH_SUB) % PATH_TILE, c = e / (PATH_SUB * PATH_TILE);
                    if (p0 + l < nP && q0 + g0 + g < nQ)
                        val[((long)c * bx + p0 + l) * by + q0 + g0 + g] = lds[(c * PATH_TILE + l) * PATH_PITCH + g];
                }
            if (pass == 1 || mirror)
                for (int e = tid; e < 4 * PATH_TILE * PATH_SUB; e += PATH_THREADS) {
                    const int l = e % PATH_TILE, g = (e / PATH_TILE) % PATH_SUB, c = e / (PATH_SUB * PATH_TILE);
                    if (p0 + l < nP && q0 + g0 + g < nQ)
                        val[((long)(4 + c) * bx + q0 + g0 + g) * by + p0 + l] = lds[(c * PATH_TILE + l) * PATH_PITCH + g];
                }
        }
    }
    __syncthreads();

    if (val)        // finite in pass 0 (already stored), not finite in pass 1: the pair is NaN
        for (int e = tid; e < PATH_TILE * PATH_TILE; e += PATH_THREADS) {
            const int c = e % PATH_TILE, r = e / PATH_TILE;
            if (!((okG[0][c] >> r) & 1ull) || ((okG[1][r] >> c) & 1ull) || row0 + r >= bx || col0 + c >= by) continue;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                val[((long)ch * bx + row0 + r) * by + col0 + c] = __builtin_nan("");
                if (mirror) val[((long)(4 + ch) * bx + col0 + c) * by + row0 + r] = __builtin_nan("");
            }
        }
    if (adj) {
        const long W = ((long)by + 63) / 64;
        if (tid < PATH_TILE) {
            if (row0 + tid < bx) adj[(long)(row0 + tid) * W + tj] = bitS[0][tid] & bitG[1][tid];
        } else if (mirror && tid < 2 * PATH_TILE) {
            const int c = tid - PATH_TILE;
            if (col0 + c < by) adj[(long)(col0 + c) * W + ti] = bitG[0][c] & bitS[1][c];
        }
    }
}

hipError_t launch_compare_path(int count, int bx, const double* px, int by, const double* py, int metric, double eps,
                               double* val, unsigned long long* adj, hipStream_t st) {
    const int self = py == nullptr;
    if (self) { by = bx; py = px; }
    const long tr = ((long)bx + PATH_TILE - 1) / PATH_TILE, tc = ((long)by + PATH_TILE - 1) / PATH_TILE;
    if (tr > 65535) return hipErrorInvalidValue;          // blockIdx.y
    hipLaunchKernelGGL(k_compare_path, dim3((unsigned)tc, (unsigned)tr), dim3(PATH_THREADS), 0, st, count, bx, px, by,
                       py, self, metric, eps, val, adj);
    return hipGetLastError();
}

}  // namespace ato
