// ato_mesh.hip -- signed distance of points to a triangle mesh (the obstacle environment of
// scripts/obstacles.py). Replaces trimesh.proximity.signed_distance / closest_point as used by
// MeshObstacle (drone3d/obstacles/mesh_obstacle.py:38-41 signed_distance, :110-145 the tube's
// largest-empty-sphere search, :1312-1327 of base_raceline.py the collision check).
//
// One thread per query point, all triangles streamed through LDS in tiles (the mesh is small:
// 8884 triangles = 640 KB as fp64 edge form; every point needs every triangle, so the kernel
// is compute bound, ~80 flop per point-triangle pair):
//   * unsigned distance: closest point on each triangle (Voronoi-region test, Ericson,
//     Real-Time Collision Detection 5.1.5), minimum over the mesh
//   * sign: parity of the crossings of a fixed ray (Moller-Trumbore); odd = inside
// Result is positive outside, negative inside (MeshObstacle.signed_distance convention).
//
// k_mesh_sdist_tiles is the second form, for coherent point sets of any two-stride layout (the clearance
// audit's 435 k to 7 M points): one wave per 64 consecutive points over Morton-ordered triangle tiles with
// boxes, read through scalar loads, with a wave-uniform skip per tile. Both kernels run the pair arithmetic
// of ato_mesh_pair.hpp and return the same distances.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../include/ato.h"
#include "ato_mesh_pair.hpp"

struct ato_mesh {
    int nf = 0;
    double* d_tri = nullptr;   // [nf][9]: a, b - a, c - a
    // the strided distance's copy: the same triangles in Morton order of their centroids, cut into tiles
    int nt = 0;
    double* d_sorted = nullptr;   // [nf][9]
    double* d_boxes = nullptr;    // [nt][6]: lo xyz, hi xyz (inflated)
};

void ato_internal_set_error(const std::string& msg);   // ato_capi.hip: ato_last_error()

namespace {

int fail(int code, const std::string& m) {
    ato_internal_set_error(m);
    return code;
}

constexpr int TILE = 256;
using namespace ato_mesh_pair;   // V3, closest_on_triangle, ray_hits: ato_mesh_pair.hpp

__global__ __launch_bounds__(TILE) void k_mesh_sdist(int n, const double* __restrict__ pts, int nf,
                                                    const double* __restrict__ tri, double* __restrict__ dist,
                                                    double* __restrict__ closest) {
    __shared__ double tile[TILE * 9];
    const int i = blockIdx.x * TILE + threadIdx.x;
    const bool live = i < n;
    const V3 p = live ? V3{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]} : V3{0, 0, 0};
    double best = 1e300;
    V3 bq = p;
    int crossings = 0;
    for (int t0 = 0; t0 < nf; t0 += TILE) {
        const int cnt = min(TILE, nf - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 9; e += TILE) tile[e] = tri[(long)t0 * 9 + e];
        __syncthreads();
        if (live) {
            for (int t = 0; t < cnt; ++t) {
                const double* q = tile + t * 9;
                const V3 a = {q[0], q[1], q[2]}, ab = {q[3], q[4], q[5]}, ac = {q[6], q[7], q[8]};
                const V3 c = closest_on_triangle(p, a, ab, ac);
                const V3 dv = sub(p, c);
                const double d2 = dot(dv, dv);
                if (d2 < best) {
                    best = d2;
                    bq = c;
                }
                crossings += ray_hits(p, a, ab, ac) ? 1 : 0;
            }
        }
    }
    if (!live) return;
    const double d = sqrt(best);
    dist[i] = (crossings & 1) ? -d : d;
    if (closest) {
        closest[3 * i] = bq.x;
        closest[3 * i + 1] = bq.y;
        closest[3 * i + 2] = bq.z;
    }
}

// Signed distance of coherent point sets: one wave = 64 consecutive points, component c of point i at
// pts[i sp + c sc]. Every wave walks the Morton-ordered tiles on its own: the tile index is wave-uniform,
// so the boxes and the triangles come through scalar loads (L2: the mesh is 640 KB), there is no LDS and
// no barrier. cull: a tile's distance pass is skipped when no lane's box lower bound is below that lane's
// best, its crossing pass when no lane's ray meets the box; the bests are seeded from the tile nearest
// the wave's first point. The lanes past n repeat point n - 1 and write nothing.
constexpr int SD_BLOCK = 256;

__global__ __launch_bounds__(SD_BLOCK) void k_mesh_sdist_tiles(long n, const double* __restrict__ pts, long sp,
                                                              long sc, int nf, int nt,
                                                              const double* __restrict__ tri,
                                                              const double* __restrict__ boxes,
                                                              double* __restrict__ dist, int cull) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long i0 = (long)blockIdx.x * SD_BLOCK + (long)wave * 64;   // the wave's first point: uniform
    if (i0 >= n) return;
    const long i = (long)blockIdx.x * SD_BLOCK + threadIdx.x;
    const long ii = i < n ? i : n - 1;
    const V3 p = {pts[ii * sp], pts[ii * sp + sc], pts[ii * sp + 2 * sc]};
    double best = 1e300;
    int crossings = 0;
    int seed = -1;
    if (cull) {
        // tile 0 unless another is strictly nearer: a non-finite first point still names a tile
        const V3 p0 = {pts[i0 * sp], pts[i0 * sp + sc], pts[i0 * sp + 2 * sc]};
        double lb0 = box_lb2(p0, boxes);
        seed = 0;
        for (int t = 1; t < nt; ++t) {
            const double lb = box_lb2(p0, boxes + (long)t * 6);
            if (lb < lb0) {
                lb0 = lb;
                seed = t;
            }
        }
        seed = __builtin_amdgcn_readfirstlane(seed);
        const int cnt = min(MESH_TILE, nf - seed * MESH_TILE);
        for (int k = 0; k < cnt; ++k) best = fmin(best, pair_dist2(p, tri + ((long)seed * MESH_TILE + k) * 9));
    }
    for (int t = 0; t < nt; ++t) {
        bool nd = true, nr = true;
        if (cull) {
            const double* bx = boxes + (long)t * 6;
            nd = t != seed && __any(box_lb2(p, bx) < best) != 0;
            nr = __any(ray_meets_box(p, bx)) != 0;
            if (!nd && !nr) continue;
        }
        const int cnt = min(MESH_TILE, nf - t * MESH_TILE);
        for (int k = 0; k < cnt; ++k) {
            const double* q = tri + ((long)t * MESH_TILE + k) * 9;
            if (nd) best = fmin(best, pair_dist2(p, q));
            if (nr) crossings += pair_ray(p, q) ? 1 : 0;
        }
    }
    if (i >= n) return;
    const double d = sqrt(best);
    dist[i] = (crossings & 1) ? -d : d;
}

}  // namespace

extern "C" {

int ato_mesh_create(const double* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                    ato_mesh** out) {
    if (!vertices || !faces || !out || n_vertices < 3 || n_faces < 1) return fail(ATO_ERR_ARG, "bad mesh arguments");
    std::vector<double> tri((size_t)n_faces * 9);
    for (int f = 0; f < n_faces; ++f) {
        int idx[3];
        for (int j = 0; j < 3; ++j) {
            idx[j] = faces[3 * f + j];
            if (idx[j] < 0 || idx[j] >= n_vertices) return fail(ATO_ERR_ARG, "face index out of range");
        }
        for (int c = 0; c < 3; ++c) {
            const double a = vertices[3 * idx[0] + c];
            tri[(size_t)f * 9 + c] = a;
            tri[(size_t)f * 9 + 3 + c] = vertices[3 * idx[1] + c] - a;
            tri[(size_t)f * 9 + 6 + c] = vertices[3 * idx[2] + c] - a;
        }
    }
    std::vector<double> sorted, boxes;
    build_tiles(tri, n_faces, sorted, boxes);
    auto* m = new ato_mesh();
    m->nf = n_faces;
    m->nt = mesh_tiles(n_faces);
    if (hipMalloc(&m->d_tri, tri.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(m->d_tri, tri.data(), tri.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&m->d_sorted, sorted.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(m->d_sorted, sorted.data(), sorted.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&m->d_boxes, boxes.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(m->d_boxes, boxes.data(), boxes.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(m->d_tri);
        (void)hipFree(m->d_sorted);
        (void)hipFree(m->d_boxes);
        delete m;
        return fail(ATO_ERR_HIP, "mesh upload failed");
    }
    *out = m;
    return ATO_OK;
}

int ato_mesh_destroy(ato_mesh* m) {
    if (!m) return ATO_OK;
    (void)hipFree(m->d_tri);
    (void)hipFree(m->d_sorted);
    (void)hipFree(m->d_boxes);
    delete m;
    return ATO_OK;
}

int ato_mesh_signed_distance(ato_mesh* m, int32_t n, const double* points, double* dist, double* closest,
                             void* stream) {
    if (!m || n < 0 || (n > 0 && (!points || !dist))) return fail(ATO_ERR_ARG, "bad distance arguments");
    if (n == 0) return ATO_OK;
    hipLaunchKernelGGL(k_mesh_sdist, dim3((n + TILE - 1) / TILE), dim3(TILE), 0, (hipStream_t)stream, n, points,
                       m->nf, (const double*)m->d_tri, dist, closest);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ATO_OK : fail(ATO_ERR_HIP, hipGetErrorString(e));
}

int ato_mesh_signed_distance_strided(ato_mesh* m, int64_t n, const double* points, int64_t stride_point,
                                     int64_t stride_comp, double* dist, int32_t cull, void* stream) {
    if (!m || n < 0 || (n > 0 && (!points || !dist)) || stride_point < 1 || stride_comp < 1 || (cull != 0 && cull != 1))
        return fail(ATO_ERR_ARG, "bad strided distance arguments");
    if (n == 0) return ATO_OK;
    const int64_t blocks = (n + SD_BLOCK - 1) / SD_BLOCK;
    if (blocks > 0x7fffffffLL) return fail(ATO_ERR_ARG, "too many points for one launch");
    hipLaunchKernelGGL(k_mesh_sdist_tiles, dim3((unsigned)blocks), dim3(SD_BLOCK), 0, (hipStream_t)stream, (long)n,
                       points, (long)stride_point, (long)stride_comp, m->nf, m->nt, (const double*)m->d_sorted,
                       (const double*)m->d_boxes, dist, (int)cull);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ATO_OK : fail(ATO_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
