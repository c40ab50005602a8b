// ato_mesh_pair.hpp -- the point-triangle pair arithmetic of the mesh kernels and the tile culling
// of the strided signed distance (ato_mesh.hip).
//
// Shared by k_mesh_sdist, k_mesh_sdist_tiles and the CPU twin (tests/native/clearance_hostcheck.cpp):
// everything below is ATO_HD or host-inline.
//   * closest_on_triangle: Voronoi-region test (Ericson, Real-Time Collision Detection 5.1.5)
//   * ray_hits: Moller-Trumbore against the fixed ray direction RAY_X/Y/Z
//   * tiles: a second copy of the triangles, sorted by the Morton code of their centroids and cut into
//     runs of MESH_TILE, each with an axis-aligned box inflated by MESH_BOX_INFLATE relative to the
//     mesh's largest coordinate
//   * box_lb2 / ray_meets_box: the two per-lane tests behind the wave-uniform skip decisions. Both err to
//     the side of visiting. The rounding of a pair's own arithmetic is a few ulps of |p| + |mesh|: for
//     points of the mesh's scale (up to 1e6 times it) the absolute pad of the boxes is orders above it;
//     for points farther away, where the distance is of the size of |p| itself, the relative
//     MESH_LB_SLACK on the bound and MESH_RAY_SLACK on the slab parameters are. A point with a
//     non-finite or absurd (>= 1e150) coordinate never lowers a best (its squared distances are inf or
//     NaN) and visits every tile for the parity, as the brute-force kernel does.
// A minimum and a crossing parity do not depend on the visiting order, so the tiled traversal (culled
// or not) returns what the brute-force kernel returns on the same points.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#ifndef ATO_HD
#ifdef __HIPCC__
#define ATO_HD __host__ __device__ __forceinline__
#else
#define ATO_HD inline
#endif
#endif
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <vector>

namespace ato_mesh_pair {

constexpr int MESH_TILE = 32;                 // triangles per tile
constexpr double MESH_BOX_INFLATE = 1e-9;     // relative inflation of a tile's box
constexpr double MESH_LB_SLACK = 1.0 - 4e-9;  // factor on the squared lower bound (2e-9 of the distance)
constexpr double MESH_RAY_SLACK = 4e-9;       // relative slack on the slab parameters
constexpr double MESH_SANE = 1e150;           // coordinates at or above it (or NaN) are not culled for parity
// fixed, generic ray direction (not aligned with any mesh edge or face of an axis-aligned arena)
constexpr double RAY_X = 0.8017837257372732, RAY_Y = 0.5345224838248488, RAY_Z = 0.2672612419124244;

struct V3 {
    double x, y, z;
};
ATO_HD V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
ATO_HD V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
ATO_HD V3 mul(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
ATO_HD double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ATO_HD V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// closest point to p on triangle (a, a + ab, a + ac)
ATO_HD V3 closest_on_triangle(V3 p, V3 a, V3 ab, V3 ac) {
    const V3 ap = sub(p, a);
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return a;
    const V3 bp = sub(ap, ab);
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return add(a, ab);
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) return add(a, mul(ab, d1 / (d1 - d3)));
    const V3 cp = sub(ap, ac);
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return add(a, ac);
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) return add(a, mul(ac, d2 / (d2 - d6)));
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        return add(add(a, ab), mul(sub(ac, ab), w));
    }
    const double den = 1.0 / (va + vb + vc);
    return add(a, add(mul(ab, vb * den), mul(ac, vc * den)));
}

// does the ray p + t RAY (t > 0) cross the triangle
ATO_HD bool ray_hits(V3 p, V3 a, V3 ab, V3 ac) {
    const V3 d = {RAY_X, RAY_Y, RAY_Z};
    const V3 pv = cross(d, ac);
    const double det = dot(ab, pv);
    if (fabs(det) < 1e-300) return false;
    const double inv = 1.0 / det;
    const V3 tv = sub(p, a);
    const double u = dot(tv, pv) * inv;
    if (u < 0.0 || u > 1.0) return false;
    const V3 qv = cross(tv, ab);
    const double v = dot(d, qv) * inv;
    if (v < 0.0 || u + v > 1.0) return false;
    return dot(ac, qv) * inv > 0.0;
}

// squared distance of p to the triangle q[9] = (a, b - a, c - a)
ATO_HD double pair_dist2(V3 p, const double* q) {
    const V3 a = {q[0], q[1], q[2]}, ab = {q[3], q[4], q[5]}, ac = {q[6], q[7], q[8]};
    const V3 dv = sub(p, closest_on_triangle(p, a, ab, ac));
    return dot(dv, dv);
}
ATO_HD bool pair_ray(V3 p, const double* q) {
    const V3 a = {q[0], q[1], q[2]}, ab = {q[3], q[4], q[5]}, ac = {q[6], q[7], q[8]};
    return ray_hits(p, a, ab, ac);
}

// lower bound of the squared distance of p to anything inside the box bx[6] = (lo xyz, hi xyz)
ATO_HD double box_lb2(V3 p, const double* bx) {
    const double dx = fmax(fmax(bx[0] - p.x, p.x - bx[3]), 0.0);
    const double dy = fmax(fmax(bx[1] - p.y, p.y - bx[4]), 0.0);
    const double dz = fmax(fmax(bx[2] - p.z, p.z - bx[5]), 0.0);
    return (dx * dx + dy * dy + dz * dz) * MESH_LB_SLACK;
}

// does the ray p + t RAY (t >= 0) meet the box (slab test; every RAY component is nonzero)
ATO_HD bool ray_meets_box(V3 p, const double* bx) {
    if (!(fabs(p.x) < MESH_SANE && fabs(p.y) < MESH_SANE && fabs(p.z) < MESH_SANE)) return true;
    const double ix = 1.0 / RAY_X, iy = 1.0 / RAY_Y, iz = 1.0 / RAY_Z;   // all positive
    const double t0 = fmax(fmax((bx[0] - p.x) * ix, (bx[1] - p.y) * iy), (bx[2] - p.z) * iz);
    const double t1 = fmin(fmin((bx[3] - p.x) * ix, (bx[4] - p.y) * iy), (bx[5] - p.z) * iz);
    const double tol = MESH_RAY_SLACK * fmax(fabs(t0), fabs(t1));
    return t1 + tol >= 0.0 && t0 <= t1 + tol;
}

inline int mesh_tiles(int nf) { return (nf + MESH_TILE - 1) / MESH_TILE; }

// Morton code of a point of [0, 1)^3 quantised to 10 bits per axis
inline uint32_t morton3(double x, double y, double z) {
    auto spread = [](uint32_t v) {
        v &= 0x3ffu;
        v = (v | (v << 16)) & 0x030000ffu;
        v = (v | (v << 8)) & 0x0300f00fu;
        v = (v | (v << 4)) & 0x030c30c3u;
        v = (v | (v << 2)) & 0x09249249u;
        return v;
    };
    auto q = [](double t) { return (uint32_t)std::min(1023.0, std::max(0.0, t * 1024.0)); };
    return spread(q(x)) | (spread(q(y)) << 1) | (spread(q(z)) << 2);
}

// tri [nf][9] (a, b - a, c - a) -> sorted [nf][9] in Morton order of the centroids (ties: face order) and
// boxes [mesh_tiles(nf)][6] of the runs of MESH_TILE, inflated
inline void build_tiles(const std::vector<double>& tri, int nf, std::vector<double>& sorted,
                        std::vector<double>& boxes) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, amax = 0.0;
    auto vertex = [&](int f, int j, int c) {
        const double* q = &tri[(size_t)f * 9];
        return j == 0 ? q[c] : q[c] + q[3 * j + c];
    };
    for (int f = 0; f < nf; ++f)
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 3; ++c) {
                const double v = vertex(f, j, c);
                lo[c] = std::min(lo[c], v);
                hi[c] = std::max(hi[c], v);
                amax = std::max(amax, std::fabs(v));
            }
    std::vector<uint32_t> code(nf);
    for (int f = 0; f < nf; ++f) {
        double u[3];
        for (int c = 0; c < 3; ++c) {
            const double cen = (vertex(f, 0, c) + vertex(f, 1, c) + vertex(f, 2, c)) / 3.0;
            u[c] = hi[c] > lo[c] ? (cen - lo[c]) / (hi[c] - lo[c]) : 0.0;
        }
        code[f] = morton3(u[0], u[1], u[2]);
    }
    std::vector<int> order(nf);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return code[a] < code[b]; });
    sorted.resize((size_t)nf * 9);
    const int nt = mesh_tiles(nf);
    boxes.assign((size_t)nt * 6, 0.0);
    const double pad = MESH_BOX_INFLATE * std::max(1.0, amax);
    for (int t = 0; t < nt; ++t) {
        double* bx = &boxes[(size_t)t * 6];
        for (int c = 0; c < 3; ++c) {
            bx[c] = 1e300;
            bx[3 + c] = -1e300;
        }
        for (int i = t * MESH_TILE; i < std::min(nf, (t + 1) * MESH_TILE); ++i) {
            const int f = order[i];
            for (int e = 0; e < 9; ++e) sorted[(size_t)i * 9 + e] = tri[(size_t)f * 9 + e];
            for (int j = 0; j < 3; ++j)
                for (int c = 0; c < 3; ++c) {
                    const double v = vertex(f, j, c);
                    bx[c] = std::min(bx[c], v);
                    bx[3 + c] = std::max(bx[3 + c], v);
                }
        }
        for (int c = 0; c < 3; ++c) {
            bx[c] -= pad;
            bx[3 + c] += pad;
        }
    }
}

}  // namespace ato_mesh_pair
