// ato_path.hpp -- racelines compared as paths: for every pair of columns of two position tables the directed
// point-to-polyline distances, both ways (include/ato.h, ato_compare_path).
//
// ato_compare_pairs (ato_compare.hpp) compares positions at equal lap fractions, so one path flown at two speed
// profiles is two lines there. Here line b is the polyline through its M samples (M - 1 segments; a closed lap
// closes by itself because f = 1 repeats f = 0) and every sample of line a is measured against all of it.
//
// Point p against segment (q0, q1), with the prepared record (q0, e, inv) of path_segment:
//   e = q1 - q0, inv = 1 / (e.e) (0 where e.e == 0), r = p - q0,
//   t = clamp((r.e) inv, 0, 1), c = r - t e by fused multiply-adds, d2 = c.c;
// the dot products are fused multiply-adds over z, y, x as compare_d2 forms them. Where (e.e) inv rounds below 1,
// inv is raised by one ulp at preparation: r == e (the far vertex itself) then gives t == 1 and c == 0 exactly,
// so a line has distance exactly zero to itself at every sample, the last one of an open line included.
// The directed record of (a -> b):
//   D_i   = min over the segments s of b, ascending, the first of equals, of d2(x_a(f_i), segment s)
//   rms   = sqrt((sum_i D_i) / M), the sum sequential in ascending i
//   max   = sqrt(max_i D_i)
//   at    = f_i of the earliest i attaining the maximum
//   where = (s* + t*) / (M - 1), the lap fraction ON b of the point nearest to that sample (t* is recomputed once
//           per pair by path_t on the same record: the loop carries the segment index only)
// Eight channels per pair: 0-3 are rms, max, at, where of a -> b, 4-7 those of b -> a; the Hausdorff distance is
// max(ch 1, ch 5); the adjacency bit is "metric(a -> b) <= eps and metric(b -> a) <= eps". A pair whose sum is not
// finite in either direction has NaN in all eight channels and no bit (a NaN d2 never wins the minimum, so a
// sample without a finite segment keeps D_i = +inf). Every number of a pair is a function of its two columns
// alone and the same instructions form (a -> b) whichever operand a is: a self-comparison is symmetric under
// swapping the channel halves bit for bit, and its diagonal is exactly zero.
//
// The kernel (ato_path.hip). A workgroup of 256 threads owns a tile of 64 x 64 pairs and runs two passes with the
// operands' roles swapped: pass 0 measures the samples of the 64 rows against the segments of the 64 columns,
// pass 1 the samples of the columns against the segments of the rows. In a pass, lane l of every wave owns
// sample-side instance l; wave w of sweep `sub` owns the PATH_C = 4 segment-side instances sub 16 + 4 w + k. A
// thread holds PATH_R = 4 sample points of its instance and a running (d2 minimum, segment) for each of the
// 4 x 4 (point, segment-side instance) combinations, and streams every segment of its four instances past them:
// the segments come through LDS in chunks of PATH_CHUNK = 32 as prepared records (16 instances x 32 segments x 8
// doubles: the seven of PathSeg and one of padding, so that a record is read in 16-byte pieces), prepared once
// per (instance, segment) when the chunk is staged, so the inner loop has no division; a wave reads a record at
// one address (a broadcast), and one read serves the R = 4 points. The samples of an instance are not spread
// over threads: the thread folds its blocks of R samples in ascending order itself (path_step), which is the
// fixed order of the contract with no exchange at all. The four channels of a sweep go through a 4 x 64 x 16 tile
// in LDS (pitch 17, in the staging buffer's place) and leave it twice: along the segment-side index (16
// consecutive doubles) and along the sample-side index (64 consecutive doubles) -- one of the two is the pass's
// own half of the channels, the other the mirror image of an off-diagonal tile of a self-comparison with the
// halves swapped, so every store runs along a row of val. Of a self-comparison only the tiles with column tile >=
// row tile run. The directed bits of pass 0 wait in LDS, as one word per row (LDS atomic OR, order-independent)
// and one per column (a wave's ballot), and are ANDed with those of pass 1; one thread stores each adjacency
// word whole: no global atomics, padding bits stay zero. Pass 1 writes NaN where pass 0 was not finite, and the
// channels pass 0 has already stored are overwritten with NaN where pass 1 turns out not finite.
// R, C, the tile and the chunk: the state of a thread is 3 R C + 6 R + 6 C = 96 registers, and the compiler keeps
// the records of the four instances and the next ones in flight beside it: 219 VGPRs, two waves per SIMD, which
// the LDS allows as well (34 816 B of tile or records plus 3 kB of bit words, 37 888 B per workgroup). R = C = 4
// is the largest square block that stays out of scratch with the records in flight; R sets the LDS traffic (7 / R
// doubles per point-segment evaluation, a broadcast), C the reuse of a thread's points. The tile is 64 wide
// because a lane is an instance and a tile row is one adjacency word; the chunk is what the result tile's space
// holds. No scratch (profiles/path/kernel_resource_usage.txt).
//
// Error bound (u = 2^-53; d the exact directed distance of the fp64 inputs, L the longest segment of the polyline
// measured against). For one point and one segment, with rho = |r| <= d_s + L:
//   * r and e are single roundings of exact differences: the computed data are a point moved by <= u rho and a
//     far vertex moved by <= u L; the distance to a segment is 1-Lipschitz in each, so the exact distance of the
//     computed data is within u (d_s + 2 L) of d_s;
//   * t: the dot product has three roundings (<= 3 u rho L absolute), e.e three, inv two and the possible ulp,
//     the product one: before the clamp t is off by <= 3 u rho / L + 7 u |t|, and the clamp is 1-Lipschitz and
//     cuts |t| to 1, so |t - t_exact| L <= 3 u rho + 7 u L <= 3 u d_s + 10 u L; a point q0 + t e of the segment
//     that far from the nearest one is at most that much farther from p (triangle inequality);
//   * c has one rounding per component (u |c|), c.c three (1.5 u on the root), the root one: 3.5 u d_s.
// Sum: |d_computed - d_s| <= u (7.5 d_s + 12 L) + O(u^2) <= 12 u (d_s + L). The minimum over the segments of
// values each that close to its own exact value is that close to the exact minimum, the maximum over i likewise:
//   |max - max_exact| <= PATH_ERR_C u (max_exact + L), PATH_ERR_C = 13 (12 and one for the second-order terms).
// rms: with D_i = (d_i + a_i)^2, |a_i| <= 12 u (d_i + L), Minkowski gives sqrt(mean D_i) within
// 12 u (rms_exact + L) of rms_exact; the sequential sum of M non-negative terms adds (M - 1) u relative, the
// division u, the root halves both and adds u:
//   |rms - rms_exact| <= (PATH_ERR_C + 1 + M / 2) u (rms_exact + L).
// where: s* + t* is rounded at magnitude < M and divided by M - 1; read back, t* is off by <= 2 M u, the point on
// b by <= 2 M u L: the exact distance from sample `at` to the point `where` is within
// PATH_ERR_C u (max + L) + 2 M u L of max.
//
// Not covered: anything but position, the curve between the samples (the polyline is compared, not the
// collocation polynomial), RK4 transcriptions. It certifies nothing.
#pragma once
#include "ato_compare.hpp"

namespace ato {

constexpr int PATH_NCH = ATO_COMPARE_PATH_NCH;
constexpr int PATH_TILE = 64;      // a workgroup's tile of pairs is PATH_TILE x PATH_TILE: one adjacency word per row
constexpr int PATH_R = 4;          // sample points a thread holds at a time
constexpr int PATH_C = 4;          // segment-side instances a thread measures them against
constexpr int PATH_CHUNK = 32;     // segments of 16 instances staged in LDS at a time, as records
constexpr int PATH_REC = 8;        // doubles per record in LDS: PathSeg and one of padding
constexpr int PATH_ERR_C = 13;     // the error bound's constant (above)
enum { PATH_CH_RMS = 0, PATH_CH_MAX = 1, PATH_CH_AT = 2, PATH_CH_WHERE = 3 };

// a prepared segment: first vertex, edge, 1 / |edge|^2
struct PathSeg {
    double qx, qy, qz, ex, ey, ez, inv;
};
ATO_HD PathSeg path_segment(double ax, double ay, double az, double bx, double by, double bz) {
    PathSeg g{ax, ay, az, bx - ax, by - ay, bz - az, 0.0};
    const double ee = fma(g.ez, g.ez, fma(g.ey, g.ey, g.ex * g.ex));
    if (ee != 0.0) {
        g.inv = 1.0 / ee;
        if (ee * g.inv < 1.0) g.inv = nextafter(g.inv, __builtin_inf());   // the far vertex projects to t == 1
    }
    return g;
}
// the clamped parameter of the point q0 + r nearest on the segment (a NaN product clamps to 0)
ATO_HD double path_t(const PathSeg& g, double rx, double ry, double rz) {
    const double dot = fma(rz, g.ez, fma(ry, g.ey, rx * g.ex));
    return fmin(fmax(dot * g.inv, 0.0), 1.0);
}
// squared distance of p to the segment
ATO_HD double path_d2(const PathSeg& g, double px, double py, double pz) {
    const double rx = px - g.qx, ry = py - g.qy, rz = pz - g.qz;
    const double t = path_t(g, rx, ry, rz);
    const double cx = fma(-t, g.ex, rx), cy = fma(-t, g.ey, ry), cz = fma(-t, g.ez, rz);
    return fma(cz, cz, fma(cy, cy, cx * cx));
}

// the running record of one directed pair and one more sample i with its D_i and nearest segment
struct PathFold {
    double sum, mx;
    int at, seg;
};
ATO_HD void path_step(PathFold& f, double D, int i, int seg) {
    f.sum += D;
    if (D > f.mx) { f.mx = D; f.at = i; f.seg = seg; }
}
// the four channels of a finished direction (t: path_t of sample f.at on segment f.seg); false: not finite
ATO_HD bool path_finish(const PathFold& f, int count, double t, double* out) {
    if (f.sum - f.sum != 0.0) {
        out[PATH_CH_RMS] = out[PATH_CH_MAX] = out[PATH_CH_AT] = out[PATH_CH_WHERE] = __builtin_nan("");
        return false;
    }
    out[PATH_CH_RMS] = sqrt(f.sum / (double)count);
    out[PATH_CH_MAX] = sqrt(f.mx);
    out[PATH_CH_AT] = (double)f.at / (double)(count - 1);
    out[PATH_CH_WHERE] = ((double)f.seg + t) / (double)(count - 1);
    return true;
}

#ifdef __HIPCC__
hipError_t launch_compare_path(int count, int bx, const double* px, int by, const double* py, int metric, double eps,
                               double* val, unsigned long long* adj, hipStream_t st);
#endif  // __HIPCC__

}  // namespace ato
