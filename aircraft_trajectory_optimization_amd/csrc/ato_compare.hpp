// ato_compare.hpp -- which solutions of a batch are the same line: pairwise distances of racelines and the
// connected components of "closer than eps".
//
// Three steps, each an entry of include/ato.h:
//   sample   positions of every instance at M equal fractions f_j = j / (M - 1) of its OWN lap, the export's state
//            channels 3-5 with `relative` (export_tstart, export_interp, export_lift of ato_export.hpp; nothing is
//            restated here), as a table [3][M][B], instance fastest, whatever the input layout.
//   pairs    for every pair (a, b) of two such tables, with d2_j = |x_a(f_j) - y_b(f_j)|^2 by compare_d2 below:
//              rms = sqrt((sum_j d2_j) / M), the sum sequential in ascending j,
//              max = sqrt(max_j d2_j),
//              at  = f_j of the earliest j whose d2_j attains that maximum (the distance is compared squared: the
//                    square root is monotone, and is taken once per pair instead of once per sample),
//            and the adjacency bit "metric <= eps". A pair whose sum is not finite (a NaN or infinite position, or
//            an overflowing difference) gets NaN in all three channels and no bit. d2 is symmetric bit for bit
//            ((a - b)^2 and (b - a)^2 round alike) and the order over j is fixed, so a pair's numbers depend on
//            nothing but its two columns: not on the batch sizes, not on the tile it falls in, not on which side it
//            is. A self-comparison computes the tiles on and above the diagonal and mirrors them; its diagonal is
//            exactly zero for finite columns.
//   groups   the connected components of the adjacency united with its transpose (single linkage at eps): every
//            instance gets the smallest index of its component.
//
// Why direct differences on the vector units and no matrix instructions: the Gram form |a|^2 + |b|^2 - 2 a.b would
// turn the pair loop into a matrix product, but it cancels catastrophically exactly for the pairs this exists to
// find (two copies of one line: d^2 ~ 1e-12 m^2 against norms of 1e4 M m^2 leaves no correct digit in fp64), and a
// product of sums cannot give the maximum over j at all.
//
// The groups kernel is one workgroup with the labels in LDS (GROUP_MAX of them). A sweep pushes the smaller label
// across every set bit (both ways: the union with the transpose) and then jumps pointers once,
// label[i] = label[label[i]]. Labels only decrease, are always the index of an instance of the same component, and
// after sweep t every instance within t edges of its component's smallest index holds it; the diameter is at most
// batch - 1, so sweep number `batch` at the latest changes nothing. The loop runs until a sweep changes nothing and
// never more than `batch` sweeps: no device loop waits on a data-dependent condition alone. Within a sweep the
// threads race on intermediate labels (LDS atomic minima and plain reads); the fixpoint -- no edge joins two
// labels, every label its component's minimum -- is unique, so the output does not depend on the race.
//
// Not covered here: an alignment in space -- two lines on one path with different speed profiles are different to
// the pair kernel; ato_path.hpp (ato_compare_path) compares the same tables as paths and feeds the same groups.
// Not covered at all: anything but position, the curve between the samples, RK4 transcriptions. It certifies nothing.
#pragma once
#include "ato_export.hpp"

namespace ato {

constexpr int CMP_NCH = ATO_COMPARE_NCH;
constexpr int CMP_TILE = 64;       // a workgroup's tile of pairs is CMP_TILE x CMP_TILE = one adjacency word per row
constexpr int CMP_RB = 4;          // a thread's register block is CMP_RB x CMP_RB pairs
constexpr int CMP_CHUNK = 16;      // samples of both operands staged in LDS at a time (2 x 3 x 16 x 64 doubles = 48 kB)
constexpr int CMP_GROUP_BLOCK = 1024;
// labels of the groups kernel: 64 kB of LDS less the two words of the "a sweep changed something" flags
constexpr int GROUP_MAX = 65536 / 4 - 2;
enum { CMP_RMS = 0, CMP_MAX = 1, CMP_AT = 2 };
enum { CMP_METRIC_MAX = 0, CMP_METRIC_RMS = 1 };

// 0 (ATO_OK) or the error code of an ato_compare_sample call: export_check's tests in export_check's order
inline int compare_sample_check(const ProbD& p, bool has_line, int batch, int layout, int count, bool has_w,
                                bool has_pos, const char** msg) {
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (int rc = check_layout(layout, msg)) return rc;
    if (count < 2) { *msg = "count must be >= 2"; return ATO_ERR_ARG; }
    if (!has_w || !has_pos) { *msg = "null buffer"; return ATO_ERR_ARG; }
    if (int rc = check_collocation(p, "comparison of RK4-transcribed problems (K = 0) is not supported", msg)) return rc;
    return check_line(p, has_line, "parametric comparison needs the centreline table (ato_clearance_set_line)", msg);
}

inline int compare_pairs_check(int count, int bx, bool has_px, int by, bool self, int metric, double eps, bool has_val,
                               bool has_adj, const char** msg) {
    *msg = "";
    if (count < 2) { *msg = "count must be >= 2"; return ATO_ERR_ARG; }
    if (bx < 1 || (!self && by < 1)) { *msg = "batch must be >= 1"; return ATO_ERR_ARG; }
    if (!has_px) { *msg = "null buffer"; return ATO_ERR_ARG; }
    if (!has_val && !has_adj) { *msg = "nothing to compare: val and adj are both NULL"; return ATO_ERR_ARG; }
    if (metric != CMP_METRIC_MAX && metric != CMP_METRIC_RMS) { *msg = "unknown metric"; return ATO_ERR_ARG; }
    if (has_adj && !(eps >= 0.0)) { *msg = "eps must be >= 0"; return ATO_ERR_ARG; }
    return ATO_OK;
}

inline int compare_groups_check(int batch, bool has_adj, bool has_group, bool has_info, const char** msg) {
    *msg = "";
    if (int rc = check_batch(batch, msg)) return rc;
    if (!has_adj || !has_group || !has_info) { *msg = "null buffer"; return ATO_ERR_ARG; }
    if (batch > GROUP_MAX) { *msg = "groups of more than 16382 instances are not supported (labels live in LDS)"; return ATO_ERR_UNSUPPORTED; }
    return ATO_OK;
}

// |a - b|^2: three differences, then x, y, z in fused multiply-adds. Bitwise symmetric in (a, b).
ATO_HD double compare_d2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

// the running record of one pair and one more sample j
struct ComparePair {
    double sum, mx;
    int at;
};
ATO_HD void compare_step(ComparePair& p, double d2, int j) {
    p.sum += d2;
    if (d2 > p.mx) { p.mx = d2; p.at = j; }
}
// the three channels of a finished pair
ATO_HD void compare_finish(const ComparePair& p, int count, double* out) {
    if (p.sum - p.sum != 0.0) {
        out[CMP_RMS] = out[CMP_MAX] = out[CMP_AT] = __builtin_nan("");
        return;
    }
    out[CMP_RMS] = sqrt(p.sum / (double)count);
    out[CMP_MAX] = sqrt(p.mx);
    out[CMP_AT] = (double)p.at / (double)(count - 1);
}

#ifdef __HIPCC__
template <class M>
hipError_t launch_compare_sample(const ExportD& a, int B, int layout, const double* w, double* pos, double* lap,
                                 hipStream_t st);
hipError_t launch_compare_pairs(int count, int bx, const double* px, int by, const double* py, int metric, double eps,
                                double* val, unsigned long long* adj, hipStream_t st);
hipError_t launch_compare_groups(int batch, const unsigned long long* adj, int* group, int* info, hipStream_t st);
#endif  // __HIPCC__

}  // namespace ato
