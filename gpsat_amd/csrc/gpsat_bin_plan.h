// gpsat_bin_plan.h -- host side of gpsat_bin_batch: the argument checks, the layout of the handle's bin buffers and the
// scalars of BinArgs.  Plain C++ without a HIP call, in the manner of gpsat_cvfold.h, so that
// tests/select_bin_host_check.cpp can run it under the host sanitizers.  Part of gpsat_capi.cpp's translation unit.
#ifndef GPSAT_BIN_PLAN_H
#define GPSAT_BIN_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "gpsat_hip.h"
#include "gpsat_key_runs_plan.h"

namespace gpsat {

// Cells of one group: (nx - 1) x (ny - 1) bins, or nx - 1 in 1-D.
inline unsigned long long bin_cells(int nx, int ny, bool two_d) {
    return (unsigned long long)(nx - 1) * (unsigned long long)(two_d ? ny - 1 : 1);
}

// Sizes, the statistics mask, both axes (1-D: y == nullptr), the two cell-count limits and, when there is a row and a group at
// all, x / v and the range of gid.  Returns an empty string, or what is wrong.
inline std::string bin_check(int64_t R, const double* x, const double* y, const double* v, const int32_t* gid, int32_t G,
                             int32_t nx, const double* ex, double x_hi, int32_t ny, const double* ey, double y_hi,
                             uint32_t stats, int64_t capacity) {
    if (R < 0 || G < 0 || capacity < 0) return "gpsat_bin_batch: bad sizes";
    if (R > 2147483647LL) return "gpsat_bin_batch: more than 2^31-1 rows in one call";
    const uint32_t all = GPSAT_BIN_COUNT | GPSAT_BIN_SUM | GPSAT_BIN_MEAN | GPSAT_BIN_STD | GPSAT_BIN_MIN | GPSAT_BIN_MAX | GPSAT_BIN_MEDIAN;
    if (stats == 0 || (stats & ~all)) return "gpsat_bin_batch: stats must be a non-empty OR of GPSAT_BIN_*";
    const bool two_d = y != nullptr;
    auto check_axis = [](const char* name, int n, const double* e, double hi) -> std::string {
        if (n < 2 || !e) return std::string("gpsat_bin_batch: ") + name + " needs at least 2 edges";
        for (int i = 0; i < n; ++i) {
            if (!std::isfinite(e[i])) return std::string("gpsat_bin_batch: ") + name + " edges must be finite";
            if (i > 0 && !(e[i] > e[i - 1])) return std::string("gpsat_bin_batch: ") + name + " edges must be strictly increasing";
        }
        if (!(hi >= e[n - 1])) return std::string("gpsat_bin_batch: the upper limit of the last ") + name + " bin is below the last edge";
        return std::string();
    };
    std::string msg = check_axis("x", nx, ex, x_hi);
    if (msg.empty() && two_d) msg = check_axis("y", ny, ey, y_hi);
    if (!msg.empty()) return msg;
    const unsigned long long cells = bin_cells(nx, ny, two_d);
    if (cells >= (1ull << 31)) return "gpsat_bin_batch: 2^31 or more cells per group";
    if (G > 0 && cells > ((1ull << 63) - 1) / (unsigned long long)G) return "gpsat_bin_batch: G * cells must stay below 2^63";
    if (R == 0 || G == 0) return std::string();        // nothing to bin: the caller returns at once
    if (!x || !v) return "gpsat_bin_batch: x / v is NULL";
    if (gid)
        for (int64_t i = 0; i < R; ++i)
            if (gid[i] < 0 || gid[i] >= G)
                return "gpsat_bin_batch: gid[" + std::to_string(i) + "] = " + std::to_string(gid[i]) + " is not in 0.." + std::to_string(G - 1);
    return std::string();
}

// Bytes of the handle's bin buffers and the byte offsets of what lies in them.  keys, rows and runs are the stage's
// (KeyRunsLayout; runs_counts: n_cells [2]), with binning's own words in and behind `runs`.
struct BinLayout : KeyRunsLayout {
    // `in`: both axes' edges (ex, then ey), rounded to 256 B, then the columns x, v, y (2-D), gid (int32, when given); the room
    // of gid is reserved either way
    size_t in_bytes, in_x, in_v, in_y, in_gid;
    size_t vals_bytes;                // [R] values in sorted order; with the median [3][R]: then one NaN pattern, then sorted per cell
    // `runs` of the stage with n_long at +32 of its 256-B block, the flags [R] rounded to 256 B, then the long cells [R / long_rows + 1]
    size_t runs_n_cells, runs_n_long, runs_long_list;     // runs_n_cells: the stage's runs_counts, by binning's name
};

inline BinLayout bin_layout(int64_t R, int nx, int ny, bool two_d, bool has_gid, bool median, int long_rows) {
    const size_t nR = (size_t)R;
    BinLayout l = {};
    static_cast<KeyRunsLayout&>(l) = key_runs_layout(R);
    const size_t edge_bytes = ((size_t)(nx + (two_d ? ny : 0)) * sizeof(double) + 255) & ~size_t(255);
    l.in_bytes = edge_bytes + (two_d ? 3 : 2) * nR * sizeof(double) + nR * sizeof(int);
    l.in_x = edge_bytes;
    l.in_v = l.in_x + nR * sizeof(double);
    l.in_y = two_d ? l.in_v + nR * sizeof(double) : 0;
    l.in_gid = has_gid ? edge_bytes + (two_d ? 3 : 2) * nR * sizeof(double) : 0;
    l.vals_bytes = (median ? 3 : 1) * nR * sizeof(double);
    l.runs_n_cells = l.runs_counts; l.runs_n_long = l.runs_counts + 32;
    l.runs_long_list = l.runs_flags + ((nR + 255) & ~size_t(255));
    l.runs_bytes = l.runs_long_list + (nR / long_rows + 1) * sizeof(unsigned);
    return l;
}

// The scalars of BinArgs: bins / (last edge - first edge) per axis, the guess of the kernel's bin search (0 where the range
// overflowed: the guess is bin 0, the correction does the rest); the key of rows outside the grid; the statistics asked for.
struct BinScales {
    double inv_x, inv_y;
    unsigned long long sentinel;      // G * cells
    int n_stat;
};

inline BinScales bin_scales(int nx, const double* ex, int ny, const double* ey, bool two_d, int32_t G, uint32_t stats) {
    BinScales s = {};
    s.inv_x = (double)(nx - 1) / (ex[nx - 1] - ex[0]);
    s.inv_y = two_d ? (double)(ny - 1) / (ey[ny - 1] - ey[0]) : 0.0;
    if (!std::isfinite(s.inv_x)) s.inv_x = 0.0;
    if (!std::isfinite(s.inv_y)) s.inv_y = 0.0;
    s.sentinel = bin_cells(nx, ny, two_d) * (unsigned long long)G;
    for (uint32_t b = 1; b <= GPSAT_BIN_MEDIAN; b <<= 1) s.n_stat += (stats & b) ? 1 : 0;
    return s;
}

}  // namespace gpsat
#endif
