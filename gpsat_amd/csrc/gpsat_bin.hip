// gpsat_bin.hip -- binning of raw observations on gfx950: the table that the expert tiles draw from.
//
// Replaces, for all groups (day, satellite, ...) at once, DataPrep.bin_data_by / DataPrep.bin_data
// (GPSat/dataprepper.py:21-401): per group a boolean mask over the whole frame and scipy.stats.binned_statistic(_2d) on a
// regular grid.  The results are scipy's BIT FOR BIT (finite values), whatever the grid, the launch or the batch:
//   * bin membership is decided by comparing the coordinate with the edge VALUES the host made with np.linspace
//     (np.digitize: edges[i] <= x < edges[i+1]); the last bin also takes [edges[-1], x_hi], the interval of scipy's
//     rounded right-edge test, found on the host with np.around itself;
//   * scipy's sum / mean / std are np.bincount sums: sequential fp64 additions from 0.0 in SOURCE ROW ORDER.  The rows are
//     sorted by cell with a STABLE radix sort, so a cell's rows stay in source order, and one lane walks its cell's rows in
//     that order with uncontracted arithmetic (__dadd_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn; -ffp-contract=on would
//     otherwise fuse d*d + q).  No float atomics, no tree reduction: both would change the order of the additions.
// Stages: (1) 64-bit cell key per row, key = (gid (ny-1) + iy)(nx-1) + ix, rows outside the grid / with a NaN coordinate
// get the sentinel key G*cells and sort behind everything; (2) the keyed sort-and-run-heads stage (gpsat_key_runs.hip), with
// the gather of the values into sorted order in the pass that writes its head flags; (3) one lane per non-empty cell, results
// written sparse in ascending key order; cells of BIN_LONG rows or more are left to one WAVE each (bin_long_kernel), which
// loads 64 values at a time and adds them in the same order.  The median sorts every cell's values (rocPRIM segmented
// radix sort, NaN last as np.lexsort has it) and is only computed when asked for.
// NaN VALUES follow scipy per statistic: count counts them; sum / mean / std / max are NaN; min ignores them (NaN only
// when the cell holds nothing else); the median orders them last.
//
// This is HBM/L2-bound streaming, no MFMA, no LDS: the edges (<= a few thousand doubles) stay in L1/L2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include "gpsat_kernels.h"

namespace gpsat {

// np.digitize(x, e) - 1 with scipy's right-edge shift; -1: outside the grid (below e[0], beyond hi, NaN)
__device__ __forceinline__ int bin_index(double x, const double* __restrict__ e, int n, double inv_step, double hi) {
    if (!(x >= e[0])) return -1;                       // below the first edge, or NaN
    if (x >= e[n - 1]) return (x <= hi) ? n - 2 : -1;   // on / just above the last edge: the last bin; +inf: outside
    // e[0] <= x < e[n-1]: a guess from the mean step, corrected against the edge values (np.linspace edges differ from
    // e[0] + k step by an ulp or two: the loops run once or twice; any increasing edges end them inside [0, n-2])
    int k = (int)fmin((x - e[0]) * inv_step, (double)(n - 2));
    while (x < e[k]) --k;
    while (x >= e[k + 1]) ++k;
    return k;
}

__global__ void __launch_bounds__(256) bin_key_kernel(const BinArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.R) return;
    const int ix = bin_index(a.x[i], a.ex, a.nx, a.inv_x, a.x_hi);
    const int iy = a.y ? bin_index(a.y[i], a.ey, a.ny, a.inv_y, a.y_hi) : 0;
    unsigned long long key = a.sentinel;
    if (ix >= 0 && iy >= 0) {
        const unsigned long long g = a.gid ? (unsigned long long)a.gid[i] : 0ull;     // 0 <= gid < G checked by the host
        const unsigned long long rows_y = a.y ? (unsigned long long)(a.ny - 1) : 1ull;
        key = (g * rows_y + (unsigned long long)iy) * (unsigned long long)(a.nx - 1) + (unsigned long long)ix;
    }
    a.keys[i] = key;
    a.rows[i] = (unsigned)i;
}

// values into sorted order (coalesced writes, scattered reads) and the head flag of every run of equal keys
__global__ void __launch_bounds__(256) bin_gather_kernel(const BinArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.R) return;
    a.vs[i] = a.v[a.perm[i]];
    a.flags[i] = key_run_head(a.keys_sorted, i);
}

// the copy the median sorts: every NaN becomes the positive quiet NaN, which the radix order puts behind +inf (a NaN with
// the sign bit set would sort in front of -inf; np.lexsort puts every NaN last)
__global__ void __launch_bounds__(256) bin_canon_kernel(long long n, const double* __restrict__ vs, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = vs[i];
    out[i] = (v != v) ? __builtin_nan("") : v;
}

constexpr unsigned BIN_LONG = 1024;   // rows from which a cell is walked by a wave instead of a lane

// one lane per non-empty cell; rows [starts[j], starts[j+1]) of the sorted order, walked in that (= source) order
__global__ void __launch_bounds__(256) bin_stat_kernel(const BinArgs a, long long n_cells) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_cells) return;
    const unsigned s = a.starts[j], e = a.starts[j + 1];
    const double* __restrict__ vs = a.vs;
    a.out_keys[j] = (long long)a.keys_sorted[s];
    const double cnt = (double)(e - s);
    double* o = a.out + j;                        // [statistic][n_cells], the statistics asked for in bit order
    if (a.mask & GPSAT_BIN_COUNT) { *o = cnt; o += n_cells; }
    // a long cell: one lane would walk it alone for a long time (a load's latency per few rows); bin_long_kernel gives it a
    // wave.  The list's order is arbitrary, a cell's result does not depend on it.
    const bool is_long = e - s >= BIN_LONG && (a.mask & (GPSAT_BIN_SUM | GPSAT_BIN_MEAN | GPSAT_BIN_STD | GPSAT_BIN_MIN | GPSAT_BIN_MAX));
    if (is_long) a.long_list[atomicAdd(a.n_long, 1u)] = (unsigned)j;
    double mean = 0.0;
    if (is_long) {
        for (unsigned b = GPSAT_BIN_SUM; b <= GPSAT_BIN_MAX; b <<= 1) if (a.mask & b) o += n_cells;
    } else {
        if (a.mask & (GPSAT_BIN_SUM | GPSAT_BIN_MEAN | GPSAT_BIN_STD)) {
            double sum = 0.0;                         // np.bincount: from 0.0, one row after the other
            for (unsigned i = s; i < e; ++i) sum = __dadd_rn(sum, vs[i]);
            mean = __ddiv_rn(sum, cnt);
            if (a.mask & GPSAT_BIN_SUM) { *o = sum; o += n_cells; }
            if (a.mask & GPSAT_BIN_MEAN) { *o = mean; o += n_cells; }
        }
        if (a.mask & GPSAT_BIN_STD) {
            double q = 0.0;
            for (unsigned i = s; i < e; ++i) {
                const double d = __dsub_rn(vs[i], mean);
                q = __dadd_rn(q, __dmul_rn(d, d));
            }
            *o = __dsqrt_rn(__ddiv_rn(q, cnt));
            o += n_cells;
        }
        if (a.mask & (GPSAT_BIN_MIN | GPSAT_BIN_MAX)) {
            double mn = __builtin_nan(""), mx = -__builtin_inf();
            bool any_nan = false;
            for (unsigned i = s; i < e; ++i) {
                const double v = vs[i];
                if (v != v) { any_nan = true; continue; }
                if (!(mn <= v)) mn = v;               // first value, or a smaller one
                if (v > mx) mx = v;
            }
            if (any_nan) mx = __builtin_nan("");      // scipy: the last of np.argsort, where NaN orders last
            if (a.mask & GPSAT_BIN_MIN) { *o = mn; o += n_cells; }
            if (a.mask & GPSAT_BIN_MAX) { *o = mx; o += n_cells; }
        }
    }
    if (a.mask & GPSAT_BIN_MEDIAN) {
        const unsigned n = e - s;
        const double lo = a.vsorted[s + (n - 1) / 2], hi = a.vsorted[s + n / 2];
        *o = __ddiv_rn(__dadd_rn(lo, hi), 2.0);
    }
}

// the value lane k holds, in every lane (k is wave-uniform)
__device__ __forceinline__ double lane_value(double v, int k) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

// acc = (...((acc + w_0) + w_1)...) + w_{n-1} over the values the first n lanes hold: the serial chain of np.bincount, every
// lane computing the same sum
__device__ __forceinline__ double chain_add(double acc, double w, int n) {
    if (n == 64) {
#pragma unroll
        for (int k = 0; k < 64; ++k) acc = __dadd_rn(acc, lane_value(w, k));
    } else {
        for (int k = 0; k < n; ++k) acc = __dadd_rn(acc, lane_value(w, k));
    }
    return acc;
}

// one WAVE per long cell (the cells bin_stat_kernel listed), persistent over the list.  64 consecutive values per coalesced
// load, the next 64 already in flight; the additions stay the sequential ones of bin_stat_kernel, in the same order.
__global__ void __launch_bounds__(256) bin_long_kernel(const BinArgs a, long long n_cells) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    const unsigned n_long = *a.n_long;
    const double* __restrict__ vs = a.vs;
    for (unsigned q = wave; q < n_long; q += n_waves) {
        const long long j = a.long_list[q];
        const unsigned s = a.starts[j], e = a.starts[j + 1];
        const double cnt = (double)(e - s);
        double* o = a.out + j;
        if (a.mask & GPSAT_BIN_COUNT) o += n_cells;
        double mean = 0.0;
        if (a.mask & (GPSAT_BIN_SUM | GPSAT_BIN_MEAN | GPSAT_BIN_STD)) {
            double sum = 0.0;
            double v = (s + lane < e) ? vs[s + lane] : 0.0;
            for (unsigned base = s; base < e; base += 64) {
                const unsigned nxt = base + 64 + lane;
                const double vn = (nxt < e) ? vs[nxt] : 0.0;
                sum = chain_add(sum, v, (int)min(64u, e - base));
                v = vn;
            }
            mean = __ddiv_rn(sum, cnt);
            if (a.mask & GPSAT_BIN_SUM) { if (lane == 0) *o = sum; o += n_cells; }
            if (a.mask & GPSAT_BIN_MEAN) { if (lane == 0) *o = mean; o += n_cells; }
        }
        if (a.mask & GPSAT_BIN_STD) {
            double qs = 0.0;
            double v = (s + lane < e) ? vs[s + lane] : 0.0;
            for (unsigned base = s; base < e; base += 64) {
                const unsigned nxt = base + 64 + lane;
                const double vn = (nxt < e) ? vs[nxt] : 0.0;
                const double d = __dsub_rn(v, mean);              // every lane its own row; the squares are added in order
                qs = chain_add(qs, __dmul_rn(d, d), (int)min(64u, e - base));
                v = vn;
            }
            if (lane == 0) *o = __dsqrt_rn(__ddiv_rn(qs, cnt));
            o += n_cells;
        }
        if (a.mask & (GPSAT_BIN_MIN | GPSAT_BIN_MAX)) {
            // order statistics: any order gives the same value
            double mn = __builtin_nan(""), mx = -__builtin_inf();
            bool any_nan = false;
            for (unsigned i = s + lane; i < e; i += 64) {
                const double v = vs[i];
                if (v != v) { any_nan = true; continue; }
                if (!(mn <= v)) mn = v;
                if (v > mx) mx = v;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double m2 = __shfl_xor(mn, off), x2 = __shfl_xor(mx, off);
                if (m2 == m2 && !(mn <= m2)) mn = m2;
                if (x2 > mx) mx = x2;
            }
            if (__ballot(any_nan) != 0ull) mx = __builtin_nan("");
            if (a.mask & GPSAT_BIN_MIN) { if (lane == 0) *o = mn; o += n_cells; }
            if (a.mask & GPSAT_BIN_MAX) { if (lane == 0) *o = mx; o += n_cells; }
        }
    }
}

static void bin_gather(const void* ctx, hipStream_t stream) {
    const BinArgs& a = *static_cast<const BinArgs*>(ctx);
    hipLaunchKernelGGL(bin_gather_kernel, dim3((unsigned)((a.R + 255) / 256)), dim3(256), 0, stream, a);
}

// temp == nullptr: only the size of the temporary storage is returned in temp_bytes
hipError_t bin_sort_rows(const BinArgs& a, void* temp, size_t& temp_bytes, hipStream_t stream) {
    if (temp) hipLaunchKernelGGL(bin_key_kernel, dim3((unsigned)((a.R + 255) / 256)), dim3(256), 0, stream, a);
    return key_runs(a, bin_gather, &a, nullptr, temp, temp_bytes, stream);
}

// temp == nullptr: only the size of the temporary storage (the median's segmented sort) is returned in temp_bytes
hipError_t bin_cell_stats(const BinArgs& a, long long n_cells, long long n_valid, void* temp, size_t& temp_bytes, hipStream_t stream) {
    const bool median = (a.mask & GPSAT_BIN_MEDIAN) != 0;
    if (!temp) {
        temp_bytes = 0;
        if (!median) return hipSuccess;
        return rocprim::segmented_radix_sort_keys(nullptr, temp_bytes, a.vcanon, a.vsorted, (unsigned)n_valid, (unsigned)n_cells, a.starts,
                                                  a.starts + 1, 0, 64, stream);
    }
    if (median) {
        hipLaunchKernelGGL(bin_canon_kernel, dim3((unsigned)((n_valid + 255) / 256)), dim3(256), 0, stream, n_valid, a.vs, a.vcanon);
        hipError_t e = rocprim::segmented_radix_sort_keys(temp, temp_bytes, a.vcanon, a.vsorted, (unsigned)n_valid, (unsigned)n_cells,
                                                          a.starts, a.starts + 1, 0, 64, stream);
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipMemsetAsync(a.n_long, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bin_stat_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, stream, a, n_cells);
    // at most n_valid / BIN_LONG long cells; the waves stride over however many the list holds (none: they leave at once)
    const long long max_long = n_valid / BIN_LONG;
    if (max_long > 0) {
        const unsigned grid = (unsigned)std::min<long long>(1024, (max_long + 3) / 4);
        hipLaunchKernelGGL(bin_long_kernel, dim3(grid), dim3(256), 0, stream, a, n_cells);
    }
    return hipGetLastError();
}

int bin_long_rows() { return (int)BIN_LONG; }

}  // namespace gpsat
