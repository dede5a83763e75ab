// gpsat_prep.hip -- the first stage of the pipeline on gfx950: raw lon / lat / time rows to x, y and a track number (fp64 and
// int32 streaming kernels, one thread per row, no MFMA).
//
//   prep_project_kernel<FORWARD, SOUTH> : Lambert azimuthal equal-area on the WGS84 ellipsoid, polar aspects -- what
//       GPSat.utils.WGS84toEASE2 / EASE2toWGS84 ask of PROJ ("+proj=laea +lat_0=+-90 +lon_0=.. +ellps=WGS84").  Forward,
//       Snyder 3-12, 24-23, 24-25:  q(phi) = (1 - e^2) [sin phi / (1 - e^2 sin^2 phi) - ln((1 - e sin phi) / (1 + e sin phi)) / (2e)],
//       rho = a sqrt(q_p -+ q), x = rho sin(lam - lam_0), y = -+ rho cos(lam - lam_0).  Inverse: q = +-(q_p - (rho / a)^2), phi by
//       Newton's iteration on q(phi) = q (Snyder 3-16) from the authalic latitude, written in the angle psi from the nearer
//       pole so that nothing cancels at either pole (see the kernel), until the step is below an ulp of psi (at most
//       PROJECT_NEWTON_MAX steps), lam = lam_0 + atan2(x, -+y).  Exact to rounding on purpose: PROJ truncates a series here.
//       Forward, q_p - q cancels towards the pole: the error of rho is about eps a^2 / rho.
//       NaN in -> NaN out; rho = 0 -> (lon_0, +-90); outside the disc ((rho / a)^2 > 2 q_p) -> +inf twice.
//   prep_delta_kernel<RUNS> : diff_distance(x, p=2, k=1) inside groups and the flag of every row -- delta > cut_off (NaN is
//       false, as guess_track_num has it) or the first row of a later group; RUNS: cols[0] differs from the row before
//       (track_num_for_date).  The rows are taken through the permutation of the keyed sort-and-run-heads stage on the group
//       codes (gpsat_key_runs.hip, behind the keyed glue's key kernel: glue_keyed_sort), so a group's rows keep the order they came in.  Difference, square, sum
//       from the left and root are single rounded operations (__dsub_rn ...): -ffp-contract has nothing to fuse.
//   the scan : track = start_track + inclusive prefix sum of the flags (RUNS: the row's position minus the inclusive prefix
//       MAXIMUM of the flagged positions), int32, three passes over blocks of PREP_BLOCK rows: prep_delta_kernel leaves what a
//       row contributes in track[] and its block's total in block_sums[]; prep_scan_sums_kernel, one workgroup, scans the
//       totals; prep_apply_kernel scans its block again and adds the blocks in front of it.  Integers in a fixed order, no
//       atomics: the same bytes on every call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpsat_kernels.h"

namespace gpsat {

constexpr int PREP_BLOCK = 256;               // rows per block of every kernel here, and the B of the scan
constexpr int PROJECT_NEWTON_MAX = 8;         // the start is within 2.3e-3 rad, the convergence quadratic: 3 steps, 1 to see it
constexpr double PREP_DEG = 0.017453292519943295;      // pi / 180
constexpr double PREP_RAD = 57.29577951308232;         // 180 / pi
constexpr double PREP_HALF_PI = 1.5707963267948966, PREP_HALF_PI_LO = 6.123233995736766e-17;      // pi / 2 in two doubles

__device__ __forceinline__ double authalic_q(double s, const ProjectArgs& a) {
    const double es = a.e * s;
    return a.one_m_e2 * (s / (1.0 - a.e2 * s * s) - log((1.0 - es) / (1.0 + es)) * a.inv_2e);
}

template <bool FORWARD, bool SOUTH>
__global__ void __launch_bounds__(PREP_BLOCK) prep_project_kernel(const ProjectArgs a) {
    const long long i = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const double u = a.in0[i], v = a.in1[i];
    double o0, o1;
    if (u != u || v != v) {
        o0 = o1 = __builtin_nan("");
    } else if (FORWARD) {
        const double s = sin(v * PREP_DEG);
        const double q = authalic_q(s, a);
        // at the pole q is q_p up to the last bit of this libm's log against the host's: the pole itself is rho = 0, and next
        // to it never the root of a negative
        const double d = s == (SOUTH ? -1.0 : 1.0) ? 0.0 : fmax(SOUTH ? a.qp + q : a.qp - q, 0.0);
        const double rho = a.a * sqrt(d);
        double sl, cl;
        sincos((u - a.lon_0) * PREP_DEG, &sl, &cl);
        o0 = rho * sl;
        o1 = SOUTH ? rho * cl : -(rho * cl);
    } else {
        const double rx = u / a.a, ry = v / a.a;
        const double r2 = rx * rx + ry * ry;
        const double pole = SOUTH ? -90.0 : 90.0;
        if (r2 > 2.0 * a.qp) {
            o0 = o1 = __builtin_inf();
        } else if (r2 == 0.0) {
            o0 = a.lon_0;
            o1 = pole;
        } else {
            // The latitude as the angle psi from the NEARER pole: q_p - |q| = delta there, and q_p - q(90 - psi), written in
            // u = 1 - cos(psi) = 2 sin^2(psi / 2), has no cancellation at either pole.  Near side: delta = (rho / a)^2.  Far side:
            // delta = 2 q_p - (rho / a)^2, a difference of numbers near 4 whose error decides phi: (rho / a)^2 and q_p in two
            // doubles (the products by fma, a^2 an exact integer, the leading difference exact).
            const double p1 = u * u, e1 = fma(u, u, -p1);
            const double p2 = v * v, e2 = fma(v, v, -p2);
            const double sh = p1 + p2, bb = sh - p1;
            const double sl = ((p1 - (sh - bb)) + (p2 - bb)) + (e1 + e2);
            const double a2 = a.a * a.a;
            const double q1 = sh / a2;
            const double q2 = (fma(-q1, a2, sh) + sl) / a2;
            const bool far = q1 > a.qp;
            const double delta = fmax(far ? (2.0 * a.qp - q1) + (2.0 * a.qp_lo - q2) : q1 + q2, 0.0);
            double psi = 2.0 * asin(sqrt(fmin(delta / (2.0 * a.qp), 1.0)));      // the authalic angle: within 0.4 %
            if (delta > 0.0) {
                const double c_atanh = a.one_m_e2 / a.e;
                for (int it = 0; it < PROJECT_NEWTON_MAX; ++it) {
                    const double h = sin(0.5 * psi);
                    const double uu = 2.0 * h * h, sc = 1.0 - uu;
                    const double z = a.e * uu / (1.0 - a.e2 * sc);
                    const double w = 1.0 - a.e2 * sc * sc;
                    const double g = uu * (1.0 + a.e2 * sc) / w + c_atanh * (0.5 * log1p(2.0 * z / (1.0 - z)));
                    const double step = (g - delta) / (2.0 * a.one_m_e2 * sin(psi) / (w * w));
                    psi -= step;
                    if (fabs(step) <= 1.1102230246251565e-16 * fabs(psi)) break;
                }
            }
            const double phi = (PREP_HALF_PI - psi) + PREP_HALF_PI_LO;
            o1 = (far != SOUTH ? -phi : phi) * PREP_RAD;
            double lon = a.lon_0 + atan2(u, SOUTH ? v : -v) * PREP_RAD;
            lon -= 360.0 * ceil((lon - 180.0) / 360.0);       // into (-180, 180]
            o0 = lon;
        }
    }
    a.out0[i] = o0;
    a.out1[i] = o1;
}

hipError_t launch_project(const ProjectArgs& a, bool forward, bool south, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.n + PREP_BLOCK - 1) / PREP_BLOCK)), block(PREP_BLOCK);
    if (forward && !south) hipLaunchKernelGGL((prep_project_kernel<true, false>), grid, block, 0, stream, a);
    else if (forward) hipLaunchKernelGGL((prep_project_kernel<true, true>), grid, block, 0, stream, a);
    else if (!south) hipLaunchKernelGGL((prep_project_kernel<false, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((prep_project_kernel<false, true>), grid, block, 0, stream, a);
    return hipGetLastError();
}

// ---- tracks
__global__ void __launch_bounds__(PREP_BLOCK) prep_key_kernel(long long n, const int* __restrict__ group, long long* __restrict__ key) {
    const long long i = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (i < n) key[i] = group[i];
}

// The two scans: flags add up (tracks); flagged positions, all >= 0, take the maximum (runs).  0 is neutral for both.
template <bool RUNS>
__device__ __forceinline__ int scan_op(int x, int y) { return RUNS ? (x > y ? x : y) : x + y; }

// Inclusive scan of one value per thread over the block, in thread order; *total: that of the whole block.  Every thread of
// the block calls it.  lds: PREP_BLOCK / 64 words.
template <bool RUNS>
__device__ __forceinline__ int block_scan(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off);
        if (lane >= off) v = scan_op<RUNS>(t, v);
    }
    __syncthreads();                                      // the words of an earlier call have been read
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    int front = 0, all = 0;
#pragma unroll
    for (int w = 0; w < PREP_BLOCK / 64; ++w) {
        const int s = lds[w];
        if (w < wave) front = scan_op<RUNS>(front, s);
        all = scan_op<RUNS>(all, s);
    }
    *total = all;
    return scan_op<RUNS>(front, v);
}

template <bool RUNS>
__global__ void __launch_bounds__(PREP_BLOCK) prep_delta_kernel(const TrackArgs a) {
    __shared__ int lds[PREP_BLOCK / 64];
    const long long i = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x;
    int val = 0;
    if (i < a.n) {
        const bool valid = !a.n_valid || i < *a.n_valid;
        const unsigned src = a.perm ? a.perm[i] : (unsigned)i;
        a.order[i] = (int)src;
        const bool head = i == 0 || (a.heads && a.heads[i]);
        const unsigned prev = head ? src : (a.perm ? a.perm[i - 1] : (unsigned)(i - 1));
        if (RUNS) {
            if (valid && (head || a.cols[0][src] != a.cols[0][prev])) val = (int)i;
        } else {
            double d = __builtin_nan("");
            if (a.mode == 2) {                                // the distances are given: every row has one
                if (valid) d = a.cols[0][src];
            } else if (valid && !head) {
                double s = 0.0;
                for (int c = 0; c < a.n_cols; ++c) {
                    const double df = __dsub_rn(a.cols[c][src], a.cols[c][prev]);
                    const double sq = __dmul_rn(df, df);
                    s = c == 0 ? sq : __dadd_rn(s, sq);
                }
                d = __dsqrt_rn(s);
            }
            a.delta[i] = d;
            if (valid && (d > a.cut_off || (head && i != 0))) val = 1;
        }
        a.track[i] = val;
    }
    int total;
    block_scan<RUNS>(val, lds, &total);
    if (threadIdx.x == 0) a.block_sums[blockIdx.x] = total;
}

// sums[j] <- the scan of sums[0 .. j]: ONE workgroup, PREP_BLOCK sums per round, the rounds joined by a carry
template <bool RUNS>
__global__ void __launch_bounds__(PREP_BLOCK) prep_scan_sums_kernel(int* __restrict__ sums, unsigned nb) {
    __shared__ int lds[PREP_BLOCK / 64];
    int carry = 0;
    for (unsigned base = 0; base < nb; base += PREP_BLOCK) {
        const unsigned j = base + threadIdx.x;
        const int v = j < nb ? sums[j] : 0;
        int total;
        const int incl = block_scan<RUNS>(v, lds, &total);
        if (j < nb) sums[j] = scan_op<RUNS>(carry, incl);
        carry = scan_op<RUNS>(carry, total);
    }
}

template <bool RUNS>
__global__ void __launch_bounds__(PREP_BLOCK) prep_apply_kernel(const TrackArgs a) {
    __shared__ int lds[PREP_BLOCK / 64];
    const long long i = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x;
    const int val = i < a.n ? a.track[i] : 0;
    int total;
    const int incl = block_scan<RUNS>(val, lds, &total);
    if (i >= a.n) return;
    const int r = scan_op<RUNS>(blockIdx.x > 0 ? a.block_sums[blockIdx.x - 1] : 0, incl);
    const bool valid = !a.n_valid || i < *a.n_valid;
    a.track[i] = !valid ? -1 : (RUNS ? (int)i - r : a.start_track + r);
}

int prep_scan_block() { return PREP_BLOCK; }

hipError_t launch_track_keys(long long n, const int* group, long long* key, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(prep_key_kernel, dim3((unsigned)((n + PREP_BLOCK - 1) / PREP_BLOCK)), dim3(PREP_BLOCK), 0, stream, n, group, key);
    return hipGetLastError();
}

template <bool RUNS>
static hipError_t launch_track_passes(const TrackArgs& a, hipStream_t stream) {
    const unsigned nb = (unsigned)((a.n + PREP_BLOCK - 1) / PREP_BLOCK);
    hipLaunchKernelGGL(prep_delta_kernel<RUNS>, dim3(nb), dim3(PREP_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(prep_scan_sums_kernel<RUNS>, dim3(1), dim3(PREP_BLOCK), 0, stream, a.block_sums, nb);
    hipLaunchKernelGGL(prep_apply_kernel<RUNS>, dim3(nb), dim3(PREP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_track(const TrackArgs& a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    return a.mode == 1 ? launch_track_passes<true>(a, stream) : launch_track_passes<false>(a, stream);
}

}  // namespace gpsat
