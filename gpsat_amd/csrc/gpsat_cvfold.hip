// gpsat_cvfold.hip -- refitted cross-validation on gfx950: the two kernels around the persistent tile kernels.
//
// gpsat_fit_predict_batch_cv_refit turns a tile of N rows with F folds into F more tiles ("derived tiles") of N - g rows with
// g prediction points, runs them as one ordinary batch, and puts their predictions back at the held-out rows.
//   cvfold_expand : source X, y (where the first launch left them, on the device) -> X', y', Xs' of every derived tile and
//                   delta = the mean of its remaining rows.  One workgroup of 256 threads per derived tile.  A thread takes
//                   whole rows, consecutive threads consecutive rows: a wave reads 64 D consecutive elements of X.  A row's
//                   place among the remaining rows is its index minus the number of fold rows below it (a binary search in
//                   the fold's ascending row list, which stays in L1/L2).
//   cvfold_scatter: one thread per source row: the derived tile's f*, f*_var, y_var at (fold, position in fold), delta added
//                   to the mean in fp64; NaN for a row that is never held out, whose fold was not fitted, or whose derived
//                   tile ended NOT_PD / NAN.
//   cvfold_lpd    : (gpsat_fit_predict_batch_cv_refit_joint, fp64) one workgroup per derived tile: the joint log density of
//                   the fold's rows under the derived tile's posterior, from its g x g covariance (see the kernel).
// delta is ONE fp64 sum in a fixed order: thread k adds rows k, k + 256, ... in ascending order, the 256 partial sums are
// added by a fixed binary tree in LDS.  The workgroup size is a compile-time constant and a derived tile belongs to one
// workgroup, so the bits do not depend on the grid or on which wave ran first; there is no float atomic.
// Both kernels are HBM/L2-bound streaming: no MFMA, 2 KiB of LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "gpsat_hip.h"
#include "gpsat_kernels.h"

namespace gpsat {

constexpr int CVF_THREADS = 256;

// number of entries of rows[0..g) below i (rows ascend)
__device__ __forceinline__ int cvf_rows_below(const int* __restrict__ rows, int g, int i) {
    int lo = 0, hi = g;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid] < i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <typename T>
__global__ __launch_bounds__(CVF_THREADS) void cvfold_expand_kernel(CvFoldArgs a) {
    __shared__ double part[CVF_THREADS];
    const int tid = threadIdx.x, D = a.D;
    for (int j = blockIdx.x; j < a.F2; j += gridDim.x) {
        const long long o0 = a.d_src_off[j], oo = a.d_obs_off[j], po = a.d_pred_off[j];
        const int N = a.d_src_n[j], f = a.d_fold[j];
        const int* __restrict__ rows = a.fold_rows + a.fold_ptr[f];
        const int g = a.fold_ptr[f + 1] - a.fold_ptr[f];
        const int* __restrict__ rf = a.row_fold + o0;
        const int* __restrict__ rp = a.row_pos + o0;
        const T* __restrict__ X = static_cast<const T*>(a.X) + o0 * D;
        const T* __restrict__ y = static_cast<const T*>(a.y) + o0;
        T* __restrict__ Xd = static_cast<T*>(a.Xd) + oo * D;
        T* __restrict__ yd = static_cast<T*>(a.yd) + oo;
        T* __restrict__ Xsd = static_cast<T*>(a.Xsd) + po * D;
        double delta = 0.0;
        if (a.recentre) {
            double s = 0.0;
            for (int i = tid; i < N; i += CVF_THREADS)
                if (rf[i] != f) s += (double)y[i];
            part[tid] = s;
            __syncthreads();
            for (int w = CVF_THREADS / 2; w > 0; w >>= 1) {
                if (tid < w) part[tid] += part[tid + w];
                __syncthreads();
            }
            delta = part[0] / (double)(N - g);
            __syncthreads();                  // part[] is written again for the next derived tile
        }
        if (tid == 0) a.delta[j] = delta;
        for (int i = tid; i < N; i += CVF_THREADS) {
            T x[4];
            for (int c = 0; c < D; ++c) x[c] = X[(long long)i * D + c];
            if (rf[i] == f) {
                const int p = rp[i];
                for (int c = 0; c < D; ++c) Xsd[(long long)p * D + c] = x[c];
            } else {
                const int k = i - cvf_rows_below(rows, g, i);
                for (int c = 0; c < D; ++c) Xd[(long long)k * D + c] = x[c];
                yd[k] = (T)((double)y[i] - delta);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(CVF_THREADS) void cvfold_scatter_kernel(CvFoldArgs a) {
    const long long r = (long long)blockIdx.x * CVF_THREADS + threadIdx.x;
    if (r >= a.sumN) return;
    const T* __restrict__ fm = static_cast<const T*>(a.fm);
    const T* __restrict__ fv = static_cast<const T*>(a.fv);
    const T* __restrict__ yv = static_cast<const T*>(a.yv);
    T* __restrict__ om = static_cast<T*>(a.cv_mean);
    T* __restrict__ of = static_cast<T*>(a.cv_f_var);
    T* __restrict__ oy = static_cast<T*>(a.cv_y_var);
    const int f = a.row_fold[r];
    const int j = f >= 0 ? a.fold_derived[f] : -1;
    const int st = j >= 0 ? a.d_status[j] : GPSAT_STATUS_NOT_PD;
    T m = (T)NAN, v = (T)NAN, w = (T)NAN;
    if (st != GPSAT_STATUS_NOT_PD && st != GPSAT_STATUS_NAN) {
        const long long p = a.d_pred_off[j] + a.row_pos[r];
        m = (T)((double)fm[p] + a.delta[j]);
        v = fv[p];
        w = yv[p];
    }
    om[r] = m;
    of[r] = v;
    if (oy) oy[r] = w;
}

// The joint log predictive density of every fitted fold (gpsat_fit_predict_batch_cv_refit_joint, fp64):
//   lpd = log N(y'_G; f*, f_cov + sn2 I) = -1/2 w^T w - sum_k log L_kk - g/2 log 2 pi,  L L^T = f_cov + sn2 I,  w = L^-1 (y'_G - f*)
// from the g x g posterior covariance the derived tile returned.  One workgroup per derived tile, everything in the tile's
// own f_cov block (lower triangle, in place) and g doubles of `resid`:
//   - r = (y_G - delta) - f*, sn2 onto the diagonal;
//   - left-looking Cholesky, column k: every thread forms the pivot from row k (the same k terms in ascending order, so
//     the value and the branch on it are uniform without a broadcast), thread i - k - 1 (mod CVF_THREADS) owns row i of the
//     column; one barrier per column;
//   - forward substitution by columns: w_k = r_k / L_kk is uniform, row i > k takes r_i -= L_ik w_k (one writer per
//     element, ascending k), thread k mod CVF_THREADS adds w_k^2 to its partial sum (ascending k);
//   - w^T w: the CVF_THREADS partial sums by the fixed binary tree in LDS that cvfold_expand uses for delta.
// No float atomic; the bits depend neither on the grid nor on which wave ran.  NaN for a derived tile that ended NOT_PD /
// NAN and for a pivot <= 0.  Latency-bound: g barriers twice per fold.
__global__ __launch_bounds__(CVF_THREADS) void cvfold_lpd_kernel(CvFoldArgs a) {
    __shared__ double part[CVF_THREADS];
    const int tid = threadIdx.x;
    constexpr double LOG_2PI = 1.8378770664093453;
    const double* __restrict__ y = static_cast<const double*>(a.y);
    const double* __restrict__ fm = static_cast<const double*>(a.fm);
    for (int j = blockIdx.x; j < a.F2; j += gridDim.x) {
        const int f = a.d_fold[j], st = a.d_status[j];
        const int* __restrict__ rows = a.fold_rows + a.fold_ptr[f];
        const int g = a.fold_ptr[f + 1] - a.fold_ptr[f];
        if (st == GPSAT_STATUS_NOT_PD || st == GPSAT_STATUS_NAN) {        // uniform: a value of the derived tile
            if (tid == 0) a.lpd[j] = NAN;
            continue;
        }
        const long long o0 = a.d_src_off[j], po = a.d_pred_off[j];
        double* S = a.f_cov + a.cov_off[j];                  // not __restrict__: rows written by other threads are read back
        double* r = a.resid + po;
        const double delta = a.delta[j], sn2 = a.sn2[j];
        for (int k = tid; k < g; k += CVF_THREADS) {
            r[k] = (y[o0 + rows[k]] - delta) - fm[po + k];
            S[(size_t)k * g + k] += sn2;
        }
        __syncthreads();
        bool bad = false;
        double sld = 0.0;
        for (int k = 0; k < g; ++k) {
            const double* Sk = S + (size_t)k * g;
            double sp = Sk[k];
            for (int m = 0; m < k; ++m) { const double l = Sk[m]; sp = fma(-l, l, sp); }
            if (!(sp > 0.0)) { bad = true; break; }
            const double dk = sqrt(sp);
            sld += log(dk);
            for (int i = k + 1 + tid; i < g; i += CVF_THREADS) {
                double* Si = S + (size_t)i * g;
                double s = Si[k];
                for (int m = 0; m < k; ++m) s = fma(-Si[m], Sk[m], s);
                Si[k] = s / dk;
            }
            __syncthreads();                                 // every read of S[k][k] lies in front of its overwrite
            if (tid == 0) S[(size_t)k * g + k] = dk;
        }
        __syncthreads();
        if (bad) {
            if (tid == 0) a.lpd[j] = NAN;
            continue;
        }
        double acc = 0.0;
        for (int k = 0; k < g; ++k) {
            const double wk = r[k] / S[(size_t)k * g + k];
            if (tid == k % CVF_THREADS) acc = fma(wk, wk, acc);
            for (int i = k + 1 + tid; i < g; i += CVF_THREADS) r[i] = fma(-S[(size_t)i * g + k], wk, r[i]);
            __syncthreads();
        }
        part[tid] = acc;
        __syncthreads();
        for (int w = CVF_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) part[tid] += part[tid + w];
            __syncthreads();
        }
        if (tid == 0) a.lpd[j] = -0.5 * part[0] - sld - 0.5 * (double)g * LOG_2PI;
        __syncthreads();                                     // part[] is written again for the next derived tile
    }
}

hipError_t launch_cvfold_lpd(const CvFoldArgs& a, hipStream_t stream) {
    if (a.F2 <= 0) return hipSuccess;
    if (!a.f64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cvfold_lpd_kernel, dim3(a.F2), dim3(CVF_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cvfold_expand(const CvFoldArgs& a, hipStream_t stream) {
    if (a.F2 <= 0) return hipSuccess;
    const int grid = a.F2;
    if (a.f64) hipLaunchKernelGGL(cvfold_expand_kernel<double>, dim3(grid), dim3(CVF_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(cvfold_expand_kernel<float>, dim3(grid), dim3(CVF_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cvfold_scatter(const CvFoldArgs& a, hipStream_t stream) {
    if (a.sumN <= 0) return hipSuccess;
    const int grid = (int)((a.sumN + CVF_THREADS - 1) / CVF_THREADS);
    if (a.f64) hipLaunchKernelGGL(cvfold_scatter_kernel<double>, dim3(grid), dim3(CVF_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(cvfold_scatter_kernel<float>, dim3(grid), dim3(CVF_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace gpsat
