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
