// gpsat_post.hip -- post-processing rows of SURVEY.md section 8f on gfx950 (fp64, HBM / ALU-bound, no MFMA):
//   smooth_kernel : Gaussian-weighted smoothing of a hyper-parameter field over the expert locations
//                   (GPSat/postprocessing.py:22-52 gaussian_2d_weight): out_i = sum_j w_ij v_j / sum_j w_ij over the
//                   non-NaN v_j, w_ij = exp(-(((x_j-x_i)/lx)^2 + ((y_j-y_i)/ly)^2)/2), NaN when the weights sum to 0;
//   glue_kernel   : Gaussian-weighted averaging of overlapping local predictions per prediction location
//                   (GPSat/postprocessing.py:447-577): rows are pre-sorted by prediction location (CSR segments),
//                   w = prod_d normpdf(pred_d; xprt_d, sigma[row]), out[var][g] = sum w v / sum w.
// One wave per output element, lanes stride over the inputs (coalesced), fixed-order wave reduction => results are
// reproducible bit for bit (the reference accumulates sequentially; agreement is to fp64 rounding, ~1e-15 relative).
// smooth_kernel is bound by fp64 ALU work (two divisions and an exp per pair: 480 G pairs/s), not by its reads (24 B per pair
// out of L1 / L2): the LDS-tiled form (one thread per output, inputs staged in tiles of 256 and read by broadcast;
// scripts/experiments/r4_smooth_kernel_lds_tiled.patch) measured 390 G pairs/s at 131 072 locations and 17 instead of 229 at
// 4 096 (a quarter of the waves in flight, one dependent accumulation chain per thread) -- not adopted.
//   glue_keyed_kernel : the same average over rows that arrive in ANY order with an integer key per row (held-out
//                   predictions keyed by observation: groups of 3..20 rows, millions of them).  The keyed sort-and-run-heads
//                   stage (gpsat_key_runs.hip: a stable sort of (key, source row), run starts, ignored rows dropped),
//                   then one TEAM of lanes per group that gathers its rows through the permutation: lane l of the team adds
//                   the group's rows l, l + W, l + 2W, ... in that order and a fixed xor tree over the team's W lanes joins
//                   them.  A group's bits are a function of its own rows in source order (the sort is stable) and of W, a
//                   compile-time constant of the product: not of the other keys, the grid or the capacity.  No float atomics.
//   glue_keyed_grad_kernel : the same walk for one value with its gradient: the glued value and the slope of the glued map,
//                   which has a term from the weights' own dependence on the prediction location.
//   glue_keyed_hess_kernel : that walk once more for a value with its gradient and its second derivatives: the glued value,
//                   the slope and the Hessian of the glued map, with the weights' first and second derivatives.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "gpsat_kernels.h"

namespace gpsat {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(256) smooth_kernel(int T, const double* __restrict__ x, const double* __restrict__ y,
                                                     const double* __restrict__ vals, double lx, double ly,
                                                     double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= T) return;
    const double x0 = x[i], y0 = y[i];
    double wv = 0.0, ws = 0.0;
    for (int j = lane; j < T; j += 64) {
        const double v = vals[j];
        if (v == v) {
            const double dx = (x[j] - x0) / lx, dy = (y[j] - y0) / ly;
            const double w = exp(-(dx * dx + dy * dy) / 2);
            wv += w * v;
            ws += w;
        }
    }
    wv = wave_sum(wv);
    ws = wave_sum(ws);
    if (lane == 0) out[i] = (ws == 0.0) ? __builtin_nan("") : wv / ws;
}

__global__ void __launch_bounds__(256) glue_kernel(int G, int ndim, int nvars, long long R, const long long* __restrict__ seg,
                                                   const double* __restrict__ pred, const double* __restrict__ xprt,
                                                   const double* __restrict__ vals, double sigma, const double* __restrict__ sigma_rows,
                                                   double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const long long a = seg[g], b = seg[g + 1];
    double ws = 0.0;
    double acc[GPSAT_GLUE_MAXVARS];
#pragma unroll
    for (int v = 0; v < GPSAT_GLUE_MAXVARS; ++v) acc[v] = 0.0;
    for (long long r = a + lane; r < b; r += 64) {
        const double sg = sigma_rows ? sigma_rows[r] : sigma;
        const double cnorm = 1.0 / (sg * 2.5066282746310002);       // 1 / (sigma sqrt(2 pi))
        double w = 1.0;
        for (int d = 0; d < ndim; ++d) {
            const double zz = (pred[(size_t)d * R + r] - xprt[(size_t)d * R + r]) / sg;
            w *= exp(-zz * zz / 2) * cnorm;
        }
        ws += w;
#pragma unroll
        for (int v = 0; v < GPSAT_GLUE_MAXVARS; ++v)
            if (v < nvars) {
                // a NaN prediction (failed tile) is left out of the weighted sum while its weight stays in the
                // denominator: what the reference's groupby(...).sum() does (it skips NaN), postprocessing.py:512-520
                const double x = vals[(size_t)v * R + r];
                if (x == x) acc[v] += w * x;
            }
    }
    ws = wave_sum(ws);
#pragma unroll
    for (int v = 0; v < GPSAT_GLUE_MAXVARS; ++v) {
        if (v < nvars) {
            const double s = wave_sum(acc[v]);
            if (lane == 0) out[(size_t)v * G + g] = s / ws;
        }
    }
}

hipError_t launch_smooth(int T, const double* x, const double* y, const double* vals, double lx, double ly, double* out,
                         hipStream_t stream) {
    hipLaunchKernelGGL(smooth_kernel, dim3((T + 3) / 4), dim3(256), 0, stream, T, x, y, vals, lx, ly, out);
    return hipGetLastError();
}

hipError_t launch_glue(int G, int ndim, int nvars, long long R, const long long* seg, const double* pred, const double* xprt,
                       const double* vals, double sigma, const double* sigma_rows, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(glue_kernel, dim3((G + 3) / 4), dim3(256), 0, stream, G, ndim, nvars, R, seg, pred, xprt, vals, sigma, sigma_rows, out);
    return hipGetLastError();
}

// ---- keyed glue
__global__ void __launch_bounds__(256) glue_key_kernel(const KeyRuns a, const long long* __restrict__ key) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.R) return;
    const long long k = key[i];
    a.keys[i] = k < 0 ? a.sentinel : (unsigned long long)k;
    a.rows[i] = (unsigned)i;
}

// W lanes per group, 256 / W groups per workgroup.  No lane leaves before the shuffles: a team past the last group walks an
// empty range and stores nothing.
template <int W>
__global__ void __launch_bounds__(256) glue_keyed_kernel(const GlueKeyedArgs a, long long G) {
    const long long g = ((long long)blockIdx.x * 256 + threadIdx.x) / W;
    const int tl = threadIdx.x & (W - 1);
    const bool live = g < G;
    const unsigned s = live ? a.starts[g] : 0u, e = live ? a.starts[g + 1] : 0u;
    const size_t R = (size_t)a.R;
    const int ndim = a.ndim, nvars = a.nvars;
    double ws = 0.0;
    int cnt = 0;
    double acc[GPSAT_GLUE_MAXVARS];
#pragma unroll
    for (int v = 0; v < GPSAT_GLUE_MAXVARS; ++v) acc[v] = 0.0;
    for (unsigned i = s + tl; i < e; i += W) {
        const size_t r = a.perm[i];
        const double sg = a.sigma_rows ? a.sigma_rows[r] : a.sigma;
        const double cnorm = 1.0 / (sg * 2.5066282746310002);       // 1 / (sigma sqrt(2 pi))
        double w = 1.0, d2 = 0.0;
        for (int d = 0; d < ndim; ++d) {
            const double df = a.pred[(size_t)d * R + r] - a.xprt[(size_t)d * R + r];
            const double zz = df / sg;
            d2 += df * df;
            w *= exp(-zz * zz / 2) * cnorm;
        }
        if (a.md2 >= 0.0 && !(d2 < a.md2)) continue;                // strict, and a NaN distance is outside
        ++cnt;
        ws += w;
#pragma unroll
        for (int v = 0; v < GPSAT_GLUE_MAXVARS; ++v)
            if (v < nvars) {
                const double x = a.vals[(size_t)v * R + r];          // NaN: out of the sum, its weight stays (glue_kernel)
                if (x == x) acc[v] += w * x;
            }
    }
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) {
        ws += __shfl_xor(ws, off);
        cnt += __shfl_xor(cnt, off);
#pragma unroll
        for (int v = 0; v < GPSAT_GLUE_MAXVARS; ++v) acc[v] += __shfl_xor(acc[v], off);
    }
    if (live && tl == 0) {
        a.out_key[g] = (long long)a.keys_sorted[s];
        a.out_count[g] = cnt;
#pragma unroll
        for (int v = 0; v < GPSAT_GLUE_MAXVARS; ++v)
            if (v < nvars) a.out[(size_t)v * (size_t)G + (size_t)g] = cnt ? acc[v] / ws : __builtin_nan("");
    }
}

// The glued value and the exact slope of the glued map F(p) = sum w_i(p) f_i(p) / sum w_i(p): the
// weights move with p, dw_i/dp_a = w_i u_ia with u_ia = (xprt_ia - pred_ia) / sigma_i^2, so
//   G_a = (S_a - F U_a) / W,   S_a = sum w_i (g_ia + u_ia f_i) over rows whose f_i and g_ia are not NaN,   U_a = sum w_i u_ia,
// with u centred on the row's own expert (coordinates are ~3e6 m, their differences a few sigma).  The team, the walk and the
// tree of glue_keyed_kernel; the weight, the limit and the value's sum are its statements, so that out[g] holds the bytes
// glue_keyed_kernel returns for nvars = 1.  a.vals: the value [R]; grad [ndim][R]; out_grad [ndim][G].
template <int W>
__global__ void __launch_bounds__(256) glue_keyed_grad_kernel(const GlueKeyedArgs a, long long G, const double* __restrict__ grad,
                                                              double* __restrict__ out_grad) {
    const long long g = ((long long)blockIdx.x * 256 + threadIdx.x) / W;
    const int tl = threadIdx.x & (W - 1);
    const bool live = g < G;
    const unsigned s = live ? a.starts[g] : 0u, e = live ? a.starts[g + 1] : 0u;
    const size_t R = (size_t)a.R;
    const int ndim = a.ndim;
    double ws = 0.0, acc = 0.0;
    int cnt = 0;
    double sa[2] = {0.0, 0.0}, ua[2] = {0.0, 0.0};
    for (unsigned i = s + tl; i < e; i += W) {
        const size_t r = a.perm[i];
        const double sg = a.sigma_rows ? a.sigma_rows[r] : a.sigma;
        const double cnorm = 1.0 / (sg * 2.5066282746310002);       // 1 / (sigma sqrt(2 pi))
        double w = 1.0, d2 = 0.0;
        double u[2] = {0.0, 0.0};
#pragma unroll
        for (int d = 0; d < 2; ++d)
            if (d < ndim) {
                const double df = a.pred[(size_t)d * R + r] - a.xprt[(size_t)d * R + r];
                const double zz = df / sg;
                d2 += df * df;
                w *= exp(-zz * zz / 2) * cnorm;
                u[d] = -df / (sg * sg);
            }
        if (a.md2 >= 0.0 && !(d2 < a.md2)) continue;                // strict, and a NaN distance is outside
        ++cnt;
        ws += w;
        const double x = a.vals[r];                                 // NaN: out of the sums, its weight stays
        const bool has = x == x;
        if (has) acc += w * x;
#pragma unroll
        for (int d = 0; d < 2; ++d)
            if (d < ndim) {
                ua[d] += w * u[d];
                const double gr = grad[(size_t)d * R + r];
                if (has && gr == gr) sa[d] += w * (gr + u[d] * x);
            }
    }
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) {
        ws += __shfl_xor(ws, off);
        cnt += __shfl_xor(cnt, off);
        acc += __shfl_xor(acc, off);
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            sa[d] += __shfl_xor(sa[d], off);
            ua[d] += __shfl_xor(ua[d], off);
        }
    }
    if (live && tl == 0) {
        a.out_key[g] = (long long)a.keys_sorted[s];
        a.out_count[g] = cnt;
        const double f = acc / ws;
        a.out[g] = cnt ? f : __builtin_nan("");
#pragma unroll
        for (int d = 0; d < 2; ++d)
            if (d < ndim) out_grad[(size_t)d * (size_t)G + (size_t)g] = cnt ? (sa[d] - f * ua[d]) / ws : __builtin_nan("");
    }
}

// The glued value, the slope and the second derivatives of the glued map: N = F W differentiated twice.
// With q_i = 1 / sigma_i^2 the weights have d2w_i/dp_a dp_b = w_i c_iab, c_iab = u_ia u_ib - delta_ab q_i, and
//   V_ab = sum w_i c_iab,   T_ab = sum w_i (h_iab + u_ia g_ib + u_ib g_ia + c_iab f_i) over rows whose f_i, g_ia, g_ib and h_iab
//   are not NaN,   H_ab = (T_ab - G_a U_b - G_b U_a - F V_ab) / W,
// for the pairs a <= b in the order (0,0), (0,1), (1,1) (ndim 1: (0,0) alone).  The team, the walk and the tree of
// glue_keyed_grad_kernel; the weight, the limit, ws, acc, sa and ua are its statements, so that out[g] and out_grad hold the
// bytes it returns (-ffp-contract=on contracts per source expression: the same statement, the same instruction).  A row's
// ten gathered columns are read at the head of the iteration, before the limit is known.  Making those loads branch-free as
// well (a column that ndim 1 lacks read as column 0) put all of them in flight at once at 116 instead of 90 VGPRs and measured
// the same reduce time within the run-to-run spread: the other waves hide the gather already.
// a.vals: the value [R]; grad [ndim][R]; hess [npair][R]; out_grad [ndim][G]; out_hess [npair][G].
template <int W>
__global__ void __launch_bounds__(256) glue_keyed_hess_kernel(const GlueKeyedArgs a, long long G, const double* __restrict__ grad,
                                                              const double* __restrict__ hess, double* __restrict__ out_grad,
                                                              double* __restrict__ out_hess) {
    const long long g = ((long long)blockIdx.x * 256 + threadIdx.x) / W;
    const int tl = threadIdx.x & (W - 1);
    const bool live = g < G;
    const unsigned s = live ? a.starts[g] : 0u, e = live ? a.starts[g + 1] : 0u;
    const size_t R = (size_t)a.R;
    const int ndim = a.ndim;
    const int npair = ndim == 2 ? 3 : 1;
    double ws = 0.0, acc = 0.0;
    int cnt = 0;
    double sa[2] = {0.0, 0.0}, ua[2] = {0.0, 0.0};
    double ta[3] = {0.0, 0.0, 0.0}, va[3] = {0.0, 0.0, 0.0};
    for (unsigned i = s + tl; i < e; i += W) {
        const size_t r = a.perm[i];
        const double sg = a.sigma_rows ? a.sigma_rows[r] : a.sigma;
        double pr[2] = {0.0, 0.0}, xp[2] = {0.0, 0.0}, gv[2] = {0.0, 0.0}, hv[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < 2; ++d)
            if (d < ndim) {
                pr[d] = a.pred[(size_t)d * R + r];
                xp[d] = a.xprt[(size_t)d * R + r];
                gv[d] = grad[(size_t)d * R + r];
            }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < npair) hv[k] = hess[(size_t)k * R + r];
        const double x = a.vals[r];                                 // NaN: out of the sums, its weight stays
        const double cnorm = 1.0 / (sg * 2.5066282746310002);       // 1 / (sigma sqrt(2 pi))
        const double q = 1.0 / (sg * sg);
        double w = 1.0, d2 = 0.0;
        double u[2] = {0.0, 0.0};
#pragma unroll
        for (int d = 0; d < 2; ++d)
            if (d < ndim) {
                const double df = pr[d] - xp[d];
                const double zz = df / sg;
                d2 += df * df;
                w *= exp(-zz * zz / 2) * cnorm;
                u[d] = -df / (sg * sg);
            }
        if (a.md2 >= 0.0 && !(d2 < a.md2)) continue;                // strict, and a NaN distance is outside
        ++cnt;
        ws += w;
        const bool has = x == x;
        if (has) acc += w * x;
#pragma unroll
        for (int d = 0; d < 2; ++d)
            if (d < ndim) {
                ua[d] += w * u[d];
                const double gr = gv[d];
                if (has && gr == gr) sa[d] += w * (gr + u[d] * x);
            }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < npair) {
                const int pa = k == 2 ? 1 : 0, pb = k == 0 ? 0 : 1;       // (0,0), (0,1), (1,1)
                const double c = pa == pb ? u[pa] * u[pb] - q : u[pa] * u[pb];
                va[k] += w * c;
                const double h = hv[k];
                if (has && gv[pa] == gv[pa] && gv[pb] == gv[pb] && h == h)
                    ta[k] += w * (h + u[pa] * gv[pb] + u[pb] * gv[pa] + c * x);
            }
    }
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) {
        ws += __shfl_xor(ws, off);
        cnt += __shfl_xor(cnt, off);
        acc += __shfl_xor(acc, off);
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            sa[d] += __shfl_xor(sa[d], off);
            ua[d] += __shfl_xor(ua[d], off);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ta[k] += __shfl_xor(ta[k], off);
            va[k] += __shfl_xor(va[k], off);
        }
    }
    if (live && tl == 0) {
        a.out_key[g] = (long long)a.keys_sorted[s];
        a.out_count[g] = cnt;
        const double f = acc / ws;
        a.out[g] = cnt ? f : __builtin_nan("");
        double gl[2] = {0.0, 0.0};
#pragma unroll
        for (int d = 0; d < 2; ++d)
            if (d < ndim) {
                gl[d] = (sa[d] - f * ua[d]) / ws;
                out_grad[(size_t)d * (size_t)G + (size_t)g] = cnt ? gl[d] : __builtin_nan("");
            }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < npair) {
                const int pa = k == 2 ? 1 : 0, pb = k == 0 ? 0 : 1;
                const double t = ta[k] - gl[pa] * ua[pb] - gl[pb] * ua[pa] - f * va[k];
                out_hess[(size_t)k * (size_t)G + (size_t)g] = cnt ? t / ws : __builtin_nan("");
            }
    }
}

hipError_t glue_keyed_sort(const KeyRuns& k, const long long* key, void* temp, size_t& temp_bytes, hipEvent_t after_sort, hipStream_t stream) {
    if (temp) hipLaunchKernelGGL(glue_key_kernel, dim3((unsigned)((k.R + 255) / 256)), dim3(256), 0, stream, k, key);
    return key_runs(k, nullptr, nullptr, after_sort, temp, temp_bytes, stream);
}

constexpr int GLUE_KEYED_TEAM = 8;
int glue_keyed_team() { return GLUE_KEYED_TEAM; }

// launch(std::integral_constant<int, W>()) for the team width W of the call
template <class Launch>
static hipError_t dispatch_team(int team, Launch launch) {
    switch (team) {
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        case 8: launch(std::integral_constant<int, 8>()); break;
        case 16: launch(std::integral_constant<int, 16>()); break;
        case 32: launch(std::integral_constant<int, 32>()); break;
        case 64: launch(std::integral_constant<int, 64>()); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The kernels take the GlueKeyedArgs part of `a` by value and the order's columns as arguments of their own.
hipError_t launch_glue_keyed(const GlueKeyedOrderArgs& a, long long G, int team, int order, hipStream_t stream) {
    if (G <= 0) return hipSuccess;
    if (order < 0 || order > 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((G * team + 255) / 256)), block(256);
    const GlueKeyedArgs& base = a;
    return dispatch_team(team, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if (order == 0) hipLaunchKernelGGL(glue_keyed_kernel<W>, grid, block, 0, stream, base, G);
        else if (order == 1) hipLaunchKernelGGL(glue_keyed_grad_kernel<W>, grid, block, 0, stream, base, G, a.grad, a.out_grad);
        else hipLaunchKernelGGL(glue_keyed_hess_kernel<W>, grid, block, 0, stream, base, G, a.grad, a.hess, a.out_grad, a.out_hess);
    });
}

}  // namespace gpsat
