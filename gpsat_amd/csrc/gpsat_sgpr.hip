// gpsat_sgpr.hip -- fp64 sparse GP experts (GPflow SGPR: the collapsed Titsias bound) for tiles of any size (gfx950).
//
// One workgroup per tile, tiles served from an atomic queue, the on-device optimiser of gpsat_opt.h as the exact kernels use
// it.  The inducing points Z are fixed (GPflowSGPRModel's default, train_inducing_points=False), so the trainable vector is
// theta = (l_0 .. l_{D-1}, kernel_variance s, likelihood_variance sn2) and only the objective, its gradient and the
// prediction are new.  Coordinates are scaled and centred per tile by the host (Z with its tile).
//
// One evaluation ("Sparse GP experts"):
//   1. ONE pass over the tile's rows on v_mfma_f64_16x16x4_f64: Phi = Kuf Kuf^T and, with the gradient, the cross products
//      Psi_d = (dKuf/dl_d) Kuf^T, d = 0..D-1 (all M x M).  Kuf is never stored: every wave owns a 32 x 32 output tile of all
//      of them and generates its A / B operands from Z (LDS) and the rows of X (global) on the fly.  A VALU pass adds
//      b = Kuf y, e_d = (dKuf/dl_d) y and y^T y.
//   2. O(M^3) algebra in the workgroup's global workspace (fp64 VALU, column-parallel, fixed order):
//      L = chol(Kuu + jitter I), Li = L^-1, P = Li Phi Li^T, LB = chol(I + P / sn2), Q = LB^-1 Li, c = Q b / sn2;
//      ELBO = -N/2 log 2pi - sum log LB_ii - N/2 log sn2 - y'y / (2 sn2) + c'c / 2 - N s / (2 sn2) + tr P / (2 sn2).
//   3. Gradient (S = sn2 Kuu + Phi, S^-1 = Q^T Q / sn2, Kuu^-1 = Li^T Li, v = S^-1 b, beta = (b - Phi v) / sn2,
//      R = Kuu^-1 / sn2 - S^-1, w = Kuu^-1 beta):
//        dELBO/dKuf = R Kuf + w alpha^T  contracted with dKuf/dl_d  = sum R . Psi_d + (w . e_d - w . Psi_d v) / sn2,
//        dELBO/dKuu = -(R Phi Kuu^-1 + w w^T) / 2 contracted with dKuu/dtheta element by element (Kuu from Z again),
//        explicit sn2 and kdiag terms in closed form.
//   The kernel returns nll = -ELBO and dNLL/dtheta = -dELBO/dtheta.
// Every sum has a fixed order (per-thread partial sums over a fixed index set, then a fixed tree): a tile's results do not
// depend on the batch it runs in.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gpsat_kernels.h"

namespace gpsat {
namespace sgpr {

typedef double f64x4 __attribute__((ext_vector_type(4)));

extern __shared__ __attribute__((aligned(16))) double lds_s[];

#define GPSAT_NW 8                // 8 waves, one workgroup per CU: two waves per SIMD
#include "gpsat_opt.h"
#undef GPSAT_NW

constexpr int VEC = 16;           // workspace vectors of length Mmax (b, e_0..e_3, v, beta, w, c, u, tmp)

__host__ __device__ inline size_t mat_stride(int Mmax) { return (size_t)Mmax * Mmax; }
__host__ __device__ inline int n_mats(int D) { return 7 + D; }

// covariance function of r^2 (r = scaled distance): kf = k / s and gg with dk/dl_d = s gg (x_d - z_d)^2 / l_d^3
#include "gpsat_kfun_f64.h"

// k(z, x) = s kf and dk/dl_d = s gg t_d^2 / l_d with t_d = (z_d - x_d) / l_d
template <int D, int KN, bool G>
__device__ __forceinline__ void keval(const double* z, const double* x, const double* il, double s, double& k, double* dk) {
    double t[D], r2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        t[d] = (z[d] - x[d]) * il[d];
        r2 = fma(t[d], t[d], r2);
    }
    double kf, gg;
    kfun<KN>(r2, kf, gg);
    k = s * kf;
    if (G) {
        const double sg = s * gg;
#pragma unroll
        for (int d = 0; d < D; ++d) dk[d] = sg * (t[d] * t[d]) * il[d];
    }
}

struct Tile {
    int tid, lane, w;
    int N, M, P, Mmax;
    const double* X;   // [N, D] rows of this tile
    const double* y;   // [N]
    double* ws;        // this workgroup's workspace
    size_t MS;         // doubles per M x M matrix slot
    double* red;       // LDS [NT] reduction scratch
    double* zl;        // LDS [M, D] inducing points
};

// fixed-order workgroup sum (every thread gets the result)
__device__ double block_sum(const Tile& c, double v) {
    c.red[c.tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (c.tid < s) c.red[c.tid] += c.red[c.tid + s];
        __syncthreads();
    }
    const double r = c.red[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------------------
// pass 1 (MFMA): Phi = Kuf Kuf^T and (G) Psi_d = dKuf_d Kuf^T over all N rows, 32 x 32 output tiles per wave
// A operand of v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][k = l >> 4]; B: B[k = l >> 4][l & 15];
// accumulator: lane l holds C[(l >> 4) + 4 r][l & 15], r = 0..3.
// ---------------------------------------------------------------------------------------------
template <int D, int KN, bool G>
__device__ void pass_products(const Tile& c, const double* il, double s, double* Phi, double* Psi) {
    constexpr int NA = G ? D + 1 : 1;
    const int M = c.M, N = c.N;
    const int nt = (M + 31) / 32;
    const int g = c.lane & 15, q = c.lane >> 4;
    for (int tile = c.w; tile < nt * nt; tile += NW) {
        const int I0 = (tile / nt) * 32, J0 = (tile % nt) * 32;
        f64x4 acc[NA][2][2];
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[a][i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
        double zi[2][D], zj[2][D];
        bool vi[2], vj[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int mi = I0 + 16 * h + g, mj = J0 + 16 * h + g;
            vi[h] = mi < M; vj[h] = mj < M;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                zi[h][d] = vi[h] ? c.zl[mi * D + d] : 0.0;
                zj[h][d] = vj[h] ? c.zl[mj * D + d] : 0.0;
            }
        }
        for (int n0 = 0; n0 < N; n0 += 4) {
            const int n = n0 + q;
            const bool vn = n < N;
            double x[D];
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = vn ? c.X[(size_t)n * D + d] : 0.0;
            double ka[2], da[2][D > 0 ? D : 1], kb[2], dummy[D];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                keval<D, KN, G>(zi[h], x, il, s, ka[h], da[h]);
                keval<D, KN, false>(zj[h], x, il, s, kb[h], dummy);
                if (!(vn && vi[h])) {
                    ka[h] = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) da[h][d] = 0.0;
                }
                if (!(vn && vj[h])) kb[h] = 0.0;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ka[i], kb[j], acc[0][i][j], 0, 0, 0);
                    if (G) {
#pragma unroll
                        for (int d = 0; d < D; ++d)
                            acc[1 + d][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[i][d], kb[j], acc[1 + d][i][j], 0, 0, 0);
                    }
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = J0 + 16 * j + g;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = I0 + 16 * i + q + 4 * r;
                    if (row < M && col < M) {
                        Phi[(size_t)row * M + col] = acc[0][i][j][r];
                        if (G) {
#pragma unroll
                            for (int d = 0; d < D; ++d) Psi[(size_t)d * c.MS + (size_t)row * M + col] = acc[1 + d][i][j][r];
                        }
                    }
                }
            }
    }
}

// pass 1 (VALU): b = Kuf y, e_d = dKuf_d y (one thread per inducing point, rows in order)
template <int D, int KN, bool G>
__device__ void pass_vectors(const Tile& c, const double* il, double s, double* b, double* e) {
    for (int m = c.tid; m < c.M; m += NT) {
        double z[D], bb = 0.0, ee[D], dk[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { z[d] = c.zl[m * D + d]; ee[d] = 0.0; }
        for (int n = 0; n < c.N; ++n) {
            double x[D];
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = c.X[(size_t)n * D + d];
            double k;
            keval<D, KN, G>(z, x, il, s, k, dk);
            const double yn = c.y[n];
            bb = fma(k, yn, bb);
            if (G) {
#pragma unroll
                for (int d = 0; d < D; ++d) ee[d] = fma(dk[d], yn, ee[d]);
            }
        }
        b[m] = bb;
        if (G) {
#pragma unroll
            for (int d = 0; d < D; ++d) e[(size_t)d * c.M + m] = ee[d];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dense M x M algebra, row-major with leading dimension M, one thread per output column
// ---------------------------------------------------------------------------------------------
// in-place Cholesky of the lower triangle (left-looking); returns false if a pivot is not positive
__device__ bool chol(const Tile& c, double* A, int* flag) {
    const int M = c.M;
    for (int j = 0; j < M; ++j) {
        if (c.w == 0) {
            double sacc = 0.0;
            for (int k = c.lane; k < j; k += 64) sacc = fma(A[(size_t)j * M + k], A[(size_t)j * M + k], sacc);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o);
            if (c.lane == 0) {
                const double dd = A[(size_t)j * M + j] - sacc;
                if (!(dd > 0.0)) *flag = 1;
                A[(size_t)j * M + j] = sqrt(fmax(dd, 0.0));
            }
        }
        __syncthreads();
        if (*flag) return false;
        const double ljj = A[(size_t)j * M + j];
        for (int i = j + 1 + c.tid; i < M; i += NT) {
            double acc = A[(size_t)i * M + j];
            for (int k = 0; k < j; ++k) acc = fma(-A[(size_t)i * M + k], A[(size_t)j * M + k], acc);
            A[(size_t)i * M + j] = acc / ljj;
        }
        __syncthreads();
    }
    return true;
}

// X = L^-1 B (L lower; B == nullptr: the identity).  X may alias B.
__device__ void trsm(const Tile& c, const double* L, const double* B, double* X) {
    const int M = c.M;
    for (int j = c.tid; j < M; j += NT) {
        for (int i = 0; i < M; ++i) {
            double acc = B ? B[(size_t)i * M + j] : (i == j ? 1.0 : 0.0);
            const int k0 = B ? 0 : j;                      // L^-1 is lower triangular: X[k][j] = 0 for k < j
            for (int k = k0; k < i; ++k) acc = fma(-L[(size_t)i * M + k], X[(size_t)k * M + j], acc);
            X[(size_t)i * M + j] = acc / L[(size_t)i * M + i];
        }
    }
    __syncthreads();
}

// C = op(A) B, op(A) = A or A^T; epi(i, j, value) consumes every entry (rows in groups of 8 per thread)
template <bool TA, class Epi>
__device__ void mm(const Tile& c, const double* A, const double* B, Epi epi) {
    const int M = c.M;
    for (int j = c.tid; j < M; j += NT) {
        for (int i0 = 0; i0 < M; i0 += 8) {
            double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int k = 0; k < M; ++k) {
                const double bk = B[(size_t)k * M + j];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int i = min(i0 + r, M - 1);
                    const double a = TA ? A[(size_t)k * M + i] : A[(size_t)i * M + k];
                    acc[r] = fma(a, bk, acc[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (i0 + r < M) epi(i0 + r, j, acc[r]);
        }
    }
    __syncthreads();
}

// y = op(A) x for vectors (one thread per row)
template <bool TA>
__device__ void mv(const Tile& c, const double* A, const double* x, double* y) {
    const int M = c.M;
    for (int i = c.tid; i < M; i += NT) {
        double acc = 0.0;
        for (int k = 0; k < M; ++k) acc = fma(TA ? A[(size_t)k * M + i] : A[(size_t)i * M + k], x[k], acc);
        y[i] = acc;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// one evaluation at sh->theta: sh->nll = -ELBO, sh->gth = -dELBO/dtheta (want_grad), sh->fail
// ---------------------------------------------------------------------------------------------
template <int D, int KN>
__device__ void evaluate(const Tile& c, Shared* sh, bool want_grad, double jitter, int* flag) {
    const int M = c.M, N = c.N;
    double il[D];
#pragma unroll
    for (int d = 0; d < D; ++d) il[d] = 1.0 / sh->theta[d];
    const double s = sh->theta[D], sn2 = sh->theta[D + 1];
    const size_t MS = c.MS;
    double* Lb = c.ws;                 // Kuu -> L -> L^-T
    double* Li = c.ws + MS;            // L^-1
    double* Tb = c.ws + 2 * MS;        // Li Phi -> Q -> Phi Kuu^-1
    double* Ph = c.ws + 3 * MS;        // Phi
    double* Bb = c.ws + 4 * MS;        // P -> B -> LB
    double* Ki = c.ws + 5 * MS;        // Kuu^-1
    double* Rb = c.ws + 6 * MS;        // R
    double* Ps = c.ws + 7 * MS;        // Psi_0 .. Psi_{D-1}
    double* vb = c.ws + (size_t)n_mats(D) * MS;
    const int Mmax = c.Mmax;
    double* b = vb;
    double* e = vb + Mmax;             // D vectors
    double* v = vb + 5 * Mmax;
    double* beta = vb + 6 * Mmax;
    double* w = vb + 7 * Mmax;
    double* cc = vb + 8 * Mmax;
    double* u = vb + 9 * Mmax;
    double* tmp = vb + 10 * Mmax;

    if (c.tid == 0) { sh->fail = 0; sh->n_eval += 1; *flag = 0; }
    __syncthreads();
    // ---- pass over the rows
    if (want_grad) {
        pass_products<D, KN, true>(c, il, s, Ph, Ps);
        pass_vectors<D, KN, true>(c, il, s, b, e);
    } else {
        pass_products<D, KN, false>(c, il, s, Ph, Ps);
        pass_vectors<D, KN, false>(c, il, s, b, e);
    }
    double yyp = 0.0;
    for (int n = c.tid; n < N; n += NT) yyp = fma(c.y[n], c.y[n], yyp);
    const double yy = block_sum(c, yyp);     // (its barriers also order pass 1 before what follows)
    // ---- Kuu + jitter I
    for (int e2 = c.tid; e2 < M * M; e2 += NT) {
        const int i = e2 / M, j = e2 % M;
        double k, dk[D];
        keval<D, KN, false>(c.zl + i * D, c.zl + j * D, il, s, k, dk);
        Lb[e2] = k + (i == j ? jitter : 0.0);
    }
    __syncthreads();
    if (!chol(c, Lb, flag)) { if (c.tid == 0) { sh->fail = 1; sh->nll = 0.0; } __syncthreads(); return; }
    trsm(c, Lb, nullptr, Li);
    // L^-T into Lb (L is no longer needed)
    for (int e2 = c.tid; e2 < M * M; e2 += NT) { const int i = e2 / M, j = e2 % M; Lb[e2] = Li[(size_t)j * M + i]; }
    __syncthreads();
    // P = Li Phi Li^T;  B = I + P / sn2
    mm<false>(c, Li, Ph, [&](int i, int j, double x) { Tb[(size_t)i * M + j] = x; });
    mm<false>(c, Tb, Lb, [&](int i, int j, double x) { Bb[(size_t)i * M + j] = x; });
    double trp = 0.0;
    for (int i = c.tid; i < M; i += NT) trp += Bb[(size_t)i * M + i];
    const double trP = block_sum(c, trp);
    for (int e2 = c.tid; e2 < M * M; e2 += NT) Bb[e2] = Bb[e2] / sn2 + ((e2 / M) == (e2 % M) ? 1.0 : 0.0);
    __syncthreads();
    if (!chol(c, Bb, flag)) { if (c.tid == 0) { sh->fail = 1; sh->nll = 0.0; } __syncthreads(); return; }
    double ldp = 0.0;
    for (int i = c.tid; i < M; i += NT) ldp += log(Bb[(size_t)i * M + i]);
    const double logdet = block_sum(c, ldp);
    // Q = LB^-1 Li;  c = Q b / sn2
    trsm(c, Bb, Li, Tb);
    mv<false>(c, Tb, b, cc);
    double ccp = 0.0;
    for (int i = c.tid; i < M; i += NT) { cc[i] /= sn2; ccp = fma(cc[i], cc[i], ccp); }
    const double ctc = block_sum(c, ccp);
    const double LOG2PI = 1.8378770664093453;
    const double el = -0.5 * N * LOG2PI - logdet - 0.5 * N * log(sn2) - 0.5 * yy / sn2 + 0.5 * ctc - 0.5 * N * s / sn2
                      + 0.5 * trP / sn2;
    if (c.tid == 0) {
        sh->nll = -el;
        if (!(el == el)) { sh->fail = 1; sh->nll = __builtin_nan(""); }
    }
    if (!want_grad) { __syncthreads(); return; }

    // ---- gradient
    mm<false>(c, Lb, Li, [&](int i, int j, double x) { Ki[(size_t)i * M + j] = x; });                      // Kuu^-1
    mm<true>(c, Tb, Tb, [&](int i, int j, double x) { Rb[(size_t)i * M + j] = (Ki[(size_t)i * M + j] - x) / sn2; });  // R
    // v = Kuu^-1 b / sn2 - R b;  u = Phi v;  beta = (b - u) / sn2;  w = Kuu^-1 beta
    mv<false>(c, Ki, b, v);
    mv<false>(c, Rb, b, tmp);
    for (int i = c.tid; i < M; i += NT) v[i] = v[i] / sn2 - tmp[i];
    __syncthreads();
    mv<false>(c, Ph, v, u);
    for (int i = c.tid; i < M; i += NT) beta[i] = (b[i] - u[i]) / sn2;
    __syncthreads();
    mv<false>(c, Ki, beta, w);
    // element-wise traces: tr(Kuu^-1 Phi), tr(R Phi), sum R . Psi_d
    double p_kp = 0.0, p_rp = 0.0, p_rs[D];
#pragma unroll
    for (int d = 0; d < D; ++d) p_rs[d] = 0.0;
    for (int e2 = c.tid; e2 < M * M; e2 += NT) {
        const double ph = Ph[e2], r = Rb[e2];
        p_kp = fma(Ki[e2], ph, p_kp);
        p_rp = fma(r, ph, p_rp);
#pragma unroll
        for (int d = 0; d < D; ++d) p_rs[d] = fma(r, Ps[(size_t)d * MS + e2], p_rs[d]);
    }
    // vector terms: b.v, v.u, w.beta, w.e_d, w.(Psi_d v)
    double p_bv = 0.0, p_vu = 0.0, p_wb = 0.0, p_we[D], p_wpv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { p_we[d] = 0.0; p_wpv[d] = 0.0; }
    for (int i = c.tid; i < M; i += NT) {
        p_bv = fma(b[i], v[i], p_bv);
        p_vu = fma(v[i], u[i], p_vu);
        p_wb = fma(w[i], beta[i], p_wb);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            p_we[d] = fma(w[i], e[(size_t)d * M + i], p_we[d]);
            double a = 0.0;
            for (int k = 0; k < M; ++k) a = fma(Ps[(size_t)d * MS + (size_t)i * M + k], v[k], a);
            p_wpv[d] = fma(w[i], a, p_wpv[d]);
        }
    }
    // dELBO/dKuu = -(R Phi Kuu^-1 + w w^T) / 2 against dKuu/dl_d and dKuu/ds = Kuu (jitter excluded) / s
    mm<false>(c, Ph, Ki, [&](int i, int j, double x) { Tb[(size_t)i * M + j] = x; });                      // Phi Kuu^-1
    double p_gu[D + 1];
#pragma unroll
    for (int d = 0; d <= D; ++d) p_gu[d] = 0.0;
    mm<false>(c, Rb, Tb, [&](int i, int j, double x) {
        const double gij = -0.5 * (x + w[i] * w[j]);
        double k, dk[D];
        keval<D, KN, true>(c.zl + i * D, c.zl + j * D, il, s, k, dk);
#pragma unroll
        for (int d = 0; d < D; ++d) p_gu[d] = fma(gij, dk[d], p_gu[d]);
        p_gu[D] = fma(gij, k, p_gu[D]);
    });
    const double trKP = block_sum(c, p_kp);
    const double trRP = block_sum(c, p_rp);
    const double bv = block_sum(c, p_bv);
    const double vu = block_sum(c, p_vu);
    const double wb = block_sum(c, p_wb);
    const double gus = block_sum(c, p_gu[D]);
    const double trSP = trKP / sn2 - trRP;                            // tr(S^-1 Phi)
    const double aa = (yy - 2.0 * bv + vu) / (sn2 * sn2);             // alpha^T alpha
    const double g_sn2 = 0.5 * (aa - (N - trSP) / sn2) + (N * s - trKP) / (2.0 * sn2 * sn2);
    const double g_s = (trRP + wb) / s + gus / s - N / (2.0 * sn2);
    double g_l[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double rs = block_sum(c, p_rs[d]);
        const double we = block_sum(c, p_we[d]);
        const double wpv = block_sum(c, p_wpv[d]);
        const double gu = block_sum(c, p_gu[d]);
        g_l[d] = rs + (we - wpv) / sn2 + gu;
    }
    if (c.tid == 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) sh->gth[d] = -g_l[d];
        sh->gth[D] = -g_s;
        sh->gth[D + 1] = -g_sn2;
        bool bad = false;
        for (int i = 0; i < D + 2; ++i) bad |= !(sh->gth[i] == sh->gth[i]);
        if (bad && !sh->fail) { sh->fail = 1; sh->nll = __builtin_nan(""); }
    }
    __syncthreads();
}

// prediction at the factors of the last evaluation: t1 = Li Kus, t2 = LB^-1 t1, f* = t2^T c,
// f*_var = s + colsum t2^2 - colsum t1^2 (one thread per prediction point, its columns in the scratch area)
template <int D, int KN>
__device__ void predict(const Tile& c, const Shared* sh, const double* Xs, double* fm, double* fv, double* yv) {
    const int M = c.M, Mmax = c.Mmax;
    double il[D];
#pragma unroll
    for (int d = 0; d < D; ++d) il[d] = 1.0 / sh->theta[d];
    const double s = sh->theta[D], sn2 = sh->theta[D + 1];
    const size_t MS = c.MS;
    const double* Li = c.ws + MS;
    const double* LB = c.ws + 4 * MS;
    const double* cc = c.ws + (size_t)n_mats(D) * MS + 8 * Mmax;
    double* U = c.ws + (size_t)n_mats(D) * MS + (size_t)VEC * Mmax;     // [Mmax][NT]  Kus column
    double* V = U + (size_t)Mmax * NT;                                   // [Mmax][NT]  t1 -> t2
    for (int p0 = 0; p0 < c.P; p0 += NT) {
        const int p = p0 + c.tid;
        if (p < c.P) {
            double x[D], dk[D];
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = Xs[(size_t)p * D + d];
            for (int k = 0; k < M; ++k) {
                double kv;
                keval<D, KN, false>(c.zl + k * D, x, il, s, kv, dk);
                U[(size_t)k * NT + c.tid] = kv;
            }
            double s1 = 0.0, s2 = 0.0, f = 0.0;
            for (int i = 0; i < M; ++i) {
                double a = 0.0;
                for (int k = 0; k <= i; ++k) a = fma(Li[(size_t)i * M + k], U[(size_t)k * NT + c.tid], a);
                V[(size_t)i * NT + c.tid] = a;
                s1 = fma(a, a, s1);
            }
            for (int i = 0; i < M; ++i) {
                double a = V[(size_t)i * NT + c.tid];
                for (int k = 0; k < i; ++k) a = fma(-LB[(size_t)i * M + k], V[(size_t)k * NT + c.tid], a);
                a /= LB[(size_t)i * M + i];
                V[(size_t)i * NT + c.tid] = a;
                s2 = fma(a, a, s2);
                f = fma(a, cc[i], f);
            }
            const double var = s + s2 - s1;
            fm[p] = f; fv[p] = var; yv[p] = var + sn2;
        }
    }
}

template <int D, int KN>
__global__ void __launch_bounds__(NT, 1) sgpr_kernel(const SgprArgs A) {
    constexpr int H = D + 2;
    Shared* sh = reinterpret_cast<Shared*>(lds_s);
    Tile c;
    c.tid = threadIdx.x; c.lane = c.tid & 63; c.w = c.tid >> 6;
    int off = (int)((sizeof(Shared) + 15) / 16) * 2;
    c.red = lds_s + off; off += NT;
    int* flag = reinterpret_cast<int*>(lds_s + off); off += 2;
    c.zl = lds_s + off;
    c.Mmax = A.Mmax;
    c.MS = mat_stride(A.Mmax);
    c.ws = A.ws + (size_t)blockIdx.x * A.ws_stride;
    const OptCfg o = opt_cfg(A);
    for (;;) {
        __syncthreads();
        if (c.tid == 0) {
            const int slot = atomicAdd(A.queue, 1);
            sh->tile = slot < A.T ? A.order[slot] : -1;
        }
        __syncthreads();
        const int t = sh->tile;
        if (t < 0) break;
        const long long o0 = A.obs_off[t], o1 = A.obs_off[t + 1];
        const long long p0 = A.pred_off[t], p1 = A.pred_off[t + 1];
        const long long z0 = A.z_off[t], z1 = A.z_off[t + 1];
        c.N = (int)(o1 - o0); c.P = (int)(p1 - p0); c.M = (int)(z1 - z0);
        c.X = A.X + (size_t)o0 * D; c.y = A.y + o0;
        if (c.N == 0) {
            if (c.tid == 0) tile_out_empty(A, H, t);
            tile_predict_prior(A, H, t, c.tid, p0, p1, A.f_mean, A.f_var, A.y_var);
            continue;
        }
        for (int i = c.tid; i < c.M * D; i += NT) c.zl[i] = A.Z[(size_t)z0 * D + i];
        if (c.tid == 0) opt_fresh_tile(sh, A, H, t, o);
        __syncthreads();
        for (;;) {
            evaluate<D, KN>(c, sh, sh->want_grad != 0, A.jitter, flag);
            if (c.tid == 0) opt_advance(sh, H, o);
            __syncthreads();
            if (sh->phase == PH_EXIT) break;
        }
        if (c.tid == 0) tile_out_finished(A, sh, H, t);
        if (c.P > 0) {
            if (!sh->fail) {
                predict<D, KN>(c, sh, A.Xs + (size_t)p0 * D, A.f_mean + p0, A.f_var + p0, A.y_var + p0);
            } else {
                tile_predict_nan(c.tid, p0, p1, A.f_mean, A.f_var, A.y_var);
            }
        }
    }
}

template <int D, int KN>
static hipError_t launch_one(const SgprArgs& a, int grid, size_t smem, hipStream_t stream) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sgpr_kernel<D, KN>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((sgpr_kernel<D, KN>), dim3(grid), dim3(NT), smem, stream, a);
    return hipGetLastError();
}

template <int D>
static hipError_t launch_d(const SgprArgs& a, int grid, size_t smem, hipStream_t stream) {
    switch (a.kernel) {
        case 0: return launch_one<D, 0>(a, grid, smem, stream);
        case 1: return launch_one<D, 1>(a, grid, smem, stream);
        case 2: return launch_one<D, 2>(a, grid, smem, stream);
        case 3: return launch_one<D, 3>(a, grid, smem, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace sgpr

size_t sgpr_shared_bytes(int D, int Mmax) {
    const size_t off = ((sizeof(sgpr::Shared) + 15) / 16) * 2 + sgpr::NT + 2;
    return (off + (size_t)Mmax * D) * sizeof(double);
}

size_t sgpr_workspace_doubles_per_wg(int D, int Mmax) {
    return (size_t)sgpr::n_mats(D) * sgpr::mat_stride(Mmax) + (size_t)sgpr::VEC * Mmax + 2 * (size_t)Mmax * sgpr::NT;
}

int sgpr_threads() { return sgpr::NT; }

hipError_t launch_sgpr(int D, const SgprArgs& a, int grid, size_t smem, hipStream_t stream) {
    switch (D) {
        case 1: return sgpr::launch_d<1>(a, grid, smem, stream);
        case 2: return sgpr::launch_d<2>(a, grid, smem, stream);
        case 3: return sgpr::launch_d<3>(a, grid, smem, stream);
        case 4: return sgpr::launch_d<4>(a, grid, smem, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace gpsat
