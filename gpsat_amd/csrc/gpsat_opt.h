// gpsat_opt.h -- what the persistent kernels (fp32 tiles, fp64 tiles and teams, sparse experts) share, device code:
//   * the per-workgroup optimiser state (Shared) and the on-device L-BFGS / L-BFGS-B / Adam driver (thread 0, fp64
//     arithmetic), advanced once per evaluation by opt_advance;
//   * the per-tile driver pieces around the evaluate / opt_advance loop (at the end of the file): OptCfg from the kernel
//     arguments, a fresh tile's optimiser state, the outputs of an empty and of a finished tile, prior and NaN predictions,
//     and the save / load of a suspended tile's state (time slicing).
// The numerics -- evaluate, predict, the prior covariance of an empty tile -- stay with each kernel.
// Included inside each kernel's namespace (under namespace gpsat), after GPSAT_NW is set.
#ifndef GPSAT_OPT_H
#define GPSAT_OPT_H

#ifndef GPSAT_NW
#define GPSAT_NW 4
#endif
constexpr int NW = GPSAT_NW;   // waves per workgroup (power of two; fp32 kernels 4, fp64 kernels see gpsat_kernels_f64.hip)
constexpr int NT = 64 * NW;    // threads per workgroup
constexpr int HMAX = 6;        // max D + 2 (D <= 4)
constexpr int MH = 10;         // L-BFGS history (SciPy L-BFGS-B maxcor default)

// ---------------------------------------------------------------------------------------------
// per-workgroup state
// ---------------------------------------------------------------------------------------------
struct Shared {
    // evaluation interface
    double theta[HMAX];
    double gth[HMAX];          // dNLL/dtheta
    double nll;
    double logdet;
    double red[8][8];          // partial sums of eight VIRTUAL waves (the 4-wave builds run two each): same sums in every build
    // optimiser state (thread 0 writes, everybody reads after a barrier)
    double lo[HMAX], hi[HMAX], shift[HMAX];
    double u[HMAX], g[HMAX], f;            // current accepted point (u-space)
    double ut[HMAX], gt[HMAX], ft;         // trial point
    double ub[HMAX], gb[HMAX];             // best sufficient-decrease point of the running line search (value f_best)
    double d[HMAX];
    double S[MH][HMAX], Y[MH][HMAX], rho_[MH];
    double m1[HMAX], m2[HMAX];             // Adam moments
    // line search
    double t, t_prev, f_prev, dphi_prev, t_lo, f_lo, dphi_lo, t_hi, f_hi, dphi_hi, dphi0, t_best, f_best, last_dec;
    int ls_phase, ls_iter, ls_done, ls_ok;
    int hist_n, hist_pos;
    int trainable[HMAX];
    int box[HMAX];
    int fail, done, status, n_eval, n_eval_opt, iter, phase, want_grad;
    int tile;
    // flags of the Cholesky / inverse sweep (phase_pt of the fp32 kernels; the fp64 kernels use g0done and gnext)
    int g0done;                 // panel index up to which group 0 of the previous panel is in memory
    int gnext[2];               // fp64 kernels: dynamic group queue heads of the PT slots (alternating)
#ifdef GPSAT_PT_FLAGS
    int ready, parked, whfree;  // panels: chain complete / group-0 k-loop parked / parked k-loop consumed
    int gdone[2];               // groups of the panel of that parity that are finished
    int qhead;                  // bulk group queue head (all panels)
    int colrow[GPSAT_PT_MAXNB]; // per block column: panels whose rows are in memory
#endif
    int gradnext;               // dynamic group queue head of the gradient phase
    int coop_seq;               // cooperative tiles: phases this workgroup has opened as an owner (not part of a tile's state)
    int coop_now;               // the running evaluation is cooperative
    int hp[8];                  // helper bookkeeping (see helper_loop of the fp32 kernels)
#ifdef GPSAT_PROFILE
    unsigned long long prof[NW * 16];      // diagnostic build: cycle counters per wave and code segment
    int tcnt[NW], tron;                    // event trace (workgroup 0): entries per wave, on/off
#else
    unsigned long long prof[1];
#endif
};


// ---------------------------------------------------------------------------------------------
// parameter transforms (reference GPSat/utils.py:2320-2400,
// GPSat/models/gpflow_models.py:490-494): box -> lo + (hi-lo) sigmoid(u); else softplus(u) + shift
// ---------------------------------------------------------------------------------------------
static __device__ inline double softplus_d(double x) { return log1p(exp(-fabs(x))) + fmax(x, 0.0); }

// A build that defines GPSAT_OPT_IDENTITY has a third code, box 3: the identity, theta = u, for a parameter that may take any
// finite real value (the constant mean of the fp64 tile kernel's -DGPSAT_F64_MEAN builds, which set the code themselves
// behind opt_fresh_tile).  Without the define these functions are what they were.
static __device__ __noinline__ double theta_of_u(const Shared* sh, int i, double u) {
#ifdef GPSAT_OPT_IDENTITY
    if (sh->box[i] == 3) return u;
#endif
    if (sh->box[i] == 2) return exp(u);          // log transform (bounded L-BFGS-B in log space, gpsat_fit_predict_batch_ms)
    if (sh->box[i]) return sh->lo[i] + (sh->hi[i] - sh->lo[i]) / (1.0 + exp(-u));
    return softplus_d(u) + sh->shift[i];
}

static __device__ __noinline__ double u_of_theta(const Shared* sh, int i, double th) {
#ifdef GPSAT_OPT_IDENTITY
    if (sh->box[i] == 3) return th;
#endif
    if (sh->box[i] == 2) return log(th);
    if (sh->box[i]) {
        const double lo = sh->lo[i], hi = sh->hi[i];
        double t = (th - lo) / (hi - lo);
        t = fmin(fmax(t, 1e-15), 1.0 - 1e-15);
        return log(t / (1.0 - t));
    }
    double y = th - sh->shift[i];
    if (y < 1e-300) y = 1e-300;
    if (y > 34.0) return y;
    if (y < 1e-15) return log(y);
    return log(-expm1(-y)) + y;
}

static __device__ inline double dtheta_du(const Shared* sh, int i, double th) {
#ifdef GPSAT_OPT_IDENTITY
    if (sh->box[i] == 3) return 1.0;
#endif
    if (sh->box[i] == 2) return th;
    if (sh->box[i]) return (th - sh->lo[i]) * (sh->hi[i] - th) / (sh->hi[i] - sh->lo[i]);
    return -expm1(-(th - sh->shift[i]));
}

// thread 0: trial u -> theta for the next evaluation
static __device__ __noinline__ void set_trial(Shared* sh, int H, const double* u) {
    for (int i = 0; i < H; ++i) {
        sh->ut[i] = u[i];
        if (sh->trainable[i]) sh->theta[i] = theta_of_u(sh, i, u[i]);
    }
}

// thread 0: after an evaluation, chain the gradient to u-space at the trial point
static __device__ __noinline__ void fetch_trial(Shared* sh, int H) {
    sh->ft = sh->fail ? __builtin_inf() : sh->nll;
    for (int i = 0; i < H; ++i)
        sh->gt[i] = (sh->trainable[i] && !sh->fail) ? sh->gth[i] * dtheta_du(sh, i, sh->theta[i]) : 0.0;
}

// L-BFGS two-loop recursion (thread 0): d = -H g
static __device__ __noinline__ void lbfgs_direction(Shared* sh, int H) {
    double q[HMAX], al[MH];
    for (int i = 0; i < H; ++i) q[i] = sh->g[i];
    const int n = sh->hist_n;
    for (int m = 0; m < n; ++m) {
        const int idx = (sh->hist_pos - 1 - m + 2 * MH) % MH;
        double a = 0.0;
        for (int i = 0; i < H; ++i) a += sh->S[idx][i] * q[i];
        a *= sh->rho_[idx];
        al[m] = a;
        for (int i = 0; i < H; ++i) q[i] -= a * sh->Y[idx][i];
    }
    if (n > 0) {
        const int idx = (sh->hist_pos - 1 + MH) % MH;
        double sy = 0.0, yy = 0.0;
        for (int i = 0; i < H; ++i) { sy += sh->S[idx][i] * sh->Y[idx][i]; yy += sh->Y[idx][i] * sh->Y[idx][i]; }
        const double gam = sy / yy;
        for (int i = 0; i < H; ++i) q[i] *= gam;
    }
    for (int m = n - 1; m >= 0; --m) {
        const int idx = (sh->hist_pos - 1 - m + 2 * MH) % MH;
        double b = 0.0;
        for (int i = 0; i < H; ++i) b += sh->Y[idx][i] * q[i];
        b *= sh->rho_[idx];
        for (int i = 0; i < H; ++i) q[i] += (al[m] - b) * sh->S[idx][i];
    }
    for (int i = 0; i < H; ++i) sh->d[i] = -q[i];
}

static __device__ inline double cubic_min(double a, double fa, double da, double b, double fb, double db) {
    // minimiser of the cubic interpolating (a,fa,da), (b,fb,db); falls back to bisection
    const double d1 = da + db - 3.0 * (fa - fb) / (a - b);
    const double rad = d1 * d1 - da * db;
    if (!(rad >= 0.0)) return 0.5 * (a + b);
    double d2 = sqrt(rad);
    if (b < a) d2 = -d2;
    const double den = db - da + 2.0 * d2;
    if (den == 0.0) return 0.5 * (a + b);
    const double t = b - (b - a) * ((db + d2 - d1) / den);
    if (!(t == t)) return 0.5 * (a + b);
    return t;
}

// strong-Wolfe line search step (thread 0).  Called after each trial evaluation.
// Sets sh->ls_done (1 accepted / 2 failed) or the next sh->t.
// stpmax: largest step that keeps the trial point in the box (bounded L-BFGS-B); >= 1e300 = no limit
static __device__ __noinline__ void ls_step(Shared* sh, int H, int max_ls, double stpmax = 1e300) {
    const double c1 = 1e-4, c2 = 0.9;
    const double t = sh->t, ft = sh->ft;
    double dphit = 0.0;
    for (int i = 0; i < H; ++i) dphit += sh->gt[i] * sh->d[i];
    const bool finite = (ft == ft) && (ft < 1e300);
    const bool armijo = finite && (ft <= sh->f + c1 * t * sh->dphi0);
    if (armijo && ft < sh->f_best) {
        sh->f_best = ft; sh->t_best = t;
        for (int i = 0; i < H; ++i) { sh->ub[i] = sh->ut[i]; sh->gb[i] = sh->gt[i]; }
    }
    sh->ls_iter += 1;
    if (armijo && fabs(dphit) <= -c2 * sh->dphi0) { sh->ls_done = 1; return; }
    if (sh->ls_phase == 1) {
        // MINPACK-2 dcsrch's "XTOL TEST SATISFIED" (xtol = 0.1 in L-BFGS-B): this trial was placed inside a bracket
        // whose relative width had already shrunk to 10 % -- the search ends here, and L-BFGS-B takes the step
        // (lnsrlb treats the warning like convergence).  The sufficient-decrease point is taken: this trial if it is
        // one, else the best one seen; with none at all the search has failed.
        const double a0 = fmin(sh->t_lo, sh->t_hi), b0 = fmax(sh->t_lo, sh->t_hi);
        if (b0 - a0 <= 0.1 * b0) {
            if (armijo) { sh->ls_done = 1; return; }
            if (sh->t_best > 0.0) {
                sh->t = sh->t_best; sh->ft = sh->f_best;
                for (int i = 0; i < H; ++i) { sh->ut[i] = sh->ub[i]; sh->gt[i] = sh->gb[i]; }
                sh->ls_done = 3;          // accepted, but the factorisation in memory belongs to another point
                return;
            }
            sh->ls_done = 2;
            return;
        }
    }
    // max_ls evaluations without meeting the strong Wolfe conditions: failure, as L-BFGS-B's `iback >= maxls` (mainlb)
    if (sh->ls_iter >= max_ls) { sh->ls_done = 2; return; }
    if (sh->ls_phase == 0) {
        if (!armijo || (sh->ls_iter > 1 && ft >= sh->f_prev)) {
            sh->t_lo = sh->t_prev; sh->f_lo = sh->f_prev; sh->dphi_lo = sh->dphi_prev;
            sh->t_hi = t; sh->f_hi = ft; sh->dphi_hi = dphit;
            sh->ls_phase = 1;
        } else if (dphit >= 0.0) {
            sh->t_lo = t; sh->f_lo = ft; sh->dphi_lo = dphit;
            sh->t_hi = sh->t_prev; sh->f_hi = sh->f_prev; sh->dphi_hi = sh->dphi_prev;
            sh->ls_phase = 1;
        } else {
            // not bracketed yet (sufficient decrease, still descending): extrapolate as More-Thuente / SciPy's dcsrch do --
            // the cubic through the last two points when its minimiser lies ahead, safeguarded to
            // [t + 1.1 (t - t_prev), t + 4 (t - t_prev)]
            if (stpmax < 1e300 && t >= stpmax) { sh->ls_done = 1; return; }   // dcsrch: "STP = STPMAX", taken by lnsrlb
            const double tp = sh->t_prev, dt = t - tp;
            double tn = cubic_min(tp, sh->f_prev, sh->dphi_prev, t, ft, dphit);
            const double lo_b = t + 1.1 * dt, hi_b = t + 4.0 * dt;
            if (!(tn > lo_b)) tn = hi_b;          // minimiser behind us or undefined: the cubic has no minimum ahead
            tn = fmin(tn, hi_b);
            if (stpmax < 1e300) tn = fmin(tn, stpmax);
            sh->t_prev = t; sh->f_prev = ft; sh->dphi_prev = dphit;
            sh->t = tn;
            return;
        }
    } else {
        if (!armijo || ft >= sh->f_lo) {
            sh->t_hi = t; sh->f_hi = ft; sh->dphi_hi = dphit;
        } else {
            if (dphit * (sh->t_hi - sh->t_lo) >= 0.0) { sh->t_hi = sh->t_lo; sh->f_hi = sh->f_lo; sh->dphi_hi = sh->dphi_lo; }
            sh->t_lo = t; sh->f_lo = ft; sh->dphi_lo = dphit;
        }
    }
    // next trial inside (lo, hi)
    const double lo = sh->t_lo, hi = sh->t_hi;
    double tn;
    const bool hi_finite = (sh->f_hi == sh->f_hi) && (sh->f_hi < 1e300);
    if (hi_finite) tn = cubic_min(lo, sh->f_lo, sh->dphi_lo, hi, sh->f_hi, sh->dphi_hi);
    else tn = 0.5 * (lo + hi);
    const double a = fmin(lo, hi), b = fmax(lo, hi), wdt = b - a;
    if (!(tn > a + 0.1 * wdt && tn < b - 0.1 * wdt)) tn = 0.5 * (a + b);
    if (wdt < 1e-12 * fmax(1.0, b)) { sh->ls_done = (armijo ? 1 : 2); return; }
    sh->t = tn;
}

// ---------------------------------------------------------------------------------------------
// optimiser driver (thread 0): a state machine advanced once per objective evaluation, so that the
// kernel has ONE inlined call site of evaluate().
// ---------------------------------------------------------------------------------------------
// per-tile status codes written by the optimiser (include/gpsat_hip.h GPSAT_STATUS_*)
enum { ST_CONVERGED = 0, ST_MAXITER = 1, ST_LS_FAILED = 6 };

enum { PH_INIT = 0, PH_LS = 1, PH_ADAM = 2, PH_FINAL = 3, PH_EXIT = 4 };

struct OptCfg {
    int optimiser, max_iter, max_ls, want_grad_out; double ftol, gtol, adam_lr, noise_rel;
    // bounded L-BFGS-B in log space with ms_S starts per tile (gpsat_fit_predict_batch_ms; ms_S = 0: the optimisers above).
    // Per-tile state lives in device memory, indexed by tile: a suspended tile resumes on any workgroup.
    int ms_S = 0;
    const double* ms_starts = nullptr;   // [T][ms_S - 1][H] further starts, constrained space, inside the bounds
    double* ms_state = nullptr;          // [T][MS_WORDS] (see ms_end_start), preset by the host
    double* ms_fout = nullptr;           // [T][ms_S] final objective of every start, or nullptr
    // The last evaluation was answered from the tile's memo of evaluations (fp32 tile kernels), and the factorisation in this
    // workgroup's memory belongs to other parameter floats: thread 0 sets it before opt_advance; ms_S = 0 only.
    int factor_stale = 0;
};

// per-tile multi-start state, MS_WORDS (gpsat_kernels.h) doubles: [0] index of the running start, [1] best f, [2] its
// iterations, [3] its status, [4] its start index (-1: none yet), [5 .. 5 + H) its u; the host presets 0, +inf, 0, 0, -1,
// u of start 0
// thread 0 reads and writes it with agent-scope word accesses, as the saved state of a suspended tile (memory, not L2)
static __device__ inline double ms_ld(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}
static __device__ inline void ms_st(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// u-space box of parameter i (log transform); a fixed parameter is pinned at its value
static __device__ inline void lb_bounds(const Shared* sh, int i, double& l, double& h) {
    if (!sh->trainable[i]) { l = h = sh->u[i]; return; }
    l = log(sh->lo[i]);                       // the host refuses lo <= 0; an infinite bound stays infinite
    h = log(sh->hi[i]);
    if (!(l == l)) l = -__builtin_inf();      // NaN bound: unbounded on that side
    if (!(h == h)) h = __builtin_inf();
}

// projected gradient max-norm (L-BFGS-B projgr) at the accepted point
static __device__ __noinline__ double lb_projgr(const Shared* sh, int H) {
    double m = 0.0;
    for (int i = 0; i < H; ++i) {
        if (!sh->trainable[i]) continue;
        double l, h; lb_bounds(sh, i, l, h);
        double gi = sh->g[i];
        if (gi < 0.0) gi = fmax(sh->u[i] - h, gi);
        else gi = fmin(sh->u[i] - l, gi);
        m = fmax(m, fabs(gi));
    }
    return m;
}

// ---------------------------------------------------------------------------------------------
// bounded L-BFGS-B (Byrd, Lu, Nocedal, Zhu 1995; SciPy's lbfgsb 3.0) for H <= 6 parameters.  The limited-memory matrix
// B = theta I - W M W^T is formed densely (H x H) by applying the stored pairs, oldest first, to theta I -- the same
// matrix as the compact form -- and the generalised Cauchy point and the subspace minimisation work on it directly.
// ---------------------------------------------------------------------------------------------
static __device__ __noinline__ void lb_matrix(const Shared* sh, int H, double B[HMAX][HMAX]) {
    double th = 1.0;
    const int n = sh->hist_n;
    if (n > 0) {
        const int last = (sh->hist_pos - 1 + MH) % MH;
        double yy = 0.0;
        for (int i = 0; i < H; ++i) yy += sh->Y[last][i] * sh->Y[last][i];
        th = yy * sh->rho_[last];                 // y'y / s'y of the newest pair (mainlb: theta = rr / dr)
    }
    for (int i = 0; i < H; ++i) for (int j = 0; j < H; ++j) B[i][j] = (i == j) ? th : 0.0;
    for (int m = n - 1; m >= 0; --m) {
        const int idx = (sh->hist_pos - 1 - m + 2 * MH) % MH;
        double Bs[HMAX], sBs = 0.0;
        for (int i = 0; i < H; ++i) {
            double a = 0.0;
            for (int j = 0; j < H; ++j) a += B[i][j] * sh->S[idx][j];
            Bs[i] = a;
            sBs += sh->S[idx][i] * a;
        }
        if (!(sBs > 0.0)) continue;
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < H; ++j)
                B[i][j] += sh->rho_[idx] * sh->Y[idx][i] * sh->Y[idx][j] - Bs[i] * Bs[j] / sBs;
    }
}

// largest step along sh->d from sh->u that stays in the box (lnsrlb's stpmx: 1 in the first iteration; recomputed
// for every trial of the line search rather than kept in Shared)
static __device__ __noinline__ double lb_stpmax(const Shared* sh, int H) {
    if (sh->iter == 0) return 1.0;
    double stpmx = 1e10;
    for (int i = 0; i < H; ++i) {
        double l, h; lb_bounds(sh, i, l, h);
        const double a1 = sh->d[i];
        if (a1 < 0.0 && l > -__builtin_inf()) {
            const double a2 = l - sh->u[i];
            if (a2 >= 0.0) stpmx = 0.0; else if (a1 * stpmx < a2) stpmx = a2 / a1;
        } else if (a1 > 0.0 && h < __builtin_inf()) {
            const double a2 = h - sh->u[i];
            if (a2 <= 0.0) stpmx = 0.0; else if (a1 * stpmx > a2) stpmx = a2 / a1;
        }
    }
    return stpmx;
}

// one L-BFGS-B iteration up to the line search: Cauchy point, subspace minimisation, search direction sh->d and the
// largest feasible step; returns that step (0: no descent direction)
static __device__ __noinline__ double lb_direction(Shared* sh, int H) {
    const double eps = 2.220446049250313e-16;
    double B[HMAX][HMAX];
    lb_matrix(sh, H, B);
    double l[HMAX], h[HMAX], x[HMAX], g[HMAX], d[HMAX], tb[HMAX], xc[HMAX];
    int fix[HMAX];
    for (int i = 0; i < H; ++i) {
        lb_bounds(sh, i, l[i], h[i]);
        x[i] = sh->u[i];
        g[i] = sh->trainable[i] ? sh->g[i] : 0.0;
        fix[i] = !sh->trainable[i] || l[i] == h[i];
        tb[i] = __builtin_inf();
        if (!fix[i]) {
            if (g[i] < 0.0 && h[i] < __builtin_inf()) tb[i] = (x[i] - h[i]) / g[i];
            else if (g[i] > 0.0 && l[i] > -__builtin_inf()) tb[i] = (x[i] - l[i]) / g[i];
        }
        if (fix[i] || tb[i] <= 0.0) { d[i] = 0.0; if (!fix[i] && g[i] != 0.0) fix[i] = 1; }
        else d[i] = -g[i];
        xc[i] = x[i];
    }
    // ---- generalised Cauchy point: piecewise search along the projected steepest-descent path
    auto quad = [&](double& f1, double& f2) {
        f1 = 0.0; f2 = 0.0;
        for (int i = 0; i < H; ++i) {
            double Bd = 0.0, Bz = 0.0;
            for (int j = 0; j < H; ++j) { Bd += B[i][j] * d[j]; Bz += B[i][j] * (xc[j] - x[j]); }
            f1 += d[i] * (g[i] + Bz);
            f2 += d[i] * Bd;
        }
    };
    double f1, f2;
    quad(f1, f2);
    const double f2_org = f2;
    double told = 0.0;
    for (;;) {
        bool moving = false;
        for (int i = 0; i < H; ++i) moving |= d[i] != 0.0;
        if (!moving) break;
        f2 = fmax(eps * f2_org, f2);
        const double dtm = -f1 / f2;
        int ib = -1;
        for (int i = 0; i < H; ++i)
            if (d[i] != 0.0 && tb[i] < __builtin_inf() && (ib < 0 || tb[i] < tb[ib])) ib = i;
        if (ib < 0 || dtm < tb[ib] - told) {
            const double tt = told + fmax(dtm, 0.0);
            for (int i = 0; i < H; ++i) if (d[i] != 0.0) xc[i] = x[i] + tt * d[i];
            break;
        }
        // the next breakpoint: variable ib reaches its bound and leaves the path
        told = tb[ib];
        for (int i = 0; i < H; ++i) if (d[i] != 0.0) xc[i] = x[i] + told * d[i];
        xc[ib] = d[ib] > 0.0 ? h[ib] : l[ib];
        d[ib] = 0.0;
        fix[ib] = 1;
        quad(f1, f2);
    }
    // ---- subspace minimisation over the variables that are free at the Cauchy point (direct primal method)
    int F[HMAX], nf = 0;
    for (int i = 0; i < H; ++i) if (!fix[i]) F[nf++] = i;
    double z[HMAX];
    for (int i = 0; i < H; ++i) z[i] = xc[i];
    if (nf > 0 && sh->hist_n > 0) {
        double A[HMAX][HMAX], r[HMAX];
        for (int a = 0; a < nf; ++a) {
            const int i = F[a];
            double Bz = 0.0;
            for (int j = 0; j < H; ++j) Bz += B[i][j] * (xc[j] - x[j]);
            r[a] = -(g[i] + Bz);
            for (int b = 0; b < nf; ++b) A[a][b] = B[i][F[b]];
        }
        bool ok = true;                            // Cholesky of the reduced matrix, then two triangular solves
        for (int a = 0; a < nf && ok; ++a) {
            for (int b = 0; b <= a; ++b) {
                double v = A[a][b];
                for (int k = 0; k < b; ++k) v -= A[a][k] * A[b][k];
                if (a == b) { if (!(v > 0.0)) { ok = false; break; } A[a][a] = sqrt(v); }
                else A[a][b] = v / A[b][b];
            }
        }
        if (ok) {
            for (int a = 0; a < nf; ++a) { double v = r[a]; for (int k = 0; k < a; ++k) v -= A[a][k] * r[k]; r[a] = v / A[a][a]; }
            for (int a = nf - 1; a >= 0; --a) { double v = r[a]; for (int k = a + 1; k < nf; ++k) v -= A[k][a] * r[k]; r[a] = v / A[a][a]; }
            // projection of the Newton point onto the box; if that is not a descent direction, the backtracking step
            double xp[HMAX], ddp = 0.0;
            for (int i = 0; i < H; ++i) xp[i] = xc[i];
            for (int a = 0; a < nf; ++a) { const int i = F[a]; xp[i] = fmin(h[i], fmax(l[i], xc[i] + r[a])); }
            for (int i = 0; i < H; ++i) ddp += (xp[i] - x[i]) * g[i];
            if (!(ddp > 0.0)) {
                for (int i = 0; i < H; ++i) z[i] = xp[i];
            } else {
                double alpha = 1.0; int ibd = -1;
                for (int a = 0; a < nf; ++a) {
                    const int i = F[a];
                    const double dk = r[a];
                    double t1 = alpha;
                    if (dk < 0.0 && l[i] > -__builtin_inf()) {
                        const double t2 = l[i] - xc[i];
                        if (t2 >= 0.0) t1 = 0.0; else if (dk * alpha < t2) t1 = t2 / dk;
                    } else if (dk > 0.0 && h[i] < __builtin_inf()) {
                        const double t2 = h[i] - xc[i];
                        if (t2 <= 0.0) t1 = 0.0; else if (dk * alpha > t2) t1 = t2 / dk;
                    }
                    if (t1 < alpha) { alpha = t1; ibd = a; }
                }
                for (int a = 0; a < nf; ++a) if (a != ibd || alpha >= 1.0) z[F[a]] = xc[F[a]] + alpha * r[a];
                if (alpha < 1.0 && ibd >= 0) z[F[ibd]] = r[ibd] > 0.0 ? h[F[ibd]] : l[F[ibd]];
            }
        }
    }
    // ---- search direction and the largest feasible step (lnsrlb)
    double dn = 0.0, gd = 0.0;
    bool boxed = true;
    for (int i = 0; i < H; ++i) {
        sh->d[i] = z[i] - x[i];
        dn += sh->d[i] * sh->d[i];
        gd += g[i] * sh->d[i];
        if (sh->trainable[i]) boxed = boxed && l[i] > -__builtin_inf() && h[i] < __builtin_inf();
    }
    sh->dphi0 = gd;
    if (!(gd < 0.0)) return 0.0;
    const double stpmx = lb_stpmax(sh, H);
    sh->t = (sh->iter == 0 && !boxed) ? fmin(1.0 / sqrt(dn), stpmx) : 1.0;
    return stpmx;
}

// trial point u + t d, kept inside the box (the step 1 lands on the subspace point, bounds exactly)
static __device__ __noinline__ void lb_set_trial(Shared* sh, int H) {
    double un[HMAX];
    for (int i = 0; i < H; ++i) {
        double l, h; lb_bounds(sh, i, l, h);
        un[i] = sh->trainable[i] ? fmin(h, fmax(l, sh->u[i] + sh->t * sh->d[i])) : sh->u[i];
    }
    set_trial(sh, H, un);
}

// the accepted point is sh->u; decide whether the factorisation in memory already belongs to it
// multi-start (o.ms_S > 0): one start's run has ended at sh->u with value sh->f.  Keep it if strictly below the best so
// far (the first start wins a tie, as sklearn's argmin), then load the next start with an empty history, or after the
// last one run the final evaluation at the best point (sklearn refits at its best theta).
static __device__ __noinline__ void ms_end_start(Shared* sh, int H, const OptCfg& o, bool factor_is_current) {
    const int t = sh->tile & 0x7fffffff;
    double* st = o.ms_state + (size_t)t * MS_WORDS;
    const int k = (int)ms_ld(st);
    const double f = sh->f;
    if (o.ms_fout) ms_st(o.ms_fout + (size_t)t * o.ms_S + k, f);
    if (f < ms_ld(st + 1)) {
        ms_st(st + 1, f); ms_st(st + 2, (double)sh->iter); ms_st(st + 3, (double)sh->status); ms_st(st + 4, (double)k);
        for (int i = 0; i < H; ++i) ms_st(st + 5 + i, sh->u[i]);
    }
    ms_st(st, (double)(k + 1));
    if (k + 1 < o.ms_S) {
        const double* th = o.ms_starts + ((size_t)t * (o.ms_S - 1) + k) * H;
        for (int i = 0; i < H; ++i)
            if (sh->trainable[i]) { sh->theta[i] = th[i]; sh->u[i] = log(th[i]); }
        sh->iter = 0; sh->hist_n = 0; sh->hist_pos = 0; sh->last_dec = 1e300; sh->fail = 0; sh->status = 1;
        sh->want_grad = 1;
        sh->phase = PH_INIT;
        return;
    }
    const int best = (int)ms_ld(st + 4);
    sh->iter = (int)ms_ld(st + 2);
    sh->status = best < 0 ? 2 : (int)ms_ld(st + 3);        // every start failed at its first evaluation: NOT_PD
    sh->f = ms_ld(st + 1);
    if (best == k && factor_is_current && !sh->fail) { sh->n_eval_opt = sh->n_eval; sh->phase = PH_EXIT; return; }
    for (int i = 0; i < H; ++i) sh->u[i] = ms_ld(st + 5 + i);
    set_trial(sh, H, sh->u);
    sh->want_grad = o.want_grad_out;
    sh->n_eval_opt = sh->n_eval + 1;              // n_eval counts every start and the final evaluation
    sh->phase = PH_FINAL;
}

static __device__ __noinline__ void opt_finish(Shared* sh, int H, const OptCfg& o, bool factor_is_current) {
    if (o.ms_S > 0) { ms_end_start(sh, H, o, factor_is_current); return; }
    sh->n_eval_opt = sh->n_eval;
    if (factor_is_current && !sh->fail && !o.factor_stale) { sh->phase = PH_EXIT; return; }
    set_trial(sh, H, sh->u);
    sh->want_grad = o.want_grad_out;
    sh->phase = PH_FINAL;
}

static __device__ __noinline__ void opt_start_iteration(Shared* sh, int H, const OptCfg& o) {
    if (o.optimiser == 2) {
        const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
        const int k = sh->iter + 1;
        double un[HMAX];
        for (int i = 0; i < H; ++i) {
            sh->m1[i] = b1 * sh->m1[i] + (1 - b1) * sh->g[i];
            sh->m2[i] = b2 * sh->m2[i] + (1 - b2) * sh->g[i] * sh->g[i];
            const double mh = sh->m1[i] / (1 - pow(b1, (double)k)), vh = sh->m2[i] / (1 - pow(b2, (double)k));
            un[i] = sh->u[i] - (sh->trainable[i] ? o.adam_lr * mh / (sqrt(vh) + eps) : 0.0);
        }
        set_trial(sh, H, un);
        sh->phase = PH_ADAM;
        return;
    }
    if (o.ms_S > 0) {
        // no descent direction inside the box (lnsrlb info = -4) is handled as a failed line search: refresh the memory
        // once, with an empty history give up
        bool descent = lb_direction(sh, H) > 0.0;
        if (!descent && sh->hist_n > 0) { sh->hist_n = 0; descent = lb_direction(sh, H) > 0.0; }
        if (!descent) {
            sh->status = ST_LS_FAILED;
            opt_finish(sh, H, o, true);
            return;
        }
        sh->ls_phase = 0; sh->ls_iter = 0; sh->ls_done = 0;
        sh->t_prev = 0.0; sh->f_prev = sh->f; sh->dphi_prev = sh->dphi0;
        sh->t_best = 0.0; sh->f_best = sh->f;
        lb_set_trial(sh, H);
        sh->phase = PH_LS;
        return;
    }
    lbfgs_direction(sh, H);
    double dphi0 = 0.0, gn = 0.0;
    for (int i = 0; i < H; ++i) { dphi0 += sh->g[i] * sh->d[i]; gn += sh->g[i] * sh->g[i]; }
    if (!(dphi0 < 0.0)) {      // not a descent direction: restart from steepest descent
        sh->hist_n = 0;
        for (int i = 0; i < H; ++i) sh->d[i] = -sh->g[i];
        dphi0 = -gn;
    }
    if (gn == 0.0) { sh->status = 0; opt_finish(sh, H, o, true); return; }
    sh->dphi0 = dphi0;
    sh->t = (sh->hist_n == 0) ? fmin(1.0, 1.0 / sqrt(gn)) : 1.0;
    sh->ls_phase = 0; sh->ls_iter = 0; sh->ls_done = 0;
    sh->t_prev = 0.0; sh->f_prev = sh->f; sh->dphi_prev = dphi0;
    sh->t_best = 0.0; sh->f_best = sh->f;
    double un[HMAX];
    for (int i = 0; i < H; ++i) un[i] = sh->u[i] + sh->t * sh->d[i];
    set_trial(sh, H, un);
    sh->phase = PH_LS;
}

static __device__ __noinline__ void opt_advance(Shared* sh, int H, const OptCfg& o) {
    switch (sh->phase) {
        case PH_INIT: {
            if (o.ms_S > 0) {
                // log transform at the evaluated point (the host clipped it into the bounds, as SciPy clips x0)
                for (int i = 0; i < H; ++i) { sh->box[i] = 2; sh->u[i] = log(sh->theta[i]); sh->ut[i] = sh->u[i]; }
                fetch_trial(sh, H);
                sh->f = sh->ft;
                for (int i = 0; i < H; ++i) sh->g[i] = sh->gt[i];
                // a start whose first evaluation fails has f = +inf (sklearn's LML is -inf on LinAlgError): skipped
                if (sh->fail) { sh->f = __builtin_inf(); sh->status = 2; ms_end_start(sh, H, o, false); return; }
                sh->status = 1;
                if (o.gtol > 0.0 && lb_projgr(sh, H) <= o.gtol) { sh->status = 0; opt_finish(sh, H, o, true); return; }
                opt_start_iteration(sh, H, o);
                return;
            }
            set_trial(sh, H, sh->u);
            fetch_trial(sh, H);
            sh->f = sh->ft;
            for (int i = 0; i < H; ++i) sh->g[i] = sh->gt[i];
            if (sh->fail) { sh->status = 2; sh->n_eval_opt = sh->n_eval; sh->phase = PH_EXIT; return; }
            sh->status = 1;
            if (o.optimiser == 1 && o.gtol > 0.0) {
                // L-BFGS-B tests the gradient norm before the first iteration too
                double gmax0 = 0.0;
                for (int i = 0; i < H; ++i) gmax0 = fmax(gmax0, fabs(sh->g[i]));
                if (gmax0 <= o.gtol) { sh->status = 0; opt_finish(sh, H, o, true); return; }
            }
            opt_start_iteration(sh, H, o);
            return;
        }
        case PH_ADAM: {
            fetch_trial(sh, H);
            if (sh->fail) { sh->status = 2; opt_finish(sh, H, o, false); return; }
            sh->f = sh->ft;
            for (int i = 0; i < H; ++i) { sh->u[i] = sh->ut[i]; sh->g[i] = sh->gt[i]; }
            sh->iter += 1;
            if (sh->iter >= o.max_iter) { sh->status = 1; opt_finish(sh, H, o, true); return; }
            opt_start_iteration(sh, H, o);
            return;
        }
        case PH_LS: {
            fetch_trial(sh, H);
            ls_step(sh, H, o.max_ls, o.ms_S > 0 ? lb_stpmax(sh, H) : 1e300);
            if (!sh->ls_done && o.ms_S > 0) { lb_set_trial(sh, H); return; }
            if (!sh->ls_done) {
                double un[HMAX];
                for (int i = 0; i < H; ++i) un[i] = sh->u[i] + sh->t * sh->d[i];
                set_trial(sh, H, un);
                return;
            }
            if (sh->ls_done == 1 || sh->ls_done == 3) {
                // accept the trial point (ls_done 1: the last evaluated one; 3: an earlier one, restored into ut / gt / ft)
                const bool current = sh->ls_done == 1;
                double sy = 0.0, yy = 0.0, gmax = 0.0;
                double sv[HMAX], yvv[HMAX];
                for (int i = 0; i < H; ++i) {
                    sv[i] = sh->ut[i] - sh->u[i];
                    yvv[i] = sh->gt[i] - sh->g[i];
                    sy += sv[i] * yvv[i];
                    yy += yvv[i] * yvv[i];
                }
                // L-BFGS-B (mainlb) skips the update when s'y <= eps (-g's); the unbounded driver when s'y <= 1e-10 y'y
                double gs = 0.0;
                for (int i = 0; i < H; ++i) gs -= sh->g[i] * sv[i];
                const bool keep = o.ms_S > 0 ? (sy > 2.220446049250313e-16 * gs && yy > 0.0) : (sy > 1e-10 * yy && yy > 0.0);
                if (keep) {
                    const int pos = sh->hist_pos;
                    for (int i = 0; i < H; ++i) { sh->S[pos][i] = sv[i]; sh->Y[pos][i] = yvv[i]; }
                    sh->rho_[pos] = 1.0 / sy;
                    sh->hist_pos = (pos + 1) % MH;
                    if (sh->hist_n < MH) sh->hist_n += 1;
                }
                const double fold = sh->f, fnew = sh->ft;
                sh->f = fnew;
                sh->last_dec = fold - fnew;
                for (int i = 0; i < H; ++i) { sh->u[i] = sh->ut[i]; sh->g[i] = sh->gt[i]; gmax = fmax(gmax, fabs(sh->gt[i])); }
                sh->iter += 1;
                const double den = fmax(fmax(fabs(fold), fabs(fnew)), 1.0);
                if (o.ms_S > 0) gmax = lb_projgr(sh, H);          // L-BFGS-B: the projected gradient
                if ((fold - fnew) <= o.ftol * den || gmax <= o.gtol) { sh->status = 0; opt_finish(sh, H, o, current); return; }
                if (sh->iter >= o.max_iter) { sh->status = 1; opt_finish(sh, H, o, current); return; }
                opt_start_iteration(sh, H, o);
                return;
            }
            // Line search failed (no step satisfying the strong Wolfe conditions within max_ls evaluations).
            //  * The last accepted step's decrease was already at the resolution of the arithmetic (noise_rel * |f|: fp32
            //    1e-3 -- the objective carries rounding ~ cond(K) eps N --, fp64 1e-12): a further decrease cannot be told
            //    from noise.  That is the finite-precision form of the ftol test: converged.  (Not with ftol switched off.)
            //  * Otherwise as L-BFGS-B (mainlb, info != 0): with a non-empty history, discard it and restart once from
            //    steepest descent at the accepted point (the restart is not an iteration); with an empty history give up
            //    -- SciPy reports ABNORMAL_TERMINATION_IN_LNSRCH, success=False, hence a status of its own.  The best
            //    sufficient-decrease point seen by the failed search (if any) is kept rather than thrown away.
            //  * Bounded L-BFGS-B (o.ms_S > 0) keeps SciPy's semantics only: no noise-floor convergence.
            if (o.ms_S == 0 && sh->iter > 0 && o.ftol >= 0.0 && sh->last_dec <= o.noise_rel * fmax(fabs(sh->f), 1.0)) {
                sh->status = ST_CONVERGED;
                opt_finish(sh, H, o, false);
                return;
            }
            if (sh->hist_n > 0) {
                sh->hist_n = 0;
                opt_start_iteration(sh, H, o);
                return;
            }
            sh->status = ST_LS_FAILED;
            if (sh->t_best > 0.0 && sh->f_best < sh->f) {
                sh->last_dec = sh->f - sh->f_best;
                sh->f = sh->f_best;
                for (int i = 0; i < H; ++i) { sh->u[i] = sh->ub[i]; sh->g[i] = sh->gb[i]; }
            }
            opt_finish(sh, H, o, false);
            return;
        }
        default:  // PH_FINAL
            sh->phase = PH_EXIT;
            return;
    }
}

// ---------------------------------------------------------------------------------------------
// per-tile driver pieces of the persistent kernels: what every kernel does around its evaluate / opt_advance loop.  `Args` is
// KernelArgs or SgprArgs (the same field names for everything read here); H = D + 2 as for opt_advance.
// ---------------------------------------------------------------------------------------------
// the multi-start fields exist in KernelArgs only: those kernels copy them at the call site
template <class Args>
static __device__ __forceinline__ OptCfg opt_cfg(const Args& A) {
    OptCfg o;
    o.optimiser = A.optimiser; o.max_iter = A.max_iter; o.max_ls = A.max_ls; o.want_grad_out = A.grad != nullptr;
    o.ftol = A.ftol; o.gtol = A.gtol; o.adam_lr = A.adam_lr; o.noise_rel = A.noise_rel;
    return o;
}

// thread 0: outputs of a tile without observations (its predictions are the prior: tile_predict_prior)
template <class Args>
static __device__ __forceinline__ void tile_out_empty(const Args& A, int H, int t) {
    A.status[t] = 4; A.n_eval[t] = 0; A.nll[t] = 0.0;
    if (A.n_iter) A.n_iter[t] = 0;
    for (int i = 0; i < H; ++i) {
        A.theta[(size_t)t * H + i] = A.theta0[(size_t)t * H + i];
        if (A.grad) A.grad[(size_t)t * H + i] = 0.0;
    }
}

// thread 0: optimiser state of a tile that starts (a resumed one loads its state: state_load)
template <class Args>
static __device__ __forceinline__ void opt_fresh_tile(Shared* sh, const Args& A, int H, int t, const OptCfg& o) {
    sh->n_eval = 0; sh->n_eval_opt = 0; sh->status = 5; sh->iter = 0; sh->hist_n = 0; sh->hist_pos = 0;
    sh->last_dec = 1e300;
    sh->fail = 0;
    for (int i = 0; i < H; ++i) {
        const double lo = A.lo[(size_t)t * H + i], hi = A.hi[(size_t)t * H + i];
        const bool box = (lo == lo) && (hi == hi) && (fabs(lo) < 1e300) && (fabs(hi) < 1e300);
        sh->box[i] = box ? 1 : 0;
        sh->lo[i] = lo; sh->hi[i] = hi;
        sh->shift[i] = (!box && i == H - 1) ? 1e-6 : 0.0;   // GPflow likelihood-variance lower bound
        sh->trainable[i] = A.trainable[i] ? 1 : 0;
        sh->theta[i] = A.theta0[(size_t)t * H + i];
        sh->u[i] = u_of_theta(sh, i, sh->theta[i]);
        sh->m1[i] = 0.0; sh->m2[i] = 0.0;
    }
    const bool optim = (o.optimiser != 0 && o.max_iter > 0);
    sh->phase = optim ? PH_INIT : PH_FINAL;
    sh->want_grad = optim ? 1 : o.want_grad_out;
}

// thread 0: outputs of a tile whose optimiser has reached PH_EXIT; a failed last evaluation gives status 2 (not positive
// definite) or 3 (NaN objective) and NaN objective / gradient
template <class Args>
static __device__ __forceinline__ void tile_out_finished(const Args& A, const Shared* sh, int H, int t) {
    int st = sh->status;
    if (sh->fail) st = (sh->nll == sh->nll) ? 2 : 3;
    A.status[t] = st;
    A.n_eval[t] = sh->n_eval_opt;
    if (A.n_iter) A.n_iter[t] = sh->iter;
    A.nll[t] = sh->fail ? __builtin_nan("") : sh->nll;
    for (int i = 0; i < H; ++i) {
        A.theta[(size_t)t * H + i] = sh->theta[i];
        if (A.grad) A.grad[(size_t)t * H + i] = sh->fail ? __builtin_nan("") : sh->gth[i];
    }
}

// all threads: predictions [p0, p1) of a tile without observations are the prior at theta0 (T: the kernel's output scalar).
// The prior covariance K_** needs the covariance function: it stays with the kernels.
template <class T, class Args>
static __device__ __forceinline__ void tile_predict_prior(const Args& A, int H, int t, int tid, long long p0, long long p1,
                                                          T* f_mean, T* f_var, T* y_var) {
    for (long long q = p0 + tid; q < p1; q += NT) {
        const T sf2 = (T)A.theta0[(size_t)t * H + H - 2], sn2 = (T)A.theta0[(size_t)t * H + H - 1];
        f_mean[q] = (T)0; f_var[q] = sf2; y_var[q] = sf2 + sn2;
    }
}

// all threads: NaN predictions [p0, p1) of a tile whose last evaluation failed; kernels with a full covariance output pass
// it (or nullptr) and the tiles' offsets into it, and tile t's elements become NaN too
template <class T>
static __device__ __forceinline__ void tile_predict_nan(int tid, long long p0, long long p1, T* f_mean, T* f_var, T* y_var,
                                                        T* f_cov = nullptr, const long long* cov_off = nullptr, int t = 0) {
    const T qnan = (T)__builtin_nan("");
    for (long long q = p0 + tid; q < p1; q += NT) { f_mean[q] = qnan; f_var[q] = qnan; y_var[q] = qnan; }
    if (f_cov)
        for (long long q = cov_off[t] + tid; q < cov_off[t + 1]; q += NT) f_cov[q] = qnan;
}

// Time slicing (KernelArgs::seg_cost > 0): a suspended tile's optimiser state, the first A.state_words words of Shared, waits
// in A.state until any workgroup pops the tile's ring entry again.
//
// The state was written by another workgroup, possibly on another XCD (whose L2 is not coherent with this one).
// It travels through agent-scope atomic word accesses, which go to memory past the caches: no cache-wide
// write-back / invalidate (an agent-scope fence costs every workgroup of the XCD its L2 contents).  Every wave of
// the writer had drained its stores (s_waitcnt vmcnt(0)) and met the workgroup barrier before one lane published
// the ring entry that this workgroup's thread 0 has polled (sc1 load) ahead of the barrier behind the pop; every load of
// the state is an sc1 load to registers (MI355X_MICROARCH.md, inter-workgroup visibility: valid forms).
static __device__ __forceinline__ void state_load(Shared* sh, const KernelArgs& A, int t, int tid) {
    const unsigned* src = A.state + (size_t)t * A.state_words;
    unsigned* dst = reinterpret_cast<unsigned*>(sh);
    for (int i = tid; i < A.state_words; i += NT)
        dst[i] = __hip_atomic_load(&src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// all threads; behind it ONE lane publishes the ring entry (ring_push, at the call site)
static __device__ __forceinline__ void state_save(const Shared* sh, const KernelArgs& A, int t, int tid) {
    unsigned* dst = A.state + (size_t)t * A.state_words;
    const unsigned* src = reinterpret_cast<const unsigned*>(sh);
    for (int i = tid; i < A.state_words; i += NT)
        __hip_atomic_store(&dst[i], src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // EVERY storing wave drains its own stores (a workgroup-scope fence emits no vmcnt wait on gfx950; inline asm
    // so that no compiler pass can drop or move it), THEN the barrier, THEN the publish
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}


#endif  // GPSAT_OPT_H
