/*
 * gpsat_hip.h -- C ABI of the MI355X-native local-expert exact-GP engine (libgpsat_hip.so).
 *
 * Drop-in boundary.  The reference (CPOMUCL/GPSat, pure Python) has no FFI; the backend it
 * calls per expert tile is a Python class satisfying BaseGPRModel
 * (GPSat/models/base_model.py:17-82) selected through model_config["oi_model"]
 * (GPSat/models/__init__.py:3-28, GPSat/local_experts.py:292-346).  Each entry point below
 * states which reference interface it replaces; the Python binding a maintainer would add
 * on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, no torch / HIP types in signatures; all pointers are caller-owned;
 *  - every function returns 0 on success or a negative GPSAT_E* code and never throws;
 *    gpsat_last_error() returns a thread-local message for the last failure;
 *  - one handle per GPU; calls on one handle must be serialised by the caller, distinct
 *    handles may be driven from distinct threads / processes;
 *  - calls are host-synchronous on return.
 *
 * Parameter vector order (H = D + 2):
 *     theta = (lengthscale_0 .. lengthscale_{D-1}, kernel_variance, likelihood_variance)
 * i.e. the reference's param_names ["lengthscales","kernel_variance","likelihood_variance"]
 * (GPSat/models/gpflow_models.py:179-184) flattened.
 * GPSAT_KERNEL_RQ has one more, its shape parameter alpha, behind them (H = D + 3, no other index moves):
 *     theta = (lengthscale_0 .. lengthscale_{D-1}, kernel_variance, likelihood_variance, alpha)
 * H of any kernel is gpsat_n_hyper(kernel, D).
 */
#ifndef GPSAT_HIP_H
#define GPSAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPSAT_ABI_VERSION 4

/* error codes */
#define GPSAT_OK            0
#define GPSAT_EINVAL       -1   /* bad argument / unsupported configuration */
#define GPSAT_ENODEV       -2   /* no usable HIP device                      */
#define GPSAT_ENOMEM       -3   /* device allocation failed                   */
#define GPSAT_EHIP         -4   /* HIP runtime error (see gpsat_last_error)   */

/* compute dtype of the bulk arrays (X, y, Xs, f_mean, f_var, y_var) */
#define GPSAT_F32 0
#define GPSAT_F64 1

/* kernels: gpflow.kernels names accepted by GPflowGPRModel (gpflow_models.py:72-75,116-135) */
#define GPSAT_KERNEL_RBF      0   /* "RBF" / "SquaredExponential" */
#define GPSAT_KERNEL_MATERN12 1   /* "Matern12" / "Exponential"   */
#define GPSAT_KERNEL_MATERN32 2   /* "Matern32" (reference default, gpflow_models.py:44) */
#define GPSAT_KERNEL_MATERN52 3   /* "Matern52" */
#define GPSAT_KERNEL_RQ       4   /* "RationalQuadratic": k = s (1 + r^2 / (2 alpha))^-alpha, r^2 = sum_d ((x_d - x'_d) / l_d)^2,  */
                                  /*   as GPflow's and scikit-learn's; H = D + 3 with alpha last.  Built into                     */
                                  /*   gpsat_fit_predict_batch (f_cov included) for GPSAT_F64 and D <= 3, one workgroup per tile; */
                                  /*   GPSAT_F32, D = 4 and every other entry point return GPSAT_EINVAL with a message.  alpha's  */
                                  /*   transform follows lo / hi like every parameter's: NaN bounds = softplus without a shift    */
                                  /*   (GPflow's positive()), finite bounds = the sigmoid box.  Callers detect the kernel by the  */
                                  /*   presence of gpsat_n_hyper; GPSAT_ABI_VERSION stays 4.                                      */

/* optimisers */
#define GPSAT_OPT_NONE  0   /* optimise=False in LocalExpertOI.run (local_experts.py:1126-1132) */
#define GPSAT_OPT_LBFGS 1   /* replaces gpflow.optimizers.Scipy / L-BFGS-B (gpflow_models.py:317-321) */
#define GPSAT_OPT_ADAM  2   /* fixed-step alternative named by BASELINE.json north_star */

/* where the bulk arrays live */
#define GPSAT_MEM_HOST   0
#define GPSAT_MEM_DEVICE 1

/* per-tile status */
#define GPSAT_STATUS_CONVERGED 0   /* optimiser met ftol / gtol (scipy success=True); also: a line */
                                   /*   search failed after a step whose decrease was already at   */
                                   /*   the resolution of the arithmetic (1e-3 |f| in fp32, 1e-12   */
                                   /*   |f| in fp64) -- not with ftol switched off                  */
#define GPSAT_STATUS_MAXITER   1   /* iteration limit reached (scipy success=False)           */
#define GPSAT_STATUS_NOT_PD    2   /* Cholesky failed at the initial / final parameters        */
#define GPSAT_STATUS_NAN       3   /* NaN encountered                                          */
#define GPSAT_STATUS_SKIPPED   4   /* tile had no observations                                 */
#define GPSAT_STATUS_NOT_OPTIMISED 5 /* optimiser == NONE: objective + predict only            */
#define GPSAT_STATUS_LS_FAILED 6   /* line search failed with an empty L-BFGS history (scipy     */
                                   /*   ABNORMAL_TERMINATION_IN_LNSRCH, success=False); theta is */
                                   /*   the best sufficient-decrease point seen                   */

typedef struct gpsat_handle gpsat_handle;

/* Hyper-parameters per tile, the H of every [T*H] and [H] array of gpsat_batch: D + 3 for GPSAT_KERNEL_RQ (D = 1..3),
 * D + 2 for the other kernels (D = 1..4); 0 for unsupported arguments. */
int gpsat_n_hyper(int kernel, int D);

typedef struct gpsat_opts {
    int32_t workgroups_per_cu;   /* persistent workgroups per CU (0 = default 2)            */
    int32_t reserved[7];
} gpsat_opts;

/*
 * One packed ragged batch of T independent expert tiles.
 *
 * Replaces, for all T tiles at once, the per-tile sequence of LocalExpertOI.run
 * (GPSat/local_experts.py:1043-1159):
 *   model = Model(data=df_local, ...)            -> X, y (already scaled / de-meaned by the host
 *                                                   exactly as base_model.py:243-245, in fp64,
 *                                                   then cast to `dtype`)
 *   model.set_parameters / load_params            -> theta0
 *   model.set_parameter_constraints(...)          -> lo, hi (already divided by coords_scale and
 *                                                   with theta0 moved within tol on the host,
 *                                                   gpflow_models.py:459-479)
 *   model.optimise_parameters(**optim_kwargs)     -> optimiser, max_iter, trainable
 *   model.get_objective_function_value()          -> nll
 *   model.get_parameters()                        -> theta
 *   model.predict(coords=prediction_coords)       -> f_mean ("f*"), f_var ("f*_var"), y_var
 */
typedef struct gpsat_batch {
    /* ---- shape ---- */
    int32_t T;                 /* number of tiles                                           */
    int32_t D;                 /* input dimension (1..4 in this build)                      */
    int32_t dtype;             /* GPSAT_F32 (fp32 MFMA kernels) | GPSAT_F64 (fp64 MFMA kernels) */
    int32_t kernel;            /* GPSAT_KERNEL_*                                            */
    int32_t memory;            /* GPSAT_MEM_HOST / GPSAT_MEM_DEVICE for the bulk arrays      */
    int32_t optimiser;         /* GPSAT_OPT_*                                               */
    int32_t max_iter;          /* optimiser iteration limit (scipy options.maxiter)         */
    int32_t max_ls;            /* max line-search evaluations per iteration (0 = 20, scipy maxls) */
    double  ftol;              /* relative objective decrease tolerance (0 = default: fp64   */
                               /*   2.2e-9 = SciPy's factr*eps, fp32 1e-6 = its fp32 analogue; */
                               /*   negative = never stop on this criterion)                  */
    double  gtol;              /* max-norm gradient tolerance in u-space (0 = default 1e-5,  */
                               /*   scipy pgtol; negative = never stop on this criterion)     */
    double  adam_lr;           /* Adam learning rate (0 = default 0.1)                      */

    /* ---- metadata: ALWAYS host memory ---- */
    const int64_t *obs_off;    /* [T+1] CSR offsets into X / y        (rows)                */
    const int64_t *pred_off;   /* [T+1] CSR offsets into Xs / outputs (rows)                */
    const double  *theta0;     /* [T*H] initial parameters, constrained space                */
    const double  *lo;         /* [T*H] lower bounds; NaN/inf => unconstrained (softplus)    */
    const double  *hi;         /* [T*H] upper bounds                                          */
    const uint8_t *trainable;  /* [H]   0 => parameter fixed (optim_kwargs.fixed_params)      */

    /* ---- bulk inputs: host or device according to `memory`, element type `dtype` ---- */
    const void *X;             /* [sum N, D] row-major, scaled coordinates                   */
    const void *y;             /* [sum N]    de-meaned / scaled observations                 */
    const void *Xs;            /* [sum P, D] row-major, scaled prediction coordinates        */

    /* ---- outputs ---- */
    double  *theta;            /* [T*H] host: learned parameters                             */
    double  *nll;              /* [T]   host: objective (negative log marginal likelihood)   */
    double  *grad;             /* [T*H] host, optional (may be NULL): dNLL/dtheta at `theta` */
    int32_t *status;           /* [T]   host: GPSAT_STATUS_*                                 */
    int32_t *n_eval;           /* [T]   host: objective+gradient evaluations performed       */
    void    *f_mean;           /* [sum P] host|device (as `memory`): "f*"                    */
    void    *f_var;            /* [sum P] "f*_var"                                           */
    void    *y_var;            /* [sum P] "y_var"                                            */

    /* ---- optional full posterior covariance (predict(full_cov=True), gpflow_models.py:245-263); ABI >= 2 ---- */
    const int64_t *cov_off;    /* [T+1] host: element offsets into f_cov, cov_off[t+1]-cov_off[t] = P_t^2; NULL = off */
    void    *f_cov;            /* [sum P_t^2] host|device (as `memory`), element type `dtype`: per tile the      */
                               /*   row-major P_t x P_t matrix "f*_cov" = K** - K*^T K^-1 K*; NULL = not wanted   */

    /* ---- ABI >= 3 ---- */
    int32_t *n_iter;           /* [T] host, optional (may be NULL): optimiser iterations completed (scipy nit)  */
} gpsat_batch;

/*
 * Multi-start bounded L-BFGS-B in log space (sklearn's GaussianProcessRegressor.fit with n_restarts_optimizer,
 * GPSat/models/sklearn_models.py): the extension of gpsat_fit_predict_batch_ms.  Callers detect it by the presence of
 * that symbol; gpsat_batch keeps its layout and GPSAT_ABI_VERSION stays 4.
 *
 * Every trainable parameter is optimised over u = log(theta) with SciPy's L-BFGS-B and its box constraints
 * [log lo, log hi] (generalised Cauchy point, subspace minimisation, feasible line search), from theta0 -- clipped into
 * the bounds, as SciPy clips x0 -- and from the S - 1 further starts, in that order.  A start whose first evaluation is
 * not positive definite has the objective +inf and is skipped.  The start with the lowest final objective wins (the
 * first one on a tie); the tile's factorisation, nll, grad and predictions are those at its parameters.
 * Outputs: n_eval counts the evaluations of every start plus the final one; n_iter and status are the winning start's;
 * status is GPSAT_STATUS_NOT_PD only when the factorisation at the winning parameters fails (or every start failed).
 * With optimiser GPSAT_OPT_NONE the batch is evaluated at theta0 as by gpsat_fit_predict_batch and f_start is not
 * written.  GPSAT_OPT_ADAM is refused.
 */
#define GPSAT_TRANSFORM_LOG 1
typedef struct gpsat_multistart {
    int32_t       n_starts;   /* S >= 1: theta0 and S - 1 further starts per tile                                  */
    int32_t       transform;  /* GPSAT_TRANSFORM_LOG                                                                */
    const double *starts;     /* [T*(S-1)*H] host, constrained space, clipped into the bounds like theta0; may be   */
                              /*   NULL if S = 1                                                                    */
    double       *f_start;    /* [T*S] host, optional (may be NULL): final objective (-LML) of every start, +inf when */
                              /*   its first evaluation failed, NaN for a tile without observations                 */
    int32_t       reserved[8];
} gpsat_multistart;

/* as gpsat_fit_predict_batch, with the multi-start extension above.  GPSAT_EINVAL (with a message) for S < 1, an
 * unknown transform, NULL starts with S > 1, a bound <= 0 (or NaN) on a trainable parameter, and non-finite bounds
 * with S > 1 (sklearn: "requires that all bounds are finite"). */
int gpsat_fit_predict_batch_ms(gpsat_handle *h, const gpsat_batch *b, const gpsat_multistart *ms);

/*
 * A trainable constant mean (GPflow's gpflow.mean_functions.Constant, the reference's mean_function="Constant",
 * GPSat/models/gpflow_models.py:143-157): the extension of gpsat_fit_predict_batch_mean.  Callers detect it by the presence
 * of that symbol; gpsat_batch keeps its layout and GPSAT_ABI_VERSION stays 4.
 *
 *     y ~ N(c 1, K_theta + sn2 I),   nll(theta, c; y) = nll_zero-mean(theta; y - c 1),   dnll/dc = -sum(K_y^-1 (y - c 1)),
 *     f*(x) = c + k*(x)^T K_y^-1 (y - c 1);  f_var, y_var and f_cov are those of the zero-mean model.
 *
 * GPSAT_MEAN_CONSTANT: one more parameter per tile, behind the others (H = D + 3 = gpsat_n_hyper_mean, no other index moves):
 *     theta = (lengthscale_0 .. lengthscale_{D-1}, kernel_variance, likelihood_variance, c)
 * in theta0, lo, hi, trainable, theta and grad.  c is unconstrained -- any finite value, zero and negatives included --
 * when its bounds are NaN (the identity transform, GPflow's plain Parameter), and boxed like every parameter when lo / hi
 * are finite.  A tile without observations predicts the prior: f_mean = c of theta0.  Built for GPSAT_F64, the kernels
 * GPSAT_KERNEL_RBF .. GPSAT_KERNEL_MATERN52 and D <= 3, one workgroup per tile, with both optimisers and f_cov.
 * GPSAT_MEAN_ZERO is gpsat_fit_predict_batch itself and returns the same bits.
 */
#define GPSAT_MEAN_ZERO     0
#define GPSAT_MEAN_CONSTANT 1
typedef struct gpsat_mean {
    int32_t kind;              /* GPSAT_MEAN_*                                                */
    int32_t reserved[7];       /* must be 0                                                   */
} gpsat_mean;                  /* 32 bytes */

/* Hyper-parameters per tile with a mean: D + 3 for GPSAT_MEAN_CONSTANT with a stationary kernel (not GPSAT_KERNEL_RQ) and
 * D <= 3; gpsat_n_hyper(kernel, D) for GPSAT_MEAN_ZERO; 0 for everything else. */
int gpsat_n_hyper_mean(int kernel, int D, int mean_kind);

/* as gpsat_fit_predict_batch, with the mean above.  GPSAT_EINVAL (with a message that names the reason; the handle stays
 * usable) for GPSAT_MEAN_CONSTANT with GPSAT_F32, D = 4 or GPSAT_KERNEL_RQ, for an unknown kind, non-zero reserved words
 * and a non-finite theta0 of c. */
int gpsat_fit_predict_batch_mean(gpsat_handle *h, const gpsat_batch *b, const gpsat_mean *m);

/*
 * Known noise variances per observation (a Gaussian likelihood whose variance is a fixed function of the row; optimal
 * interpolation's observation-error variance): the extension of gpsat_fit_predict_batch_noise.  Callers detect it by the
 * presence of that symbol; gpsat_batch keeps its layout and GPSAT_ABI_VERSION stays 4.
 *
 *     y ~ N(0, K_theta + sn2 I + diag(v)),   v_i >= 0 finite, given per row of y and not trained.
 *
 * theta, H = D + 2, the transforms, the lower bound of likelihood_variance, the optimisers and the status codes are those of
 * gpsat_fit_predict_batch; likelihood_variance is the variance that v does not explain (fix it through `trainable` to trust
 * v alone).  Objective and gradient are the plain formulas with K_y as above (dK_y/dtheta does not involve v).  Predictions:
 * f* = k*^T K_y^-1 y, f_var = k** - k*^T K_y^-1 k*, y_var = f_var + sn2 (a new point carries the homogeneous part only);
 * f_cov uses the same K_y; a tile without observations predicts the prior.  Built for GPSAT_F64, the kernels
 * GPSAT_KERNEL_RBF .. GPSAT_KERNEL_MATERN52 and D <= 4, one workgroup per tile, with both optimisers and f_cov.
 * v == 0 everywhere, and obs_var == NULL, return the bits of gpsat_fit_predict_batch in every output.
 */
typedef struct gpsat_noise {
    const void *obs_var;       /* [sum N] doubles, host|device as b->memory; NULL = the plain call */
    int32_t reserved[8];       /* must be 0                                                   */
} gpsat_noise;                 /* 40 bytes */

/* as gpsat_fit_predict_batch, with the noise variances above.  GPSAT_EINVAL (with a message that names the reason; the
 * handle stays usable) for GPSAT_F32, GPSAT_KERNEL_RQ, a NULL nz, non-zero reserved words and, in host mode, a negative or
 * non-finite entry of obs_var (the message names the tile and the row).  Device mode: obs_var is not inspected, as y is not. */
int gpsat_fit_predict_batch_noise(gpsat_handle *h, const gpsat_batch *b, const gpsat_noise *nz);

/*
 * The gradient of the posterior mean with respect to the prediction point, with its posterior variance per component: the
 * extension of gpsat_fit_predict_batch_grad.  Callers detect it by the presence of that symbol; gpsat_batch keeps its layout
 * and GPSAT_ABI_VERSION stays 4.
 *
 * At the returned theta, for every prediction point x* of a tile and every input dimension a, with K_y = L L^T, z = L^-1 y,
 * d_i = (x_i - x*) / l (per dimension), r^2 = sum d_i^2 and gg(r^2) = -k'(r) / r of the unit-variance kernel:
 *   g_a[i] = dk(x*, x_i)/dx*_a = sf2 gg(r^2) d_{i,a} / l_a,   V_a = L^-1 g_a,
 *   f_grad[a] = V_a^T z = d f*(x*) / dx*_a,   f_grad_var[a] = sf2 gg(0) / l_a^2 - V_a^T V_a = var(df/dx_a at x* | y),
 * gg(0) = 1 (GPSAT_KERNEL_RBF), 3 (GPSAT_KERNEL_MATERN32), 5/3 (GPSAT_KERNEL_MATERN52).  Both are [sum P, D] row-major doubles
 * in the units of y (y^2) per unit of X.  A tile without observations returns the prior at theta0 (gradient 0, variance
 * sf2 gg(0) / l_a^2), a tile whose status is GPSAT_STATUS_NOT_PD or GPSAT_STATUS_NAN returns NaN in both.  The covariance
 * between components and between points is not returned.  Built for GPSAT_F64, the three kernels above and D <= 4, one
 * workgroup per tile, with both optimisers.  Every other output of the call has the bits gpsat_fit_predict_batch returns;
 * a tile's two outputs have the same bits alone, inside any batch and on a second call.
 */
typedef struct gpsat_pred_grad {
    void *f_grad;              /* [sum P * D] doubles, host|device as b->memory: out           */
    void *f_grad_var;          /* [sum P * D] doubles: out                                     */
    int32_t reserved[8];       /* must be 0                                                   */
} gpsat_pred_grad;             /* 48 bytes */

/* as gpsat_fit_predict_batch, with the two outputs above.  GPSAT_EINVAL (with a message that names the reason; the handle
 * stays usable) for GPSAT_F32, GPSAT_KERNEL_MATERN12 (not mean-square differentiable), GPSAT_KERNEL_RQ, a NULL pg, a NULL
 * output when sum P > 0, non-zero reserved words, and cov_off / f_cov given (no full covariance in the same call). */
int gpsat_fit_predict_batch_grad(gpsat_handle *h, const gpsat_batch *b, const gpsat_pred_grad *pg);

/*
 * The second derivatives of the posterior mean with respect to the prediction point, with their posterior variances, and a
 * weighted Laplacian: the extension of gpsat_fit_predict_batch_hess.  Callers detect it by the presence of that symbol;
 * gpsat_batch keeps its layout and GPSAT_ABI_VERSION stays 4.
 *
 * With the notation of gpsat_pred_grad and one more radial factor, hh(r^2) = -2 dgg/d(r^2) (GPSAT_KERNEL_RBF: exp(-r^2 / 2);
 * GPSAT_KERNEL_MATERN52: (25/3) exp(-sqrt(5) r); hh(0) = 1 and 25/3): for the set S of coordinates named by the bits of
 * `dims` (bit a: coordinate a; |S| = m) and every pair a <= b in S, a ascending, then b -- the m (m + 1) / 2 columns of the
 * two outputs --
 *   h_ab[i] = d2k(x*, x_i)/dx*_a dx*_b = sf2 (hh d_{i,a} d_{i,b} / (l_a l_b) - delta_ab gg / l_a^2),   V_ab = L^-1 h_ab,
 *   f_hess[ab] = V_ab^T z = d2 f*(x*) / dx*_a dx*_b,
 *   f_hess_var[ab] = sf2 hh(0) (1 + 2 delta_ab) / (l_a^2 l_b^2) - V_ab^T V_ab = var(d2f/dx_a dx_b at x* | y).
 * The weighted Laplacian sum_{a in S} c_a d2f/dx_a^2, c = lap_weight >= 0, has a solve of its own, because its variance holds
 * the covariances between the f_aa, which are not returned otherwise:
 *   h_lap = sum_a c_a h_aa,   f_lap = V_lap^T z,
 *   f_lap_var = sf2 hh(0) (2 sum_a c_a^2 / l_a^4 + (sum_a c_a / l_a^2)^2) - V_lap^T V_lap.
 * f_lap and f_lap_var both NULL and every weight 0: no such pass.  f_grad and f_grad_var, when given, are the two outputs of
 * gpsat_fit_predict_batch_grad with its bits, from the same launch.  Units: those of y (y^2) per unit of X squared (to the
 * fourth); a caller whose coordinates were scaled unequally gives c_a = 1 / scale_a^2 for the Laplacian in raw coordinates.
 * A tile without observations returns the prior at theta0 (zeros and the prior terms above), a tile whose status is
 * GPSAT_STATUS_NOT_PD or GPSAT_STATUS_NAN returns NaN.  No other covariance between components or points is returned.  Built for
 * GPSAT_F64, the two kernels above and D <= 4, one workgroup per tile, with both optimisers.  Every other output of the call has
 * the bits gpsat_fit_predict_batch returns; a tile's outputs have the same bits alone, inside any batch and on a second call.
 */
typedef struct gpsat_pred_hess {
    void *f_hess;              /* [sum P * m(m+1)/2] doubles, host|device as b->memory: out     */
    void *f_hess_var;          /* [sum P * m(m+1)/2] doubles: out                               */
    void *f_lap;               /* [sum P] doubles: out, or NULL                                 */
    void *f_lap_var;           /* [sum P] doubles: out, or NULL                                 */
    void *f_grad;              /* [sum P * D] doubles: out, or NULL                             */
    void *f_grad_var;          /* [sum P * D] doubles: out, or NULL                             */
    double lap_weight[4];      /* c_a >= 0 per coordinate; 0 outside dims and beyond D         */
    uint32_t dims;             /* bit a set: coordinate a is in S                              */
    int32_t reserved[7];       /* must be 0                                                   */
} gpsat_pred_hess;             /* 112 bytes */

/* as gpsat_fit_predict_batch, with the outputs above.  GPSAT_EINVAL (with a message that names the reason; the handle stays
 * usable) for GPSAT_F32, GPSAT_KERNEL_MATERN12 and GPSAT_KERNEL_MATERN32 (the derivative process is not mean-square
 * differentiable), GPSAT_KERNEL_RQ (not built), a NULL ph, dims empty or naming a coordinate >= D, a NULL output when
 * sum P > 0 (f_lap / f_lap_var: when the other or a weight is given; f_grad / f_grad_var: when the other is given), a negative
 * or non-finite weight or a weight on a coordinate outside dims, non-zero reserved words, and cov_off / f_cov given. */
int gpsat_fit_predict_batch_hess(gpsat_handle *h, const gpsat_batch *b, const gpsat_pred_hess *ph);

/*
 * Held-out (cross-validation) predictions from every tile's own factor: the extension of gpsat_fit_predict_batch_cv
 * (fp64 only).  Callers detect it by the presence of that symbol; gpsat_batch keeps its layout and GPSAT_ABI_VERSION stays 4.
 *
 * After the tile's last evaluation, at the returned theta, every fold G of the tile (rows with the same label) is predicted
 * from all OTHER rows of the tile, with A = K_y^-1 = L^-T L^-1 and alpha = K_y^-1 y:
 *   A_GG = (L^-1[:, G])^T (L^-1[:, G]),  cv_mean_G = y_G - A_GG^-1 alpha_G,  cv_y_var_G = diag(A_GG^-1),
 *   cv_f_var_G = cv_y_var_G - likelihood variance          (one row: Rasmussen & Williams eq. 5.12).
 * theta is NOT fitted again without the fold.  Every other output of the call has the bits gpsat_fit_predict_batch returns.
 * A tile's held-out values have the same bits alone, inside any batch and on a second call.  Rows of a fold whose A_GG is
 * not positive definite, and all rows of a tile with status NOT_PD or NAN, are NaN.  A fold that is the whole tile returns
 * the prior (mean 0, cv_f_var = kernel variance) up to rounding.
 * Limits and memory: a fold holds at most gpsat_max_cv_fold() = 256 rows; the folds' matrices (sum g^2 <= 256 N doubles per
 * tile) live in the prediction scratch of the tile's workspace, so the call needs no workspace beyond
 * gpsat_fit_predict_batch's; the handle keeps the fold tables (about 3 int32 per row, 2 per fold, 1 per 16 x 16 block that
 * holds two rows of one fold) and, in host mode, the three outputs (24 bytes per row) until gpsat_destroy.
 * One workgroup runs every tile (no teams).
 */
typedef struct gpsat_cv {
    const int32_t *fold;   /* [sum N] host; rows of one tile with equal label >= 0 are held out together;
                              label < 0: the row is never held out (its outputs are NaN);
                              NULL: every row is its own fold (leave-one-out).  Any int32 >= 0 is a label; labels need
                              not be dense or sorted; the same value in two tiles names two unrelated folds */
    void *cv_mean;         /* [sum N] host|device as b->memory, element type b->dtype */
    void *cv_f_var;        /* [sum N] */
    void *cv_y_var;        /* [sum N], may be NULL */
    int32_t reserved[8];
} gpsat_cv;

/* as gpsat_fit_predict_batch, with the held-out predictions above.  GPSAT_EINVAL (with a message) for a dtype other than
 * GPSAT_F64, a fold above the limit (the message names the tile and the label), cov_off / f_cov in the same call, a NULL
 * cv, and a NULL cv_mean or cv_f_var. */
int gpsat_fit_predict_batch_cv(gpsat_handle *h, const gpsat_batch *b, const gpsat_cv *cv);

/* largest fold of gpsat_fit_predict_batch_cv (256 for GPSAT_F64, D = 1..4); 0 for GPSAT_F32 and unsupported arguments */
int gpsat_max_cv_fold(int dtype, int D);

/*
 * Cross-validation that fits every held-out fold again: the extension of gpsat_fit_predict_batch_cv_refit (both dtypes).
 * Callers detect it by the presence of that symbol; gpsat_batch keeps its layout and GPSAT_ABI_VERSION stays 4.
 * Replaces the reference's cross-validation runs (examples/create_xval_config.py: one LocalExpertOI run per held-out track,
 * which removes the track, fits every expert's parameters on what is left, de-means what is left again and predicts at the
 * held-out rows).
 *
 * 1. The batch is run exactly as gpsat_fit_predict_batch runs it: every plain output has that call's bits.
 * 2. For every fold G of every tile (rows with the same label >= 0; folds of a tile are numbered by ascending label,
 *    fold_off[t] + k is fold k of tile t) that leaves at least max(min_obs, 1) rows, a derived tile is formed on the device:
 *    observations = the tile's other rows in source order, y' = dtype(double(y) - delta) with delta = their fp64 mean
 *    (recentre = 1) or 0, prediction points = the fold's rows in source order, theta0 = the batch's theta0 of the tile
 *    (start = 0) or the tile's returned theta (start = 1; the batch's theta0 where that theta is not finite and positive),
 *    the tile's lo / hi and the batch's trainable, optimiser and tolerances.
 * 3. All derived tiles, in fold order, are run as ONE batch through gpsat_fit_predict_batch's own path (device-resident
 *    inputs in buffers of the handle): a fold's outputs have the bits that batch has from any caller.
 * 4. cv_mean of a fold's rows = dtype(double(f*) + delta), i.e. in the units of the tile's y; cv_f_var / cv_y_var are the
 *    derived tile's.  Rows of label < 0, of a fold that was not fitted and of a fold whose derived tile ended NOT_PD or NAN
 *    are NaN.
 * 5. Per fold: theta, objective, status, evaluations, iterations, rows fitted, delta and the label.  A fold that was not
 *    fitted has status GPSAT_STATUS_SKIPPED, NaN theta / nll / shift and 0 evaluations.
 * delta is one fp64 sum in a fixed order: a second call returns the same bits.  There is no limit on the size of a fold (it
 * is a prediction set).  GPSAT_OPT_NONE evaluates every fold at theta0.  gpsat_last_timing covers both launches and the two
 * kernels around the second.
 * Memory: the handle keeps, until gpsat_destroy, the derived inputs (expanded_rows (D + 1) + R D elements, R <= sum N the
 * held-out rows), three outputs of R elements, in host mode the three cv outputs (3 sum N elements), and the fold tables
 * (about 3 int32 per row, 40 bytes per fold).  The call does NOT split itself: size it with gpsat_cv_refit_count, which
 * returns expanded_rows -- at D = 3 about 16 (fp32) or 32 (fp64) bytes per expanded row -- and hand over consecutive ranges
 * of tiles whose expanded_rows fit the device.  A failed allocation is GPSAT_ENOMEM.
 */
typedef struct gpsat_cv_refit {
    const int32_t *fold;      /* [sum N] host, labels as in gpsat_cv (>= 0 held out together, < 0 never held out); must not be NULL */
    int32_t start;            /* 0: every fold starts from b->theta0 (the reference: a fresh run); 1: from the tile's full-data theta */
    int32_t recentre;         /* 1: the remaining rows are de-meaned by their own mean (obs_mean="local" without the fold) */
    int32_t min_obs;          /* a fold that leaves fewer than max(min_obs, 1) rows is not fitted (fold_status SKIPPED, rows NaN) */
    const int64_t *fold_off;  /* [T+1] host: from gpsat_cv_refit_count; sizes the per-fold outputs */
    void    *cv_mean, *cv_f_var, *cv_y_var;   /* [sum N] host|device as b->memory, element type b->dtype; cv_y_var may be NULL */
    double  *fold_theta;      /* [F*H] host */
    double  *fold_nll;        /* [F] host */
    double  *fold_shift;      /* [F] host: delta */
    int32_t *fold_status, *fold_n_eval, *fold_n_iter, *fold_n_obs, *fold_label;   /* [F] host; n_iter may be NULL */
    int32_t reserved[8];
} gpsat_cv_refit;

/* Folds per tile as CSR offsets fold_off [T+1] (F = fold_off[T]) and expanded_rows = the sum over all folds of N_t - g, the
 * observation rows gpsat_fit_predict_batch_cv_refit will hold on the device.  Host code only: works without a GPU.
 * GPSAT_EINVAL for a NULL argument, bad offsets, or more than 2^31 - 1 rows. */
int gpsat_cv_refit_count(int32_t T, const int64_t *obs_off, const int32_t *fold, int64_t *fold_off, int64_t *expanded_rows);

/* as gpsat_fit_predict_batch, with the refitted held-out predictions above.  GPSAT_EINVAL (with a message that names the
 * argument) for a NULL cv, fold, fold_off, cv_mean, cv_f_var or required per-fold output, a fold_off that differs from
 * gpsat_cv_refit_count's, start or recentre outside {0, 1}, and cov_off / f_cov in the same call. */
int gpsat_fit_predict_batch_cv_refit(gpsat_handle *h, const gpsat_batch *b, const gpsat_cv_refit *cv);

/*
 * The joint log predictive density of every fold, an optional output of both cross-validation calls: one fp64 number per
 * fold, in the units of the tile's y as cv_mean is.  Callers detect it by the presence of the two symbols below; no
 * existing struct changes its layout and GPSAT_ABI_VERSION stays 4.  Summed over a tile's folds it is the cross-validation
 * pseudo-likelihood (Rasmussen & Williams section 5.4.2).
 *   gpsat_fit_predict_batch_cv_joint: with A = K_y^-1, alpha = A y, L_A the lower Cholesky factor of A_GG and
 *     u = L_A^-1 alpha_G:   fold_lpd = log N(y_G; cv_mean_G, A_GG^-1) = -1/2 u^T u + sum_k log (L_A)_kk - g/2 log 2 pi
 *     (one row: -1/2 alpha_i^2 / A_ii - 1/2 log(2 pi / A_ii)).  Every other output has the bits of
 *     gpsat_fit_predict_batch_cv; a tile's fold_lpd has the same bits alone, inside any batch and on a second call.
 *   gpsat_fit_predict_batch_cv_refit_joint (GPSAT_F64 only: the g x g factorisation of an fp32 covariance would need a
 *     tolerance nobody has measured): for the fold's derived tile at its own fitted theta,
 *     fold_lpd = log N(y'_G; f*, f_cov + sn2 I), y'_G the fold's rows shifted by the fold's delta as the remaining rows
 *     were, sn2 the fold's fitted likelihood variance.  The derived batch returns its posterior covariances for it, into a
 *     buffer of the handle (sum over the fitted folds of g^2 doubles, kept until gpsat_destroy; a fold has no size limit),
 *     so that batch is planned as a batch with f_cov is: its predictions need not have the bits of
 *     gpsat_fit_predict_batch_cv_refit's.  A second call returns the same bits.
 * NaN: where the fold's rows are NaN (a failed tile, a pivot <= 0 in A_GG, a derived tile that ended NOT_PD / NAN), a fold
 * that was not fitted (refit: fewer than max(min_obs, 1) rows left) and a pivot <= 0 in the refit flavour's g x g
 * factorisation.  Rows of label < 0 belong to no fold.
 * Folds are numbered as gpsat_cv_refit_count numbers them, in both calls: fold_off[t] + k is fold k of tile t, folds of a
 * tile in ascending label; with gpsat_cv.fold == NULL (leave-one-out) fold k of a tile is its row k, so fold_off = obs_off.
 */
typedef struct gpsat_cv_joint {
    const int64_t *fold_off;   /* [T+1] host, from gpsat_cv_refit_count (fold == NULL: fold_off = obs_off) */
    double        *fold_lpd;   /* [F] host, F = fold_off[T] */
    int32_t        reserved[8];/* must be 0 */
} gpsat_cv_joint;

/* as the call without _joint, which refuses what it refuses as before.  GPSAT_EINVAL (with a message; the handle stays
 * usable) also for a NULL joint, a NULL member of it, non-zero reserved words and a fold_off that differs from
 * gpsat_cv_refit_count's (the message names the index); the refit flavour also for GPSAT_F32. */
int gpsat_fit_predict_batch_cv_joint(gpsat_handle *h, const gpsat_batch *b, const gpsat_cv *cv, const gpsat_cv_joint *joint);
int gpsat_fit_predict_batch_cv_refit_joint(gpsat_handle *h, const gpsat_batch *b, const gpsat_cv_refit *cv,
                                           const gpsat_cv_joint *joint);

/* library / ABI version (GPSAT_ABI_VERSION) */
int gpsat_version(void);

/* thread-local description of the last error returned on this thread */
const char *gpsat_last_error(void);

/* number of HIP devices visible (0 when there is none); never fails */
int gpsat_device_count(void);

/*
 * Largest number of observations one tile may hold for `dtype` (GPSAT_F32 / GPSAT_F64) and input dimension D: the
 * tile's coordinates, observations and solve vectors stay in the 160 KiB LDS of its CU for the whole fit, and no tile
 * holds more than 4,096.  D = 1 / 2 / 3 / 4: 4,096 / 3,392 / 2,832 / 2,416 in fp64 (the reference's published N = 2,500
 * fp64 fit, docs/notebooks/using_gpus.ipynb:77,165, fits) and 4,096 / 4,096 / 3,168 / 2,592 in fp32.  A batch holding a
 * larger tile is refused with GPSAT_EINVAL.  0 for unsupported arguments.  ABI >= 3.
 */
int gpsat_max_tile_obs(int dtype, int D);

/*
 * Create an engine bound to one GPU.  Replaces model construction-time device discovery
 * (BaseGPRModel._get_device_names, base_model.py:279-300).  `opts` may be NULL.
 */
int gpsat_create(int device_id, const gpsat_opts *opts, gpsat_handle **out);

/* device name of the handle's GPU (reference: model.gpu_name, local_experts.py:1180) */
int gpsat_device_name(gpsat_handle *h, char *buf, int buflen);

/* release every device resource owned by the handle */
int gpsat_destroy(gpsat_handle *h);

/* fit (optional) + objective + predict for one packed batch; see gpsat_batch */
int gpsat_fit_predict_batch(gpsat_handle *h, const gpsat_batch *b);

/*
 * Batched tile selection: which rows of a point table belong to each of T expert tiles.
 * Replaces DataLoader.local_data_select (GPSat/dataloader.py:2352-2447) and the max_dist filter of
 * PredictionLocations (GPSat/prediction_locations.py:18-43) for all experts at once, in fp64 with the reference's
 * comparison arithmetic (bit-exact membership, source row order).
 *   kind 0: points[cols[k][0]] <comp> (refs[cols[k][0]] + val[k])       comp: 0 >=, 1 >, 2 ==, 3 <, 4 <=
 *   kind 1: sum_m (points[cols[k][m]] - refs[cols[k][m]])^2 <= val[k]^2  (comp 4, observations: inclusive ball)
 *                                                          <  val[k]^2  (comp 3, prediction locations: strict)
 *   kind 2: bounds[t][cols[k][1]][0] <= points[cols[k][0]] < bounds[t][cols[k][1]][1]   (per-expert interval, fp64; a NaN
 *           point is never inside; comp, ncols and val are not read).  Only gpsat_select_batch_ex takes it.  GPSat's dynamic
 *           global_select entries (dataloader.py:2893-2978) arrive this way: the source column rank-coded, one rank
 *           interval per expert.
 */
#define GPSAT_SEL_MAXCRIT 4
typedef struct gpsat_select_spec {
    int32_t n_crit;                        /* 1 .. GPSAT_SEL_MAXCRIT criteria, ANDed                 */
    int32_t kind[GPSAT_SEL_MAXCRIT];
    int32_t comp[GPSAT_SEL_MAXCRIT];
    int32_t ncols[GPSAT_SEL_MAXCRIT];      /* kind 1: 1..3 columns                                   */
    int32_t cols[GPSAT_SEL_MAXCRIT][3];    /* column indices (same numbering in points and refs)      */
    double  val[GPSAT_SEL_MAXCRIT];
} gpsat_select_spec;

/*
 * points: host, column-major [C][M] fp64;  refs: host, row-major [T][C] fp64.
 * off  : host out [T+1] CSR offsets (always written).
 * idx  : host out [capacity] selected row indices per expert, ascending; may be NULL (count only).
 * Returns GPSAT_EINVAL if capacity < off[T] (off is still valid: call again with a larger buffer).
 * Two-call use (sizes with idx = NULL, then the same arguments with idx): the indices of the first call stay on the device
 * and the second call only copies them out -- PROVIDED `points` and `refs` are the same buffers with unchanged contents and
 * no other call was made on the handle in between.  The library checks the arguments and a fingerprint of the contents (all
 * of refs, a sample of points) and selects again when anything differs; do not rely on the sample to catch a partial refill
 * of `points`.
 */
int gpsat_select_batch(gpsat_handle *h, const gpsat_select_spec *spec, int64_t M, int32_t C, const double *points,
                       int32_t T, const double *refs, int64_t *off, int32_t *idx, int64_t capacity);

/*
 * gpsat_select_batch with per-expert interval criteria (kind 2; added within ABI 4, check for the symbol).
 * bounds: host [T][n_bounds][2] fp64 {lo, hi}; a kind-2 criterion k reads bound pair cols[k][1] (0 <= cols[k][1] < n_bounds).
 * n_bounds = 0 with bounds = NULL is gpsat_select_batch.  The two-call cache also compares `bounds` (pointer and contents).
 */
int gpsat_select_batch_ex(gpsat_handle *h, const gpsat_select_spec *spec, int64_t M, int32_t C, const double *points,
                          int32_t T, const double *refs, int32_t n_bounds, const double *bounds, int64_t *off, int32_t *idx,
                          int64_t capacity);

/*
 * Gaussian smoothing of one hyper-parameter field over T expert locations (one "other dimensions" slice).
 * Replaces gaussian_2d_weight (GPSat/postprocessing.py:22-52) as called by smooth_hyperparameters (:277-288, after
 * the min/max clipping done by the caller).  x, y, vals, out: host fp64 [T]; NaN vals are skipped; out is NaN when
 * all weights vanish.
 */
int gpsat_smooth_batch(gpsat_handle *h, int32_t T, const double *x, const double *y, const double *vals, double l_x,
                       double l_y, double *out);

/*
 * Gluing of overlapping local predictions (GPSat/postprocessing.py:447-577): R prediction rows pre-sorted by
 * prediction location into G segments seg[G+1]; pred, xprt: host fp64 [ndim][R] (ndim 1 or 2); vals: host fp64
 * [nvars][R] (nvars <= 4); sigma = inference_radius / R_factor, or per row in sigma_rows [R] when not NULL (the
 * per-expert inference_radius dict of :490-493); out: host fp64 [nvars][G] = sum w v / sum w with
 * w = prod_d normpdf(pred_d; xprt_d, sigma).
 */
int gpsat_glue_batch(gpsat_handle *h, int64_t R, int32_t G, int32_t ndim, int32_t nvars, const int64_t *seg,
                     const double *pred, const double *xprt, const double *vals, double sigma,
                     const double *sigma_rows, double *out);

/*
 * Gluing by an integer key, rows in ANY order (added within ABI 4, check for the symbol): what gpsat_glue_batch computes,
 * for callers whose groups are named by an integer instead of a pre-sorted segment table -- held-out predictions keyed by
 * the observation they predict: millions of groups of a few rows each.  The grouping runs on the device (a stable radix
 * sort of (key, row) over the bits of the largest key, run heads, one team of 8 lanes per group).
 *
 * key        : host [R]; every distinct key >= 0 yields one output record, in ascending key order; key < 0: the row is
 *              ignored altogether.
 * pred, xprt : host fp64 [ndim][R], ndim 1 or 2;  vals: host fp64 [nvars][R], nvars <= 4 (GPSAT_GLUE_MAXVARS).
 * sigma, sigma_rows: as gpsat_glue_batch (sigma finite and > 0 unless sigma_rows [R] is given).
 * max_dist   : finite and > 0: a row takes part only if sum_d (pred_d - xprt_d)^2 < max_dist^2 (strict: a row exactly on
 *              the limit is out, as is one whose distance is NaN); +inf or <= 0: every row takes part.
 * Within a key, out = sum w v / sum w over the rows that take part, w = prod_d normpdf(pred_d; xprt_d, sigma).  A NaN value
 * is left out of the numerator and its weight stays in the denominator (the rule of gpsat_glue_batch).  A key whose rows
 * all fall outside max_dist has count 0 and NaN outputs.
 *   G        : host out [1], the number of distinct keys >= 0; written whenever the arguments pass the checks;
 *   out_key  : host out [capacity], ascending;  out_count: host out [capacity], the rows that took part;
 *   out      : host out fp64, variable v of record j at out[v * capacity + j].
 * capacity = R always suffices.  GPSAT_EINVAL (the handle stays usable) for a NULL required pointer, ndim outside {1, 2},
 * nvars outside 1..4, a sigma that is not finite and positive with sigma_rows == NULL, a NaN max_dist, R > 2^31 - 1, and
 * capacity < G (G is valid then: call again).  R = 0 returns G = 0.
 * A group's bits depend on its own rows in their source order only -- not on the other keys of the call, nor on the grid
 * or the capacity -- and a second call returns the same bytes: the sort is stable, lane l of a team adds the group's rows
 * l, l + 8, ... in order, a fixed tree joins the 8 lanes, and there are no atomics.  They are not the bits of
 * gpsat_glue_batch, whose tree is 64 lanes wide.  A group is walked by its one team: a call whose rows all share a few
 * keys is slow next to gpsat_glue_batch.
 * The device workspace (about 32 + 8 (2 ndim + nvars + 2) bytes per row) is owned by the handle.  gpsat_last_timing covers
 * the call: kernel_ms = keys, sort, run heads, reduction; gpsat_glue_keyed_timing splits it: ms[0] sort, ms[1] run heads,
 * ms[2] reduction, of the last call on the handle.
 */
int gpsat_glue_keyed_batch(gpsat_handle *h, int64_t R, int32_t ndim, int32_t nvars, const int64_t *key,
                           const double *pred, const double *xprt, const double *vals, double sigma,
                           const double *sigma_rows, double max_dist, int64_t capacity, int64_t *G, int64_t *out_key,
                           int32_t *out_count, double *out);
int gpsat_glue_keyed_timing(gpsat_handle *h, double *ms);

/*
 * The glued value with the exact slope of the glued map, by key (added within ABI 4, check for the symbol).  Every row
 * carries a value f_i and its gradient g_ia = df_i/dp_a along the ndim glue axes.  The glued map is
 * F(p) = sum w_i(p) f_i(p) / sum w_i(p), and its weights move with p: dw_i/dp_a = w_i u_ia with
 * u_ia = (xprt_ia - pred_ia) / sigma_i^2.  Per key, over the rows that take part (the rules of gpsat_glue_keyed_batch):
 *     W = sum w_i,   F = (sum_{f_i not NaN} w_i f_i) / W,   U_a = sum w_i u_ia,
 *     S_a = sum_{f_i and g_ia not NaN} w_i (g_ia + u_ia f_i),   G_a = (S_a - F U_a) / W.
 * G_a is the derivative of the formula of gpsat_glue_keyed_batch, its NaN rule included; the plain weighted average of the
 * g_ia leaves out the term of size (disagreement of neighbouring experts) x (their spacing) / sigma^2.
 * val        : host fp64 [R];  grad: host fp64 [ndim][R].
 *   out_val  : host out [capacity], F: the bytes gpsat_glue_keyed_batch returns for nvars = 1, vals = val on these rows;
 *   out_grad : host out, component a of record j at out_grad[a * capacity + j].
 * Everything else -- key, pred, xprt, sigma, sigma_rows, max_dist, capacity, G, out_key, out_count, the return codes (capacity
 * < G: GPSAT_EINVAL with G valid), the determinism, the workspace (1 + ndim value columns) and the timing calls -- is as
 * in gpsat_glue_keyed_batch.  A key with count 0 has NaN in F and every G_a.
 */
int gpsat_glue_keyed_grad_batch(gpsat_handle *h, int64_t R, int32_t ndim, const int64_t *key, const double *pred,
                                const double *xprt, const double *val, const double *grad, double sigma,
                                const double *sigma_rows, double max_dist, int64_t capacity, int64_t *G, int64_t *out_key,
                                int32_t *out_count, double *out_val, double *out_grad);

/*
 * The glued value with the exact slope and the exact second derivatives of the glued map, by key (added within ABI 4, check
 * for the symbol).  Every row carries a value f_i, its gradient g_ia and its second derivatives h_iab = d2f_i/dp_a dp_b for
 * the pairs a <= b of the ndim glue axes, npair = ndim (ndim + 1) / 2 of them in the order (0,0), (0,1), (1,1) (ndim 1:
 * (0,0) alone).  With u_ia as in gpsat_glue_keyed_grad_batch and q_i = 1 / sigma_i^2 the weights have
 * d2w_i/dp_a dp_b = w_i (u_ia u_ib - delta_ab q_i).  Per key, over the rows that take part, with W, F, U_a, S_a and G_a of
 * gpsat_glue_keyed_grad_batch:
 *     V_ab = sum w_i (u_ia u_ib - delta_ab q_i),
 *     T_ab = sum_{f_i, g_ia, g_ib and h_iab not NaN} w_i (h_iab + u_ia g_ib + u_ib g_ia + (u_ia u_ib - delta_ab q_i) f_i),
 *     H_ab = (T_ab - G_a U_b - G_b U_a - F V_ab) / W,
 * which is N = F W differentiated twice.  A row whose entries are NaN stays out of the numerators (of F with a NaN f_i, of
 * S_a with a NaN f_i or g_ia, of T_ab with a NaN among f_i, g_ia, g_ib, h_iab); its weight stays in W, U and V.  The plain
 * weighted average of the h_iab leaves out terms of size (disagreement of neighbouring experts) / sigma^2 and
 * (disagreement of their slopes) x (their spacing) / sigma^2: it is the Hessian of nothing.
 * val        : host fp64 [R];  grad: host fp64 [ndim][R];  hess: host fp64 [npair][R].
 *   out_val  : host out [capacity], F;  out_grad: host out, G_a of record j at out_grad[a * capacity + j]: both the bytes
 *              gpsat_glue_keyed_grad_batch returns on these rows;
 *   out_hess : host out, pair k of record j at out_hess[k * capacity + j].
 * Everything else -- key, pred, xprt, sigma, sigma_rows, max_dist, capacity, G, out_key, out_count, the return codes (capacity
 * < G: GPSAT_EINVAL with G valid), the determinism and the timing calls -- is as in gpsat_glue_keyed_batch; the workspace
 * holds 1 + ndim + npair value columns (about 32 + 8 (3 ndim + npair + 3) bytes per row).  A key with count 0 has NaN in F,
 * every G_a and every H_ab.
 */
int gpsat_glue_keyed_hess_batch(gpsat_handle *h, int64_t R, int32_t ndim, const int64_t *key, const double *pred,
                                const double *xprt, const double *val, const double *grad, const double *hess,
                                double sigma, const double *sigma_rows, double max_dist, int64_t capacity, int64_t *G,
                                int64_t *out_key, int32_t *out_count, double *out_val, double *out_grad, double *out_hess);

/*
 * Binning of raw observations on a regular grid, all groups in one call (added within ABI 4, check for the symbol).
 * Replaces DataPrep.bin_data_by / DataPrep.bin_data (GPSat/dataprepper.py:21-401): per group (day, satellite, ...) a
 * scipy.stats.binned_statistic_2d (1-D: binned_statistic) of `v` over the bins of `ex` x `ey`.  Every statistic of every
 * cell equals scipy's bit for bit for finite values: membership is np.digitize on the edge values (edges[i] <= x <
 * edges[i+1], rows below the first edge, beyond the last bin or with a NaN coordinate are outside), and sum / mean / std
 * add a cell's rows one after the other in source row order, as np.bincount does.  NaN values follow scipy: counted by
 * count; sum, mean, std and max NaN; ignored by min (NaN when the cell holds nothing else); ordered last by the median.
 *
 * x, y, v : host fp64 [R]; y = NULL bins in one dimension (ny, ey and y_hi are then not read).
 * gid     : host [R], the group of every row, 0 <= gid < G; NULL puts every row into group 0.
 * ex, ey  : host fp64 [nx], [ny]: the bin EDGES, finite and strictly increasing, at least 2 per axis, exactly as the
 *           caller's np.linspace made them (the library never restates them).
 * x_hi, y_hi: inclusive upper limit of the LAST bin, >= the last edge: scipy puts x >= edges[-1] into the last bin when
 *           np.around(x, d) == np.around(edges[-1], d), d = int(-log10(min(diff(edges)))) + 6; np.around is monotone, so
 *           that set is the interval [edges[-1], x_hi], which the caller finds with np.around itself.  x_hi = edges[-1]
 *           takes the edge alone.
 * stats   : a non-empty OR of GPSAT_BIN_*.
 * Output, sparse: one record per non-empty cell, ascending key; key = (gid (ny-1) + iy)(nx-1) + ix (1-D: gid (nx-1) + ix).
 *   n_cells: host out [1], always written;  keys: host out [capacity];
 *   out    : host out fp64 [number of statistics][capacity], the statistics asked for in ascending bit order, statistic s
 *            of record j at out[s * capacity + j] (count is returned as fp64, exact below 2^53).
 * The caller sizes the outputs: capacity >= min(R, G (nx-1)(ny-1)) always suffices.  GPSAT_EINVAL when capacity < n_cells
 * (n_cells is valid: call again), for bad sizes, fewer than 2 edges, edges that do not increase, a limit below the last
 * edge, gid out of range, an empty or unknown `stats`.  R = 0 and G = 0 are valid and return n_cells = 0.
 * Limits: R <= 2^31 - 1 rows per call (the sort carries a 32-bit source row), (nx-1)(ny-1) < 2^31 cells per group,
 * G (nx-1)(ny-1) < 2^63.  A cell's rows are added one after the other, in order (by one lane, by one wave from 1,024
 * rows): that is what keeps scipy's bits, and it makes a table whose rows all fall into a few cells slow next to a tree
 * reduction, which is not used (10 M rows in one cell: 0.13 s per sum).
 * The device workspace (about 60 bytes per row, 16 more with the median) is owned by the handle and kept until
 * gpsat_destroy.  gpsat_last_timing covers it: kernel_ms = keys, sort and statistics, total_ms = with the copies.
 */
#define GPSAT_BIN_COUNT  1u
#define GPSAT_BIN_SUM    2u
#define GPSAT_BIN_MEAN   4u
#define GPSAT_BIN_STD    8u
#define GPSAT_BIN_MIN    16u
#define GPSAT_BIN_MAX    32u
#define GPSAT_BIN_MEDIAN 64u
int gpsat_bin_batch(gpsat_handle *h, int64_t R, const double *x, const double *y, const double *v, const int32_t *gid,
                    int32_t G, int32_t nx, const double *ex, double x_hi, int32_t ny, const double *ey, double y_hi,
                    uint32_t stats, int64_t capacity, int64_t *n_cells, int64_t *keys, double *out);

/*
 * Raw rows to the columns the pipeline starts from (added within ABI 4, check for the symbols): the projection of lon / lat
 * to EASE2 metres and back, and the track number of every row.  Replaces GPSat.utils.WGS84toEASE2 / EASE2toWGS84 (pyproj,
 * "+proj=laea +lat_0=.. +lon_0=.. +ellps=WGS84") and diff_distance / guess_track_num / track_num_for_date (numba loops) as
 * examples/generate_track_id.py TrackId.assign_tracks / add_tracks uses them.
 *
 * gpsat_project_batch: Lambert azimuthal equal-area on the WGS84 ellipsoid (a = 6378137, 1/f = 298.257223563), POLAR aspects
 * only, fp64 (Snyder 3-12, 24-23, 24-25; the inverse solves q(phi) = q by Newton's iteration, Snyder 3-16, to the last bit
 * instead of PROJ's truncated authalic-latitude series).
 *   direction GPSAT_PROJECT_FORWARD: in0 = lon, in1 = lat (degrees) -> out0 = x, out1 = y (metres);
 *   direction GPSAT_PROJECT_INVERSE: in0 = x, in1 = y (metres) -> out0 = lon in (-180, 180], out1 = lat (degrees).
 *   A NaN in either input gives NaN in both outputs.  The inverse of (0, 0) is (lon_0, lat_0); a point outside the
 *   projection's disc gives +inf in both outputs.
 * in0, in1, out0, out1: [n] fp64, host pointers (GPSAT_MEM_HOST) or device pointers (GPSAT_MEM_DEVICE: nothing is copied,
 * the arrays are not inspected; out may alias in).  GPSAT_EINVAL: lat_0 not +90 / -90, lon_0 not finite, an unknown
 * direction or memory flag, n < 0 or > 2^31 - 1, a NULL array with n > 0, non-zero reserved words.  n = 0 is valid.
 */
#define GPSAT_PROJECT_FORWARD 0
#define GPSAT_PROJECT_INVERSE 1
typedef struct gpsat_project {
    int64_t       n;
    int32_t       direction;   /* GPSAT_PROJECT_*                         */
    int32_t       memory;      /* GPSAT_MEM_*                             */
    double        lon_0;       /* central meridian, degrees               */
    double        lat_0;       /* +90 or -90                              */
    const double *in0, *in1;   /* [n] */
    double       *out0, *out1; /* [n] */
    int32_t       reserved[8]; /* 0 */
} gpsat_project;
int gpsat_project_batch(gpsat_handle *h, const gpsat_project *p);

/*
 * gpsat_track_batch: the rows are taken group by group (groups in ascending code, a group's rows in the order given: a
 * stable sort), every row gets the distance to its predecessor IN ITS GROUP, and
 *   mode GPSAT_TRACK_CUT  : track = start_track + the number of flags up to and including the row, where a row is flagged
 *                           when delta > cut_off (NaN compares false) or when it is the first row of a group other than the
 *                           first: guess_track_num per group with start_track = the previous group's max + 1, in one pass;
 *   mode GPSAT_TRACK_RUNS : out_track = rows since the last row whose cols[0] differed from its predecessor's (!=, so a NaN
 *                           restarts) or that began a group: track_num_for_date.  n_cols must be 1; cut_off and start_track
 *                           are not read; out_delta may be NULL.
 *   mode GPSAT_TRACK_GIVEN: as GPSAT_TRACK_CUT on distances that are there already: delta = cols[0] itself, a group's first
 *                           row included (guess_track_num on a column of diff_distance).  n_cols must be 1.
 * cols     : n_cols (1..3) arrays [n] fp64; delta = sqrt(sum_c (cols[c][i] - cols[c][i-1])^2): difference, square, sum from
 *            the left, root, none of them fused; NaN for the first row of a group (diff_distance(x, p=2, k=1)).
 * group    : [n] int32 codes >= 0 numbered in order of first appearance (pd.factorize), -1: the row is in no group; NULL: one
 *            group.  Rows of code -1 come last in out_order, with delta NaN and track -1.
 * Outputs, in the order the rows were TAKEN: out_order[i] is the source row taken i-th, out_delta[i] and out_track[i] are
 * its values.  Without groups out_order is 0, 1, 2, ...
 * Host or device pointers by `memory`, as gpsat_project.  GPSAT_EINVAL: n_cols outside 1..3, cut_off not finite,
 * start_track < 0 or start_track + n > 2^31 - 1, an unknown mode or memory flag, n < 0 or > 2^31 - 1, a NULL array with
 * n > 0, non-zero reserved words, and in host mode a group code below -1 (the message names the row).  The results are
 * integers and exact doubles of fixed operation order: a second call returns the same bytes.
 * gpsat_last_timing covers both calls: kernel_ms = the kernels (with the sort), total_ms = with the copies of host mode.
 */
#define GPSAT_TRACK_CUT  0
#define GPSAT_TRACK_RUNS 1
#define GPSAT_TRACK_GIVEN 2
typedef struct gpsat_track {
    int64_t        n;
    int32_t        n_cols;      /* 1..3 */
    int32_t        memory;      /* GPSAT_MEM_* */
    const double  *cols[3];     /* n_cols arrays [n] */
    const int32_t *group;       /* [n] or NULL */
    double         cut_off;
    int32_t        start_track;
    int32_t        mode;        /* GPSAT_TRACK_* */
    double        *out_delta;   /* [n] */
    int32_t       *out_track;   /* [n] */
    int32_t       *out_order;   /* [n] */
    int32_t        reserved[8]; /* 0 */
} gpsat_track;
int gpsat_track_batch(gpsat_handle *h, const gpsat_track *t);

/*
 * Timing of the last gpsat_fit_predict_batch on this handle, measured with HIP events on the
 * handle's stream: kernel_ms = the persistent tile kernel alone, total_ms = H2D + kernel + D2H.
 */
int gpsat_last_timing(gpsat_handle *h, double *kernel_ms, double *total_ms);

/*
 * Sparse GP experts (ABI >= 4): GPflow SGPR, the collapsed Titsias bound, with FIXED inducing points Z
 * (GPflowSGPRModel, GPSat/models/gpflow_models.py:666-901, train_inducing_points=False).  Replaces, per tile,
 * model = GPflowSGPRModel(...); model.optimise_parameters(); model.get_objective_function_value(); model.predict(...).
 * A tile holds at most 2^31 - 1 observations and prediction points (the kernel counts rows in 32-bit integers), no
 * other limit than device memory, and 1 <= M_t <= gpsat_max_inducing(dtype, D) inducing points.
 * Workspace: (7 + D) Mmax^2 + (16 + 1024) Mmax doubles per resident workgroup (Mmax = the batch's largest M_t; about
 * 100 MB at Mmax = 1024, D = 4), at most one workgroup per CU and at most 16 GiB in all.  The handle keeps the largest
 * workspace it has allocated until gpsat_destroy.
 */
typedef struct gpsat_sparse {
    const int64_t *z_off;   /* [T+1] host: CSR row offsets into Z; 1 <= M_t <= gpsat_max_inducing(dtype, D) */
    const void    *Z;       /* [sum M, D] inducing points, same frame / memory / dtype as X                  */
    double         jitter;  /* 0 = 1e-6 (GPflow default_jitter)                                              */
    int32_t        reserved[8];
} gpsat_sparse;

/*
 * fit (optional) + objective + predict of T sparse expert tiles.  `b` as for gpsat_fit_predict_batch, except:
 * dtype must be GPSAT_F64, cov_off / f_cov must be NULL (no full covariance), there is no per-tile observation limit,
 * nll is the negative ELBO and grad its gradient.  Status codes as for the exact path: a failed Cholesky of Kuu or of
 * I + A A^T gives GPSAT_STATUS_NOT_PD, a tile without observations GPSAT_STATUS_SKIPPED.  gpsat_last_timing covers it.
 */
int gpsat_sgpr_fit_predict_batch(gpsat_handle *h, const gpsat_batch *b, const gpsat_sparse *s);

/* Largest number of inducing points per tile for gpsat_sgpr_fit_predict_batch: 1024 for GPSAT_F64 and D = 1..4
 * (a workspace choice: (7 + D) M^2 doubles per workgroup); 0 for GPSAT_F32 and unsupported arguments.  ABI >= 4. */
int gpsat_max_inducing(int dtype, int D);

#ifdef __cplusplus
}
#endif
#endif /* GPSAT_HIP_H */
