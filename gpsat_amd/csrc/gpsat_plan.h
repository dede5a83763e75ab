// gpsat_plan.h -- the launch plan of gpsat_fit_predict_batch: which of the four kernel builds runs a batch, on what grid, with
// teams, cooperative tiles, time slicing or the deferred-prediction pool.  plan_tiles() is a pure function of host data (no HIP
// call, no handle, no device allocation), so every launch rule can be exercised without a GPU (tests/test_abi.py calls it
// through its exported symbol).  Part of gpsat_capi.cpp's translation unit: include it nowhere else.
#ifndef GPSAT_PLAN_H
#define GPSAT_PLAN_H
#include <algorithm>
#include <cstdio>

#include "gpsat_hip.h"
#include "gpsat_kernels.h"

namespace gpsat {

// The four builds of the tile kernels behind one interface (gpsat_kernels.h declares the functions).
struct Build {
    size_t (*shared_bytes)(int D, int NBmax);
    size_t (*workspace_per_wg)(int NBmax, int PCcov);         // floats (fp32 builds) or doubles (fp64 builds)
    int (*state_words)();
    size_t (*pq_floats_per_slot)(int D, int NBmax);           // nullptr: the build has no deferred predictions
    // the tile loop per F64Variant (`cv`: the held-out variant's arguments, `nz`: the noise variant's, `gr`: the gradient
    // variant's, `hs`: the second-derivative variant's, else null); nullptr: the build has no such variant
    F64Launch* launch_variant[7];
};
enum { BUILD_F32_W4 = 0, BUILD_F32_W8 = 1, BUILD_F64_W8 = 2, BUILD_F64_W4 = 3 };
// The variants of the fp64 tile loop (gpsat_kernels_f64.hip): held-out predictions, the RationalQuadratic covariance function,
// a trainable constant mean, known noise variances per observation, the gradient of the posterior mean at the prediction points,
// its second derivatives there.
// A job is one of them; every one but PLAIN runs one workgroup per tile.
enum F64Variant { PLAIN = 0, CV = 1, RQ = 2, MEAN = 3, NOISE = 4, GRAD = 5, HESS = 6 };
// the fp32 builds (no variants) behind the same signature
inline hipError_t launch_f32_w4(int D, const KernelArgs& a, const CvArgs*, const NoiseArgs*, const GradArgs*, const HessArgs*, int grid, size_t smem, hipStream_t stream) { return launch_tiles(D, a, grid, smem, stream); }
inline hipError_t launch_f32_w8(int D, const KernelArgs& a, const CvArgs*, const NoiseArgs*, const GradArgs*, const HessArgs*, int grid, size_t smem, hipStream_t stream) { return launch_tiles_w8(D, a, grid, smem, stream); }
const Build builds[4] = {
    {shared_bytes, workspace_floats_per_wg, state_words, pq_floats_per_slot, {launch_f32_w4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}},
    {shared_bytes_w8, workspace_floats_per_wg_w8, state_words_w8, nullptr, {launch_f32_w8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}},
    {shared_bytes_f64, workspace_doubles_per_wg_f64, state_words_f64, nullptr,
     {launch_tiles_f64, launch_tiles_f64_cv, launch_tiles_f64_rq, launch_tiles_f64_mean, launch_tiles_f64_noise, launch_tiles_f64_grad,
      launch_tiles_f64_hess}},
    {shared_bytes_f64_w4, workspace_doubles_per_wg_f64_w4, state_words_f64_w4, nullptr,
     {launch_tiles_f64_w4, launch_tiles_f64_cv_w4, launch_tiles_f64_rq_w4, launch_tiles_f64_mean_w4, launch_tiles_f64_noise_w4, launch_tiles_f64_grad_w4,
      launch_tiles_f64_hess_w4}},
};

// One developer knob (GPSAT_DEBUG_*, read through dev_env() only): whether it is set, and atoi of its text.
struct Knob { int set = 0, v = 0; };
struct DevKnobs { Knob team, coop, coop_xcd, coop_min_nb, coop_hdiv, grid, seg, defer; };

// All plain data (ints and one pointer), so that a test can fill it through ctypes.
struct PlanInput {
    int T, D, f64;
    const int64_t* obs_off;       // [T+1] host
    long long maxP;               // largest prediction count of a tile (read with want_cov only)
    int want_cov, has_pred;       // full covariance asked for; any prediction point at all
    int optimiser, max_iter;
    int num_cu, wg_per_cu;        // of the handle
    int solo, unsliced;           // the two reruns: one workgroup per tile after a team barrier gave up; no time slicing
    DevKnobs knobs;
};

struct TilePlan {
    int build;                    // index into builds[]
    int NBmax, PCcov, grid, team;
    int coop, coop_min_nb, coop_hdiv, coop_force;
    int seg_cost, state_words;
    int pq_slots;                 // deferred-prediction snapshot slots wanted (0: every prediction inline)
    size_t smem, ws_stride;       // LDS bytes; workspace elements per workgroup (or team)
    size_t ring_cap;              // entries of the time-slicing ring (0 when seg_cost == 0)
    size_t pq_stride;             // floats per snapshot slot
};

// false: the largest tile does not fit the LDS of a CU in the build the rules pick
bool plan_tiles(const PlanInput& in, TilePlan& p) {
    const int T = in.T, D = in.D, num_cu = in.num_cu;
    const bool f64 = in.f64 != 0;
    const DevKnobs& k = in.knobs;
    const int bs = f64 ? 16 : 32;
    long long maxN = 0;
    for (int t = 0; t < T; ++t) maxN = std::max<long long>(maxN, in.obs_off[t + 1] - in.obs_off[t]);
    const int NBmax = std::max(1, (int)((maxN + bs - 1) / bs));
    const int PCcov = in.want_cov ? std::max(1, (int)((in.maxP + bs - 1) / bs)) : 0;
    // fp32: two 4-wave workgroups per CU while a workgroup's LDS fits twice; beyond that one 8-wave workgroup per CU
    // (the 8-wave build of the same kernels), so that every SIMD still has two waves to overlap
    // ... and launches with fewer tiles than CUs: every tile has a CU to itself, eight waves use it better than four, and
    // the 8-wave build is the one with cooperative tiles
    const bool w8 = !f64 && (builds[BUILD_F32_W4].shared_bytes(D, NBmax) > 80 * 1024 || in.wg_per_cu == 1 || T < num_cu);
    // fp64: the same rule with the 4-wave / 8-wave builds of the fp64 kernels
    const bool d4 = f64 && builds[BUILD_F64_W4].shared_bytes(D, NBmax) <= 80 * 1024 && in.wg_per_cu != 1;
    p.build = f64 ? (d4 ? BUILD_F64_W4 : BUILD_F64_W8) : (w8 ? BUILD_F32_W8 : BUILD_F32_W4);
    const Build& bd = builds[p.build];
    p.NBmax = NBmax; p.PCcov = PCcov;
    p.ws_stride = bd.workspace_per_wg(NBmax, PCcov);
    p.state_words = bd.state_words();
    int grid = std::min(T, num_cu * (f64 ? 2 : in.wg_per_cu));
    p.smem = bd.shared_bytes(D, NBmax);
    if (p.smem > 160 * 1024) return false;
    if (w8 || (f64 && !d4)) grid = std::min(grid, num_cu);
    // teams (fp64 kernels, 8-wave build): with few large tiles, G workgroups run every tile together (gpsat_kernels_f64.hip)
    int team = 1;
    if (f64 && !d4 && NBmax >= 64 && 2 * T <= num_cu) team = std::min(16, num_cu / T);
    if (k.team.set) { if (f64 && !d4) team = std::max(1, std::min(32, k.team.v)); }
    if (in.solo) team = 1;
    if (team > 1) grid = std::min(T, std::max(1, num_cu / team)) * team;
    // cooperative tiles (fp32 kernels): a workgroup without a tile helps a running one (gpsat_coop.h).  With fewer tiles than
    // resident workgroups the launch is widened by the helpers the large tiles can use.
    bool coop = !f64;
    p.coop_min_nb = 12; p.coop_hdiv = 12; p.coop_force = 0;
    if (k.coop.set) {                                            // developer: 0 = off, 2 = cooperative code path always
        coop = coop && k.coop.v != 0;
        p.coop_force = k.coop.v == 2;
    }
    if (k.coop_xcd.set) p.coop_force |= (k.coop_xcd.v & 3) << 2;   // developer: 1 same-XCD helpers only, 2 others only
    if (k.coop_min_nb.set) p.coop_min_nb = std::max(2, k.coop_min_nb.v);
    if (k.coop_hdiv.set) p.coop_hdiv = std::max(1, k.coop_hdiv.v);
    // Helpers must be capacity that would otherwise idle.  8-wave build: one workgroup per CU, a workgroup without a tile
    // leaves its CU empty -- always on.  4-wave build (two workgroups per CU): an idle workgroup's CU-mate already runs 1.4 x
    // faster alone, and a helper takes that back (measured on BASELINE configs[1]: the helped tail is 2 % SLOWER) -- off; a
    // launch with fewer tiles than CUs runs the 8-wave build anyway, widened to at most one workgroup per CU.
    if (coop && !w8) coop = false;
    if (coop) {
        const int cap = num_cu;
        long long want = grid;
        for (int t = 0; t < T && want < cap; ++t) {
            const int nb = (int)((in.obs_off[t + 1] - in.obs_off[t] + bs - 1) / bs);
            if (nb >= p.coop_min_nb) want += std::min(7, std::max(1, nb / p.coop_hdiv));
        }
        if (T < cap) grid = (int)std::min<long long>(cap, want);
    }
    if (k.grid.set) grid = std::max(1, std::min(grid, k.grid.v));   // developer: fewer resident workgroups
    p.grid = grid; p.team = team; p.coop = coop;
    // ---- time slicing of the optimisation (fp32): with few tiles per resident workgroup, whole tiles as the scheduling unit
    // leave the GPU half empty while the last ones finish (4096 tiles on 512 workgroups: 8 % of the launch).  Tiles of
    // similar cost are therefore served in slices of ~4 evaluations of a 512-point tile (both precisions); a batch whose largest tile
    // dominates keeps the largest-first run-to-completion order (its critical path must not wait in a queue).
    int seg_cost = 0;
    if (in.optimiser != GPSAT_OPT_NONE && in.max_iter > 0) {
        double sum_cost = 0.0, max_cost = 0.0;
        for (int t = 0; t < T; ++t) {
            const double nb = (double)((in.obs_off[t + 1] - in.obs_off[t] + bs - 1) / bs);
            sum_cost += nb * nb * nb;
            max_cost = std::max(max_cost, nb * nb * nb);
        }
        const double tiles_per_wg = (double)T / grid;
        if (T > grid && max_cost * 4.0 * grid <= sum_cost && tiles_per_wg <= 64.0) seg_cost = 4 * (512 / bs) * (512 / bs) * (512 / bs);
        // developer / tests: slice length in NB^3 units (0 = off, 1 = every evaluation), whatever the batch looks like
        if (k.seg.set) seg_cost = std::max(0, k.seg.v);
        if (in.unsliced || team > 1) seg_cost = 0;
    }
    p.seg_cost = seg_cost;
    p.ring_cap = 0;
    if (seg_cost > 0) {
        size_t cap = 1; while (cap < (size_t)T + (size_t)grid + 1) cap <<= 1;
        p.ring_cap = cap;
    }
    // ---- deferred predictions (fp32 4-wave build, time-sliced, no full covariance): a tile that finishes while others wait
    // leaves its prediction in a snapshot slot for the workgroups that idle at the end of the launch (gpsat_ring.h).  One slot
    // per tile up to a fixed budget; tiles past it predict inline.
    p.pq_slots = 0; p.pq_stride = 0;
    if (seg_cost > 0 && bd.pq_floats_per_slot && !in.want_cov && in.has_pred) {
        p.pq_stride = bd.pq_floats_per_slot(D, NBmax);
        const size_t budget = (size_t)5 << 29;                    // 2.5 GiB: every tile of a 4096-tile launch of N = 500
        long long slots = std::min<long long>(T, (long long)(budget / (p.pq_stride * sizeof(float))));
        // developer / tests: 0 = every prediction inline, n = at most n snapshot slots
        if (k.defer.set) slots = std::min<long long>(slots, std::max(0, k.defer.v));
        p.pq_slots = (int)slots;
    }
    return true;
}

// gpsat_fit_predict_batch_mean's own checks (behind check_batch, which has seen T, D, dtype, kernel and the metadata pointers): a
// pure function of host data like plan_tiles, reached by tests through its exported symbol.  GPSAT_OK, or GPSAT_EINVAL with the
// reason in *why (a string literal).  GPSAT_MEAN_ZERO asks nothing of the batch: it is gpsat_fit_predict_batch.
int check_mean(const gpsat_batch* b, const gpsat_mean* m, const char** why) {
    *why = nullptr;
    if (m->kind != GPSAT_MEAN_ZERO && m->kind != GPSAT_MEAN_CONSTANT) { *why = "mean: unknown kind (GPSAT_MEAN_ZERO or GPSAT_MEAN_CONSTANT)"; return GPSAT_EINVAL; }
    for (int i = 0; i < 7; ++i)
        if (m->reserved[i] != 0) { *why = "mean: reserved words must be 0"; return GPSAT_EINVAL; }
    if (m->kind == GPSAT_MEAN_ZERO) return GPSAT_OK;
    if (b->dtype != GPSAT_F64) { *why = "a constant mean (GPSAT_MEAN_CONSTANT) is built for GPSAT_F64 only"; return GPSAT_EINVAL; }
    if (b->kernel == GPSAT_KERNEL_RQ) { *why = "a constant mean (GPSAT_MEAN_CONSTANT) is not built for GPSAT_KERNEL_RQ: H would be D + 4"; return GPSAT_EINVAL; }
    if (b->D > 3) { *why = "a constant mean (GPSAT_MEAN_CONSTANT) is built for D <= 3: H = D + 3 parameters, at most 6"; return GPSAT_EINVAL; }
    const int H = b->D + 3;
    for (int t = 0; t < b->T; ++t) {
        const double c0 = b->theta0[(size_t)t * H + H - 1];
        if (!(c0 - c0 == 0.0)) { *why = "theta0 of the constant mean (the last parameter) must be finite"; return GPSAT_EINVAL; }
    }
    return GPSAT_OK;
}

// gpsat_fit_predict_batch_noise's own checks (behind check_batch, which has seen T, D, dtype, kernel, the metadata pointers and
// that obs_off is a valid offset table): a pure function of host data like check_mean, reached by tests through its exported
// symbol.  GPSAT_OK, or GPSAT_EINVAL with the reason in why[why_len] (the entry that fails is named: no string literal will
// do).  obs_var == NULL asks nothing of the batch: it is gpsat_fit_predict_batch.  Device mode: obs_var is not read, as y is not.
int check_noise(const gpsat_batch* b, const gpsat_noise* nz, char* why, size_t why_len) {
    if (why_len > 0) why[0] = 0;
    if (!nz) { std::snprintf(why, why_len, "gpsat_fit_predict_batch_noise: noise is NULL"); return GPSAT_EINVAL; }
    for (int i = 0; i < 8; ++i)
        if (nz->reserved[i] != 0) { std::snprintf(why, why_len, "noise: reserved words must be 0"); return GPSAT_EINVAL; }
    if (!nz->obs_var) return GPSAT_OK;
    if (b->dtype != GPSAT_F64) { std::snprintf(why, why_len, "noise variances per observation (obs_var) are built for GPSAT_F64 only"); return GPSAT_EINVAL; }
    if (b->kernel == GPSAT_KERNEL_RQ) { std::snprintf(why, why_len, "noise variances per observation (obs_var) are not built for GPSAT_KERNEL_RQ"); return GPSAT_EINVAL; }
    if (b->memory != GPSAT_MEM_HOST) return GPSAT_OK;
    const double* v = static_cast<const double*>(nz->obs_var);
    for (int t = 0; t < b->T; ++t)
        for (int64_t i = b->obs_off[t]; i < b->obs_off[t + 1]; ++i)
            if (!(v[i] >= 0.0) || !(v[i] - v[i] == 0.0)) {
                std::snprintf(why, why_len, "obs_var must be finite and not negative: tile %d, row %lld is %g", t, (long long)(i - b->obs_off[t]), v[i]);
                return GPSAT_EINVAL;
            }
    return GPSAT_OK;
}

// gpsat_fit_predict_batch_grad's own checks (behind check_batch, which has seen T, D, dtype, kernel, the metadata pointers and
// that pred_off is a valid offset table): a pure function of host data like check_noise, reached by tests through its exported
// symbol.  GPSAT_OK, or GPSAT_EINVAL with the reason in why[why_len].  The outputs are not dereferenced in either memory mode.
int check_pred_grad(const gpsat_batch* b, const gpsat_pred_grad* pg, char* why, size_t why_len) {
    if (why_len > 0) why[0] = 0;
    if (!pg) { std::snprintf(why, why_len, "gpsat_fit_predict_batch_grad: pred_grad is NULL"); return GPSAT_EINVAL; }
    for (int i = 0; i < 8; ++i)
        if (pg->reserved[i] != 0) { std::snprintf(why, why_len, "pred_grad: reserved words must be 0"); return GPSAT_EINVAL; }
    if (b->dtype != GPSAT_F64) { std::snprintf(why, why_len, "the gradient of the posterior mean (pred_grad) is built for GPSAT_F64 only"); return GPSAT_EINVAL; }
    if (b->kernel == GPSAT_KERNEL_MATERN12) {
        std::snprintf(why, why_len, "the gradient of the posterior mean (pred_grad) does not exist for GPSAT_KERNEL_MATERN12: the process is not mean-square differentiable");
        return GPSAT_EINVAL;
    }
    if (b->kernel == GPSAT_KERNEL_RQ) { std::snprintf(why, why_len, "the gradient of the posterior mean (pred_grad) is not built for GPSAT_KERNEL_RQ"); return GPSAT_EINVAL; }
    if (b->cov_off || b->f_cov) {
        std::snprintf(why, why_len, "pred_grad and the full covariance cannot be asked for in the same call: cov_off / f_cov must be NULL");
        return GPSAT_EINVAL;
    }
    if (b->pred_off[b->T] > 0) {
        if (!pg->f_grad) { std::snprintf(why, why_len, "pred_grad: f_grad is NULL"); return GPSAT_EINVAL; }
        if (!pg->f_grad_var) { std::snprintf(why, why_len, "pred_grad: f_grad_var is NULL"); return GPSAT_EINVAL; }
    }
    return GPSAT_OK;
}

// gpsat_fit_predict_batch_hess's own checks, as check_pred_grad: a pure function of host data behind check_batch, reached by
// tests through its exported symbol.  GPSAT_OK, or GPSAT_EINVAL with the reason in why[why_len].  No output is dereferenced.
int check_pred_hess(const gpsat_batch* b, const gpsat_pred_hess* ph, char* why, size_t why_len) {
    if (why_len > 0) why[0] = 0;
    if (!ph) { std::snprintf(why, why_len, "gpsat_fit_predict_batch_hess: pred_hess is NULL"); return GPSAT_EINVAL; }
    for (int i = 0; i < 7; ++i)
        if (ph->reserved[i] != 0) { std::snprintf(why, why_len, "pred_hess: reserved words must be 0"); return GPSAT_EINVAL; }
    if (b->dtype != GPSAT_F64) { std::snprintf(why, why_len, "the second derivatives of the posterior mean (pred_hess) are built for GPSAT_F64 only"); return GPSAT_EINVAL; }
    if (b->kernel == GPSAT_KERNEL_MATERN12 || b->kernel == GPSAT_KERNEL_MATERN32) {
        std::snprintf(why, why_len, "the second derivatives of the posterior mean (pred_hess) do not exist for GPSAT_KERNEL_MATERN%s: "
                      "the derivative process is not mean-square differentiable", b->kernel == GPSAT_KERNEL_MATERN12 ? "12" : "32");
        return GPSAT_EINVAL;
    }
    if (b->kernel != GPSAT_KERNEL_RBF && b->kernel != GPSAT_KERNEL_MATERN52) {
        std::snprintf(why, why_len, "the second derivatives of the posterior mean (pred_hess) are not built for kernel %d, only for GPSAT_KERNEL_RBF and GPSAT_KERNEL_MATERN52", (int)b->kernel);
        return GPSAT_EINVAL;
    }
    if (b->cov_off || b->f_cov) {
        std::snprintf(why, why_len, "pred_hess and the full covariance cannot be asked for in the same call: cov_off / f_cov must be NULL");
        return GPSAT_EINVAL;
    }
    if (ph->dims == 0) { std::snprintf(why, why_len, "pred_hess: dims is empty, it names no coordinate"); return GPSAT_EINVAL; }
    if (b->D < 32 && (ph->dims >> b->D) != 0) { std::snprintf(why, why_len, "pred_hess: dims names a coordinate >= D = %d", (int)b->D); return GPSAT_EINVAL; }
    bool lap = ph->f_lap || ph->f_lap_var;
    for (int a = 0; a < 4; ++a) {
        const double w = ph->lap_weight[a];
        if (!(w >= 0.0) || !(w <= 1.79769313486231570815e308)) { std::snprintf(why, why_len, "pred_hess: lap_weight[%d] is negative or not finite", a); return GPSAT_EINVAL; }
        if (w > 0.0 && !((ph->dims >> a) & 1u)) { std::snprintf(why, why_len, "pred_hess: lap_weight[%d] is set for a coordinate outside dims", a); return GPSAT_EINVAL; }
        lap = lap || w > 0.0;
    }
    if (!ph->f_grad != !ph->f_grad_var) { std::snprintf(why, why_len, "pred_hess: f_grad and f_grad_var are given together or not at all"); return GPSAT_EINVAL; }
    if (b->pred_off[b->T] > 0) {
        if (!ph->f_hess) { std::snprintf(why, why_len, "pred_hess: f_hess is NULL"); return GPSAT_EINVAL; }
        if (!ph->f_hess_var) { std::snprintf(why, why_len, "pred_hess: f_hess_var is NULL"); return GPSAT_EINVAL; }
        if (lap && !ph->f_lap) { std::snprintf(why, why_len, "pred_hess: f_lap is NULL, with a lap_weight or f_lap_var given"); return GPSAT_EINVAL; }
        if (lap && !ph->f_lap_var) { std::snprintf(why, why_len, "pred_hess: f_lap_var is NULL, with a lap_weight or f_lap given"); return GPSAT_EINVAL; }
    }
    return GPSAT_OK;
}

// The memo of evaluations of the fp32 tile kernels (KernelArgs::memo, gpsat_kernels.hip): bytes of device memory a batch of T
// tiles needs for it, 0 when the batch runs without one.  It serves the unbounded L-BFGS driver's line search only: no fp64
// batch (the key would be the fp64 theta), no Adam, no multi-start, nothing without an optimisation; `off`: the developer
// switched it off (GPSAT_DEBUG_EVAL_CACHE=0).  Kept apart from TilePlan, whose layout tests/test_abi.py mirrors.
size_t eval_cache_bytes(int T, int f64, int optimiser, int max_iter, int multistart, int off) {
    if (T <= 0 || f64 || optimiser != GPSAT_OPT_LBFGS || max_iter <= 0 || multistart || off) return 0;
    return (size_t)T * MEMO_WORDS * sizeof(unsigned);
}

}  // namespace gpsat
#endif
