// gpsat_glue_plan.h -- host side of gpsat_glue_keyed_batch, gpsat_glue_keyed_grad_batch and gpsat_glue_keyed_hess_batch: the argument checks, the key range of
// a call and the layout of the handle's buffers.  Plain C++ without a HIP call, in the manner of gpsat_bin_plan.h; the checks are exported like
// gpsat::check_noise (gpsat_plan.h), so that tests drive every refusal without a device.  Part of gpsat_capi.cpp's
// translation unit.
#ifndef GPSAT_GLUE_PLAN_H
#define GPSAT_GLUE_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "gpsat_hip.h"
#include "gpsat_key_runs_plan.h"

#ifndef GPSAT_GLUE_MAXVARS
#define GPSAT_GLUE_MAXVARS 4
#endif

namespace gpsat {

// The refusals of the keyed glues, in their order, under the entry point's name.  nvars: nullptr where the entry point
// has none.  have_in / have_out: every input (asked for with R > 0) / every output (with capacity > 0) is there.
inline int check_glue_keyed_common(const char* entry, int64_t R, int32_t ndim, const int32_t* nvars, double sigma,
                                   const double* sigma_rows, double max_dist, int64_t capacity, const int64_t* G, bool have_in,
                                   const char* no_in, bool have_out, const char* no_out, char* why, size_t why_len) {
    if (why_len > 0) why[0] = 0;
    auto bad = [&](const char* msg) { std::snprintf(why, why_len, "%s: %s", entry, msg); return GPSAT_EINVAL; };
    if (!G) return bad("G is NULL");
    if (R < 0 || capacity < 0) return bad("R and capacity must not be negative");
    if (R > 2147483647LL) return bad("more than 2^31-1 rows in one call");
    if (ndim < 1 || ndim > 2) return bad("ndim must be 1 or 2");
    if (nvars && (*nvars < 1 || *nvars > GPSAT_GLUE_MAXVARS)) return bad("nvars must be 1..4 (GPSAT_GLUE_MAXVARS)");
    if (!sigma_rows && (!(sigma > 0.0) || !std::isfinite(sigma))) return bad("sigma must be finite and positive when sigma_rows is NULL");
    if (max_dist != max_dist) return bad("max_dist is NaN (+inf or a value <= 0 switches the limit off)");
    if (R > 0 && !have_in) return bad(no_in);
    if (capacity > 0 && !have_out) return bad(no_out);
    return GPSAT_OK;
}

// Everything gpsat_glue_keyed_batch can refuse before it has counted the keys (the handle is the entry point's to check).
// GPSAT_OK, or GPSAT_EINVAL with the reason in why[why_len].  G is required whatever R is; the inputs with R > 0; the outputs
// with capacity > 0.
int check_glue_keyed(int64_t R, int32_t ndim, int32_t nvars, const int64_t* key, const double* pred, const double* xprt,
                     const double* vals, double sigma, const double* sigma_rows, double max_dist, int64_t capacity,
                     const int64_t* G, const int64_t* out_key, const int32_t* out_count, const double* out, char* why,
                     size_t why_len) {
    return check_glue_keyed_common("gpsat_glue_keyed_batch", R, ndim, &nvars, sigma, sigma_rows, max_dist, capacity, G,
                                   key && pred && xprt && vals, "key / pred / xprt / vals is NULL",
                                   out_key && out_count && out, "out_key / out_count / out is NULL", why, why_len);
}

// The same for gpsat_glue_keyed_grad_batch: one value column and its gradient, [ndim][R], instead of vals [nvars][R].
int check_glue_keyed_grad(int64_t R, int32_t ndim, const int64_t* key, const double* pred, const double* xprt, const double* val,
                          const double* grad, double sigma, const double* sigma_rows, double max_dist, int64_t capacity,
                          const int64_t* G, const int64_t* out_key, const int32_t* out_count, const double* out_val,
                          const double* out_grad, char* why, size_t why_len) {
    return check_glue_keyed_common("gpsat_glue_keyed_grad_batch", R, ndim, nullptr, sigma, sigma_rows, max_dist, capacity, G,
                                   key && pred && xprt && val && grad, "key / pred / xprt / val / grad is NULL",
                                   out_key && out_count && out_val && out_grad, "out_key / out_count / out_val / out_grad is NULL", why, why_len);
}

// The same for gpsat_glue_keyed_hess_batch: the value, its gradient [ndim][R] and its second derivatives [npair][R],
// npair = ndim (ndim + 1) / 2.
int check_glue_keyed_hess(int64_t R, int32_t ndim, const int64_t* key, const double* pred, const double* xprt, const double* val,
                          const double* grad, const double* hess, double sigma, const double* sigma_rows, double max_dist,
                          int64_t capacity, const int64_t* G, const int64_t* out_key, const int32_t* out_count,
                          const double* out_val, const double* out_grad, const double* out_hess, char* why, size_t why_len) {
    return check_glue_keyed_common("gpsat_glue_keyed_hess_batch", R, ndim, nullptr, sigma, sigma_rows, max_dist, capacity, G,
                                   key && pred && xprt && val && grad && hess, "key / pred / xprt / val / grad / hess is NULL",
                                   out_key && out_count && out_val && out_grad && out_hess,
                                   "out_key / out_count / out_val / out_grad / out_hess is NULL", why, why_len);
}

// After the keys are counted: the outputs must hold one record per distinct key.
int check_glue_capacity(int64_t capacity, int64_t G, char* why, size_t why_len) {
    if (why_len > 0) why[0] = 0;
    if (capacity >= G) return GPSAT_OK;
    std::snprintf(why, why_len, "gpsat_glue_keyed_batch: capacity %lld < G %lld", (long long)capacity, (long long)G);
    return GPSAT_EINVAL;
}

// The key that rows with a negative key are given on the device: one above the largest key of the call, so that they sort
// behind every group and the sort runs over the bits of the largest key only.  0: no row has a key >= 0.
inline unsigned long long glue_keyed_sentinel(int64_t R, const int64_t* key) {
    int64_t mx = -1;
    for (int64_t i = 0; i < R; ++i) mx = key[i] > mx ? key[i] : mx;
    return (unsigned long long)(mx + 1);       // mx <= 2^63 - 1: no overflow in 64 unsigned bits
}

// max_dist as the kernel takes it: the square, or a negative value when there is no limit (+inf, <= 0)
inline double glue_keyed_md2(double max_dist) {
    return (max_dist > 0.0 && std::isfinite(max_dist)) ? max_dist * max_dist : -1.0;
}

// Bytes of the handle's buffers and the offsets of what lies in them; keys, rows and runs are the stage's (runs_counts: n_groups [2]).
struct GlueKeyedLayout : KeyRunsLayout {
    // `in`: key [R] (int64), pred and xprt [ndim][R], vals [nvars][R], sigma_rows [R] (room reserved either way)
    size_t in_bytes, in_pred, in_xprt, in_vals, in_sigma;
};

inline GlueKeyedLayout glue_keyed_layout(int64_t R, int ndim, int nvars) {
    const size_t nR = (size_t)R;
    GlueKeyedLayout l = {};
    static_cast<KeyRunsLayout&>(l) = key_runs_layout(R);
    l.in_pred = nR * sizeof(int64_t);
    l.in_xprt = l.in_pred + (size_t)ndim * nR * sizeof(double);
    l.in_vals = l.in_xprt + (size_t)ndim * nR * sizeof(double);
    l.in_sigma = l.in_vals + (size_t)nvars * nR * sizeof(double);
    l.in_bytes = l.in_sigma + nR * sizeof(double);
    return l;
}

}  // namespace gpsat
#endif
