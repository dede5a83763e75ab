// gpsat_capi.cpp -- C ABI of libgpsat_hip.so (see include/gpsat_hip.h for the contract and the
// reference interfaces each entry point replaces).  Host-side responsibilities only: argument
// validation, device buffers owned by the handle, cost-sorted tile order, launch, copy-back.
// Every entry point reads as a sequence of named steps; what is pure host arithmetic lives in a HIP-free header of this
// translation unit, where it runs without a GPU (tests/test_abi.py, tests/cvfold_host_check.cpp, tests/select_bin_host_check.cpp):
//   gpsat_fit_predict_batch: check_batch / check_multistart / check_cv / check_mean / check_noise / check_pred_grad / check_pred_hess, plan_tiles (gpsat_plan.h), stage_batch, stage_cv,
//     stage_derived, setup_*, launch, fetch_batch / fetch_cv / fetch_derived, record_timing.
//   gpsat_fit_predict_batch_cv_refit (fit_predict_cv_refit) calls it twice: for the batch, and for the batch of its folds that
//     gpsat_cvfold.hip builds on the device from the tables of gpsat_cvfold.h (cvfold_tables, cvfold_derive, cvfold_pack):
//     cvr_stage_expand, cvr_derived_batch, cvr_unpack, cvr_scatter_fetch.
//   gpsat_fit_predict_batch_cv_joint / _cv_refit_joint: the same two with the folds' joint densities (check_cv_joint,
//     check_cv_joint_offsets; stage_cv / fetch_cv carry CvArgs::fold_lpd; cvr_joint_stage and cvr_joint_run around the derived batch).
//   gpsat_select_batch_ex (gpsat_select_plan.h): check -> cache hit? -> chunks -> stage -> bin (select_bin_table, optional) ->
//     boxes -> count -> scan -> fill -> unbin (select_unbin_indices, optional) -> fetch -> remember.
//   gpsat_bin_batch (gpsat_bin_plan.h): check -> layout, scales -> stage -> sort -> read counts -> stats -> fetch.
//   gpsat_glue_keyed_batch, gpsat_glue_keyed_grad_batch, gpsat_glue_keyed_hess_batch (gpsat_glue_plan.h): check, then
//     glue_keyed_run by order 0, 1, 2: key range, layout -> stage -> sort, run heads -> read the group count -> reduce -> fetch.
//   gpsat_project_batch / gpsat_track_batch (gpsat_prep_plan.h): check -> constants / layout -> stage (host mode) -> kernels
//     (tracks with groups: keys, the keyed glue's sort and run heads) -> fetch (host mode).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "gpsat_hip.h"
#include "gpsat_kernels.h"
#include "gpsat_plan.h"
#include "gpsat_cvfold.h"
#include "gpsat_select_plan.h"
#include "gpsat_key_runs_plan.h"
#include "gpsat_bin_plan.h"
#include "gpsat_glue_plan.h"
#include "gpsat_prep_plan.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(e_ == hipErrorOutOfMemory ? GPSAT_ENOMEM : GPSAT_EHIP,                    \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                       \
    } while (0)

// Developer knobs (GPSAT_DEBUG_*: grid size, slice length, cooperative-tile modes, team size, statistics) are read ONLY when
// GPSAT_DEVELOPER=1 is set in the environment: a stray GPSAT_DEBUG_* variable never changes what the shipped library does.
inline const char* dev_env(const char* name) {
    const char* d = std::getenv("GPSAT_DEVELOPER");
    if (!d || d[0] != '1' || d[1] != '\0') return nullptr;
    return std::getenv(name);
}

// the knobs of the launch plan, read once per call
gpsat::DevKnobs read_dev_knobs() {
    gpsat::DevKnobs k;
    auto read = [](const char* name, gpsat::Knob& kn) {
        if (const char* e = dev_env(name)) { kn.set = 1; kn.v = std::atoi(e); }
    };
    read("GPSAT_DEBUG_TEAM", k.team); read("GPSAT_DEBUG_COOP", k.coop); read("GPSAT_DEBUG_COOP_XCD", k.coop_xcd);
    read("GPSAT_DEBUG_COOP_MIN_NB", k.coop_min_nb); read("GPSAT_DEBUG_COOP_HDIV", k.coop_hdiv);
    read("GPSAT_DEBUG_GRID", k.grid); read("GPSAT_DEBUG_SEG", k.seg); read("GPSAT_DEBUG_DEFER", k.defer);
    return k;
}

// A device allocation that grows on demand and frees itself with its owner (the handle).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return GPSAT_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(GPSAT_ENOMEM, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
        }
        cap = want;
        return GPSAT_OK;
    }
};

// What one user of the keyed sort-and-run-heads stage (gpsat_key_runs.hip) holds on the device: the three buffers of
// gpsat_key_runs_plan.h and the stage's scratch.  bind: the stage's arrays of k.R rows, behind reserve() for that many rows.
struct KeyRunBufs {
    DevBuf keys, rows, runs, tmp;
    int reserve(const gpsat::KeyRunsLayout& l) {
        if (int rc = keys.reserve(l.keys_bytes)) return rc;
        if (int rc = rows.reserve(l.rows_bytes)) return rc;
        return runs.reserve(l.runs_bytes);
    }
    void bind(gpsat::KeyRuns& k) const {
        const gpsat::KeyRunsLayout l = gpsat::key_runs_layout(k.R);
        char* d_runs = static_cast<char*>(runs.p);
        k.keys = static_cast<unsigned long long*>(keys.p); k.keys_sorted = k.keys + k.R;
        k.rows = static_cast<unsigned*>(rows.p); k.perm = k.rows + k.R;
        k.starts = reinterpret_cast<unsigned*>(d_runs);
        k.counts = reinterpret_cast<long long*>(d_runs + l.runs_counts);
        k.n_runs = reinterpret_cast<unsigned*>(d_runs + l.runs_n_runs);
        k.flags = reinterpret_cast<unsigned char*>(d_runs + l.runs_flags);
    }
};

// Stream and events of a handle.  A base of gpsat_handle, so that they are destroyed AFTER the handle's members: the device
// buffers are freed first, then the events, then the stream.
struct HandleQueue {
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~HandleQueue() {
        for (int i = 0; i < 4; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace

struct gpsat_handle : HandleQueue {
    int device = 0;
    int num_cu = 0;
    int wg_per_cu = 2;
    char name[256] = {0};
    double last_kernel_ms = 0.0, last_total_ms = 0.0;
    // The two-call selection (gpsat_select_plan.h).  Its d_result points into sel.idx or sel.keys, buffers that a later call may
    // grow (and so free): that is safe only because begin_call, where every entry point starts its device work, ends the cache.
    gpsat::SelectCache selc;
    // device buffers (grown lazily, owned by the handle, freed by its destructor)
    DevBuf meta_i64, meta_f64, meta_misc, out_f64, out_i32, bulk_in, bulk_out, ws, prof, ring, state, coop, pq;
    DevBuf cv;                        // held-out predictions: fold tables, then the three outputs [sumN] each
    DevBuf cvr_cov;                   // refitted cross-validation with the joint density: cov_off, the derived batch's f_cov, sn2, residuals, lpd
    DevBuf cvr_tab, cvr_in, cvr_out;  // refitted cross-validation: fold tables, the derived batch's inputs, its predictions (+ host mode: cv outputs)
    DevBuf derived;                   // gpsat_fit_predict_batch_grad / _hess, host mode: their outputs, one behind the other (stage_derived)
    DevBuf memo;                      // 64 bytes of developer statistics, then the evaluation memo [T][MEMO_WORDS] (fp32 L-BFGS batches)
    DevBuf ms;                        // multi-start: [T][MS_WORDS] state, [T][S-1][H] starts, [T][S] objectives
    // gpsat_select_batch_ex.  gpsat_smooth_batch and gpsat_glue_batch stage their inputs in sel.pts (glue: its segments in
    // sel.cnt) instead of buffers of their own: the post-processing follows the selection, whose tables are no longer needed
    // then, and no call leaves anything in the two for a later one (the selection cache holds neither).
    struct SelectBufs { DevBuf pts, refs, cnt, idx, box, perm, keys, tmp, ord, bnd; } sel;
    struct BinBufs { DevBuf in, vals, out; KeyRunBufs kr; } bin;             // gpsat_bin_batch (layout: gpsat_bin_plan.h)
    // gpsat_glue_keyed_batch (layout: gpsat_glue_plan.h); ev: after the sort, after the run heads, in front of the reduce
    // kernel; ms: the last call's sort, run detection and reduce (gpsat_glue_keyed_timing)
    struct GlueBufs {
        DevBuf in, out;
        KeyRunBufs kr;
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        double ms[3] = {0.0, 0.0, 0.0};
        ~GlueBufs() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    } glue;
    struct PrepBufs { DevBuf in, out; KeyRunBufs kr; } prep;                 // gpsat_project_batch / gpsat_track_batch (layout: gpsat_prep_plan.h)
    float* dump_dev = nullptr;         // diagnostic build (-DGPSAT_DUMP): caller's device buffer for per-tile factor dumps
    size_t dump_stride = 0;
    unsigned long long prof_host[64 + 8 * 1024 + 4096] = {0};     // counters + event trace + per-workgroup start / end / first empty ring / CU (diagnostic build)
};

namespace {

// Every entry point that uses the device starts its device work here.  Any call on the handle ends a pending two-call
// selection (the selection's own sizes call sets it up again at its end).
int begin_call(gpsat_handle* h) {
    h->selc.forget();
    HIP_TRY(hipSetDevice(h->device));
    return GPSAT_OK;
}

// Kernel time ev[1]..ev[2] and total time ev[t0]..ev[t1] of the call that just synchronised the stream.
int record_timing(gpsat_handle* h, int t0 = 0, int t1 = 3) {
    float km = 0.f, tm = 0.f;
    HIP_TRY(hipEventElapsedTime(&km, h->ev[1], h->ev[2]));
    HIP_TRY(hipEventElapsedTime(&tm, h->ev[t0], h->ev[t1]));
    h->last_kernel_ms = km;
    h->last_total_ms = tm;
    return GPSAT_OK;
}

// The two-pass idiom of the sort-based steps (select_bin_rows, select_unbin, bin_cell_stats; key_runs behind bin_sort_rows and glue_keyed_sort): step(nullptr, bytes)
// only reports the scratch it needs, step(scratch, bytes) runs.  `mark`, when given, is recorded between the two: after the
// reservation, so that an allocation is not timed as kernel time.
template <class Step>
int run_with_temp(gpsat_handle* h, DevBuf& tmp, const char* what, hipEvent_t mark, Step step) {
    auto failed = [&](hipError_t e) { return fail(e == hipErrorOutOfMemory ? GPSAT_ENOMEM : GPSAT_EHIP, std::string(what) + ": " + hipGetErrorString(e)); };
    size_t bytes = 0;
    hipError_t e = step(nullptr, bytes);
    if (e != hipSuccess) return failed(e);
    if (int rc = tmp.reserve(std::max<size_t>(bytes, 16))) return rc;
    if (mark) HIP_TRY(hipEventRecord(mark, h->stream));
    e = step(tmp.p, bytes);
    return e != hipSuccess ? failed(e) : GPSAT_OK;
}

// The counts the keyed sort-and-run-heads stage left on the device, on the host: {groups, rows in them}.  Synchronises.
int read_key_run_counts(gpsat_handle* h, const gpsat::KeyRuns& k, long long info[2]) {
    HIP_TRY(hipMemcpyAsync(info, k.counts, 2 * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GPSAT_OK;
}

// Hyper-parameters per tile: D + 2, or D + 3 with the RationalQuadratic kernel's alpha behind them (gpsat_n_hyper).  Read
// behind check_batch only, which refuses the arguments it answers with 0.  `mean`: GPSAT_MEAN_* of the call
// (gpsat_fit_predict_batch_mean; a constant mean is one more parameter, last), behind gpsat::check_mean.
int n_hyper(const gpsat_batch* b, int mean = GPSAT_MEAN_ZERO) { return gpsat_n_hyper_mean(b->kernel, b->D, mean); }

struct BatchDims { long long sumN = 0, sumP = 0, sumC = 0, sumM = 0, maxN = 0, maxP = 0; bool want_cov = false; };

// The argument checks the dense and the sparse entry point share, in the order of the dense one, up to the CSR offsets
// (largest tile and sums into `d`).  `f64_only`: the sparse entry point's dtype rule.  T == 0 is the caller's early return.
int check_batch(const gpsat_batch* b, bool f64_only, BatchDims& d) {
    if (b->T < 0) return fail(GPSAT_EINVAL, "T < 0");
    if (b->D < 1 || b->D > 4) return fail(GPSAT_EINVAL, "D must be 1..4 in this build");
    if (f64_only && b->dtype != GPSAT_F64) return fail(GPSAT_EINVAL, "sparse GP experts are built for GPSAT_F64 only");
    if (b->dtype != GPSAT_F32 && b->dtype != GPSAT_F64) return fail(GPSAT_EINVAL, "unknown dtype");
    if (b->kernel < 0 || b->kernel > GPSAT_KERNEL_RQ) return fail(GPSAT_EINVAL, "unknown kernel id");
    if (b->optimiser < 0 || b->optimiser > 2) return fail(GPSAT_EINVAL, "unknown optimiser id");
    if (b->memory != GPSAT_MEM_HOST && b->memory != GPSAT_MEM_DEVICE) return fail(GPSAT_EINVAL, "bad memory flag");
    if (!b->obs_off || !b->pred_off || !b->theta0 || !b->lo || !b->hi || !b->trainable)
        return fail(GPSAT_EINVAL, "metadata pointer is NULL");
    if (!b->theta || !b->nll || !b->status || !b->n_eval) return fail(GPSAT_EINVAL, "output pointer is NULL");
    // ---- validate CSR offsets, find the largest tile
    if (b->obs_off[0] != 0 || b->pred_off[0] != 0) return fail(GPSAT_EINVAL, "offsets must start at 0");
    for (int t = 0; t < b->T; ++t) {
        const long long n = b->obs_off[t + 1] - b->obs_off[t], p = b->pred_off[t + 1] - b->pred_off[t];
        if (n < 0 || p < 0) return fail(GPSAT_EINVAL, "offsets must be non-decreasing");
        d.maxN = std::max(d.maxN, n);
    }
    d.sumN = b->obs_off[b->T]; d.sumP = b->pred_off[b->T];
    return GPSAT_OK;
}

// GPSAT_KERNEL_RQ is built into gpsat_fit_predict_batch alone, in fp64 and for D <= 3 (H = D + 3 <= 6, the optimiser state's
// HMAX).  `entry`: nullptr for that call, else the name of the entry point that refuses the kernel.
int check_rq(const gpsat_batch* b, const char* entry) {
    if (b->kernel != GPSAT_KERNEL_RQ) return GPSAT_OK;
    const std::string who = "RationalQuadratic (GPSAT_KERNEL_RQ) ";
    if (entry) return fail(GPSAT_EINVAL, who + "is built for gpsat_fit_predict_batch only, not for " + entry);
    if (b->dtype != GPSAT_F64) return fail(GPSAT_EINVAL, who + "is built for GPSAT_F64 only");
    if (b->D > 3) return fail(GPSAT_EINVAL, who + "is built for D <= 3: H = D + 3 parameters, at most 6");
    return GPSAT_OK;
}

// ... and the checks that follow the offsets in both: data pointers against the sums, theta0
// (a constant mean, the last parameter, may be any finite value: gpsat::check_mean has looked at it)
int check_batch_data(const gpsat_batch* b, const BatchDims& d, int mean = GPSAT_MEAN_ZERO) {
    if (d.sumN > 0 && (!b->X || !b->y)) return fail(GPSAT_EINVAL, "X / y is NULL");
    if (d.sumP > 0 && (!b->Xs || !b->f_mean || !b->f_var || !b->y_var)) return fail(GPSAT_EINVAL, "prediction pointer is NULL");
    const size_t H = (size_t)n_hyper(b, mean);
    for (size_t e = 0; e < (size_t)b->T * H; ++e) {
        if (mean == GPSAT_MEAN_CONSTANT && e % H == H - 1) continue;
        if (!(b->theta0[e] > 0.0) || !std::isfinite(b->theta0[e])) return fail(GPSAT_EINVAL, "theta0 must be finite and positive");
    }
    return GPSAT_OK;
}

// x clipped into the bounds of the trainable parameters, n rows of H per tile (SciPy clips x0 into the bounds,
// _minimize_lbfgsb; the further starts likewise: L-BFGS-B works inside the box only)
std::vector<double> clip_to_bounds(const gpsat_batch* b, const double* x, int n) {
    const int T = b->T, H = n_hyper(b);
    std::vector<double> out(x, x + (size_t)T * n * H);
    for (int t = 0; t < T; ++t)
        for (int k = 0; k < n; ++k)
            for (int i = 0; i < H; ++i)
                if (b->trainable[i]) {
                    double& v = out[((size_t)t * n + k) * H + i];
                    v = std::min(std::max(v, b->lo[(size_t)t * H + i]), b->hi[(size_t)t * H + i]);
                }
    return out;
}

// ---- multi-start bounded L-BFGS-B (gpsat_fit_predict_batch_ms): checks, then theta0 and the starts clipped into the box
// when the optimiser runs at all (`ms_on`)
int check_multistart(const gpsat_batch* b, const gpsat_multistart* ms, bool ms_on, std::vector<double>& theta0_clipped,
                     std::vector<double>& starts_clipped) {
    const int T = b->T, H = n_hyper(b), S = ms->n_starts;
    if (S < 1) return fail(GPSAT_EINVAL, "multistart: n_starts must be >= 1");
    if (ms->transform != GPSAT_TRANSFORM_LOG) return fail(GPSAT_EINVAL, "multistart: unknown transform (GPSAT_TRANSFORM_LOG only)");
    if (S > 1 && !ms->starts) return fail(GPSAT_EINVAL, "multistart: starts is NULL with n_starts > 1");
    if (b->optimiser == GPSAT_OPT_ADAM) return fail(GPSAT_EINVAL, "multistart: the optimiser must be L-BFGS-B or none");
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < H; ++i) {
            if (!b->trainable[i]) continue;
            const double lo = b->lo[(size_t)t * H + i], hi = b->hi[(size_t)t * H + i];
            if (!(lo > 0.0) || !(hi > 0.0) || !(lo <= hi))
                return fail(GPSAT_EINVAL, "multistart: the bounds of a trainable parameter must be positive with lo <= hi (log transform)");
            if (S > 1 && (!std::isfinite(lo) || !std::isfinite(hi)))
                return fail(GPSAT_EINVAL, "multistart: restarts require that all bounds are finite");
        }
    if (S > 1)
        for (size_t e = 0; e < (size_t)T * (S - 1) * H; ++e)
            if (!(ms->starts[e] > 0.0) || !std::isfinite(ms->starts[e]))
                return fail(GPSAT_EINVAL, "multistart: starts must be finite and positive");
    if (ms_on) theta0_clipped = clip_to_bounds(b, b->theta0, 1);
    if (ms_on && S > 1) starts_clipped = clip_to_bounds(b, ms->starts, S - 1);
    return GPSAT_OK;
}

// ---- held-out predictions (gpsat_fit_predict_batch_cv).  The caller's labels as the tables the kernel reads, all int32 in one
// host vector (one copy): pair_off [T+1], fold_off [T+1], fold_ptr [F+1], fold_a [F], fold_rows [R], row_fold [sumN],
// row_pos [sumN], pairs.  Folds of a tile are numbered by ascending label, a fold's rows keep the order of the tile.
struct CvTables {
    std::vector<int> all;
    size_t o_pair_off = 0, o_fold_off = 0, o_fold_ptr = 0, o_fold_a = 0, o_fold_rows = 0, o_row_fold = 0, o_row_pos = 0, o_pairs = 0;
};

int check_cv(const gpsat_batch* b, const gpsat_cv* cv, const BatchDims& d, CvTables& tb) {
    if (b->dtype != GPSAT_F64) return fail(GPSAT_EINVAL, "held-out predictions are built for GPSAT_F64 only");
    if (b->cov_off || b->f_cov) return fail(GPSAT_EINVAL, "held-out predictions and the full covariance cannot be asked for in the same call: cov_off / f_cov must be NULL");
    if (!cv->cv_mean || !cv->cv_f_var) return fail(GPSAT_EINVAL, "gpsat_cv: cv_mean / cv_f_var is NULL");
    const int T = b->T, gmax = gpsat_max_cv_fold(b->dtype, b->D);
    const size_t sumN = (size_t)d.sumN;
    std::vector<int> pair_off(T + 1, 0), fold_off(T + 1, 0), fold_ptr(1, 0), fold_a, fold_rows, row_fold(sumN, -1), row_pos(sumN, 0), pairs;
    std::vector<int> idx;
    std::vector<unsigned char> mark;
    for (int t = 0; t < T; ++t) {
        const long long o0 = b->obs_off[t];
        const int N = (int)(b->obs_off[t + 1] - o0), NB = (N + 15) / 16;
        const int32_t* lab = cv->fold ? cv->fold + o0 : nullptr;
        idx.clear();
        for (int i = 0; i < N; ++i) if (!lab || lab[i] >= 0) idx.push_back(i);
        if (lab) std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return lab[x] < lab[y]; });
        mark.assign((size_t)NB * NB, 0);
        int a_off = 0;
        for (size_t s0 = 0; s0 < idx.size();) {
            size_t s1 = s0 + 1;
            while (lab && s1 < idx.size() && lab[idx[s1]] == lab[idx[s0]]) ++s1;
            const int g = (int)(s1 - s0), f = (int)fold_ptr.size() - 1;
            if (g > gmax)
                return fail(GPSAT_EINVAL, "tile " + std::to_string(t) + ": fold " + std::to_string(lab[idx[s0]]) + " holds " + std::to_string(g) +
                                              " rows, at most " + std::to_string(gmax) + " are held out together (gpsat_max_cv_fold)");
            for (size_t k = s0; k < s1; ++k) {
                const int i = idx[k];
                row_fold[o0 + i] = f; row_pos[o0 + i] = (int)(k - s0);
                fold_rows.push_back(i);
                for (size_t k2 = s0; k2 <= k; ++k2) {
                    const int bi = i / 16, bj = idx[k2] / 16;      // rows of a fold ascend
                    mark[(size_t)std::max(bi, bj) * NB + std::min(bi, bj)] = 1;
                }
            }
            fold_a.push_back(g > 1 ? a_off : 0);
            if (g > 1) a_off += g * g;
            fold_ptr.push_back((int)fold_rows.size());
            s0 = s1;
        }
        for (int a = 0; a < NB; ++a)                                   // ascending a: the longest sums first
            for (int c = 0; c <= a; ++c)
                if (mark[(size_t)a * NB + c]) pairs.push_back((a << 16) | c);
        fold_off[t + 1] = (int)fold_ptr.size() - 1;
        pair_off[t + 1] = (int)pairs.size();
    }
    auto put = [&](const std::vector<int>& v, size_t& off) { off = tb.all.size(); tb.all.insert(tb.all.end(), v.begin(), v.end()); };
    put(pair_off, tb.o_pair_off); put(fold_off, tb.o_fold_off); put(fold_ptr, tb.o_fold_ptr); put(fold_a, tb.o_fold_a);
    put(fold_rows, tb.o_fold_rows); put(row_fold, tb.o_row_fold); put(row_pos, tb.o_row_pos); put(pairs, tb.o_pairs);
    return GPSAT_OK;
}

// The joint density's extension struct (both flavours), in front of everything else; and its fold_off against the count's
// (`who`: the struct's name in messages, as check_cv_refit names its own).
int check_cv_joint(const gpsat_cv_joint* jt, const char* entry) {
    const std::string who = std::string(entry) + ": ";
    if (!jt) return fail(GPSAT_EINVAL, who + "NULL gpsat_cv_joint");
    if (!jt->fold_off) return fail(GPSAT_EINVAL, who + "gpsat_cv_joint: fold_off is NULL");
    if (!jt->fold_lpd) return fail(GPSAT_EINVAL, who + "gpsat_cv_joint: fold_lpd is NULL");
    for (int i = 0; i < 8; ++i)
        if (jt->reserved[i] != 0) return fail(GPSAT_EINVAL, who + "gpsat_cv_joint: reserved[" + std::to_string(i) + "] must be 0");
    return GPSAT_OK;
}

template <class Off>
int check_cv_joint_offsets(const gpsat_cv_joint* jt, int T, const Off* fold_off) {
    for (int t = 0; t <= T; ++t)
        if (jt->fold_off[t] != (int64_t)fold_off[t])
            return fail(GPSAT_EINVAL, "gpsat_cv_joint: fold_off[" + std::to_string(t) + "] = " + std::to_string(jt->fold_off[t]) +
                                          " differs from gpsat_cv_refit_count's " + std::to_string((int64_t)fold_off[t]));
    return GPSAT_OK;
}

// The fold tables to the device; the outputs in the handle's buffer (host mode, or no cv_y_var) or the caller's device arrays.
int stage_cv(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv* cv, const gpsat_cv_joint* jt, const BatchDims& d, const CvTables& tb,
             gpsat::CvArgs& ca) {
    const size_t nint = (tb.all.size() + 1) & ~size_t(1), sumN = (size_t)d.sumN;
    const size_t F = jt ? tb.o_fold_a - tb.o_fold_ptr - 1 : 0;       // the joint density: one double per fold behind the outputs
    int rc;
    if ((rc = h->cv.reserve(nint * sizeof(int) + (3 * std::max<size_t>(sumN, 1) + F) * sizeof(double)))) return rc;
    int* base = static_cast<int*>(h->cv.p);
    HIP_TRY(hipMemcpyAsync(base, tb.all.data(), tb.all.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    ca.pair_off = base + tb.o_pair_off; ca.pairs = base + tb.o_pairs; ca.fold_off = base + tb.o_fold_off;
    ca.fold_ptr = base + tb.o_fold_ptr; ca.fold_rows = base + tb.o_fold_rows; ca.fold_a = base + tb.o_fold_a;
    ca.row_fold = base + tb.o_row_fold; ca.row_pos = base + tb.o_row_pos;
    double* out = reinterpret_cast<double*>(base + nint);
    const bool dev = b->memory == GPSAT_MEM_DEVICE;
    ca.mean = dev ? static_cast<double*>(cv->cv_mean) : out;
    ca.f_var = dev ? static_cast<double*>(cv->cv_f_var) : out + sumN;
    ca.y_var = dev && cv->cv_y_var ? static_cast<double*>(cv->cv_y_var) : out + 2 * sumN;
    ca.fold_lpd = F ? out + 3 * std::max<size_t>(sumN, 1) : nullptr;
    return GPSAT_OK;
}

int fetch_cv(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv* cv, const gpsat_cv_joint* jt, const BatchDims& d, const gpsat::CvArgs& ca) {
    if (ca.fold_lpd)                                  // host memory in either mode
        HIP_TRY(hipMemcpyAsync(jt->fold_lpd, ca.fold_lpd, (size_t)jt->fold_off[b->T] * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (b->memory != GPSAT_MEM_HOST || d.sumN == 0) return GPSAT_OK;
    void* const host[3] = {cv->cv_mean, cv->cv_f_var, cv->cv_y_var};
    const double* const dev[3] = {ca.mean, ca.f_var, ca.y_var};
    for (int i = 0; i < 3; ++i)
        if (host[i]) HIP_TRY(hipMemcpyAsync(host[i], dev[i], (size_t)d.sumN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return GPSAT_OK;
}

// The derived outputs of a call: the two of gpsat_fit_predict_batch_grad, or the (up to) six of gpsat_fit_predict_batch_hess.
// Of each one asked for: the caller's pointer, the kernel's pointer, the byte count.
struct DerivedOuts {
    struct { void* user; double** dev; size_t bytes; } o[6];
    int n = 0;
    void add(void* user, double*& dev, size_t bytes) { o[n++] = {user, &dev, bytes}; }
};

// Fill GradArgs or HessArgs (kernel parameters: their layouts are the kernels') from the caller's struct.  The kernel writes
// into the caller's device memory, or (host mode) into the handle's buffer, one output behind the other, which fetch_derived
// copies back behind the launch: device mode returns host mode's bits.
int stage_derived(gpsat_handle* h, const gpsat_batch* b, const BatchDims& d, const gpsat_pred_grad* pg, const gpsat_pred_hess* ph,
                  gpsat::GradArgs& ga, gpsat::HessArgs& ha, DerivedOuts& t) {
    const size_t grad_bytes = (size_t)d.sumP * b->D * sizeof(double);
    if (pg) {
        t.add(pg->f_grad, ga.f_grad, grad_bytes);
        t.add(pg->f_grad_var, ga.f_grad_var, grad_bytes);
    }
    if (ph) {
        const int m = __builtin_popcount(ph->dims);
        ha.dims = ph->dims;
        ha.npair = m * (m + 1) / 2;
        bool lap = ph->f_lap || ph->f_lap_var;
        for (int k = 0; k < 4; ++k) { ha.lap_w[k] = ph->lap_weight[k]; lap = lap || ph->lap_weight[k] > 0.0; }
        const size_t pair_bytes = (size_t)d.sumP * ha.npair * sizeof(double), lap_bytes = (size_t)d.sumP * sizeof(double);
        t.add(ph->f_hess, ha.f_hess, pair_bytes);
        t.add(ph->f_hess_var, ha.f_hess_var, pair_bytes);
        if (lap) {
            t.add(ph->f_lap, ha.f_lap, lap_bytes);
            t.add(ph->f_lap_var, ha.f_lap_var, lap_bytes);
        }
        if (ph->f_grad) {
            t.add(ph->f_grad, ha.f_grad, grad_bytes);
            t.add(ph->f_grad_var, ha.f_grad_var, grad_bytes);
        }
    }
    const bool host = b->memory == GPSAT_MEM_HOST;
    size_t total = 0, at = 0;
    for (int k = 0; k < t.n; ++k) total += t.o[k].bytes;
    if (host && t.n > 0)
        if (int rc = h->derived.reserve(std::max<size_t>(total, 16))) return rc;
    for (int k = 0; k < t.n; ++k) {
        if (host) *t.o[k].dev = reinterpret_cast<double*>(static_cast<char*>(h->derived.p) + at);
        else *t.o[k].dev = static_cast<double*>(d.sumP > 0 ? t.o[k].user : h->ws.p);     // sum P = 0: nothing is written, so any valid address serves
        at += t.o[k].bytes;
    }
    return GPSAT_OK;
}

int fetch_derived(gpsat_handle* h, const gpsat_batch* b, const DerivedOuts& t) {
    if (b->memory != GPSAT_MEM_HOST) return GPSAT_OK;
    for (int k = 0; k < t.n; ++k)
        if (t.o[k].bytes > 0) HIP_TRY(hipMemcpyAsync(t.o[k].user, *t.o[k].dev, t.o[k].bytes, hipMemcpyDeviceToHost, h->stream));
    return GPSAT_OK;
}

// Device pointers of a staged batch.
struct Staged {
    const char *X = nullptr, *y = nullptr, *Xs = nullptr, *Z = nullptr;
    const double* obs_var = nullptr;  // [sumN] noise variances per observation (gpsat_fit_predict_batch_noise), or nullptr
    char *fm = nullptr, *fv = nullptr, *yv = nullptr, *cov = nullptr;
    long long* i64 = nullptr;         // [3][T+1]: obs_off, pred_off, then cov_off (dense) or z_off (sparse)
    double *f64 = nullptr, *out_f64 = nullptr;    // [3][T*H]: theta0, lo, hi; theta [T*H], nll [T], grad [T*H]
    int *out_i32 = nullptr, *queue = nullptr, *order = nullptr;   // status, n_eval, n_iter: [T] each; queue head; [T] tile order
    unsigned char* train = nullptr;
};

// Reserve the metadata, output, workspace and (host mode) bulk buffers, lay them out, record ev[0] and issue the host-to-device
// copies.  `off3`: the third offset table or nullptr; `Z`: the sparse path's inducing points (d.sumM rows) or nullptr;
// `obs_var`: the caller's noise variances per observation (d.sumN doubles, host or device as the bulk arrays) or nullptr.
// `order` is pageable host memory of the caller and must outlive the launch.
int stage_batch(gpsat_handle* h, const gpsat_batch* b, const BatchDims& d, const double* theta0, const std::vector<int>& order,
                const int64_t* off3, const void* Z, size_t ws_bytes, Staged& s, int mean = GPSAT_MEAN_ZERO,
                const void* obs_var = nullptr) {
    const int T = b->T, D = b->D, H = n_hyper(b, mean);
    const size_t esz = b->dtype == GPSAT_F64 ? sizeof(double) : sizeof(float);
    const size_t sumN = (size_t)d.sumN, sumP = (size_t)d.sumP, sumM = (size_t)d.sumM;
    int rc;
    if ((rc = h->meta_i64.reserve(3 * (size_t)(T + 1) * sizeof(long long)))) return rc;
    if ((rc = h->meta_f64.reserve(3 * (size_t)T * H * sizeof(double)))) return rc;
    if ((rc = h->meta_misc.reserve((size_t)T * sizeof(int) + 64 + 16))) return rc;
    if ((rc = h->out_f64.reserve(((size_t)T * H * 2 + (size_t)T) * sizeof(double)))) return rc;
    if ((rc = h->out_i32.reserve((size_t)T * 3 * sizeof(int)))) return rc;
    if ((rc = h->ws.reserve(ws_bytes))) return rc;
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    if (b->memory == GPSAT_MEM_HOST) {
        const size_t in_e = sumN * D + sumN + sumP * D + sumM * D + (obs_var ? sumN : 0);     // (obs_var: fp64 only, esz = 8)
        if ((rc = h->bulk_in.reserve(std::max<size_t>(in_e, 1) * esz))) return rc;
        if ((rc = h->bulk_out.reserve(std::max<size_t>(sumP * 3 + (size_t)d.sumC, 1) * esz))) return rc;
        char* base = static_cast<char*>(h->bulk_in.p);
        s.X = base; s.y = s.X + sumN * D * esz; s.Xs = s.y + sumN * esz; s.Z = s.Xs + sumP * D * esz;
        if (sumN > 0) {
            HIP_TRY(hipMemcpyAsync(base, b->X, sumN * D * esz, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(const_cast<char*>(s.y), b->y, sumN * esz, hipMemcpyHostToDevice, h->stream));
        }
        if (sumP > 0) HIP_TRY(hipMemcpyAsync(const_cast<char*>(s.Xs), b->Xs, sumP * D * esz, hipMemcpyHostToDevice, h->stream));
        if (Z) HIP_TRY(hipMemcpyAsync(const_cast<char*>(s.Z), Z, sumM * D * esz, hipMemcpyHostToDevice, h->stream));
        if (obs_var) {
            double* dv = reinterpret_cast<double*>(const_cast<char*>(s.Z) + sumM * D * esz);
            if (sumN > 0) HIP_TRY(hipMemcpyAsync(dv, obs_var, sumN * sizeof(double), hipMemcpyHostToDevice, h->stream));
            s.obs_var = dv;
        }
        s.fm = static_cast<char*>(h->bulk_out.p); s.fv = s.fm + sumP * esz; s.yv = s.fv + sumP * esz;
        if (d.want_cov) s.cov = s.yv + sumP * esz;
    } else {
        s.cov = static_cast<char*>(b->f_cov);
        s.X = static_cast<const char*>(b->X); s.y = static_cast<const char*>(b->y); s.Xs = static_cast<const char*>(b->Xs);
        s.Z = static_cast<const char*>(Z);
        s.obs_var = static_cast<const double*>(obs_var);
        s.fm = static_cast<char*>(b->f_mean); s.fv = static_cast<char*>(b->f_var); s.yv = static_cast<char*>(b->y_var);
    }
    s.i64 = static_cast<long long*>(h->meta_i64.p);
    s.f64 = static_cast<double*>(h->meta_f64.p);
    const int64_t* offs[3] = {b->obs_off, b->pred_off, off3};
    const double* pars[3] = {theta0, b->lo, b->hi};
    for (int i = 0; i < 3; ++i)
        if (offs[i]) HIP_TRY(hipMemcpyAsync(s.i64 + i * (T + 1), offs[i], (size_t)(T + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    for (int i = 0; i < 3; ++i)
        HIP_TRY(hipMemcpyAsync(s.f64 + i * (size_t)T * H, pars[i], (size_t)T * H * sizeof(double), hipMemcpyHostToDevice, h->stream));
    unsigned char* d_misc = static_cast<unsigned char*>(h->meta_misc.p);
    s.queue = reinterpret_cast<int*>(d_misc);                 // 16 bytes reserved
    s.train = d_misc + 16;                                    // 64 bytes reserved
    s.order = reinterpret_cast<int*>(d_misc + 16 + 64);
    HIP_TRY(hipMemsetAsync(s.queue, 0, 16, h->stream));
    HIP_TRY(hipMemcpyAsync(s.train, b->trainable, (size_t)H, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(s.order, order.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, h->stream));
    s.out_f64 = static_cast<double*>(h->out_f64.p);
    s.out_i32 = static_cast<int*>(h->out_i32.p);
    return GPSAT_OK;
}

// The fields KernelArgs and SgprArgs have in common: sizes, optimiser settings with their defaults, staged pointers.
template <class Args>
void fill_common_args(Args& a, const gpsat_batch* b, const Staged& s, int mean = GPSAT_MEAN_ZERO) {
    const int T = b->T, H = n_hyper(b, mean);
    const bool f64 = b->dtype == GPSAT_F64;
    a.T = T; a.kernel = b->kernel; a.optimiser = b->optimiser; a.max_iter = b->max_iter;
    a.max_ls = b->max_ls > 0 ? b->max_ls : 20;                                 // SciPy L-BFGS-B maxls
    // 0 = default (fp64: SciPy's factr*eps; fp32: its analogue above the fp32 noise floor); negative = criterion off
    a.ftol = b->ftol > 0 ? b->ftol : (b->ftol < 0 ? -1.0 : (f64 ? 2.220446049250313e-9 : 1e-6));
    a.gtol = b->gtol > 0 ? b->gtol : (b->gtol < 0 ? -1.0 : 1e-5);
    a.adam_lr = b->adam_lr > 0 ? b->adam_lr : 0.1;
    // relative resolution of the objective: fp32 rounding ~ cond(K) eps N reaches 2e-4 |f| on the reference's 1-D tutorial
    // tile (cond ~ 2e4, docs/notebooks/1d_local_expert_model_part_2.ipynb); fp64: rounding level only
    a.noise_rel = f64 ? 1e-12 : 1e-3;
    a.obs_off = s.i64; a.pred_off = s.i64 + (T + 1);
    a.theta0 = s.f64; a.lo = s.f64 + (size_t)T * H; a.hi = s.f64 + 2 * (size_t)T * H;
    a.trainable = s.train;
    a.X = reinterpret_cast<decltype(a.X)>(s.X); a.y = reinterpret_cast<decltype(a.y)>(s.y); a.Xs = reinterpret_cast<decltype(a.Xs)>(s.Xs);
    a.theta = s.out_f64; a.nll = s.out_f64 + (size_t)T * H;
    a.grad = b->grad ? s.out_f64 + (size_t)T * H + T : nullptr;
    a.status = s.out_i32; a.n_eval = s.out_i32 + T; a.n_iter = s.out_i32 + 2 * (size_t)T;
    a.f_mean = reinterpret_cast<decltype(a.f_mean)>(s.fm); a.f_var = reinterpret_cast<decltype(a.f_var)>(s.fv);
    a.y_var = reinterpret_cast<decltype(a.y_var)>(s.yv);
    a.order = s.order; a.queue = s.queue;
}

// Device-to-host copies of the results (host mode: the predictions and the covariance too).
int fetch_batch(gpsat_handle* h, const gpsat_batch* b, const BatchDims& d, const Staged& s, int mean = GPSAT_MEAN_ZERO) {
    const size_t T = (size_t)b->T, H = (size_t)n_hyper(b, mean), esz = b->dtype == GPSAT_F64 ? sizeof(double) : sizeof(float);
    HIP_TRY(hipMemcpyAsync(b->theta, s.out_f64, T * H * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(b->nll, s.out_f64 + T * H, T * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (b->grad) HIP_TRY(hipMemcpyAsync(b->grad, s.out_f64 + T * H + T, T * H * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(b->status, s.out_i32, T * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(b->n_eval, s.out_i32 + T, T * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (b->n_iter) HIP_TRY(hipMemcpyAsync(b->n_iter, s.out_i32 + 2 * T, T * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    void* const host[3] = {b->f_mean, b->f_var, b->y_var};
    const char* const dev[3] = {s.fm, s.fv, s.yv};
    for (int i = 0; i < 3 && b->memory == GPSAT_MEM_HOST && d.sumP > 0; ++i)
        HIP_TRY(hipMemcpyAsync(host[i], dev[i], (size_t)d.sumP * esz, hipMemcpyDeviceToHost, h->stream));
    if (b->memory == GPSAT_MEM_HOST && d.want_cov && d.sumC > 0)
        HIP_TRY(hipMemcpyAsync(b->f_cov, s.cov, (size_t)d.sumC * esz, hipMemcpyDeviceToHost, h->stream));
    return GPSAT_OK;
}

// ---- time slicing: the ring preset with the tiles in `order`, its counters, the saved-state area
int setup_ring(gpsat_handle* h, const gpsat::TilePlan& p, const std::vector<int>& order, gpsat::KernelArgs& a) {
    a.ring = nullptr; a.ring_ctl = nullptr; a.state = nullptr;
    a.ring_mask = 0; a.state_words = p.state_words; a.seg_cost = p.seg_cost;
    if (p.seg_cost <= 0) return GPSAT_OK;
    const int T = (int)order.size();
    const size_t cap = p.ring_cap;
    int rc;
    if ((rc = h->ring.reserve(cap * sizeof(unsigned long long) + 256))) return rc;
    if ((rc = h->state.reserve((size_t)T * p.state_words * sizeof(unsigned)))) return rc;
    a.ring_mask = (int)(cap - 1);
    a.ring_ctl = static_cast<int*>(h->ring.p);
    a.ring = reinterpret_cast<unsigned long long*>(static_cast<char*>(h->ring.p) + 256);
    a.state = static_cast<unsigned*>(h->state.p);
    std::vector<unsigned long long> init(cap, 0ull);       // local host memory, like `ctl`: synchronised below, before they go
    for (int i = 0; i < T; ++i) init[i] = ((unsigned long long)(i + 1) << 32) | (unsigned)order[i];
    int ctl[64] = {0};
    ctl[16] = T; ctl[32] = T;
    HIP_TRY(hipMemcpyAsync(a.ring_ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(a.ring, init.data(), cap * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // `init` and `ctl` are stack / local host memory
    return GPSAT_OK;
}

// ---- cooperative tiles, or teams: both keep their control blocks in h->coop (fp32 / fp64 kernels, never both)
int setup_coop_and_team(gpsat_handle* h, const gpsat::TilePlan& p, const int* T_host, gpsat::KernelArgs& a) {
    int rc;
    a.coop = nullptr; a.coop_live = nullptr; a.coop_min_nb = p.coop_min_nb; a.coop_hdiv = p.coop_hdiv; a.coop_force = p.coop_force;
    if (p.coop) {
        // [grid] control blocks of 1 KiB, zeroed every launch, then the count of unfinished tiles
        const size_t cb = (size_t)p.grid * 1024;
        if ((rc = h->coop.reserve(cb + 64))) return rc;
        HIP_TRY(hipMemsetAsync(h->coop.p, 0, cb + 64, h->stream));
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(h->coop.p) + cb, T_host, sizeof(int), hipMemcpyHostToDevice, h->stream));
        a.coop = h->coop.p;
        a.coop_live = reinterpret_cast<int*>(static_cast<char*>(h->coop.p) + cb);
    }
    a.team_size = p.team; a.team_ctl = nullptr;
    if (p.team > 1) {
        const size_t tb = (size_t)(p.grid / p.team) * 256;
        if ((rc = h->coop.reserve(tb))) return rc;
        HIP_TRY(hipMemsetAsync(h->coop.p, 0, tb, h->stream));
        a.team_ctl = h->coop.p;
    }
    return GPSAT_OK;
}

// ---- multi-start: per-tile state (log theta0, best so far), the clipped further starts, the objectives of every start
int setup_multistart(gpsat_handle* h, const gpsat_batch* b, int S, const double* theta0, const std::vector<double>& starts,
                     gpsat::KernelArgs& a) {
    const int T = b->T, H = n_hyper(b);
    const size_t n_state = (size_t)T * gpsat::MS_WORDS, n_starts = (size_t)T * (S - 1) * H, n_f = (size_t)T * S;
    int rc;
    if ((rc = h->ms.reserve((n_state + n_starts + n_f) * sizeof(double)))) return rc;
    // state, then NaN in f_start for tiles that run no start (no observations)
    std::vector<double> init(n_state + n_f, 0.0);          // local host memory: synchronised below, before it goes
    std::fill(init.begin() + n_state, init.end(), std::numeric_limits<double>::quiet_NaN());
    for (int t = 0; t < T; ++t) {
        double* st = init.data() + (size_t)t * gpsat::MS_WORDS;
        st[1] = std::numeric_limits<double>::infinity();     // best f
        st[4] = -1.0;                                         // best start: none yet
        for (int i = 0; i < H; ++i) st[5 + i] = std::log(theta0[(size_t)t * H + i]);
    }
    double* d_ms = static_cast<double*>(h->ms.p);
    HIP_TRY(hipMemcpyAsync(d_ms, init.data(), n_state * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (n_starts) HIP_TRY(hipMemcpyAsync(d_ms + n_state, starts.data(), n_starts * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_ms + n_state + n_starts, init.data() + n_state, n_f * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // `init` is local host memory
    a.ms_S = S; a.ms_state = d_ms; a.ms_starts = d_ms + n_state; a.ms_fout = d_ms + n_state + n_starts;
    return GPSAT_OK;
}

// ---- the memo of evaluations (gpsat_plan.h eval_cache_bytes): the tiles clear their own headers, nothing to preset
int setup_eval_cache(gpsat_handle* h, const gpsat_batch* b, bool ms_on, gpsat::KernelArgs& a) {
    a.memo = nullptr; a.memo_stats = nullptr;
    const char* knob = dev_env("GPSAT_DEBUG_EVAL_CACHE");
    const bool f64 = b->dtype == GPSAT_F64;
    const size_t bytes = gpsat::eval_cache_bytes(b->T, f64, b->optimiser, b->max_iter, ms_on, knob && std::atoi(knob) == 0);
    const bool stats = !f64 && dev_env("GPSAT_DEBUG_EVAL_CACHE_STATS");
    if (bytes == 0 && !stats) return GPSAT_OK;
    int rc;
    if ((rc = h->memo.reserve(64 + bytes))) return rc;
    if (stats) {
        HIP_TRY(hipMemsetAsync(h->memo.p, 0, 64, h->stream));
        a.memo_stats = static_cast<unsigned*>(h->memo.p);
    }
    if (bytes) a.memo = static_cast<unsigned*>(h->memo.p) + 16;
    return GPSAT_OK;
}

// ---- deferred predictions: the snapshot pool the plan asked for (gpsat_ring.h), or none when there is no memory for it
int setup_deferred(gpsat_handle* h, const gpsat::TilePlan& p, gpsat::KernelArgs& a) {
    a.pq = nullptr; a.pq_ctl = nullptr; a.cu_busy = nullptr; a.pq_snap = nullptr; a.pq_stride = 0; a.pq_slots = 0;
    size_t slots = (size_t)p.pq_slots;
    // (head rounded to 256 B: the snapshots move as 16-B block accesses)
    const size_t head = (256 + 2048 * sizeof(int) + slots * sizeof(unsigned long long) + 255) & ~size_t(255);
    if (slots > 0 && h->pq.reserve(head + slots * p.pq_stride * sizeof(float)) != GPSAT_OK) {
        // no memory for the pool: every prediction inline (the same results), not an error
        g_err.clear();
        (void)hipGetLastError();
        slots = 0;
    }
    if (slots == 0) return GPSAT_OK;
    HIP_TRY(hipMemsetAsync(h->pq.p, 0, head, h->stream));
    char* q = static_cast<char*>(h->pq.p);
    a.pq_ctl = reinterpret_cast<int*>(q);
    a.cu_busy = reinterpret_cast<int*>(q + 256);
    a.pq = reinterpret_cast<unsigned long long*>(q + 256 + 2048 * sizeof(int));
    a.pq_snap = reinterpret_cast<float*>(q + head);
    a.pq_stride = p.pq_stride; a.pq_slots = (int)slots;
    return GPSAT_OK;
}

// What the host reads back about a launch besides the results: the two rerun conditions and the developer statistics.
struct LaunchReport {
    std::vector<int> team, coop;      // TeamCtl / CoopCtl blocks
    int pq_taken = -1, unfinished = 0;
    unsigned memo[9] = {0};               // KernelArgs::memo_stats
    bool team_gave_up = false;
};

// the copies of the report, queued behind the results; the caller synchronises the stream before `r` is read or goes
int queue_report(gpsat_handle* h, const gpsat::TilePlan& p, const gpsat::KernelArgs& a, LaunchReport& r) {
    if (p.team > 1) {
        r.team.resize((size_t)(p.grid / p.team) * 64);
        HIP_TRY(hipMemcpyAsync(r.team.data(), h->coop.p, r.team.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    if (p.coop && dev_env("GPSAT_DEBUG_COOP_STATS")) {
        r.coop.resize((size_t)p.grid * 256);
        HIP_TRY(hipMemcpyAsync(r.coop.data(), h->coop.p, (size_t)p.grid * 1024, hipMemcpyDeviceToHost, h->stream));
    }
    if (a.pq_ctl && dev_env("GPSAT_DEBUG_DEFER_STATS"))
        HIP_TRY(hipMemcpyAsync(&r.pq_taken, a.pq_ctl, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (a.memo_stats) HIP_TRY(hipMemcpyAsync(r.memo, a.memo_stats, sizeof(r.memo), hipMemcpyDeviceToHost, h->stream));
    if (p.seg_cost > 0) HIP_TRY(hipMemcpyAsync(&r.unfinished, a.ring_ctl + 32, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return GPSAT_OK;
}

// after the synchronisation: the developer statistics on stderr, and whether a team barrier gave up
void read_report(const gpsat::TilePlan& p, const gpsat::KernelArgs& a, LaunchReport& r) {
    const int grid = p.grid, T = a.T;
    if (!r.coop.empty()) {
        long long st[8] = {0};
        for (int g = 0; g < grid; ++g) for (int i = 0; i < 8; ++i) st[i] += r.coop[(size_t)g * 256 + 32 + GPSAT_PT_MAXNB + i];
        std::fprintf(stderr, "gpsat coop: grid %d T %d: cooperative evaluations %lld, helper phases %lld, helper groups (sweep) %lld, "
                             "flag waits given up %lld, owner waits given up %lld, pivot failures %lld, helper unwinds %lld\n",
                     grid, T, st[0], st[1], st[2], st[3], st[4], st[5], st[6]);
    }
    if (dev_env("GPSAT_DEBUG_DEFER_STATS"))       // developer / tests: how many predictions were deferred
        std::fprintf(stderr, "gpsat defer: T %d: deferred predictions %d of %d snapshot slots\n", T,
                     r.pq_taken < 0 ? 0 : std::min(r.pq_taken, a.pq_slots), a.pq_slots);
    if (a.memo_stats)                             // developer / tests: what the memo of evaluations answered
        std::fprintf(stderr, "gpsat eval cache: T %d: memo %s, evaluations %u, answered from the memo %u, of those the previous key again %u, "
                             "tiles with such an evaluation %u, tiles that finished on one %u; tiles with 30 evaluations or more %u, answered "
                             "from the memo in those %u; most evaluations of a tile %u, most computed evaluations of a tile %u\n",
                     T, a.memo ? "on" : "off", r.memo[0], r.memo[1], r.memo[2], r.memo[3], r.memo[4], r.memo[6], r.memo[5], r.memo[7], r.memo[8]);
    if (!r.team.empty() && dev_env("GPSAT_DEBUG_TEAM_STATS"))
        std::fprintf(stderr, "gpsat team 0 (size %d), factorisation, owner thread 0, s_memtime ticks: own work of (A) %d, (A) wait + barrier %d, (B) + barrier %d, "
                             "(C) + barrier %d\n", p.team, r.team[24], r.team[25], r.team[26], r.team[27]);
    for (size_t g = 0; g < r.team.size() / 64; ++g)
        if (r.team[g * 64 + 5]) r.team_gave_up = true;    // TeamCtl::timeout: a team barrier gave up (never by design)
}

// What check_* leave for the runs of one dense batch.
struct DenseJob {
    const gpsat_batch* b;
    const gpsat_multistart* ms;       // nullptr: gpsat_fit_predict_batch
    const gpsat_cv* cv = nullptr;     // held-out predictions (gpsat_fit_predict_batch_cv), with their fold tables
    CvTables cv_tables;
    const gpsat_cv_joint* cv_joint = nullptr;     // ... and the folds' joint densities (gpsat_fit_predict_batch_cv_joint)
    int mean = GPSAT_MEAN_ZERO;       // GPSAT_MEAN_CONSTANT: gpsat_fit_predict_batch_mean with a trainable constant mean
    const void* obs_var = nullptr;    // gpsat_fit_predict_batch_noise: noise variances per observation, behind gpsat::check_noise
    const gpsat_pred_grad* pred_grad = nullptr;   // gpsat_fit_predict_batch_grad: the two outputs, behind gpsat::check_pred_grad
    const gpsat_pred_hess* pred_hess = nullptr;   // gpsat_fit_predict_batch_hess: outputs, dims and weights, behind gpsat::check_pred_hess
    bool ms_on;                       // ms given and the optimiser runs
    BatchDims dims;
    const double* theta0;             // the caller's, or clipped into the bounds (multi-start)
    std::vector<double> theta0_clipped, starts_clipped;
    std::vector<int> order;           // tiles, largest cost first
};

// One run of a checked batch: plan, stage, set up, launch, fetch, synchronise.  `solo` / `unsliced`: the two reruns.
int run_tiles(gpsat_handle* h, const DenseJob& j, bool solo, bool unsliced, LaunchReport& r) {
    const gpsat_batch* b = j.b;
    const BatchDims& d = j.dims;
    const bool f64 = b->dtype == GPSAT_F64;
    const gpsat::F64Variant variant = j.cv ? gpsat::CV : b->kernel == GPSAT_KERNEL_RQ ? gpsat::RQ
                                      : j.mean == GPSAT_MEAN_CONSTANT ? gpsat::MEAN : j.obs_var ? gpsat::NOISE
                                      : j.pred_grad ? gpsat::GRAD : j.pred_hess ? gpsat::HESS : gpsat::PLAIN;
    gpsat::PlanInput in = {b->T, b->D, f64, b->obs_off, d.maxP, d.want_cov, d.sumP > 0, b->optimiser, b->max_iter,
                           h->num_cu, h->wg_per_cu, solo || variant != gpsat::PLAIN, unsliced, read_dev_knobs()};     // a variant: one workgroup per tile
    gpsat::TilePlan p;
    if (!gpsat::plan_tiles(in, p)) return fail(GPSAT_EINVAL, "tile too large for LDS");
    Staged s;
    int rc;
    // one workspace per workgroup, or per team
    const size_t ws_bytes = (size_t)(p.grid / p.team) * p.ws_stride * (f64 ? sizeof(double) : sizeof(float));
    if ((rc = stage_batch(h, b, d, j.theta0, j.order, d.want_cov ? b->cov_off : nullptr, nullptr, ws_bytes, s, j.mean, j.obs_var))) return rc;
    gpsat::KernelArgs a;
    fill_common_args(a, b, s, j.mean);
    a.NBmax = p.NBmax;
    a.ws = static_cast<float*>(h->ws.p); a.ws_stride = p.ws_stride;     // fp64: the kernel reinterprets ws as doubles
    a.prof = nullptr;
    a.cov_off = d.want_cov ? s.i64 + 2 * (b->T + 1) : nullptr;
    a.f_cov = d.want_cov ? reinterpret_cast<float*>(s.cov) : nullptr;
    a.PCmax = p.PCcov;
    a.dump = nullptr; a.dump_stride = 0;
    if ((rc = setup_ring(h, p, j.order, a))) return rc;
    if ((rc = setup_coop_and_team(h, p, &b->T, a))) return rc;
    if (j.ms_on && (rc = setup_multistart(h, b, j.ms->n_starts, j.theta0, j.starts_clipped, a))) return rc;
    if ((rc = setup_deferred(h, p, a))) return rc;
    if ((rc = setup_eval_cache(h, b, j.ms_on, a))) return rc;
    const auto launch = gpsat::builds[p.build].launch_variant[variant];
    if (!launch) return fail(GPSAT_EINVAL, variant == gpsat::CV ? "held-out predictions: no kernel in this build" : "no kernel for this model in this build");
    gpsat::NoiseArgs na;
    na.obs_var = s.obs_var;
    // the outputs of the gradient or second-derivative call: the caller's device memory, or (host mode) the handle's
    gpsat::GradArgs ga;
    gpsat::HessArgs ha;
    DerivedOuts derived;
    if ((rc = stage_derived(h, b, d, j.pred_grad, j.pred_hess, ga, ha, derived))) return rc;
    gpsat::CvArgs ca;
    if (j.cv && (rc = stage_cv(h, b, j.cv, j.cv_joint, d, j.cv_tables, ca))) return rc;
#ifdef GPSAT_DUMP
    if (h->dump_dev && !f64) {
        const size_t need = ((size_t)p.NBmax * p.NBmax + p.NBmax) * 1024 + 2 * (size_t)p.NBmax * 32 + 16 + 8 * 1024;
        if (h->dump_stride < need) return fail(GPSAT_EINVAL, "dump stride too small: need " + std::to_string(need) + " floats per tile");
        a.dump = h->dump_dev; a.dump_stride = h->dump_stride;
    }
#endif
#ifdef GPSAT_PROFILE
    if ((rc = h->prof.reserve(sizeof(h->prof_host)))) return rc;
    HIP_TRY(hipMemsetAsync(h->prof.p, 0, sizeof(h->prof_host), h->stream));
    a.prof = static_cast<unsigned long long*>(h->prof.p);
#endif
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(launch(b->D, a, j.cv ? &ca : nullptr, j.obs_var ? &na : nullptr, j.pred_grad ? &ga : nullptr, j.pred_hess ? &ha : nullptr,
                   p.grid, p.smem, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    if ((rc = fetch_batch(h, b, d, s, j.mean))) return rc;
    if (j.cv && (rc = fetch_cv(h, b, j.cv, j.cv_joint, d, ca))) return rc;
    if ((rc = fetch_derived(h, b, derived))) return rc;
    if (j.ms_on && j.ms->f_start)
        HIP_TRY(hipMemcpyAsync(j.ms->f_start, a.ms_fout, (size_t)b->T * j.ms->n_starts * sizeof(double), hipMemcpyDeviceToHost, h->stream));
#ifdef GPSAT_PROFILE
    HIP_TRY(hipMemcpyAsync(h->prof_host, h->prof.p, sizeof(h->prof_host), hipMemcpyDeviceToHost, h->stream));
#endif
    if ((rc = queue_report(h, p, a, r))) return rc;
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    read_report(p, a, r);
    return GPSAT_OK;
}

int fit_predict(gpsat_handle* h, const gpsat_batch* b, const gpsat_multistart* ms, const gpsat_cv* cv = nullptr,
                const gpsat_mean* mn = nullptr, const gpsat_noise* nz = nullptr, const gpsat_cv_joint* jt = nullptr,
                const gpsat_pred_grad* pg = nullptr, const gpsat_pred_hess* ph = nullptr) {
    if (!h || !b) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch: NULL handle or batch");
    if (b->T == 0) return GPSAT_OK;
    DenseJob j;
    j.b = b; j.ms = ms; j.cv = cv; j.cv_joint = jt;
    int rc;
    if ((rc = check_batch(b, false, j.dims))) return rc;
    if ((rc = check_rq(b, ms ? "gpsat_fit_predict_batch_ms" : cv ? "gpsat_fit_predict_batch_cv" : nullptr))) return rc;
    if (mn) {
        const char* why = nullptr;
        if ((rc = gpsat::check_mean(b, mn, &why))) return fail(rc, why);
        j.mean = mn->kind;
    }
    if (nz) {
        char why[160];
        if ((rc = gpsat::check_noise(b, nz, why, sizeof(why)))) return fail(rc, why);
        j.obs_var = nz->obs_var;
    }
    if (pg) {
        char why[200];
        if ((rc = gpsat::check_pred_grad(b, pg, why, sizeof(why)))) return fail(rc, why);
        j.pred_grad = pg;
    }
    if (ph) {
        char why[240];
        if ((rc = gpsat::check_pred_hess(b, ph, why, sizeof(why)))) return fail(rc, why);
        j.pred_hess = ph;
    }
    BatchDims& d = j.dims;
    d.want_cov = b->f_cov != nullptr;             // optional full posterior covariance: one P_t x P_t block per tile
    if (d.want_cov) {
        if (!b->cov_off) return fail(GPSAT_EINVAL, "f_cov given without cov_off");
        if (b->cov_off[0] != 0) return fail(GPSAT_EINVAL, "cov_off must start at 0");
        for (int t = 0; t < b->T; ++t) {
            const long long p = b->pred_off[t + 1] - b->pred_off[t];
            if (b->cov_off[t + 1] - b->cov_off[t] != p * p) return fail(GPSAT_EINVAL, "cov_off[t+1]-cov_off[t] must equal P_t^2");
            d.maxP = std::max(d.maxP, p);
        }
        d.sumC = b->cov_off[b->T];
    }
    if (d.maxN > gpsat_max_tile_obs(b->dtype, b->D))
        return fail(GPSAT_EINVAL, "tile too large for the LDS of a CU: at most " + std::to_string(gpsat_max_tile_obs(b->dtype, b->D)) +
                                      " observations per tile for this dtype and D (gpsat_max_tile_obs)");
    if ((rc = check_batch_data(b, d, j.mean))) return rc;
    if (cv && (rc = check_cv(b, cv, d, j.cv_tables))) return rc;
    if (jt && (rc = check_cv_joint_offsets(jt, b->T, j.cv_tables.all.data() + j.cv_tables.o_fold_off))) return rc;
    j.ms_on = ms && b->optimiser != GPSAT_OPT_NONE && b->max_iter > 0;
    if (ms && (rc = check_multistart(b, ms, j.ms_on, j.theta0_clipped, j.starts_clipped))) return rc;
    j.theta0 = j.ms_on ? j.theta0_clipped.data() : b->theta0;
    if ((rc = begin_call(h))) return rc;
    // ---- tile order: largest cost first (N^3), stable so equal tiles keep the reference order.  A multi-start batch costs
    // S times as much per tile, alike for every tile: neither the order nor the slicing decision of the plan changes with S.
    j.order.resize(b->T);
    std::iota(j.order.begin(), j.order.end(), 0);
    std::stable_sort(j.order.begin(), j.order.end(), [&](int a, int c) {
        return (b->obs_off[a + 1] - b->obs_off[a]) > (b->obs_off[c + 1] - b->obs_off[c]);
    });
    for (bool solo = false, unsliced = false;;) {
        LaunchReport r;
        if ((rc = run_tiles(h, j, solo, unsliced, r))) return rc;
        if (r.team_gave_up) {             // run the batch again, one workgroup per tile
            std::fprintf(stderr, "gpsat: a team barrier gave up; re-running the batch with one workgroup per tile\n");
            solo = true;
        } else if (r.unfinished != 0) {
            // A queue anomaly (an escape hatch of ring_pop taken: gpsat_ring.h) must not cost the caller the batch: run it again
            // with every tile run to completion from the plain queue (same results: slicing does not change a bit of them).
            if (unsliced) return fail(GPSAT_EHIP, "tile queue ended with " + std::to_string(r.unfinished) + " unfinished tiles");
            std::fprintf(stderr, "gpsat: time-sliced tile queue ended with %d unfinished tiles; re-running the batch unsliced\n", r.unfinished);
            unsliced = true;
        } else {
            return record_timing(h);
        }
    }
}

// ---- refitted cross-validation (gpsat_fit_predict_batch_cv_refit): the plain batch, then every fitted fold as a tile of a
// second, device-resident batch through fit_predict itself; gpsat_cvfold.hip builds that batch and puts its predictions back.
int check_cv_refit(const gpsat_batch* b, const gpsat_cv_refit* cv, gpsat::CvFoldTables& tb) {
    const char* who = "gpsat_cv_refit: ";
    if (!cv->fold) return fail(GPSAT_EINVAL, std::string(who) + "fold is NULL");
    if (!cv->fold_off) return fail(GPSAT_EINVAL, std::string(who) + "fold_off is NULL");
    if (!cv->cv_mean) return fail(GPSAT_EINVAL, std::string(who) + "cv_mean is NULL");
    if (!cv->cv_f_var) return fail(GPSAT_EINVAL, std::string(who) + "cv_f_var is NULL");
    if (cv->start != 0 && cv->start != 1) return fail(GPSAT_EINVAL, std::string(who) + "start must be 0 (theta0) or 1 (the tile's full-data theta)");
    if (cv->recentre != 0 && cv->recentre != 1) return fail(GPSAT_EINVAL, std::string(who) + "recentre must be 0 or 1");
    if (b->cov_off || b->f_cov)
        return fail(GPSAT_EINVAL, std::string(who) + "refitted held-out predictions and the full covariance cannot be asked for in the same call: cov_off / f_cov must be NULL");
    const std::string err = gpsat::cvfold_tables(b->T, b->obs_off, cv->fold, true, tb);
    if (!err.empty()) return fail(GPSAT_EINVAL, who + err);
    for (int t = 0; t <= b->T; ++t)
        if (cv->fold_off[t] != tb.fold_off[t])
            return fail(GPSAT_EINVAL, std::string(who) + "fold_off[" + std::to_string(t) + "] = " + std::to_string(cv->fold_off[t]) +
                                          " differs from gpsat_cv_refit_count's " + std::to_string(tb.fold_off[t]));
    if (tb.fold_off[b->T] > 0) {
        const std::pair<const void*, const char*> outs[] = {{cv->fold_theta, "fold_theta"}, {cv->fold_nll, "fold_nll"}, {cv->fold_shift, "fold_shift"},
            {cv->fold_status, "fold_status"}, {cv->fold_n_eval, "fold_n_eval"}, {cv->fold_n_obs, "fold_n_obs"}, {cv->fold_label, "fold_label"}};
        for (const auto& o : outs)
            if (!o.first) return fail(GPSAT_EINVAL, std::string(who) + o.second + " is NULL");
    }
    return GPSAT_OK;
}

// Stage and expand: the packed tables to the device, CvFoldArgs laid out over the handle's three cvr buffers, the rows of every
// derived tile written by the device, `delta` (the mean each tile was shifted by) read back.  Synchronises and records the timing.
int cvr_stage_expand(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv_refit* cv, size_t sumN, const gpsat::CvFoldDerived& dv,
                     const gpsat::CvFoldPacked& pk, gpsat::CvFoldArgs& a, std::vector<double>& delta) {
    const int D = b->D;
    const bool f64 = b->dtype == GPSAT_F64, host = b->memory == GPSAT_MEM_HOST;
    const size_t esz = f64 ? sizeof(double) : sizeof(float);
    const size_t F2 = dv.d_fold.size(), E = (size_t)dv.d_obs_off[F2], P2 = (size_t)dv.d_pred_off[F2];
    int rc;
    if ((rc = h->cvr_tab.reserve(pk.n64 * 8 + pk.n32 * sizeof(int)))) return rc;
    if ((rc = h->cvr_in.reserve(std::max<size_t>(E * (D + 1) + P2 * D, 1) * esz))) return rc;
    if ((rc = h->cvr_out.reserve(std::max<size_t>(3 * P2 + (host ? 3 * sumN : 0), 1) * esz))) return rc;
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    long long* d64 = static_cast<long long*>(h->cvr_tab.p);
    int* d32 = reinterpret_cast<int*>(d64 + pk.n64);
    HIP_TRY(hipMemcpyAsync(d64, pk.t64.data(), pk.t64.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d32, pk.t32.data(), pk.t32.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    a.F2 = (int)F2; a.D = D; a.f64 = f64; a.recentre = cv->recentre; a.sumN = (long long)sumN;
    a.d_obs_off = d64 + pk.o_obs_off; a.d_pred_off = d64 + pk.o_pred_off; a.d_src_off = d64 + pk.o_src_off;
    a.delta = reinterpret_cast<double*>(d64 + pk.o_delta);
    a.d_src_n = d32 + pk.o_src_n; a.d_fold = d32 + pk.o_fold; a.d_status = d32 + pk.o_status;
    a.fold_ptr = d32 + pk.o_fold_ptr; a.fold_rows = d32 + pk.o_fold_rows; a.fold_derived = d32 + pk.o_fold_derived;
    a.row_fold = d32 + pk.o_row_fold; a.row_pos = d32 + pk.o_row_pos;
    // the source rows: the caller's device arrays, or where stage_batch left them for the first launch (X, then y)
    a.X = host ? h->bulk_in.p : b->X;
    a.y = host ? static_cast<const void*>(static_cast<const char*>(h->bulk_in.p) + sumN * D * esz) : b->y;
    char* in = static_cast<char*>(h->cvr_in.p);
    a.Xd = in; a.yd = in + E * D * esz; a.Xsd = in + E * (D + 1) * esz;
    char* out = static_cast<char*>(h->cvr_out.p);
    a.fm = out; a.fv = out + P2 * esz; a.yv = out + 2 * P2 * esz;
    a.cv_mean = host ? out + 3 * P2 * esz : cv->cv_mean;
    a.cv_f_var = host ? out + (3 * P2 + sumN) * esz : cv->cv_f_var;
    a.cv_y_var = host ? out + (3 * P2 + 2 * sumN) * esz : cv->cv_y_var;
    delta.assign(F2, 0.0);
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(gpsat::launch_cvfold_expand(a, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    if (F2) HIP_TRY(hipMemcpyAsync(delta.data(), a.delta, F2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // pk's tables are host memory of the caller
    return record_timing(h);
}

// The derived batch: every fitted fold a tile of a device-resident batch, its rows where the expansion left them.  A fold
// starts from its tile's full-data theta (cv->start == 1, where that is finite and positive) or from theta0, in its tile's bounds.
struct DerivedBatch {
    std::vector<double> th0, lo, hi, theta, nll;
    std::vector<int> status, n_eval, n_iter;
    gpsat_batch b2;
};

void cvr_derived_batch(const gpsat_batch* b, const gpsat_cv_refit* cv, const gpsat::CvFoldTables& tb, const gpsat::CvFoldDerived& dv,
                       const gpsat::CvFoldArgs& a, DerivedBatch& db) {
    const int H = n_hyper(b);
    const size_t F2 = dv.d_fold.size();
    db.th0.resize(F2 * H); db.lo.resize(F2 * H); db.hi.resize(F2 * H); db.theta.resize(F2 * H); db.nll.resize(F2);
    db.status.assign(F2, GPSAT_STATUS_SKIPPED); db.n_eval.resize(F2); db.n_iter.resize(F2);
    for (size_t j = 0; j < F2; ++j) {
        const size_t t = (size_t)tb.fold_tile[dv.d_fold[j]];
        bool full = cv->start == 1;
        for (int i = 0; i < H && full; ++i) full = b->theta[t * H + i] > 0.0 && std::isfinite(b->theta[t * H + i]);
        for (int i = 0; i < H; ++i) {
            db.th0[j * H + i] = full ? b->theta[t * H + i] : b->theta0[t * H + i];
            db.lo[j * H + i] = b->lo[t * H + i]; db.hi[j * H + i] = b->hi[t * H + i];
        }
    }
    gpsat_batch& b2 = db.b2;
    b2 = *b;
    b2.T = (int)F2; b2.memory = GPSAT_MEM_DEVICE;
    b2.obs_off = dv.d_obs_off.data(); b2.pred_off = dv.d_pred_off.data();
    b2.theta0 = db.th0.data(); b2.lo = db.lo.data(); b2.hi = db.hi.data();
    b2.X = a.Xd; b2.y = a.yd; b2.Xs = a.Xsd;
    b2.theta = db.theta.data(); b2.nll = db.nll.data(); b2.grad = nullptr;
    b2.status = db.status.data(); b2.n_eval = db.n_eval.data(); b2.n_iter = db.n_iter.data();
    b2.f_mean = const_cast<void*>(a.fm); b2.f_var = const_cast<void*>(a.fv); b2.y_var = const_cast<void*>(a.yv);
    b2.cov_off = nullptr; b2.f_cov = nullptr;
}

// The caller's per-fold outputs: `skipped` for every fold (before anything runs), then what the derived batch returned
void cvr_folds_skipped(const gpsat_batch* b, const gpsat_cv_refit* cv, const gpsat::CvFoldTables& tb) {
    const int H = n_hyper(b);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t f = 0; f < (size_t)tb.fold_off[b->T]; ++f) {
        for (int i = 0; i < H; ++i) cv->fold_theta[f * H + i] = nan;
        cv->fold_nll[f] = nan; cv->fold_shift[f] = nan;
        cv->fold_status[f] = GPSAT_STATUS_SKIPPED; cv->fold_n_eval[f] = 0;
        if (cv->fold_n_iter) cv->fold_n_iter[f] = 0;
        cv->fold_n_obs[f] = tb.fold_n_obs[f]; cv->fold_label[f] = tb.fold_label[f];
    }
}

void cvr_unpack(const gpsat_batch* b, const gpsat_cv_refit* cv, const gpsat::CvFoldDerived& dv, const DerivedBatch& db,
                const std::vector<double>& delta) {
    const int H = n_hyper(b);
    for (size_t j = 0; j < dv.d_fold.size(); ++j) {
        const size_t f = (size_t)dv.d_fold[j];
        for (int i = 0; i < H; ++i) cv->fold_theta[f * H + i] = db.theta[j * H + i];
        cv->fold_nll[f] = db.nll[j]; cv->fold_shift[f] = delta[j];
        cv->fold_status[f] = db.status[j]; cv->fold_n_eval[f] = db.n_eval[j];
        if (cv->fold_n_iter) cv->fold_n_iter[f] = db.n_iter[j];
    }
}

// Scatter and fetch: the status of every derived tile to the device, its predictions back at the rows they were held out
// from, and (host mode) those to the caller.  Synchronises and records the timing.
int cvr_scatter_fetch(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv_refit* cv, size_t sumN, const gpsat::CvFoldArgs& a,
                      const std::vector<int>& status) {
    const size_t esz = b->dtype == GPSAT_F64 ? sizeof(double) : sizeof(float), F2 = status.size();
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    if (F2) HIP_TRY(hipMemcpyAsync(const_cast<int*>(a.d_status), status.data(), F2 * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(gpsat::launch_cvfold_scatter(a, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    if (b->memory == GPSAT_MEM_HOST) {
        void* const hp[3] = {cv->cv_mean, cv->cv_f_var, cv->cv_y_var};
        void* const dp[3] = {a.cv_mean, a.cv_f_var, a.cv_y_var};
        for (int i = 0; i < 3; ++i)
            if (hp[i]) HIP_TRY(hipMemcpyAsync(hp[i], dp[i], sumN * esz, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return record_timing(h);
}

// The joint density of the fitted folds, in front of the derived batch: that batch returns its posterior covariances into
// h->cvr_cov, laid out as doubles [C] f_cov, [F2] sn2, [P2] residuals, [F2] lpd, then cov_off [F2+1].  `cov_off`: host
// memory of the caller, alive until the derived batch has run.
int cvr_joint_stage(gpsat_handle* h, const gpsat::CvFoldDerived& dv, std::vector<int64_t>& cov_off, gpsat::CvFoldArgs& a, gpsat_batch& b2) {
    const size_t F2 = dv.d_fold.size(), P2 = (size_t)dv.d_pred_off[F2];
    cov_off = gpsat::cvfold_cov_off(dv);
    const size_t C = (size_t)cov_off[F2];
    int rc;
    if ((rc = h->cvr_cov.reserve((C + 2 * F2 + P2 + F2 + 1) * sizeof(double)))) return rc;
    double* base = static_cast<double*>(h->cvr_cov.p);
    a.f_cov = base; a.sn2 = base + C; a.resid = base + C + F2; a.lpd = base + C + F2 + P2;
    a.cov_off = reinterpret_cast<const long long*>(base + C + 2 * F2 + P2);
    HIP_TRY(hipMemcpyAsync(const_cast<long long*>(a.cov_off), cov_off.data(), (F2 + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    b2.cov_off = cov_off.data(); b2.f_cov = a.f_cov;
    return GPSAT_OK;
}

// ... and behind it: status and likelihood variance of every derived tile to the device, cvfold_lpd, the numbers to the
// caller's folds.  Synchronises and records the timing.
int cvr_joint_run(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv_joint* jt, const gpsat::CvFoldDerived& dv, const DerivedBatch& db,
                  const gpsat::CvFoldArgs& a) {
    const size_t F2 = dv.d_fold.size(), H = (size_t)n_hyper(b);
    std::vector<double> sn2(F2), lpd(F2);
    for (size_t j = 0; j < F2; ++j) sn2[j] = db.theta[j * H + b->D + 1];
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    HIP_TRY(hipMemcpyAsync(const_cast<int*>(a.d_status), db.status.data(), F2 * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(const_cast<double*>(a.sn2), sn2.data(), F2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(gpsat::launch_cvfold_lpd(a, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    HIP_TRY(hipMemcpyAsync(lpd.data(), a.lpd, F2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // sn2, lpd and the status are host memory of this call
    for (size_t j = 0; j < F2; ++j) jt->fold_lpd[dv.d_fold[j]] = lpd[j];
    return record_timing(h);
}

// The batch itself, then its fitted folds as a second batch through fit_predict; the timing is the sum of the four steps
// (five with the joint density `jt`).
int fit_predict_cv_refit(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv_refit* cv, const gpsat_cv_joint* jt = nullptr) {
    if (!h || !b) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_cv_refit: NULL handle or batch");
    if (!cv) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_cv_refit: NULL gpsat_cv_refit");
    if (b->T == 0) return GPSAT_OK;
    BatchDims d;
    int rc;
    if ((rc = check_batch(b, false, d))) return rc;
    if ((rc = check_rq(b, "gpsat_fit_predict_batch_cv_refit"))) return rc;
    if (jt && b->dtype != GPSAT_F64)
        return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_cv_refit_joint: the joint density of refitted folds is built for GPSAT_F64 only");
    gpsat::CvFoldTables tb;
    if ((rc = check_cv_refit(b, cv, tb))) return rc;
    if (jt && (rc = check_cv_joint_offsets(jt, b->T, tb.fold_off.data()))) return rc;
    if ((rc = fit_predict(h, b, nullptr))) return rc;
    double kernel_ms = h->last_kernel_ms, total_ms = h->last_total_ms;
    gpsat::CvFoldDerived dv;
    gpsat::cvfold_derive(tb, b->obs_off, cv->min_obs, dv);
    cvr_folds_skipped(b, cv, tb);
    if (jt) std::fill(jt->fold_lpd, jt->fold_lpd + tb.fold_off[b->T], std::numeric_limits<double>::quiet_NaN());
    const size_t sumN = (size_t)d.sumN, F2 = dv.d_fold.size();
    if (sumN == 0) return GPSAT_OK;
    const gpsat::CvFoldPacked pk = gpsat::cvfold_pack(tb, dv);
    gpsat::CvFoldArgs a;
    std::vector<double> delta;
    if ((rc = cvr_stage_expand(h, b, cv, sumN, dv, pk, a, delta))) return rc;
    const double expand_ms = h->last_kernel_ms;
    kernel_ms += h->last_kernel_ms; total_ms += h->last_total_ms;
    DerivedBatch db;
    cvr_derived_batch(b, cv, tb, dv, a, db);
    std::vector<int64_t> cov_off;
    if (F2) {
        if (jt && (rc = cvr_joint_stage(h, dv, cov_off, a, db.b2))) return rc;
        if ((rc = fit_predict(h, &db.b2, nullptr))) return rc;
        kernel_ms += h->last_kernel_ms; total_ms += h->last_total_ms;
        if (jt) {
            if ((rc = cvr_joint_run(h, b, jt, dv, db, a))) return rc;
            kernel_ms += h->last_kernel_ms; total_ms += h->last_total_ms;
        }
    }
    cvr_unpack(b, cv, dv, db, delta);
    if ((rc = cvr_scatter_fetch(h, b, cv, sumN, a, db.status))) return rc;
    if (dev_env("GPSAT_DEBUG_CVFOLD_STATS"))      // developer / scripts/cv_bench.py: the two streaming kernels on their own
        std::fprintf(stderr, "gpsat cvfold: %zu derived tiles, %zu expanded rows, %zu held-out rows: expand %.4f ms, scatter %.4f ms\n",
                     F2, (size_t)dv.d_obs_off[F2], (size_t)dv.d_pred_off[F2], expand_ms, h->last_kernel_ms);
    h->last_kernel_ms += kernel_ms; h->last_total_ms += total_ms;
    return GPSAT_OK;
}

// ---- the steps of gpsat_select_batch_ex that are more than a call

// The fill call of a two-call selection that the cache answers: the offsets from the host, the indices from the device.
int select_from_cache(gpsat_handle* h, int32_t T, int64_t* off, int32_t* idx, int64_t capacity) {
    const int64_t total = h->selc.total;
    h->selc.forget();
    std::memcpy(off, h->selc.off.data(), (size_t)(T + 1) * sizeof(int64_t));
    if (capacity < total) return fail(GPSAT_EINVAL, "gpsat_select_batch: idx capacity too small (see off[T])");
    if (int rc = begin_call(h)) return rc;
    if (total > 0) HIP_TRY(hipMemcpy(idx, h->selc.d_result, (size_t)total * sizeof(int), hipMemcpyDeviceToHost));
    return GPSAT_OK;
}

// The staged table sorted by the cells of `bin` (a.pts: the sorted copy, d_perm: the source row of every position), and the
// order of the experts on the device (a.eorder).
int select_bin_table(gpsat_handle* h, const gpsat::BinSpec& bin, const double* refs, gpsat::SelectArgs& a, const int*& d_perm) {
    gpsat_handle::SelectBufs& sb = h->sel;
    const long long M = a.M;
    const int C = a.C, T = a.T;
    int rc;
    const size_t perm_bytes = ((size_t)M * 2 * sizeof(int) + 255) & ~size_t(255);
    if ((rc = sb.perm.reserve(perm_bytes + (size_t)M * C * sizeof(double)))) return rc;
    if ((rc = sb.keys.reserve((size_t)M * 2 * sizeof(unsigned)))) return rc;
    int* d_rows = static_cast<int*>(sb.perm.p);
    int* d_p = d_rows + M;
    double* d_pp = reinterpret_cast<double*>(static_cast<char*>(sb.perm.p) + perm_bytes);
    unsigned* d_k = static_cast<unsigned*>(sb.keys.p);
    const double* pts = a.pts;
    if ((rc = run_with_temp(h, sb.tmp, "select_bin_rows", nullptr, [&](void* temp, size_t& tb) {
             return gpsat::select_bin_rows(M, C, pts, bin, d_k, d_k + M, d_rows, d_p, d_pp, temp, tb, h->stream);
         })))
        return rc;
    a.pts = d_pp;
    d_perm = d_p;
    const std::vector<int> eord = gpsat::select_expert_order(bin, refs, T, C);
    if ((rc = sb.ord.reserve((size_t)T * sizeof(int) + (size_t)(T + 1) * sizeof(unsigned)))) return rc;
    HIP_TRY(hipMemcpyAsync(sb.ord.p, eord.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // `eord` is local host memory
    a.eorder = static_cast<const int*>(sb.ord.p);
    return GPSAT_OK;
}

// Positions of the binned table -> source rows, every expert's list ascending (source row order); d_result: where they are.
int select_unbin_indices(gpsat_handle* h, int64_t M, int32_t T, const int64_t* off, const int* d_perm, int* d_idx, const int*& d_result) {
    gpsat_handle::SelectBufs& sb = h->sel;
    int rc;
    if (off[T] > 2147483647LL) return fail(GPSAT_EINVAL, "gpsat_select_batch: more than 2^31-1 selected rows");
    std::vector<unsigned> off32(T + 1);
    for (int t = 0; t <= T; ++t) off32[t] = (unsigned)off[t];
    unsigned* d_off32 = reinterpret_cast<unsigned*>(static_cast<char*>(sb.ord.p) + (size_t)T * sizeof(int));
    HIP_TRY(hipMemcpyAsync(d_off32, off32.data(), (size_t)(T + 1) * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if ((rc = sb.keys.reserve(std::max((size_t)M * 2 * sizeof(unsigned), (size_t)off[T] * sizeof(int))))) return rc;
    int* d_sorted = static_cast<int*>(sb.keys.p);            // the row keys are no longer needed
    if ((rc = run_with_temp(h, sb.tmp, "select_unbin", nullptr, [&](void* temp, size_t& tb) {
             return gpsat::select_unbin(T, off[T], d_off32, d_perm, d_idx, d_sorted, temp, tb, h->stream);
         })))
        return rc;
    d_result = d_sorted;
    return GPSAT_OK;
}

}  // namespace

extern "C" {

int gpsat_version(void) { return GPSAT_ABI_VERSION; }

const char* gpsat_last_error(void) { return g_err.c_str(); }

int gpsat_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int gpsat_max_tile_obs(int dtype, int D) {
    // the largest tile, at most GPSAT_MAX_TILE_OBS observations, whose workgroup state (coordinates, y, z, alpha, factor
    // buffers, optimiser state) fits the 160 KiB LDS of a CU with one workgroup per CU (8-wave builds); fp32 tiles also
    // have at most GPSAT_PT_MAXNB block columns (the sweep flags).  D = 1 / 2 / 3 / 4:
    //   fp32  4096 / 4096 / 3168 / 2592        fp64  4096 / 3392 / 2832 / 2416
    // (pinned by tests/test_abi.py)
    if (D < 1 || D > 4 || (dtype != GPSAT_F32 && dtype != GPSAT_F64)) return 0;
    const bool f64 = dtype == GPSAT_F64;
    const int bs = f64 ? 16 : 32;
    const int nb_max = f64 ? GPSAT_MAX_TILE_OBS / bs : std::min(GPSAT_MAX_TILE_OBS / bs, GPSAT_PT_MAXNB);
    const gpsat::Build& w8 = gpsat::builds[f64 ? gpsat::BUILD_F64_W8 : gpsat::BUILD_F32_W8];
    for (int NB = nb_max; NB >= 1; --NB)
        if (w8.shared_bytes(D, NB) <= 160 * 1024) return NB * bs;
    return 0;
}

int gpsat_n_hyper(int kernel, int D) {
    if (D < 1 || D > 4 || kernel < 0 || kernel > GPSAT_KERNEL_RQ) return 0;
    if (kernel == GPSAT_KERNEL_RQ) return D <= 3 ? D + 3 : 0;
    return D + 2;
}

int gpsat_n_hyper_mean(int kernel, int D, int mean_kind) {
    if (mean_kind == GPSAT_MEAN_ZERO) return gpsat_n_hyper(kernel, D);
    if (mean_kind != GPSAT_MEAN_CONSTANT || D < 1 || D > 3 || kernel < 0 || kernel >= GPSAT_KERNEL_RQ) return 0;
    return D + 3;
}

int gpsat_create(int device_id, const gpsat_opts* opts, gpsat_handle** out) {
    if (!out) return fail(GPSAT_EINVAL, "gpsat_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(GPSAT_ENODEV, "gpsat_create: no HIP device visible");
    if (device_id < 0 || device_id >= n) return fail(GPSAT_EINVAL, "gpsat_create: device_id out of range");
    HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    gpsat_handle* h = new (std::nothrow) gpsat_handle();
    if (!h) return fail(GPSAT_ENOMEM, "gpsat_create: host allocation failed");
    h->device = device_id;
    h->num_cu = prop.multiProcessorCount;
    std::snprintf(h->name, sizeof(h->name), "%s (%s)", prop.name, prop.gcnArchName);
    if (opts && opts->workgroups_per_cu > 0) h->wg_per_cu = std::min(opts->workgroups_per_cu, 8);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(GPSAT_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    for (int i = 0; i < 4; ++i) {
        e = hipEventCreate(&h->ev[i]);
        if (e != hipSuccess) { gpsat_destroy(h); return fail(GPSAT_EHIP, std::string("hipEventCreate: ") + hipGetErrorString(e)); }
    }
    *out = h;
    return GPSAT_OK;
}

int gpsat_device_name(gpsat_handle* h, char* buf, int buflen) {
    if (!h || !buf || buflen <= 0) return fail(GPSAT_EINVAL, "gpsat_device_name: bad argument");
    std::snprintf(buf, (size_t)buflen, "%s", h->name);
    return GPSAT_OK;
}

int gpsat_destroy(gpsat_handle* h) {
    if (!h) return GPSAT_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;                         // every device buffer, then the events, then the stream
    return GPSAT_OK;
}

int gpsat_last_timing(gpsat_handle* h, double* kernel_ms, double* total_ms) {
    if (!h) return fail(GPSAT_EINVAL, "gpsat_last_timing: handle is NULL");
    if (kernel_ms) *kernel_ms = h->last_kernel_ms;
    if (total_ms) *total_ms = h->last_total_ms;
    return GPSAT_OK;
}

int gpsat_fit_predict_batch(gpsat_handle* h, const gpsat_batch* b) { return fit_predict(h, b, nullptr); }

int gpsat_fit_predict_batch_mean(gpsat_handle* h, const gpsat_batch* b, const gpsat_mean* m) {
    if (!m) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_mean: mean is NULL");
    return fit_predict(h, b, nullptr, nullptr, m);
}

int gpsat_fit_predict_batch_noise(gpsat_handle* h, const gpsat_batch* b, const gpsat_noise* nz) {
    if (!nz) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_noise: noise is NULL");
    return fit_predict(h, b, nullptr, nullptr, nullptr, nz);
}

int gpsat_fit_predict_batch_grad(gpsat_handle* h, const gpsat_batch* b, const gpsat_pred_grad* pg) {
    if (!pg) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_grad: pred_grad is NULL");
    return fit_predict(h, b, nullptr, nullptr, nullptr, nullptr, nullptr, pg);
}

int gpsat_fit_predict_batch_hess(gpsat_handle* h, const gpsat_batch* b, const gpsat_pred_hess* ph) {
    if (!ph) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_hess: pred_hess is NULL");
    return fit_predict(h, b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ph);
}

int gpsat_fit_predict_batch_ms(gpsat_handle* h, const gpsat_batch* b, const gpsat_multistart* ms) {
    if (!ms) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_ms: NULL multistart");
    return fit_predict(h, b, ms);
}

int gpsat_max_cv_fold(int dtype, int D) {
    if (D < 1 || D > 4 || dtype != GPSAT_F64) return 0;
    return GPSAT_MAX_CV_FOLD;
}

int gpsat_fit_predict_batch_cv(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv* cv) {
    if (!cv) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_cv: NULL gpsat_cv");
    if (b && b->dtype != GPSAT_F64) return fail(GPSAT_EINVAL, "held-out predictions are built for GPSAT_F64 only");
    return fit_predict(h, b, nullptr, cv);
}

int gpsat_cv_refit_count(int32_t T, const int64_t* obs_off, const int32_t* fold, int64_t* fold_off, int64_t* expanded_rows) {
    if (!fold_off || !expanded_rows) return fail(GPSAT_EINVAL, "gpsat_cv_refit_count: fold_off / expanded_rows is NULL");
    gpsat::CvFoldTables tb;
    const std::string err = gpsat::cvfold_tables(T, obs_off, fold, false, tb);
    if (!err.empty()) return fail(GPSAT_EINVAL, "gpsat_cv_refit_count: " + err);
    std::copy(tb.fold_off.begin(), tb.fold_off.end(), fold_off);
    *expanded_rows = tb.expanded_rows;
    return GPSAT_OK;
}

int gpsat_fit_predict_batch_cv_refit(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv_refit* cv) {
    return fit_predict_cv_refit(h, b, cv);
}

int gpsat_fit_predict_batch_cv_joint(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv* cv, const gpsat_cv_joint* joint) {
    if (int rc = check_cv_joint(joint, "gpsat_fit_predict_batch_cv_joint")) return rc;
    if (!cv) return fail(GPSAT_EINVAL, "gpsat_fit_predict_batch_cv: NULL gpsat_cv");
    if (b && b->dtype != GPSAT_F64) return fail(GPSAT_EINVAL, "held-out predictions are built for GPSAT_F64 only");
    return fit_predict(h, b, nullptr, cv, nullptr, nullptr, joint);
}

int gpsat_fit_predict_batch_cv_refit_joint(gpsat_handle* h, const gpsat_batch* b, const gpsat_cv_refit* cv, const gpsat_cv_joint* joint) {
    if (int rc = check_cv_joint(joint, "gpsat_fit_predict_batch_cv_refit_joint")) return rc;
    return fit_predict_cv_refit(h, b, cv, joint);
}

#ifdef GPSAT_DUMP
// diagnostic build only: device buffer [T][stride_floats] that every fp32 batch call fills (KernelArgs::dump)
int gpsat_debug_set_dump(gpsat_handle* h, void* dev, unsigned long long stride_floats) {
    if (!h) return GPSAT_EINVAL;
    h->dump_dev = static_cast<float*>(dev); h->dump_stride = (size_t)stride_floats;
    return GPSAT_OK;
}
#endif

int gpsat_max_inducing(int dtype, int D) {
    if (D < 1 || D > 4 || dtype != GPSAT_F64) return 0;       // fp32 SGPR is not built (a 1e-6 jitter on an fp32 Cholesky)
    return GPSAT_MAX_INDUCING;
}

int gpsat_sgpr_fit_predict_batch(gpsat_handle* h, const gpsat_batch* b, const gpsat_sparse* sp) {
    if (!h || !b) return fail(GPSAT_EINVAL, "gpsat_sgpr_fit_predict_batch: NULL handle or batch");
    if (!sp || !sp->z_off) return fail(GPSAT_EINVAL, "gpsat_sgpr_fit_predict_batch: NULL sparse description or z_off");
    if (b->T == 0) return GPSAT_OK;
    BatchDims d;
    int rc;
    if ((rc = check_batch(b, true, d))) return rc;
    if ((rc = check_rq(b, "gpsat_sgpr_fit_predict_batch"))) return rc;
    if (b->cov_off || b->f_cov) return fail(GPSAT_EINVAL, "sparse GP experts do not return the full covariance: cov_off / f_cov must be NULL");
    if (!(sp->jitter >= 0.0) || !std::isfinite(sp->jitter)) return fail(GPSAT_EINVAL, "jitter must be finite and >= 0");
    const int T = b->T, D = b->D;
    const int mlim = gpsat_max_inducing(b->dtype, D);
    if (sp->z_off[0] != 0) return fail(GPSAT_EINVAL, "offsets must start at 0");
    int Mmax = 1;
    for (int t = 0; t < T; ++t) {
        const long long n = b->obs_off[t + 1] - b->obs_off[t], p = b->pred_off[t + 1] - b->pred_off[t];
        const long long m = sp->z_off[t + 1] - sp->z_off[t];
        if (n > 0x7fffffffLL || p > 0x7fffffffLL) return fail(GPSAT_EINVAL, "a tile holds more than 2^31-1 rows");
        if (m < 1 || m > mlim)
            return fail(GPSAT_EINVAL, "every tile needs 1.." + std::to_string(mlim) + " inducing points (gpsat_max_inducing); tile " +
                                          std::to_string(t) + " has " + std::to_string(m));
        Mmax = std::max(Mmax, (int)m);
    }
    d.sumM = sp->z_off[T];
    if (!sp->Z) return fail(GPSAT_EINVAL, "Z is NULL");
    if ((rc = check_batch_data(b, d))) return rc;
    const size_t smem = gpsat::sgpr_shared_bytes(D, Mmax);
    if (smem > 160 * 1024) return fail(GPSAT_EINVAL, "inducing points do not fit the LDS");

    if ((rc = begin_call(h))) return rc;
    // tile order: largest cost first (N M^2), stable.  Pageable host memory that a copy reads: alive until the final synchronise
    std::vector<int> order(T);
    std::iota(order.begin(), order.end(), 0);
    auto cost = [&](int t) {
        const double m = (double)(sp->z_off[t + 1] - sp->z_off[t]);
        return (double)(b->obs_off[t + 1] - b->obs_off[t]) * m * m + m * m * m;
    };
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return cost(a) > cost(c); });
    // one workgroup per CU; the workspaces together stay below 16 GiB
    const size_t wsd = gpsat::sgpr_workspace_doubles_per_wg(D, Mmax);
    int grid = std::min(T, h->num_cu);
    grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)16 << 30) / (wsd * sizeof(double))));
    Staged s;
    if ((rc = stage_batch(h, b, d, b->theta0, order, sp->z_off, sp->Z, (size_t)grid * wsd * sizeof(double), s))) return rc;

    gpsat::SgprArgs a;
    fill_common_args(a, b, s);
    a.Mmax = Mmax;
    a.jitter = sp->jitter > 0.0 ? sp->jitter : 1e-6;
    a.z_off = s.i64 + 2 * (T + 1);
    a.Z = reinterpret_cast<const double*>(s.Z);
    a.ws = static_cast<double*>(h->ws.p); a.ws_stride = wsd;

    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(gpsat::launch_sgpr(D, a, grid, smem, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    if ((rc = fetch_batch(h, b, d, s))) return rc;
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return record_timing(h);
}


int gpsat_select_batch(gpsat_handle* h, const gpsat_select_spec* sp, int64_t M, int32_t C, const double* points,
                       int32_t T, const double* refs, int64_t* off, int32_t* idx, int64_t capacity) {
    return gpsat_select_batch_ex(h, sp, M, C, points, T, refs, 0, nullptr, off, idx, capacity);
}

int gpsat_select_batch_ex(gpsat_handle* h, const gpsat_select_spec* sp, int64_t M, int32_t C, const double* points,
                          int32_t T, const double* refs, int32_t n_bounds, const double* bounds, int64_t* off, int32_t* idx,
                          int64_t capacity) {
    if (!h || !sp || !off) return fail(GPSAT_EINVAL, "gpsat_select_batch: NULL argument");
    if (T < 0 || M < 0 || C < 1 || n_bounds < 0) return fail(GPSAT_EINVAL, "gpsat_select_batch: bad sizes");
    if (M > 2147483647LL) return fail(GPSAT_EINVAL, "gpsat_select_batch: more than 2^31-1 rows");
    gpsat::SelectArgs a;
    std::memset(&a, 0, sizeof(a));
    const std::string bad = gpsat::select_check_spec(sp, C, n_bounds, a);
    if (!bad.empty()) return fail(GPSAT_EINVAL, bad);
    off[0] = 0;
    if (T == 0) return GPSAT_OK;
    if ((M > 0 && !points) || !refs || (n_bounds > 0 && !bounds)) return fail(GPSAT_EINVAL, "gpsat_select_batch: NULL table");
    const gpsat::SelectCache::Call call = {sp, M, C, points, T, refs, n_bounds, bounds};
    if (idx && h->selc.matches(call)) return select_from_cache(h, T, off, idx, capacity);
    int rc;
    if ((rc = begin_call(h))) return rc;
    gpsat_handle::SelectBufs& sb = h->sel;
    // ---- stage: the tables to the device, one count per (expert, row chunk) cell
    if ((rc = sb.pts.reserve(std::max<size_t>((size_t)M * C, 1) * sizeof(double)))) return rc;
    if ((rc = sb.refs.reserve((size_t)T * C * sizeof(double)))) return rc;
    const long long sub = gpsat::select_sub_rows();             // rows per bounding box: chunks are whole numbers of them
    const gpsat::SelectChunks ch = gpsat::select_chunks(M, T, sub);
    const size_t ncell = (size_t)T * ch.n_chunks;
    if ((rc = sb.cnt.reserve(2 * ncell * sizeof(long long)))) return rc;
    if (M > 0) HIP_TRY(hipMemcpyAsync(sb.pts.p, points, (size_t)M * C * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(sb.refs.p, refs, (size_t)T * C * sizeof(double), hipMemcpyHostToDevice, h->stream));
    a.n_bounds = n_bounds;
    a.bounds = nullptr;
    if (n_bounds > 0) {
        const size_t nB = (size_t)T * n_bounds * 2;
        if ((rc = sb.bnd.reserve(nB * sizeof(double)))) return rc;
        HIP_TRY(hipMemcpyAsync(sb.bnd.p, bounds, nB * sizeof(double), hipMemcpyHostToDevice, h->stream));
        a.bounds = static_cast<const double*>(sb.bnd.p);
    }
    a.M = M; a.C = C; a.T = T;
    a.n_chunks = ch.n_chunks; a.chunk_rows = ch.chunk_rows;
    a.eorder = nullptr;
    a.pts = static_cast<const double*>(sb.pts.p);
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    // ---- bin (gpsat_select.hip): large tables are sorted on the device by the grid cell of the criteria's columns, and the
    // experts are dealt to the waves in the order of their own cells
    gpsat::BinSpec bin = {};
    if (M >= 65536 && !dev_env("GPSAT_DEBUG_NO_BINNING")) bin = gpsat::select_bin_dims(a, points, M, C);
    const int* d_perm = nullptr;
    if (bin.ndim > 0 && (rc = select_bin_table(h, bin, refs, a, d_perm))) return rc;
    a.refs = static_cast<const double*>(sb.refs.p);
    a.counts = static_cast<long long*>(sb.cnt.p);
    // ---- boxes: per-column [min, max] of every `sub` rows, which let a wave skip sub-chunks none of its experts can select from
    a.box = nullptr;
    if (M > 0) {
        const size_t nsub = (size_t)((M + sub - 1) / sub);
        if ((rc = sb.box.reserve(nsub * C * 2 * sizeof(double)))) return rc;
        HIP_TRY(gpsat::launch_select_boxes(M, C, a.pts, static_cast<double*>(sb.box.p), h->stream));
        a.box = static_cast<const double*>(sb.box.p);
    }
    // ---- count, scan on the host (cnt becomes the start offset of every cell)
    HIP_TRY(gpsat::launch_select(a, false, h->stream));
    std::vector<long long> cnt(ncell);
    HIP_TRY(hipMemcpyAsync(cnt.data(), a.counts, ncell * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    gpsat::select_scan(cnt.data(), T, ch.n_chunks, off);
    if (idx && capacity < off[T]) return fail(GPSAT_EINVAL, "gpsat_select_batch: idx capacity too small (see off[T])");
    // ---- fill, unbin, fetch
    const int* d_result = nullptr;
    if (off[T] > 0) {
        if ((rc = sb.idx.reserve((size_t)off[T] * sizeof(int)))) return rc;
        long long* d_off = static_cast<long long*>(sb.cnt.p) + ncell;
        HIP_TRY(hipMemcpyAsync(d_off, cnt.data(), ncell * sizeof(long long), hipMemcpyHostToDevice, h->stream));
        a.off = d_off;
        a.idx = static_cast<int*>(sb.idx.p);
        HIP_TRY(gpsat::launch_select(a, true, h->stream));
        d_result = a.idx;
        if (d_perm && (rc = select_unbin_indices(h, M, T, off, d_perm, a.idx, d_result))) return rc;
        HIP_TRY(hipEventRecord(h->ev[2], h->stream));
        if (idx) HIP_TRY(hipMemcpyAsync(idx, d_result, (size_t)off[T] * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    } else {
        HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if ((rc = record_timing(h))) return rc;                     // kernel time: count + scan round trip + fill
    // sizes asked for: the indices stay on the device for the call that follows with the same arguments
    if (!idx) h->selc.remember(call, off, d_result);
    return GPSAT_OK;
}

int gpsat_bin_batch(gpsat_handle* h, int64_t R, const double* x, const double* y, const double* v, const int32_t* gid,
                    int32_t G, int32_t nx, const double* ex, double x_hi, int32_t ny, const double* ey, double y_hi,
                    uint32_t stats, int64_t capacity, int64_t* n_cells, int64_t* keys, double* out) {
    if (!h || !n_cells) return fail(GPSAT_EINVAL, "gpsat_bin_batch: NULL handle or n_cells");
    *n_cells = 0;
    const std::string bad = gpsat::bin_check(R, x, y, v, gid, G, nx, ex, x_hi, ny, ey, y_hi, stats, capacity);
    if (!bad.empty()) return fail(GPSAT_EINVAL, bad);
    if (R == 0 || G == 0) return GPSAT_OK;
    const bool two_d = y != nullptr, median = (stats & GPSAT_BIN_MEDIAN) != 0;
    const gpsat::BinLayout l = gpsat::bin_layout(R, nx, ny, two_d, gid != nullptr, median, gpsat::bin_long_rows());
    const gpsat::BinScales sc = gpsat::bin_scales(nx, ex, ny, ey, two_d, G, stats);
    int rc;
    if ((rc = begin_call(h))) return rc;
    gpsat_handle::BinBufs& bb = h->bin;
    if ((rc = bb.in.reserve(l.in_bytes))) return rc;
    if ((rc = bb.vals.reserve(l.vals_bytes))) return rc;
    if ((rc = bb.kr.reserve(l))) return rc;
    // ---- stage: edges and columns to the device
    const size_t nR = (size_t)R;
    gpsat::BinArgs a;
    std::memset(&a, 0, sizeof(a));
    a.R = R; a.nx = nx; a.ny = two_d ? ny : 2;
    char* d_in = static_cast<char*>(bb.in.p);
    double* d_e = reinterpret_cast<double*>(d_in);
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    HIP_TRY(hipMemcpyAsync(d_e, ex, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
    a.ex = d_e;
    if (two_d) {
        HIP_TRY(hipMemcpyAsync(d_e + nx, ey, (size_t)ny * sizeof(double), hipMemcpyHostToDevice, h->stream));
        a.ey = d_e + nx;
    }
    HIP_TRY(hipMemcpyAsync(d_in + l.in_x, x, nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
    a.x = reinterpret_cast<const double*>(d_in + l.in_x);
    HIP_TRY(hipMemcpyAsync(d_in + l.in_v, v, nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
    a.v = reinterpret_cast<const double*>(d_in + l.in_v);
    if (two_d) {
        HIP_TRY(hipMemcpyAsync(d_in + l.in_y, y, nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
        a.y = reinterpret_cast<const double*>(d_in + l.in_y);
    }
    if (gid) {
        HIP_TRY(hipMemcpyAsync(d_in + l.in_gid, gid, nR * sizeof(int), hipMemcpyHostToDevice, h->stream));
        a.gid = reinterpret_cast<const int*>(d_in + l.in_gid);
    }
    a.x_hi = x_hi; a.y_hi = y_hi;
    a.inv_x = sc.inv_x; a.inv_y = sc.inv_y; a.sentinel = sc.sentinel;
    bb.kr.bind(a);
    a.vs = static_cast<double*>(bb.vals.p);
    if (median) { a.vcanon = a.vs + nR; a.vsorted = a.vs + 2 * nR; }
    char* d_runs = static_cast<char*>(bb.kr.runs.p);
    a.n_long = reinterpret_cast<unsigned*>(d_runs + l.runs_n_long);
    a.long_list = reinterpret_cast<unsigned*>(d_runs + l.runs_long_list);
    a.mask = stats;
    // ---- sort (the kernel time starts once its scratch is there), read the counts
    if ((rc = run_with_temp(h, bb.kr.tmp, "bin_sort_rows", h->ev[1], [&](void* temp, size_t& tb) { return gpsat::bin_sort_rows(a, temp, tb, h->stream); })))
        return rc;
    long long info[2];
    if ((rc = read_key_run_counts(h, a, info))) return rc;
    const long long nc = info[0], n_valid = info[1];
    *n_cells = nc;
    // ---- stats, fetch
    if (nc > 0 && capacity >= nc) {
        if (!keys || !out) return fail(GPSAT_EINVAL, "gpsat_bin_batch: keys / out is NULL");
        if ((rc = bb.out.reserve((size_t)nc * (sc.n_stat + 1) * sizeof(double)))) return rc;
        a.out_keys = static_cast<long long*>(bb.out.p);
        a.out = reinterpret_cast<double*>(a.out_keys + nc);
        if ((rc = run_with_temp(h, bb.kr.tmp, "bin_cell_stats", nullptr,
                                [&](void* temp, size_t& tb) { return gpsat::bin_cell_stats(a, nc, n_valid, temp, tb, h->stream); })))
            return rc;
        HIP_TRY(hipEventRecord(h->ev[2], h->stream));
        HIP_TRY(hipMemcpyAsync(keys, a.out_keys, (size_t)nc * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        for (int s = 0; s < sc.n_stat; ++s)
            HIP_TRY(hipMemcpyAsync(out + (size_t)s * capacity, a.out + (size_t)s * nc, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
        HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if ((rc = record_timing(h))) return rc;
    if (capacity < nc) return fail(GPSAT_EINVAL, "gpsat_bin_batch: capacity " + std::to_string(capacity) + " < n_cells " + std::to_string(nc));
    return GPSAT_OK;
}

int gpsat_smooth_batch(gpsat_handle* h, int32_t T, const double* x, const double* y, const double* vals, double l_x,
                       double l_y, double* out) {
    if (!h || T < 0 || (T > 0 && (!x || !y || !vals || !out))) return fail(GPSAT_EINVAL, "gpsat_smooth_batch: bad argument");
    if (!(l_x > 0.0) || !(l_y > 0.0)) return fail(GPSAT_EINVAL, "gpsat_smooth_batch: length scales must be positive");
    if (T == 0) return GPSAT_OK;
    int rc;
    if ((rc = begin_call(h))) return rc;
    if ((rc = h->sel.pts.reserve((size_t)4 * T * sizeof(double)))) return rc;
    double* d = static_cast<double*>(h->sel.pts.p);
    HIP_TRY(hipMemcpyAsync(d, x, (size_t)T * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d + T, y, (size_t)T * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d + 2 * (size_t)T, vals, (size_t)T * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(gpsat::launch_smooth(T, d, d + T, d + 2 * (size_t)T, l_x, l_y, d + 3 * (size_t)T, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    HIP_TRY(hipMemcpyAsync(out, d + 3 * (size_t)T, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return record_timing(h, 1, 2);                              // no ev[0] / ev[3] here: the total is the kernel time
}

int gpsat_glue_batch(gpsat_handle* h, int64_t R, int32_t G, int32_t ndim, int32_t nvars, const int64_t* seg,
                     const double* pred, const double* xprt, const double* vals, double sigma,
                     const double* sigma_rows, double* out) {
    if (!h || R < 0 || G < 0) return fail(GPSAT_EINVAL, "gpsat_glue_batch: bad sizes");
    if (ndim < 1 || ndim > 2 || nvars < 1 || nvars > GPSAT_GLUE_MAXVARS) return fail(GPSAT_EINVAL, "gpsat_glue_batch: ndim 1..2, nvars 1..4");
    if (!sigma_rows && !(sigma > 0.0)) return fail(GPSAT_EINVAL, "gpsat_glue_batch: sigma must be positive");
    if (G == 0) return GPSAT_OK;
    if (!seg || !pred || !xprt || !vals || !out) return fail(GPSAT_EINVAL, "gpsat_glue_batch: NULL argument");
    if (seg[0] != 0 || seg[G] != R) return fail(GPSAT_EINVAL, "gpsat_glue_batch: seg must run from 0 to R");
    int rc;
    if ((rc = begin_call(h))) return rc;
    const size_t nd = (size_t)(2 * ndim + nvars + 1) * R + (size_t)nvars * G;
    if ((rc = h->sel.pts.reserve(std::max<size_t>(nd, 1) * sizeof(double)))) return rc;
    if ((rc = h->sel.cnt.reserve((size_t)(G + 1) * sizeof(long long)))) return rc;
    double* d = static_cast<double*>(h->sel.pts.p);
    double* dp = d; double* dx = d + (size_t)ndim * R; double* dv = dx + (size_t)ndim * R; double* dsig = dv + (size_t)nvars * R; double* dout = dsig + R;
    HIP_TRY(hipMemcpyAsync(dp, pred, (size_t)ndim * R * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dx, xprt, (size_t)ndim * R * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dv, vals, (size_t)nvars * R * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (sigma_rows) HIP_TRY(hipMemcpyAsync(dsig, sigma_rows, (size_t)R * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->sel.cnt.p, seg, (size_t)(G + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(gpsat::launch_glue(G, ndim, nvars, R, static_cast<const long long*>(h->sel.cnt.p), dp, dx, dv, sigma, sigma_rows ? dsig : nullptr, dout, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    HIP_TRY(hipMemcpyAsync(out, dout, (size_t)nvars * G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return record_timing(h, 1, 2);                              // no ev[0] / ev[3] here: the total is the kernel time
}

// What the keyed glue of order 1 (grad [ndim][R] -> out_grad [ndim][capacity]) and of order 2 (hess [npair][R] -> out_hess
// [npair][capacity] as well) has beside the columns of order 0; nullptr where the order has none.
struct GlueKeyedDerivs { const double *grad, *hess; double *out_grad, *out_hess; };

// The three keyed glues behind their checks (gpsat_glue_plan.h): key range -> stage -> sort, run heads -> read the group count
// -> reduce -> fetch.  Order 0: gpsat_glue_keyed_batch, vals [nvars][R] -> out [nvars][capacity].  Order 1:
// gpsat_glue_keyed_grad_batch, nvars is 1, vals the value [R] -> out the glued value [capacity].  Order 2:
// gpsat_glue_keyed_hess_batch.  The value columns, the gradient and the second derivatives are staged one behind the other as
// nvars + ndim + npair columns of the layout, and so are their outputs.
static int glue_keyed_run(gpsat_handle* h, int order, int64_t R, int32_t ndim, int32_t nvars, const int64_t* key, const double* pred,
                          const double* xprt, const double* vals, const GlueKeyedDerivs& dv, double sigma, const double* sigma_rows,
                          double max_dist, int64_t capacity, int64_t* G, int64_t* out_key, int32_t* out_count, double* out) {
    char why[160];
    int rc;
    const int ngrad = order >= 1 ? ndim : 0, npair = order >= 2 ? ndim * (ndim + 1) / 2 : 0;
    const int ncols = nvars + ngrad + npair;
    *G = 0;
    h->glue.ms[0] = h->glue.ms[1] = h->glue.ms[2] = 0.0;
    const unsigned long long sentinel = gpsat::glue_keyed_sentinel(R, key);
    if (sentinel == 0) return GPSAT_OK;                         // no row, or no key >= 0
    int team = gpsat::glue_keyed_team();
    if (const char* e = dev_env("GPSAT_DEBUG_GLUE_TEAM")) team = std::atoi(e);       // scripts/cv_glue_bench.py
    if (team != 1 && team != 4 && team != 8 && team != 16 && team != 32 && team != 64)
        return fail(GPSAT_EINVAL, "GPSAT_DEBUG_GLUE_TEAM must be 1, 4, 8, 16, 32 or 64");
    const gpsat::GlueKeyedLayout l = gpsat::glue_keyed_layout(R, ndim, ncols);
    if ((rc = begin_call(h))) return rc;
    gpsat_handle::GlueBufs& gb = h->glue;
    for (hipEvent_t& ev : gb.ev)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    if ((rc = gb.in.reserve(l.in_bytes))) return rc;
    if ((rc = gb.kr.reserve(l))) return rc;
    // ---- stage
    const size_t nR = (size_t)R;
    gpsat::GlueKeyedOrderArgs a;
    std::memset(&a, 0, sizeof(a));
    a.R = R; a.ndim = ndim; a.nvars = nvars; a.sentinel = sentinel;
    a.sigma = sigma; a.md2 = gpsat::glue_keyed_md2(max_dist);
    char* d_in = static_cast<char*>(gb.in.p);
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    HIP_TRY(hipMemcpyAsync(d_in, key, nR * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_in + l.in_pred, pred, (size_t)ndim * nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_in + l.in_xprt, xprt, (size_t)ndim * nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
    double* d_vals = reinterpret_cast<double*>(d_in + l.in_vals);
    double *d_grad = d_vals + (size_t)nvars * nR, *d_hess = d_grad + (size_t)ngrad * nR;    // behind the value columns, behind the gradient
    HIP_TRY(hipMemcpyAsync(d_vals, vals, (size_t)nvars * nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (ngrad) HIP_TRY(hipMemcpyAsync(d_grad, dv.grad, (size_t)ngrad * nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (npair) HIP_TRY(hipMemcpyAsync(d_hess, dv.hess, (size_t)npair * nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (sigma_rows) HIP_TRY(hipMemcpyAsync(d_in + l.in_sigma, sigma_rows, nR * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const long long* d_key = reinterpret_cast<const long long*>(d_in);
    a.pred = reinterpret_cast<const double*>(d_in + l.in_pred);
    a.xprt = reinterpret_cast<const double*>(d_in + l.in_xprt);
    a.vals = d_vals;
    a.grad = ngrad ? d_grad : nullptr;
    a.hess = npair ? d_hess : nullptr;
    a.sigma_rows = sigma_rows ? reinterpret_cast<const double*>(d_in + l.in_sigma) : nullptr;
    gb.kr.bind(a);
    // ---- sort and run heads (the kernel time starts once the scratch is there), read the counts
    if ((rc = run_with_temp(h, gb.kr.tmp, "glue_keyed_sort", h->ev[1],
                            [&](void* temp, size_t& tb) { return gpsat::glue_keyed_sort(a, d_key, temp, tb, gb.ev[0], h->stream); })))
        return rc;
    HIP_TRY(hipEventRecord(gb.ev[1], h->stream));
    long long info[2];
    if ((rc = read_key_run_counts(h, a, info))) return rc;
    const long long ng = info[0];
    *G = ng;
    // ---- reduce, fetch
    if (ng > 0 && capacity >= ng) {
        const size_t nG = (size_t)ng;
        if ((rc = gb.out.reserve(nG * ((size_t)ncols + 1) * sizeof(double) + nG * sizeof(int)))) return rc;
        a.out_key = static_cast<long long*>(gb.out.p);
        a.out = reinterpret_cast<double*>(a.out_key + nG);
        a.out_count = reinterpret_cast<int*>(a.out + (size_t)ncols * nG);
        a.out_grad = ngrad ? a.out + (size_t)nvars * nG : nullptr;                    // behind the value columns
        a.out_hess = npair ? a.out + (size_t)(nvars + ngrad) * nG : nullptr;          // behind the slope
        HIP_TRY(hipEventRecord(gb.ev[2], h->stream));           // behind the reservation
        HIP_TRY(gpsat::launch_glue_keyed(a, ng, team, order, h->stream));
        HIP_TRY(hipEventRecord(h->ev[2], h->stream));
        HIP_TRY(hipMemcpyAsync(out_key, a.out_key, nG * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(out_count, a.out_count, nG * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        const struct { double* host; const double* dev; int n; } outs[3] = {{out, a.out, nvars}, {dv.out_grad, a.out_grad, ngrad}, {dv.out_hess, a.out_hess, npair}};
        for (const auto& o : outs)
            for (int c = 0; c < o.n; ++c)
                HIP_TRY(hipMemcpyAsync(o.host + (size_t)c * capacity, o.dev + (size_t)c * nG, nG * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
        HIP_TRY(hipEventRecord(gb.ev[2], h->stream));           // no reduction: an empty interval
        HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if ((rc = record_timing(h))) return rc;                     // kernel time: keys, sort, run heads, count round trip, reduce
    float ms[3] = {0.f, 0.f, 0.f};
    HIP_TRY(hipEventElapsedTime(&ms[0], h->ev[1], gb.ev[0]));
    HIP_TRY(hipEventElapsedTime(&ms[1], gb.ev[0], gb.ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms[2], gb.ev[2], h->ev[2]));
    for (int i = 0; i < 3; ++i) gb.ms[i] = ms[i];
    if ((rc = gpsat::check_glue_capacity(capacity, ng, why, sizeof(why)))) return fail(rc, why);
    return GPSAT_OK;
}

int gpsat_glue_keyed_batch(gpsat_handle* h, int64_t R, int32_t ndim, int32_t nvars, const int64_t* key, const double* pred,
                           const double* xprt, const double* vals, double sigma, const double* sigma_rows, double max_dist,
                           int64_t capacity, int64_t* G, int64_t* out_key, int32_t* out_count, double* out) {
    if (!h) return fail(GPSAT_EINVAL, "gpsat_glue_keyed_batch: handle is NULL");
    char why[160];
    if (int rc = gpsat::check_glue_keyed(R, ndim, nvars, key, pred, xprt, vals, sigma, sigma_rows, max_dist, capacity, G, out_key,
                                         out_count, out, why, sizeof(why)))
        return fail(rc, why);
    return glue_keyed_run(h, 0, R, ndim, nvars, key, pred, xprt, vals, {nullptr, nullptr, nullptr, nullptr}, sigma, sigma_rows, max_dist,
                          capacity, G, out_key, out_count, out);
}

int gpsat_glue_keyed_grad_batch(gpsat_handle* h, int64_t R, int32_t ndim, const int64_t* key, const double* pred,
                                const double* xprt, const double* val, const double* grad, double sigma, const double* sigma_rows,
                                double max_dist, int64_t capacity, int64_t* G, int64_t* out_key, int32_t* out_count,
                                double* out_val, double* out_grad) {
    if (!h) return fail(GPSAT_EINVAL, "gpsat_glue_keyed_grad_batch: handle is NULL");
    char why[160];
    if (int rc = gpsat::check_glue_keyed_grad(R, ndim, key, pred, xprt, val, grad, sigma, sigma_rows, max_dist, capacity, G, out_key,
                                              out_count, out_val, out_grad, why, sizeof(why)))
        return fail(rc, why);
    return glue_keyed_run(h, 1, R, ndim, 1, key, pred, xprt, val, {grad, nullptr, out_grad, nullptr}, sigma, sigma_rows, max_dist,
                          capacity, G, out_key, out_count, out_val);
}

int gpsat_glue_keyed_hess_batch(gpsat_handle* h, int64_t R, int32_t ndim, const int64_t* key, const double* pred,
                                const double* xprt, const double* val, const double* grad, const double* hess, double sigma,
                                const double* sigma_rows, double max_dist, int64_t capacity, int64_t* G, int64_t* out_key,
                                int32_t* out_count, double* out_val, double* out_grad, double* out_hess) {
    if (!h) return fail(GPSAT_EINVAL, "gpsat_glue_keyed_hess_batch: handle is NULL");
    char why[160];
    if (int rc = gpsat::check_glue_keyed_hess(R, ndim, key, pred, xprt, val, grad, hess, sigma, sigma_rows, max_dist, capacity, G,
                                              out_key, out_count, out_val, out_grad, out_hess, why, sizeof(why)))
        return fail(rc, why);
    return glue_keyed_run(h, 2, R, ndim, 1, key, pred, xprt, val, {grad, hess, out_grad, out_hess}, sigma, sigma_rows, max_dist,
                          capacity, G, out_key, out_count, out_val);
}

int gpsat_glue_keyed_timing(gpsat_handle* h, double* ms) {
    if (!h || !ms) return fail(GPSAT_EINVAL, "gpsat_glue_keyed_timing: NULL argument");
    for (int i = 0; i < 3; ++i) ms[i] = h->glue.ms[i];
    return GPSAT_OK;
}

// check (gpsat_prep_plan.h) -> constants -> stage (host mode) -> kernel -> fetch (host mode)
int gpsat_project_batch(gpsat_handle* h, const gpsat_project* p) {
    if (!h) return fail(GPSAT_EINVAL, "gpsat_project_batch: handle is NULL");
    char why[160];
    int rc;
    if ((rc = gpsat::check_project(p, why, sizeof(why)))) return fail(rc, why);
    if (p->n == 0) return GPSAT_OK;
    const gpsat::ProjConst pc = gpsat::proj_const();
    if ((rc = begin_call(h))) return rc;
    const size_t nb = (size_t)p->n * sizeof(double);
    const bool host = p->memory == GPSAT_MEM_HOST;
    gpsat::ProjectArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = p->n; a.lon_0 = p->lon_0;
    a.a = pc.a; a.e = pc.e; a.e2 = pc.e2; a.one_m_e2 = pc.one_m_e2; a.inv_2e = pc.inv_2e; a.qp = pc.qp; a.qp_lo = pc.qp_lo;
    a.in0 = p->in0; a.in1 = p->in1; a.out0 = p->out0; a.out1 = p->out1;
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    if (host) {
        if ((rc = h->prep.in.reserve(2 * nb))) return rc;
        if ((rc = h->prep.out.reserve(2 * nb))) return rc;
        double* d_in = static_cast<double*>(h->prep.in.p);
        double* d_out = static_cast<double*>(h->prep.out.p);
        HIP_TRY(hipMemcpyAsync(d_in, p->in0, nb, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(d_in + p->n, p->in1, nb, hipMemcpyHostToDevice, h->stream));
        a.in0 = d_in; a.in1 = d_in + p->n; a.out0 = d_out; a.out1 = d_out + p->n;
    }
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    HIP_TRY(gpsat::launch_project(a, p->direction == GPSAT_PROJECT_FORWARD, p->lat_0 < 0.0, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    if (host) {
        HIP_TRY(hipMemcpyAsync(p->out0, a.out0, nb, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(p->out1, a.out1, nb, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return record_timing(h);
}

// check (gpsat_prep_plan.h) -> layout -> stage (host mode) -> with groups: keys, sort, run heads (the keyed glue's) -> distances
// and flags, scan -> fetch (host mode)
int gpsat_track_batch(gpsat_handle* h, const gpsat_track* t) {
    if (!h) return fail(GPSAT_EINVAL, "gpsat_track_batch: handle is NULL");
    char why[160];
    int rc;
    unsigned long long sentinel = 0;
    if ((rc = gpsat::check_track(t, &sentinel, why, sizeof(why)))) return fail(rc, why);
    if (t->n == 0) return GPSAT_OK;
    const bool host = t->memory == GPSAT_MEM_HOST, grouped = t->group != nullptr;
    const gpsat::TrackLayout l = gpsat::track_layout(t->n, t->n_cols, grouped, host, gpsat::prep_scan_block());
    if ((rc = begin_call(h))) return rc;
    gpsat_handle::PrepBufs& pb = h->prep;
    if ((rc = pb.in.reserve(std::max<size_t>(l.in_bytes, 16)))) return rc;
    if ((rc = pb.out.reserve(l.out_bytes))) return rc;
    if (grouped && (rc = pb.kr.reserve(l))) return rc;
    const size_t nN = (size_t)t->n;
    char* d_in = static_cast<char*>(pb.in.p);
    char* d_out = static_cast<char*>(pb.out.p);
    gpsat::TrackArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = t->n; a.n_cols = t->n_cols; a.mode = t->mode;
    a.cut_off = t->cut_off; a.start_track = t->start_track;
    const int32_t* d_group = t->group;
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    if (host) {
        for (int c = 0; c < t->n_cols; ++c) {
            double* d_c = reinterpret_cast<double*>(d_in + l.in_cols) + (size_t)c * nN;
            HIP_TRY(hipMemcpyAsync(d_c, t->cols[c], nN * sizeof(double), hipMemcpyHostToDevice, h->stream));
            a.cols[c] = d_c;
        }
        if (grouped) {
            HIP_TRY(hipMemcpyAsync(d_in + l.in_group, t->group, nN * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            d_group = reinterpret_cast<const int32_t*>(d_in + l.in_group);
        }
        a.delta = reinterpret_cast<double*>(d_out);
        a.track = reinterpret_cast<int*>(d_out + l.out_track);
        a.order = reinterpret_cast<int*>(d_out + l.out_order);
    } else {
        for (int c = 0; c < t->n_cols; ++c) a.cols[c] = t->cols[c];
        a.delta = t->out_delta; a.track = t->out_track; a.order = t->out_order;
    }
    a.block_sums = reinterpret_cast<int*>(d_out + l.out_sums);
    if (grouped) {
        gpsat::KeyRuns g;
        std::memset(&g, 0, sizeof(g));
        g.R = t->n; g.sentinel = sentinel;
        pb.kr.bind(g);
        long long* d_key = reinterpret_cast<long long*>(d_in + l.in_key);
        // the kernel time starts in front of the keys, once the sort's scratch is there
        if ((rc = run_with_temp(h, pb.kr.tmp, "glue_keyed_sort", h->ev[1], [&](void* temp, size_t& tb) {
                if (temp) {
                    const hipError_t e = gpsat::launch_track_keys(t->n, d_group, d_key, h->stream);
                    if (e != hipSuccess) return e;
                }
                return gpsat::glue_keyed_sort(g, d_key, temp, tb, nullptr, h->stream);
            })))
            return rc;
        a.perm = g.perm; a.heads = g.flags; a.n_valid = g.counts + 1;
    } else {
        HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    }
    HIP_TRY(gpsat::launch_track(a, h->stream));
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    if (host) {
        if (t->mode != GPSAT_TRACK_RUNS) HIP_TRY(hipMemcpyAsync(t->out_delta, a.delta, nN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(t->out_track, a.track, nN * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(t->out_order, a.order, nN * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return record_timing(h);
}

#ifdef GPSAT_PROFILE
// diagnostic build only: per-wave, per-segment cycle counters of the last call ([4 waves][16 slots])
int gpsat_debug_profile(gpsat_handle* h, unsigned long long* out64) {
    if (!h || !out64) return GPSAT_EINVAL;
    std::memcpy(out64, h->prof_host, 64 * sizeof(unsigned long long));
    return GPSAT_OK;
}
// per-workgroup first-tile start and kernel-exit times in 100 MHz ticks: [1024] starts then [1024] ends
int gpsat_debug_spans(gpsat_handle* h, unsigned long long* out2048) {
    if (!h || !out2048) return GPSAT_EINVAL;
    std::memcpy(out2048, h->prof_host + 64 + 8 * 1024, 2048 * sizeof(unsigned long long));
    return GPSAT_OK;
}
// per-workgroup time it first found the time-sliced ring without a waiting tile (100 MHz ticks, 0 = never) and its CU
// (XCC_ID << 8 | HW_ID[15:8]): [1024] times then [1024] CUs
int gpsat_debug_idle(gpsat_handle* h, unsigned long long* out2048) {
    if (!h || !out2048) return GPSAT_EINVAL;
    std::memcpy(out2048, h->prof_host + 64 + 8 * 1024 + 2048, 2048 * sizeof(unsigned long long));
    return GPSAT_OK;
}
// event trace of the first evaluation of workgroup 0: [8 waves][1024] entries (cycle << 16 | arg << 8 | code), 0 = unused
int gpsat_debug_trace(gpsat_handle* h, unsigned long long* out8192) {
    if (!h || !out8192) return GPSAT_EINVAL;
    std::memcpy(out8192, h->prof_host + 64, 8 * 1024 * sizeof(unsigned long long));
    return GPSAT_OK;
}
#endif

}  // extern "C"
