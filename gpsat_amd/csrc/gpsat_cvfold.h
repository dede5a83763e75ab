// gpsat_cvfold.h -- host side of gpsat_fit_predict_batch_cv_refit: the caller's fold labels as the tables the two kernels of
// gpsat_cvfold.hip read, and the derived batch (one tile per fitted fold).  Plain C++ without a HIP call, so that
// gpsat_cv_refit_count works without a GPU and tests/cvfold_host_check.cpp can run it under the host sanitizers.
#ifndef GPSAT_CVFOLD_H
#define GPSAT_CVFOLD_H

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace gpsat {

// Folds of a tile are numbered by ascending label (stable sort, as check_cv numbers them); fold_off[t] + k is fold k of tile t.
// A fold's rows keep the order of the tile, so they ascend.
struct CvFoldTables {
    std::vector<int64_t> fold_off;     // [T+1]
    int64_t expanded_rows = 0;         // sum over folds of N_t - g
    std::vector<int> fold_ptr;         // [F+1] into fold_rows
    std::vector<int> fold_rows;        // [R] tile-local rows of every fold, ascending
    std::vector<int> fold_label, fold_tile, fold_n_obs;     // [F]; fold_n_obs = N_t - g
    std::vector<int> row_fold;         // [sumN] fold of the row (numbered over the batch), -1: never held out
    std::vector<int> row_pos;          // [sumN] position of the row in its fold
};

// `full` = false: fold_off and expanded_rows only (gpsat_cv_refit_count).  Returns an empty string, or what is wrong.
inline std::string cvfold_tables(int32_t T, const int64_t* obs_off, const int32_t* fold, bool full, CvFoldTables& tb) {
    if (T < 0) return "T < 0";
    if (!obs_off) return "obs_off is NULL";
    if (obs_off[0] != 0) return "offsets must start at 0";
    for (int t = 0; t < T; ++t)
        if (obs_off[t + 1] < obs_off[t]) return "offsets must be non-decreasing";
    const int64_t sumN = obs_off[T];
    if (sumN > 0x7fffffffLL) return "the batch holds more than 2^31-1 rows";
    if (sumN > 0 && !fold) return "fold is NULL";
    tb = CvFoldTables();
    tb.fold_off.assign((size_t)T + 1, 0);
    if (full) { tb.fold_ptr.assign(1, 0); tb.row_fold.assign((size_t)sumN, -1); tb.row_pos.assign((size_t)sumN, 0); }
    std::vector<int> idx;
    int64_t F = 0;
    for (int t = 0; t < T; ++t) {
        const int64_t o0 = obs_off[t];
        const int N = (int)(obs_off[t + 1] - o0);
        const int32_t* lab = fold + o0;
        idx.clear();
        for (int i = 0; i < N; ++i) if (lab[i] >= 0) idx.push_back(i);
        std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return lab[x] < lab[y]; });
        for (size_t s0 = 0; s0 < idx.size();) {
            size_t s1 = s0 + 1;
            while (s1 < idx.size() && lab[idx[s1]] == lab[idx[s0]]) ++s1;
            const int g = (int)(s1 - s0);
            if (F == 0x7fffffffLL) return "more than 2^31-1 folds";
            if (full) {
                for (size_t k = s0; k < s1; ++k) {
                    tb.row_fold[(size_t)(o0 + idx[k])] = (int)F; tb.row_pos[(size_t)(o0 + idx[k])] = (int)(k - s0);
                    tb.fold_rows.push_back(idx[k]);
                }
                tb.fold_ptr.push_back((int)tb.fold_rows.size());
                tb.fold_label.push_back(lab[idx[s0]]); tb.fold_tile.push_back(t); tb.fold_n_obs.push_back(N - g);
            }
            tb.expanded_rows += N - g;
            ++F;
            s0 = s1;
        }
        tb.fold_off[(size_t)t + 1] = F;
    }
    return std::string();
}

// The derived batch: one tile per fold that leaves at least max(min_obs, 1) rows, in fold order.
struct CvFoldDerived {
    std::vector<int> fold_derived;           // [F] derived tile of the fold, -1: not fitted
    std::vector<int> d_fold, d_src_n;        // [F2] fold and rows of the source tile
    std::vector<int64_t> d_src_off;          // [F2] first row of the source tile
    std::vector<int64_t> d_obs_off, d_pred_off;     // [F2+1] CSR offsets of the derived batch
};

inline void cvfold_derive(const CvFoldTables& tb, const int64_t* obs_off, int min_obs, CvFoldDerived& dv) {
    const size_t F = tb.fold_label.size();
    const int need = std::max(min_obs, 1);
    dv = CvFoldDerived();
    dv.fold_derived.assign(F, -1);
    dv.d_obs_off.assign(1, 0); dv.d_pred_off.assign(1, 0);
    for (size_t f = 0; f < F; ++f) {
        if (tb.fold_n_obs[f] < need) continue;
        const int t = tb.fold_tile[f], g = tb.fold_ptr[f + 1] - tb.fold_ptr[f];
        dv.fold_derived[f] = (int)dv.d_fold.size();
        dv.d_fold.push_back((int)f);
        dv.d_src_n.push_back((int)(obs_off[t + 1] - obs_off[t]));
        dv.d_src_off.push_back(obs_off[t]);
        dv.d_obs_off.push_back(dv.d_obs_off.back() + tb.fold_n_obs[f]);
        dv.d_pred_off.push_back(dv.d_pred_off.back() + g);
    }
}

// The joint density of the fitted folds (gpsat_fit_predict_batch_cv_refit_joint): the derived batch returns its posterior
// covariances, g_j x g_j per derived tile.  cov_off [F2+1] in elements, cov_off[j+1] - cov_off[j] = g_j^2.
inline std::vector<int64_t> cvfold_cov_off(const CvFoldDerived& dv) {
    const size_t F2 = dv.d_fold.size();
    std::vector<int64_t> off(F2 + 1, 0);
    for (size_t j = 0; j < F2; ++j) {
        const int64_t g = dv.d_pred_off[j + 1] - dv.d_pred_off[j];
        off[j + 1] = off[j] + g * g;
    }
    return off;
}

// The tables the two kernels read, packed for one copy each: a block of 64-bit words and a block of int32, laid out once for the
// host copy and the device.  Each block ends with F2 words that only the device holds (delta as doubles; d_status).
struct CvFoldPacked {
    std::vector<long long> t64;        // d_obs_off [F2+1], d_pred_off [F2+1], d_src_off [F2]
    size_t o_obs_off = 0, o_pred_off = 0, o_src_off = 0, o_delta = 0, n64 = 0;     // offsets into the 64-bit block, and its words
    std::vector<int> t32;              // d_src_n, d_fold [F2]; fold_ptr [F+1]; fold_rows [R]; fold_derived [F]; row_fold, row_pos [sumN]
    size_t o_src_n = 0, o_fold = 0, o_fold_ptr = 0, o_fold_rows = 0, o_fold_derived = 0, o_row_fold = 0, o_row_pos = 0, o_status = 0, n32 = 0;
};

inline CvFoldPacked cvfold_pack(const CvFoldTables& tb, const CvFoldDerived& dv) {
    CvFoldPacked p;
    const size_t F2 = dv.d_fold.size();
    auto put64 = [&](const std::vector<int64_t>& v, size_t& off) { off = p.t64.size(); p.t64.insert(p.t64.end(), v.begin(), v.end()); };
    put64(dv.d_obs_off, p.o_obs_off); put64(dv.d_pred_off, p.o_pred_off); put64(dv.d_src_off, p.o_src_off);
    p.o_delta = p.t64.size();
    p.n64 = p.t64.size() + F2;
    auto put = [&](const std::vector<int>& v, size_t& off) { off = p.t32.size(); p.t32.insert(p.t32.end(), v.begin(), v.end()); };
    put(dv.d_src_n, p.o_src_n); put(dv.d_fold, p.o_fold); put(tb.fold_ptr, p.o_fold_ptr); put(tb.fold_rows, p.o_fold_rows);
    put(dv.fold_derived, p.o_fold_derived); put(tb.row_fold, p.o_row_fold); put(tb.row_pos, p.o_row_pos);
    p.o_status = p.t32.size();
    p.n32 = p.t32.size() + F2;
    return p;
}

}  // namespace gpsat
#endif
