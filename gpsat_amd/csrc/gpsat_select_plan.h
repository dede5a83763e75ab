// gpsat_select_plan.h -- host side of gpsat_select_batch_ex: the checks of the criteria, the row chunks, the binning
// dimensions, the order of the experts, the scan of the cell counts and the two-call cache.  Plain C++ without a HIP call, in the
// manner of gpsat_cvfold.h, so that tests/select_bin_host_check.cpp can run it under the host sanitizers.  Part of
// gpsat_capi.cpp's translation unit.
#ifndef GPSAT_SELECT_PLAN_H
#define GPSAT_SELECT_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "gpsat_hip.h"
#include "gpsat_select_types.h"

namespace gpsat {

// The caller's criteria checked and normalised into `a` (a 1-D compare has one column; kind 2, the per-expert interval, keeps
// its bound index in cols[k][1] and is accepted only with bounds).  Returns an empty string, or what is wrong.
inline std::string select_check_spec(const gpsat_select_spec* sp, int C, int n_bounds, SelectCriteria& a) {
    if (sp->n_crit < 1 || sp->n_crit > GPSAT_SEL_MAXCRIT) return "gpsat_select_batch: n_crit out of range";
    a = SelectCriteria();
    a.n_crit = sp->n_crit;
    for (int k = 0; k < sp->n_crit; ++k) {
        // kind 2 (per-expert interval) only through gpsat_select_batch_ex, which passes the bounds
        if (sp->kind[k] != 0 && sp->kind[k] != 1 && !(sp->kind[k] == 2 && n_bounds > 0)) return "gpsat_select_batch: bad criterion kind";
        if (sp->comp[k] < 0 || sp->comp[k] > 4) return "gpsat_select_batch: bad comparison";
        if (sp->kind[k] == 2) {
            if (sp->cols[k][0] < 0 || sp->cols[k][0] >= C) return "gpsat_select_batch: column index out of range";
            if (sp->cols[k][1] < 0 || sp->cols[k][1] >= n_bounds) return "gpsat_select_batch: bound index out of range";
            a.kind[k] = 2; a.comp[k] = sp->comp[k]; a.ncols[k] = 1;
            a.cols[k][0] = sp->cols[k][0]; a.cols[k][1] = sp->cols[k][1];
            continue;
        }
        const int nc = sp->kind[k] == 0 ? 1 : sp->ncols[k];
        if (nc < 1 || nc > 3) return "gpsat_select_batch: ball criteria take 1..3 columns";
        if (sp->kind[k] == 1 && sp->comp[k] != 3 && sp->comp[k] != 4) return "gpsat_select_batch: ball criteria are < or <=";
        a.kind[k] = sp->kind[k]; a.comp[k] = sp->comp[k]; a.ncols[k] = nc; a.val[k] = sp->val[k];
        for (int m = 0; m < nc; ++m) {
            if (sp->cols[k][m] < 0 || sp->cols[k][m] >= C) return "gpsat_select_batch: column index out of range";
            a.cols[k][m] = sp->cols[k][m];
        }
    }
    return std::string();
}

// Row chunks: enough workgroups to fill the chip (T/32 workgroups per chunk), every chunk a whole number of `sub_rows` (the
// rows of one bounding box, select_sub_rows()).
struct SelectChunks { int n_chunks; long long chunk_rows; };

inline SelectChunks select_chunks(int64_t M, int T, long long sub_rows) {
    const long long sub = sub_rows;
    const int wgs_per_chunk = std::max(1, (T + 31) / 32);
    int n_chunks = (int)std::min<long long>(std::max<long long>(1, (4096 + wgs_per_chunk - 1) / wgs_per_chunk), std::max<long long>(1, (M + 4095) / 4096));
    long long chunk_rows = ((M + n_chunks - 1) / n_chunks + sub - 1) / sub * sub;
    if (chunk_rows < sub) chunk_rows = sub;
    n_chunks = (int)std::max<long long>(1, (M + chunk_rows - 1) / chunk_rows);
    return {n_chunks, chunk_rows};
}

// The grid the point table is sorted by: a two-sided 1-D window's column with cells of half its width (first: GPSat's time
// column), then a ball criterion's columns with cells of its radius, at most three columns, each once.  A column without a
// finite range and a cell width that is not a positive number are passed over; ndim == 0: no binning.  `points`: [C][M] host.
inline BinSpec select_bin_dims(const SelectCriteria& a, const double* points, int64_t M, int C) {
    (void)C;
    BinSpec bin = {};
    auto add_dim = [&](int col, double cell) {
        if (bin.ndim >= 3 || !(cell > 0.0) || !std::isfinite(cell)) return;
        for (int d = 0; d < bin.ndim; ++d) if (bin.col[d] == col) return;
        double mn = INFINITY, mx = -INFINITY;
        const double* x = points + (size_t)col * M;
        for (int64_t i = 0; i < M; ++i) { const double v = x[i]; if (v < mn) mn = v; if (v > mx) mx = v; }
        if (!(mn <= mx) || !std::isfinite(mn) || !std::isfinite(mx)) return;
        const double nc = std::min(1024.0, std::max(1.0, std::ceil((mx - mn) / cell)));
        bin.col[bin.ndim] = col; bin.origin[bin.ndim] = mn; bin.ncell[bin.ndim] = (int)nc;
        bin.inv_cell[bin.ndim] = (mx > mn) ? nc / (mx - mn) : 0.0;
        ++bin.ndim;
    };
    for (int k = 0; k < a.n_crit; ++k) {              // two-sided windows first (GPSat: the time column)
        if (a.kind[k] != 0 || !(a.comp[k] == 3 || a.comp[k] == 4)) continue;
        for (int k2 = 0; k2 < a.n_crit; ++k2)
            if (a.kind[k2] == 0 && (a.comp[k2] == 0 || a.comp[k2] == 1) && a.cols[k2][0] == a.cols[k][0] && a.val[k] > a.val[k2])
                add_dim(a.cols[k][0], 0.5 * (a.val[k] - a.val[k2]));
    }
    for (int k = 0; k < a.n_crit; ++k)
        if (a.kind[k] == 1) for (int m = 0; m < a.ncols[k]; ++m) add_dim(a.cols[k][m], a.val[k]);
    return bin;
}

// The experts in the order of their own cells (stable: experts of one cell keep their order), so that the experts a wave is
// dealt are neighbours.  `refs`: [T][C] host.
inline std::vector<int> select_expert_order(const BinSpec& bin, const double* refs, int T, int C) {
    std::vector<unsigned> ekey(T);
    for (int t = 0; t < T; ++t) {
        unsigned key = 0;
        for (int d = 0; d < bin.ndim; ++d) {
            const double cf = (refs[(size_t)t * C + bin.col[d]] - bin.origin[d]) * bin.inv_cell[d];
            const int cell = (cf >= 0.0) ? (int)std::min(cf, (double)(bin.ncell[d] - 1)) : 0;
            key = key * (unsigned)bin.ncell[d] + (unsigned)cell;
        }
        ekey[t] = key;
    }
    std::vector<int> eord(T);
    std::iota(eord.begin(), eord.end(), 0);
    std::stable_sort(eord.begin(), eord.end(), [&](int x, int y) { return ekey[x] < ekey[y]; });
    return eord;
}

// Exclusive scan over the (expert, chunk) cells, expert-major: cnt [T][n_chunks] becomes the start offset of every cell,
// off[0..T] the CSR offsets of the experts.
inline void select_scan(long long* cnt, int T, int n_chunks, int64_t* off) {
    long long run = 0;
    for (int t = 0; t < T; ++t) {
        off[t] = run;
        for (int cc = 0; cc < n_chunks; ++cc) { const long long v = cnt[(size_t)t * n_chunks + cc]; cnt[(size_t)t * n_chunks + cc] = run; run += v; }
    }
    off[T] = run;
}

// FNV-1a over all of `refs` and `bounds` and a sample of at most 65 536 evenly spaced elements of `points` (plus both ends): a
// caller who refills the same host buffers between the sizes call and the fill call gets a fresh selection, not the cached one
inline unsigned long long sel_fingerprint(const double* points, long long nP, const double* refs, long long nR,
                                          const double* bounds, long long nB) {
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const double* p) {
        unsigned long long v;
        std::memcpy(&v, p, 8);
        h = (h ^ v) * 1099511628211ull;
    };
    for (long long i = 0; i < nR; ++i) mix(refs + i);
    for (long long i = 0; i < nB; ++i) mix(bounds + i);
    const long long step = std::max<long long>(1, nP / 65536);
    for (long long i = 0; i < nP; i += step) mix(points + i);
    for (long long i = std::max<long long>(0, nP - 64); i < nP; ++i) mix(points + i);
    return h;
}

// gpsat_select_batch is called twice per selection (sizes, then indices): the first call already leaves the indices on the
// device; the second, when it repeats the first call's arguments over unchanged tables, only copies them out.
struct SelectCache {
    // What identifies a selection.  The one list of it: remember() stores what matches() compares.
    struct Call {
        const gpsat_select_spec* sp;
        int64_t M;
        int32_t C;
        const double* points;
        int32_t T;
        const double* refs;
        int32_t n_bounds;
        const double* bounds;
        bool same_arguments(const Call& o, const gpsat_select_spec& o_sp) const {
            return points == o.points && refs == o.refs && M == o.M && C == o.C && T == o.T && n_bounds == o.n_bounds &&
                   bounds == o.bounds && std::memcmp(sp, &o_sp, sizeof(o_sp)) == 0;
        }
        unsigned long long fingerprint() const {      // of the tables' CONTENTS
            return sel_fingerprint(points, (long long)M * C, refs, (long long)T * C, bounds, (long long)T * n_bounds * 2);
        }
    };
    Call call = {};                    // of the sizes call (call.sp is not kept: `sp` is the copy)
    gpsat_select_spec sp = {};
    unsigned long long fp = 0;
    int64_t total = -1;                // selected rows of the sizes call; -1: nothing remembered
    const int* d_result = nullptr;     // their indices on the device
    std::vector<int64_t> off;          // [T+1]

    void forget() { total = -1; }
    bool matches(const Call& now) const { return total >= 0 && now.same_arguments(call, sp) && fp == now.fingerprint(); }
    void remember(const Call& now, const int64_t* off_now, const int* d_idx) {
        call = now; sp = *now.sp; call.sp = nullptr;
        fp = now.fingerprint();
        d_result = d_idx; total = off_now[now.T];
        off.assign(off_now, off_now + now.T + 1);
    }
};

}  // namespace gpsat
#endif
