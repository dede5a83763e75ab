// Stand-alone driver of the host side of gpsat_fit_predict_batch_cv_refit (gpsat_amd/csrc/gpsat_cvfold.h: what
// gpsat_cv_refit_count returns, the fold tables, the derived batch and its packing), for a build with the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gpsat_amd/csrc tests/cvfold_host_check.cpp
// usage: cvfold_host_check MIN_OBS T off_0 .. off_T label_0 .. label_{sumN-1}
// prints "fold_off ...", "expanded_rows n", "fold_n_obs ...", "fold_label ...", "derived ..." (derived tile of every fold),
// "d_obs_off ..." and "d_pred_off ...", after checking the tables against each other and the packed blocks (cvfold_pack) against
// the tables.  tests/test_cv_refit_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpsat_cvfold.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); return 2; } } while (0)

template <class V>
static void show(const char* name, const V& v) {
    std::printf("%s", name);
    for (auto x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 4) return 1;
    const int min_obs = std::atoi(argv[1]), T = std::atoi(argv[2]);
    if (T < 0 || argc < 3 + T + 1) return 1;
    std::vector<int64_t> off((size_t)T + 1);
    for (int t = 0; t <= T; ++t) off[t] = std::atoll(argv[3 + t]);
    const int64_t sumN = off[T];
    if (argc != 3 + T + 1 + sumN) return 1;
    std::vector<int32_t> lab((size_t)sumN);
    for (int64_t i = 0; i < sumN; ++i) lab[i] = (int32_t)std::atoll(argv[3 + T + 1 + i]);

    gpsat::CvFoldTables cnt, tb;
    std::string err = gpsat::cvfold_tables(T, off.data(), lab.data(), false, cnt);
    if (!err.empty()) { std::printf("error %s\n", err.c_str()); return 0; }
    err = gpsat::cvfold_tables(T, off.data(), lab.data(), true, tb);
    CHECK(err.empty());
    CHECK(cnt.fold_off == tb.fold_off && cnt.expanded_rows == tb.expanded_rows);
    const size_t F = (size_t)tb.fold_off[T];
    CHECK(tb.fold_ptr.size() == F + 1 && tb.fold_label.size() == F && tb.fold_tile.size() == F && tb.fold_n_obs.size() == F);
    CHECK(tb.row_fold.size() == (size_t)sumN && tb.row_pos.size() == (size_t)sumN);
    // every held-out row is where its fold lists it; a fold's rows ascend; the labels of a tile's folds ascend
    for (size_t f = 0; f < F; ++f) {
        const int t = tb.fold_tile[f];
        CHECK((int64_t)f >= tb.fold_off[t] && (int64_t)f < tb.fold_off[t + 1]);
        if ((int64_t)f > tb.fold_off[t]) CHECK(tb.fold_label[f - 1] < tb.fold_label[f]);
        for (int k = tb.fold_ptr[f]; k < tb.fold_ptr[f + 1]; ++k) {
            const int i = tb.fold_rows[k];
            CHECK(i >= 0 && i < off[t + 1] - off[t]);
            if (k > tb.fold_ptr[f]) CHECK(tb.fold_rows[k - 1] < i);
            CHECK(lab[off[t] + i] == tb.fold_label[f]);
            CHECK(tb.row_fold[off[t] + i] == (int)f && tb.row_pos[off[t] + i] == k - tb.fold_ptr[f]);
        }
    }
    for (int64_t r = 0; r < sumN; ++r) CHECK((lab[r] < 0) == (tb.row_fold[r] < 0));
    gpsat::CvFoldDerived dv;
    gpsat::cvfold_derive(tb, off.data(), min_obs, dv);
    CHECK(dv.fold_derived.size() == F && dv.d_obs_off.size() == dv.d_fold.size() + 1 && dv.d_pred_off.size() == dv.d_fold.size() + 1);
    for (size_t j = 0; j < dv.d_fold.size(); ++j) {
        const int f = dv.d_fold[j];
        CHECK(dv.fold_derived[f] == (int)j);
        CHECK(dv.d_obs_off[j + 1] - dv.d_obs_off[j] == tb.fold_n_obs[f]);
        CHECK(dv.d_obs_off[j + 1] - dv.d_obs_off[j] + dv.d_pred_off[j + 1] - dv.d_pred_off[j] == dv.d_src_n[j]);
        CHECK(dv.d_src_off[j] == off[tb.fold_tile[f]]);
    }
    // the packed blocks hold every table, whole and in its own place, at the offset they report; F2 words follow each
    const gpsat::CvFoldPacked pk = gpsat::cvfold_pack(tb, dv);
    const size_t F2 = dv.d_fold.size();
    size_t words64 = 0, words32 = 0;
    auto holds = [](const auto& block, size_t off, const auto& v, size_t& words) {
        words += v.size();
        if (off + v.size() > block.size()) return false;
        for (size_t i = 0; i < v.size(); ++i) if ((long long)block[off + i] != (long long)v[i]) return false;
        return true;
    };
    CHECK(holds(pk.t64, pk.o_obs_off, dv.d_obs_off, words64) && holds(pk.t64, pk.o_pred_off, dv.d_pred_off, words64));
    CHECK(holds(pk.t64, pk.o_src_off, dv.d_src_off, words64));
    CHECK(pk.o_obs_off == 0 && pk.o_pred_off == F2 + 1 && pk.o_src_off == 2 * (F2 + 1));      // in this order, nothing between
    CHECK(words64 == pk.t64.size() && pk.o_delta == pk.t64.size() && pk.n64 == pk.o_delta + F2);
    CHECK(holds(pk.t32, pk.o_src_n, dv.d_src_n, words32) && holds(pk.t32, pk.o_fold, dv.d_fold, words32));
    CHECK(holds(pk.t32, pk.o_fold_ptr, tb.fold_ptr, words32) && holds(pk.t32, pk.o_fold_rows, tb.fold_rows, words32));
    CHECK(holds(pk.t32, pk.o_fold_derived, dv.fold_derived, words32));
    CHECK(holds(pk.t32, pk.o_row_fold, tb.row_fold, words32) && holds(pk.t32, pk.o_row_pos, tb.row_pos, words32));
    CHECK(words32 == pk.t32.size() && pk.o_status == pk.t32.size() && pk.n32 == pk.o_status + F2);
    const size_t starts[] = {pk.o_src_n, pk.o_fold, pk.o_fold_ptr, pk.o_fold_rows, pk.o_fold_derived, pk.o_row_fold, pk.o_row_pos, pk.o_status};
    const size_t sizes[] = {F2, F2, F + 1, tb.fold_rows.size(), F, (size_t)sumN, (size_t)sumN};
    CHECK(starts[0] == 0);
    for (int i = 0; i < 7; ++i) CHECK(starts[i + 1] == starts[i] + sizes[i]);      // no table overlaps the next
    show("fold_off", tb.fold_off);
    std::printf("expanded_rows %lld\n", (long long)tb.expanded_rows);
    show("fold_n_obs", tb.fold_n_obs);
    show("fold_label", tb.fold_label);
    show("derived", dv.fold_derived);
    show("d_obs_off", dv.d_obs_off);
    show("d_pred_off", dv.d_pred_off);
    return 0;
}
