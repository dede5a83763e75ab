// Stand-alone driver of the host side of gpsat_fit_predict_batch_cv_refit_joint (gpsat_amd/csrc/gpsat_cvfold.h: cvfold_cov_off,
// the offsets of the derived batch's g x g covariances), for a build with the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gpsat_amd/csrc tests/cvfold_cov_host_check.cpp
// usage: cvfold_cov_host_check MIN_OBS T off_0 .. off_T label_0 .. label_{sumN-1}
// prints "cov_off ..." after checking it against the derived batch: one block per derived tile, g^2 elements each, in
// order, nothing between, every element of every block inside the buffer the C ABI sizes with cov_off[F2] (written here as
// the kernel indexes it).  tests/test_cv_joint_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpsat_cvfold.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); return 2; } } while (0)

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

    gpsat::CvFoldTables tb;
    const std::string err = gpsat::cvfold_tables(T, off.data(), lab.data(), true, tb);
    if (!err.empty()) { std::printf("error %s\n", err.c_str()); return 0; }
    gpsat::CvFoldDerived dv;
    gpsat::cvfold_derive(tb, off.data(), min_obs, dv);
    const std::vector<int64_t> cov_off = gpsat::cvfold_cov_off(dv);
    const size_t F2 = dv.d_fold.size();
    CHECK(cov_off.size() == F2 + 1 && cov_off[0] == 0);
    std::vector<unsigned char> hit((size_t)cov_off[F2], 0);
    for (size_t j = 0; j < F2; ++j) {
        const int f = dv.d_fold[j];
        const int64_t g = tb.fold_ptr[f + 1] - tb.fold_ptr[f];
        CHECK(g == dv.d_pred_off[j + 1] - dv.d_pred_off[j]);
        CHECK(cov_off[j + 1] - cov_off[j] == g * g);
        for (int64_t i = 0; i < g; ++i)
            for (int64_t k = 0; k < g; ++k) {
                const int64_t e = cov_off[j] + i * g + k;
                CHECK(e >= 0 && e < cov_off[F2] && !hit[(size_t)e]);
                hit[(size_t)e] = 1;
            }
    }
    for (unsigned char h : hit) CHECK(h == 1);
    std::printf("cov_off");
    for (int64_t v : cov_off) std::printf(" %lld", (long long)v);
    std::printf("\n");
    return 0;
}
