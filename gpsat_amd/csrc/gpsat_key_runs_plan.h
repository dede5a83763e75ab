// gpsat_key_runs_plan.h -- host side of the keyed sort-and-run-heads stage (gpsat_key_runs.hip): the three buffers a user of
// the stage holds and where the stage's arrays lie in them.  Plain C++ without a HIP call, in the manner of gpsat_bin_plan.h;
// the layouts of the stage's users (BinLayout, GlueKeyedLayout, TrackLayout) are built on it.
#ifndef GPSAT_KEY_RUNS_PLAN_H
#define GPSAT_KEY_RUNS_PLAN_H

#include <cstddef>
#include <cstdint>

namespace gpsat {

struct KeyRunsLayout {
    size_t keys_bytes;                // [2][n] 64-bit keys: as the key kernel wrote them, sorted
    size_t rows_bytes;                // [2][n] 32-bit rows: source, sorted
    // `runs`: starts [n + 1] rounded to 256 B; a 256-B block with the counts [2] at +0 and n_runs at +16 (a user may put
    // words of its own from +32); the head flags [n]
    size_t runs_bytes, runs_counts, runs_n_runs, runs_flags;
};

inline KeyRunsLayout key_runs_layout(int64_t n) {
    const size_t nN = (size_t)n;
    KeyRunsLayout l = {};
    l.keys_bytes = 2 * nN * sizeof(unsigned long long);
    l.rows_bytes = 2 * nN * sizeof(unsigned);
    const size_t starts_bytes = ((nN + 1) * sizeof(unsigned) + 255) & ~size_t(255);
    l.runs_counts = starts_bytes;
    l.runs_n_runs = starts_bytes + 16;
    l.runs_flags = starts_bytes + 256;
    l.runs_bytes = l.runs_flags + nN;
    return l;
}

}  // namespace gpsat
#endif
