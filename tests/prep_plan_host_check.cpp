// Host check of gpsat_amd/csrc/gpsat_prep_plan.h: the launch geometry, the buffer layout and the refusals of
// gpsat_project_batch / gpsat_track_batch, without a device; and of gpsat_key_runs_plan.h, the layout of the keyed
// sort-and-run-heads stage, with the three layouts built on it (tracks here, binning and the keyed glues from their headers).  Built with the host sanitizers and run directly:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gpsat_amd/csrc -I include tests/prep_plan_host_check.cpp
// usage: prep_plan_host_check BLOCK      (gpsat::prep_scan_block() of the library)
// Prints one line per case ("blocks n value", "scan n blocks rounds", "layout ...", "key_runs ...", "refuse <what>: <message>"); a failed
// internal check ends it non-zero.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "gpsat_prep_plan.h"
#include "gpsat_bin_plan.h"
#include "gpsat_glue_plan.h"

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static gpsat_project good_project(int64_t n, const double* in, double* out) {
    gpsat_project p;
    std::memset(&p, 0, sizeof(p));
    p.n = n; p.direction = GPSAT_PROJECT_FORWARD; p.memory = GPSAT_MEM_HOST; p.lon_0 = 0.0; p.lat_0 = 90.0;
    p.in0 = in; p.in1 = in; p.out0 = out; p.out1 = out;
    return p;
}

static gpsat_track good_track(int64_t n, const double* col, const int32_t* group, double* delta, int32_t* track, int32_t* order) {
    gpsat_track t;
    std::memset(&t, 0, sizeof(t));
    t.n = n; t.n_cols = 2; t.memory = GPSAT_MEM_HOST; t.cols[0] = col; t.cols[1] = col; t.group = group;
    t.cut_off = 600000.0; t.start_track = 0; t.mode = GPSAT_TRACK_CUT; t.out_delta = delta; t.out_track = track; t.out_order = order;
    return t;
}

template <class S, class Edit>
static void refuse_project(const char* what, S base, Edit edit) {
    char why[160];
    edit(base);
    const int rc = gpsat::check_project(&base, why, sizeof(why));
    CHECK(rc == GPSAT_EINVAL);
    CHECK(std::strlen(why) > 0);
    std::printf("refuse project %s: %s\n", what, why);
}

template <class S, class Edit>
static void refuse_track(const char* what, S base, Edit edit) {
    char why[160];
    unsigned long long sentinel = 99;
    edit(base);
    const int rc = gpsat::check_track(&base, &sentinel, why, sizeof(why));
    CHECK(rc == GPSAT_EINVAL);
    CHECK(std::strlen(why) > 0);
    std::printf("refuse track %s: %s\n", what, why);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s BLOCK\n", argv[0]); return 2; }
    const int B = std::atoi(argv[1]);
    if (B < 64 || B > 1024 || B % 64) { std::fprintf(stderr, "BLOCK must be a multiple of 64 in 64..1024\n"); return 2; }
    const int64_t NMAX = gpsat::PREP_MAX_ROWS;
    const int64_t sizes[] = {0, 1, 2, B - 1, B, B + 1, 3LL * B + 7, (int64_t)B * B - 1, (int64_t)B * B, (int64_t)B * B + 1, NMAX - 1, NMAX};

    // ---- launch geometry: the blocks cover every row, no block is empty, and 32 bits hold every index the kernels form
    for (int64_t n : sizes) {
        const unsigned nb = gpsat::prep_blocks(n, B);
        CHECK((int64_t)nb * B >= n);
        CHECK(n == 0 ? nb == 0 : (int64_t)(nb - 1) * B < n);
        CHECK((int64_t)nb * B - 1 <= (int64_t)std::numeric_limits<uint32_t>::max());       // the last thread's row as unsigned
        std::printf("blocks %lld %u\n", (long long)n, nb);
        const gpsat::ScanGeometry g = gpsat::prep_scan_geometry(n, B);
        CHECK(g.blocks == nb);
        CHECK((int64_t)g.rounds * B >= (int64_t)g.blocks);
        CHECK(g.blocks == 0 ? g.rounds == 0 : (int64_t)(g.rounds - 1) * B < (int64_t)g.blocks);
        std::printf("scan %lld %u %u\n", (long long)n, g.blocks, g.rounds);
    }

    // ---- layout: the parts follow each other without overlap, doubles and 64-bit keys on 8 bytes
    for (int64_t n : sizes)
        for (int n_cols = 1; n_cols <= 3; ++n_cols)
            for (int grouped = 0; grouped <= 1; ++grouped)
                for (int host = 0; host <= 1; ++host) {
                    const gpsat::TrackLayout l = gpsat::track_layout(n, n_cols, grouped, host, B);
                    const size_t nN = (size_t)n;
                    size_t want_in = 0;
                    if (host) { CHECK(l.in_cols == 0); want_in += (size_t)n_cols * nN * 8; }
                    if (grouped) {
                        if (host) { CHECK(l.in_group == want_in); want_in += (nN * 4 + 7) / 8 * 8; }
                        CHECK(l.in_key == want_in && l.in_key % 8 == 0);
                        want_in += nN * 8;
                        CHECK(l.keys_bytes == 16 * nN && l.rows_bytes == 8 * nN);
                        CHECK(l.runs_n_groups >= (nN + 1) * 4 && l.runs_n_groups % 256 == 0);
                        CHECK(l.runs_n_runs == l.runs_n_groups + 16 && l.runs_flags == l.runs_n_groups + 256);
                        CHECK(l.runs_bytes == l.runs_flags + nN);
                    } else {
                        CHECK(l.keys_bytes == 0 && l.rows_bytes == 0 && l.runs_bytes == 0);
                    }
                    CHECK(l.in_bytes == want_in);
                    size_t want_out = 0;
                    if (host) {
                        CHECK(l.out_track == nN * 8 && l.out_order == nN * 12);
                        want_out = (nN * 16 + 7) / 8 * 8;
                    }
                    CHECK(l.out_sums == want_out && l.out_sums % 4 == 0);
                    CHECK(l.out_bytes == want_out + (size_t)gpsat::prep_blocks(n, B) * 4);
                    if (n_cols == 2)
                        std::printf("layout %lld %d %d %zu %zu %zu %zu %zu\n", (long long)n, grouped, host, l.in_bytes, l.in_key, l.runs_bytes,
                                    l.out_sums, l.out_bytes);
                }

    // ---- the stage's layout: keys and rows twice, starts [n + 1] rounded to 256 B, the counts at +0 and n_runs at +16 of a
    // 256-B block, the flags [n] behind it; and its three users' layouts, field by field
    for (int64_t n : {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024}) {
        const gpsat::KeyRunsLayout k = gpsat::key_runs_layout(n);
        const size_t nN = (size_t)n, starts = ((nN + 1) * 4 + 255) / 256 * 256;
        CHECK(k.keys_bytes == 16 * nN && k.rows_bytes == 8 * nN);
        CHECK(k.runs_counts == starts && k.runs_n_runs == starts + 16 && k.runs_flags == starts + 256);
        CHECK(k.runs_bytes == starts + 256 + nN);
        auto same = [&](const gpsat::KeyRunsLayout& l) {
            return l.keys_bytes == k.keys_bytes && l.rows_bytes == k.rows_bytes && l.runs_counts == k.runs_counts &&
                   l.runs_n_runs == k.runs_n_runs && l.runs_flags == k.runs_flags;
        };
        const gpsat::TrackLayout t = gpsat::track_layout(n, 2, true, true, B);
        CHECK(same(t) && t.runs_bytes == k.runs_bytes && t.runs_n_groups == k.runs_counts);
        const gpsat::GlueKeyedLayout g = gpsat::glue_keyed_layout(n, 2, 3);
        CHECK(same(g) && g.runs_bytes == k.runs_bytes);
        // binning: n_long at +32 of the block, the flags rounded to 256 B, the list of long cells behind them
        const gpsat::BinLayout b = gpsat::bin_layout(n, 11, 11, true, true, true, 1024);
        const size_t flags = (nN + 255) / 256 * 256;
        CHECK(same(b) && b.runs_n_cells == k.runs_counts && b.runs_n_long == starts + 32 && b.runs_long_list == starts + 256 + flags);
        CHECK(b.runs_bytes == starts + 256 + flags + (nN / 1024 + 1) * 4);
        std::printf("key_runs %lld %zu %zu %zu %zu %zu %zu\n", (long long)n, k.keys_bytes, k.rows_bytes, k.runs_bytes, k.runs_counts,
                    k.runs_n_runs, k.runs_flags);
    }

    // ---- the constants of the projection
    const gpsat::ProjConst pc = gpsat::proj_const();
    CHECK(pc.a == 6378137.0 && pc.e2 > 0.00669437999 && pc.e2 < 0.00669438001 && pc.qp > 1.9955310875 && pc.qp < 1.9955310876);
    CHECK(pc.qp + pc.qp_lo == 1.9955310875028367 && std::fabs(pc.qp_lo) < 1e-14);       // the true q_p, rounded
    std::printf("const %.17g %.17g %.17g %.17g %.17g\n", pc.e2, pc.e, pc.inv_2e, pc.qp, pc.qp_lo);

    // ---- what passes
    std::vector<double> col(8, 1.0), outd(8);
    std::vector<int32_t> grp = {0, 0, 1, -1, 1, 2, 0, 5}, tr(8), ord(8);
    char why[160];
    unsigned long long sentinel = 0;
    {
        gpsat_project p = good_project(8, col.data(), outd.data());
        CHECK(gpsat::check_project(&p, why, sizeof(why)) == GPSAT_OK && why[0] == 0);
        p.lat_0 = -90.0; p.direction = GPSAT_PROJECT_INVERSE; p.memory = GPSAT_MEM_DEVICE;
        CHECK(gpsat::check_project(&p, why, sizeof(why)) == GPSAT_OK);
        p = good_project(0, nullptr, nullptr);
        CHECK(gpsat::check_project(&p, why, sizeof(why)) == GPSAT_OK);
        gpsat_track t = good_track(8, col.data(), grp.data(), outd.data(), tr.data(), ord.data());
        CHECK(gpsat::check_track(&t, &sentinel, why, sizeof(why)) == GPSAT_OK && sentinel == 6);
        t.group = nullptr;
        CHECK(gpsat::check_track(&t, &sentinel, why, sizeof(why)) == GPSAT_OK && sentinel == (1ull << 31));
        t.group = grp.data(); t.memory = GPSAT_MEM_DEVICE;                    // device mode: the codes are not read
        CHECK(gpsat::check_track(&t, &sentinel, why, sizeof(why)) == GPSAT_OK && sentinel == (1ull << 31));
        t = good_track(8, col.data(), nullptr, nullptr, tr.data(), ord.data());
        t.mode = GPSAT_TRACK_RUNS; t.n_cols = 1; t.cut_off = std::numeric_limits<double>::quiet_NaN(); t.start_track = -5;
        CHECK(gpsat::check_track(&t, &sentinel, why, sizeof(why)) == GPSAT_OK);     // runs: neither is read
        t = good_track(0, nullptr, nullptr, nullptr, nullptr, nullptr);
        CHECK(gpsat::check_track(&t, &sentinel, why, sizeof(why)) == GPSAT_OK);
        t = good_track(NMAX - 7, col.data(), nullptr, outd.data(), tr.data(), ord.data());
        t.memory = GPSAT_MEM_DEVICE; t.start_track = 7;
        CHECK(gpsat::check_track(&t, &sentinel, why, sizeof(why)) == GPSAT_OK);     // start_track + n = 2^31 - 1
        std::vector<int32_t> none(8, -1);
        t = good_track(8, col.data(), none.data(), outd.data(), tr.data(), ord.data());
        CHECK(gpsat::check_track(&t, &sentinel, why, sizeof(why)) == GPSAT_OK && sentinel == 0);
    }

    // ---- every refusal
    const gpsat_project P = good_project(8, col.data(), outd.data());
    CHECK(gpsat::check_project(nullptr, why, sizeof(why)) == GPSAT_EINVAL);
    refuse_project("lat_0 = 45", P, [](gpsat_project& p) { p.lat_0 = 45.0; });
    refuse_project("lat_0 = 0", P, [](gpsat_project& p) { p.lat_0 = 0.0; });
    refuse_project("lat_0 NaN", P, [](gpsat_project& p) { p.lat_0 = std::numeric_limits<double>::quiet_NaN(); });
    refuse_project("lon_0 inf", P, [](gpsat_project& p) { p.lon_0 = std::numeric_limits<double>::infinity(); });
    refuse_project("lon_0 NaN", P, [](gpsat_project& p) { p.lon_0 = std::numeric_limits<double>::quiet_NaN(); });
    refuse_project("direction", P, [](gpsat_project& p) { p.direction = 2; });
    refuse_project("memory", P, [](gpsat_project& p) { p.memory = 2; });
    refuse_project("n < 0", P, [](gpsat_project& p) { p.n = -1; });
    refuse_project("n = 2^31", P, [](gpsat_project& p) { p.n = 2147483648LL; });
    refuse_project("in1 NULL", P, [](gpsat_project& p) { p.in1 = nullptr; });
    refuse_project("out0 NULL", P, [](gpsat_project& p) { p.out0 = nullptr; });
    for (int i = 0; i < 8; ++i) refuse_project("reserved", P, [i](gpsat_project& p) { p.reserved[i] = 1; });

    const gpsat_track T = good_track(8, col.data(), grp.data(), outd.data(), tr.data(), ord.data());
    CHECK(gpsat::check_track(nullptr, &sentinel, why, sizeof(why)) == GPSAT_EINVAL);
    refuse_track("n_cols = 0", T, [](gpsat_track& t) { t.n_cols = 0; });
    refuse_track("n_cols = 4", T, [](gpsat_track& t) { t.n_cols = 4; });
    refuse_track("runs with 2 columns", T, [](gpsat_track& t) { t.mode = GPSAT_TRACK_RUNS; });
    refuse_track("given with 2 columns", T, [](gpsat_track& t) { t.mode = GPSAT_TRACK_GIVEN; });
    refuse_track("mode", T, [](gpsat_track& t) { t.mode = 3; });
    refuse_track("memory", T, [](gpsat_track& t) { t.memory = -1; });
    refuse_track("cut_off NaN", T, [](gpsat_track& t) { t.cut_off = std::numeric_limits<double>::quiet_NaN(); });
    refuse_track("cut_off inf", T, [](gpsat_track& t) { t.cut_off = std::numeric_limits<double>::infinity(); });
    refuse_track("start_track < 0", T, [](gpsat_track& t) { t.start_track = -1; });
    refuse_track("start_track + n", T, [](gpsat_track& t) { t.start_track = 2147483647 - 7; });
    refuse_track("n < 0", T, [](gpsat_track& t) { t.n = -1; });
    refuse_track("n = 2^31", T, [](gpsat_track& t) { t.n = 2147483648LL; t.memory = GPSAT_MEM_DEVICE; });
    refuse_track("cols[1] NULL", T, [](gpsat_track& t) { t.cols[1] = nullptr; });
    refuse_track("out_delta NULL", T, [](gpsat_track& t) { t.out_delta = nullptr; });
    refuse_track("out_track NULL", T, [](gpsat_track& t) { t.out_track = nullptr; });
    refuse_track("out_order NULL", T, [](gpsat_track& t) { t.out_order = nullptr; });
    for (int i = 0; i < 8; ++i) refuse_track("reserved", T, [i](gpsat_track& t) { t.reserved[i] = -1; });
    {
        std::vector<int32_t> bad = grp;
        bad[6] = -2;
        gpsat_track t = T;
        t.group = bad.data();
        CHECK(gpsat::check_track(&t, &sentinel, why, sizeof(why)) == GPSAT_EINVAL);
        CHECK(std::string(why).find("group[6] = -2") != std::string::npos);
        std::printf("refuse track code: %s\n", why);
    }
    // a short message buffer is filled, not overrun
    {
        char small[8];
        gpsat_track t = T;
        t.n_cols = 9;
        CHECK(gpsat::check_track(&t, nullptr, small, sizeof(small)) == GPSAT_EINVAL && std::strlen(small) == 7);
    }
    std::printf("done %d\n", failures);
    return failures ? 1 : 0;
}
