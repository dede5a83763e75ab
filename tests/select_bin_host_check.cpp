// Stand-alone driver of the host side of gpsat_select_batch_ex and gpsat_bin_batch (gpsat_amd/csrc/gpsat_select_plan.h,
// gpsat_bin_plan.h), for a build with the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gpsat_amd/csrc -I include tests/select_bin_host_check.cpp
// usage: select_bin_host_check SUB_ROWS LONG_ROWS      (gpsat::select_sub_rows() and gpsat::bin_long_rows() of the library)
// Prints one line per case, "<section> <case>: <results>"; tests/test_select_bin_plan_cpu.py compares them with
// tests/golden/select_bin_plan.txt, which the statements of gpsat_capi.cpp printed for the same cases before they became these
// functions.  The two-call cache had no counterpart to record: it is checked here, one remembered argument at a time.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "gpsat_select_plan.h"
#include "gpsat_bin_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); return 2; } } while (0)

static const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

struct Crit { int kind, comp, ncols, c0, c1, c2; double val; };

static gpsat_select_spec make_spec(const std::vector<Crit>& cr, int n_crit = -1) {
    gpsat_select_spec sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.n_crit = n_crit < 0 ? (int)cr.size() : n_crit;
    for (size_t k = 0; k < cr.size() && k < GPSAT_SEL_MAXCRIT; ++k) {
        sp.kind[k] = cr[k].kind; sp.comp[k] = cr[k].comp; sp.ncols[k] = cr[k].ncols;
        sp.cols[k][0] = cr[k].c0; sp.cols[k][1] = cr[k].c1; sp.cols[k][2] = cr[k].c2;
        sp.val[k] = cr[k].val;
    }
    return sp;
}

static void show_check_spec(const char* name, const std::vector<Crit>& cr, int C, int n_bounds, int n_crit = -1) {
    const gpsat_select_spec sp = make_spec(cr, n_crit);
    gpsat::SelectCriteria a;
    std::memset(&a, 0, sizeof(a));
    const std::string msg = gpsat::select_check_spec(&sp, C, n_bounds, a);
    std::printf("check_spec %s:", name);
    if (!msg.empty()) { std::printf(" refused: %s\n", msg.c_str()); return; }
    std::printf(" n_crit %d", a.n_crit);
    for (int k = 0; k < GPSAT_SEL_MAXCRIT; ++k)
        std::printf(" | kind %d comp %d ncols %d cols %d %d %d val %.17g", a.kind[k], a.comp[k], a.ncols[k], a.cols[k][0], a.cols[k][1],
                    a.cols[k][2], a.val[k]);
    std::printf("\n");
}

// points [C][M], column-major
static int show_bin_dims(const char* name, const std::vector<Crit>& cr, const std::vector<std::vector<double>>& cols) {
    const int C = (int)cols.size();
    const int64_t M = (int64_t)cols[0].size();
    std::vector<double> pts;
    for (const auto& c : cols) pts.insert(pts.end(), c.begin(), c.end());
    const gpsat_select_spec sp = make_spec(cr);
    gpsat::SelectCriteria a;
    std::memset(&a, 0, sizeof(a));
    CHECK(gpsat::select_check_spec(&sp, C, 0, a).empty());
    const gpsat::BinSpec b = gpsat::select_bin_dims(a, pts.data(), M, C);
    std::printf("bin_dims %s: ndim %d", name, b.ndim);
    for (int d = 0; d < b.ndim; ++d) std::printf(" | col %d origin %.17g ncell %d inv_cell %.17g", b.col[d], b.origin[d], b.ncell[d], b.inv_cell[d]);
    std::printf("\n");
    return 0;
}

static void show_order(const char* name, const gpsat::BinSpec& b, const std::vector<double>& refs, int C) {
    const int T = (int)(refs.size() / C);
    const std::vector<int> o = gpsat::select_expert_order(b, refs.data(), T, C);
    std::printf("expert_order %s:", name);
    for (int t : o) std::printf(" %d", t);
    std::printf("\n");
}

static void show_scan(const char* name, std::vector<long long> cnt, int T, int n_chunks) {
    std::vector<int64_t> off((size_t)T + 1, -1);
    gpsat::select_scan(cnt.data(), T, n_chunks, off.data());
    std::printf("scan %s: off", name);
    for (int64_t v : off) std::printf(" %lld", (long long)v);
    std::printf(" | starts");
    for (long long v : cnt) std::printf(" %lld", v);
    std::printf("\n");
}

struct BinCase {
    int64_t R = 4;
    bool has_x = true, has_y = false, has_v = true;
    std::vector<int32_t> gid;
    int32_t G = 1;
    std::vector<double> ex = {0.0, 1.0, 2.0}, ey = {0.0, 1.0};
    int nx = -1, ny = -1;              // -1: the vectors' sizes
    bool null_ex = false, null_ey = false;
    double x_hi = 2.0, y_hi = 1.0;
    uint32_t stats = GPSAT_BIN_MEAN;
    int64_t capacity = 16;
};

static void show_bin_check(const char* name, const BinCase& c) {
    static const double col[4] = {0.5, 1.5, 0.25, 1.75};
    const std::string msg = gpsat::bin_check(c.R, c.has_x ? col : nullptr, c.has_y ? col : nullptr, c.has_v ? col : nullptr,
                                             c.gid.empty() ? nullptr : c.gid.data(), c.G, c.nx < 0 ? (int)c.ex.size() : c.nx,
                                             c.null_ex ? nullptr : c.ex.data(), c.x_hi, c.ny < 0 ? (int)c.ey.size() : c.ny,
                                             c.null_ey ? nullptr : c.ey.data(), c.y_hi, c.stats, c.capacity);
    std::printf("bin_check %s: %s\n", name, msg.empty() ? "ok" : msg.c_str());
}

static std::vector<double> ramp(int n) {
    std::vector<double> e((size_t)n);
    for (int i = 0; i < n; ++i) e[i] = (double)i;
    return e;
}

static int check_cache() {
    const int C = 2, T = 3, n_bounds = 1;
    const int64_t M = 5;
    std::vector<double> pts(2 * (M + 1) * (C + 1), 0.25), refs(2 * (T + 1) * (C + 1), 0.5), bounds(2 * (T + 1) * 2 * (n_bounds + 1), 0.75);
    std::vector<double> pts2 = pts, refs2 = refs, bounds2 = bounds;
    gpsat_select_spec sp = make_spec({{0, 0, 1, 0, 0, 0, 1.0}, {1, 3, 2, 0, 1, 0, 2.0}, {2, 0, 1, 1, 0, 0, 0.0}});
    const int64_t off[T + 1] = {0, 2, 2, 7};
    const int on_device = 0;
    gpsat::SelectCache cache;
    const gpsat::SelectCache::Call call = {&sp, M, C, pts.data(), T, refs.data(), n_bounds, bounds.data()};
    CHECK(!cache.matches(call));                       // nothing remembered
    cache.remember(call, off, &on_device);
    CHECK(cache.total == 7 && cache.d_result == &on_device && cache.off == std::vector<int64_t>(off, off + T + 1));
    CHECK(cache.matches(call));
    int n = 0;
    // every argument on its own (the tables behind the other pointers hold the same values)
    { gpsat::SelectCache::Call c = call; c.M = M + 1; CHECK(!cache.matches(c)); ++n; }
    { gpsat::SelectCache::Call c = call; c.C = C + 1; CHECK(!cache.matches(c)); ++n; }
    { gpsat::SelectCache::Call c = call; c.T = T + 1; CHECK(!cache.matches(c)); ++n; }
    { gpsat::SelectCache::Call c = call; c.n_bounds = n_bounds + 1; CHECK(!cache.matches(c)); ++n; }
    { gpsat::SelectCache::Call c = call; c.points = pts2.data(); CHECK(!cache.matches(c)); ++n; }
    { gpsat::SelectCache::Call c = call; c.refs = refs2.data(); CHECK(!cache.matches(c)); ++n; }
    { gpsat::SelectCache::Call c = call; c.bounds = bounds2.data(); CHECK(!cache.matches(c)); ++n; }
    // every field of the criteria, through a copy (another address alone does not matter) and in place
    { gpsat_select_spec s2 = sp; gpsat::SelectCache::Call c = call; c.sp = &s2; CHECK(cache.matches(c)); }
    { gpsat_select_spec s2 = sp; s2.n_crit = 2; gpsat::SelectCache::Call c = call; c.sp = &s2; CHECK(!cache.matches(c)); ++n; }
    for (int k = 0; k < GPSAT_SEL_MAXCRIT; ++k) {
        { gpsat_select_spec s2 = sp; s2.kind[k] ^= 1; gpsat::SelectCache::Call c = call; c.sp = &s2; CHECK(!cache.matches(c)); ++n; }
        { gpsat_select_spec s2 = sp; s2.comp[k] += 1; gpsat::SelectCache::Call c = call; c.sp = &s2; CHECK(!cache.matches(c)); ++n; }
        { gpsat_select_spec s2 = sp; s2.ncols[k] += 1; gpsat::SelectCache::Call c = call; c.sp = &s2; CHECK(!cache.matches(c)); ++n; }
        { gpsat_select_spec s2 = sp; s2.val[k] += 1.0; gpsat::SelectCache::Call c = call; c.sp = &s2; CHECK(!cache.matches(c)); ++n; }
        for (int m = 0; m < 3; ++m) { gpsat_select_spec s2 = sp; s2.cols[k][m] += 1; gpsat::SelectCache::Call c = call; c.sp = &s2; CHECK(!cache.matches(c)); ++n; }
    }
    sp.val[1] = 3.0; CHECK(!cache.matches(call)); ++n; sp.val[1] = 2.0; CHECK(cache.matches(call));
    // the contents: every element of the three tables that the call covers
    for (int64_t i = 0; i < M * C; ++i) { pts[i] = 9.0; CHECK(!cache.matches(call)); ++n; pts[i] = 0.25; }
    for (int i = 0; i < T * C; ++i) { refs[i] = 9.0; CHECK(!cache.matches(call)); ++n; refs[i] = 0.5; }
    for (int i = 0; i < T * n_bounds * 2; ++i) { bounds[i] = 9.0; CHECK(!cache.matches(call)); ++n; bounds[i] = 0.75; }
    pts[M * C] = 9.0; CHECK(cache.matches(call)); pts[M * C] = 0.25;          // past the table: not part of the selection
    CHECK(cache.matches(call));
    cache.forget();
    CHECK(!cache.matches(call)); ++n;
    // a selection of nothing is remembered too (total 0), without bounds
    const gpsat::SelectCache::Call empty = {&sp, 0, C, nullptr, T, refs.data(), 0, nullptr};
    const int64_t off0[T + 1] = {0, 0, 0, 0};
    cache.remember(empty, off0, nullptr);
    CHECK(cache.total == 0 && cache.matches(empty) && !cache.matches(call));
    std::printf("cache: %d changes of one argument refused\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    const long long sub = std::atoll(argv[1]);
    const int long_rows = std::atoi(argv[2]);
    if (sub < 1 || long_rows < 1) return 1;

    // ---- chunks
    const long long Ms[] = {0, 1, sub - 1, sub, sub + 1, 4096, 65535, 65536, 1000000, 2147483647LL};
    const int Ts[] = {1, 31, 32, 33, 4096, 131072};
    for (long long M : Ms)
        for (int T : Ts) {
            const gpsat::SelectChunks ch = gpsat::select_chunks(M, T, sub);
            CHECK(ch.n_chunks >= 1 && ch.chunk_rows >= sub && ch.chunk_rows % sub == 0 && (long long)ch.n_chunks * ch.chunk_rows >= M);
            std::printf("chunks M=%lld T=%d: n_chunks %d chunk_rows %lld\n", M, T, ch.n_chunks, ch.chunk_rows);
        }

    // ---- select_check_spec: every refusal, then what it normalises
    show_check_spec("n_crit 0", {}, 3, 0, 0);
    show_check_spec("n_crit 5", {{0, 0, 1, 0, 0, 0, 1.0}}, 3, 0, 5);
    show_check_spec("kind 3", {{3, 0, 1, 0, 0, 0, 1.0}}, 3, 1);
    show_check_spec("kind -1", {{-1, 0, 1, 0, 0, 0, 1.0}}, 3, 1);
    show_check_spec("kind 2 without bounds", {{2, 0, 1, 0, 0, 0, 0.0}}, 3, 0);
    show_check_spec("comp -1", {{0, -1, 1, 0, 0, 0, 1.0}}, 3, 0);
    show_check_spec("comp 5", {{1, 5, 1, 0, 0, 0, 1.0}}, 3, 0);
    show_check_spec("kind 2 comp 5", {{2, 5, 1, 0, 0, 0, 1.0}}, 3, 1);
    show_check_spec("kind 2 column -1", {{2, 0, 1, -1, 0, 0, 0.0}}, 3, 2);
    show_check_spec("kind 2 column C", {{2, 0, 1, 3, 0, 0, 0.0}}, 3, 2);
    show_check_spec("kind 2 bound -1", {{2, 0, 1, 0, -1, 0, 0.0}}, 3, 2);
    show_check_spec("kind 2 bound n_bounds", {{2, 0, 1, 0, 2, 0, 0.0}}, 3, 2);
    show_check_spec("ball of 0 columns", {{1, 3, 0, 0, 0, 0, 1.0}}, 3, 0);
    show_check_spec("ball of 4 columns", {{1, 3, 4, 0, 1, 2, 1.0}}, 3, 0);
    show_check_spec("ball >=", {{1, 0, 2, 0, 1, 0, 1.0}}, 3, 0);
    show_check_spec("ball ==", {{1, 2, 2, 0, 1, 0, 1.0}}, 3, 0);
    show_check_spec("compare column -1", {{0, 0, 1, -1, 0, 0, 1.0}}, 3, 0);
    show_check_spec("compare column C", {{0, 0, 1, 3, 0, 0, 1.0}}, 3, 0);
    show_check_spec("ball third column C", {{1, 4, 3, 0, 1, 3, 1.0}}, 3, 0);
    show_check_spec("second criterion bad", {{0, 0, 1, 0, 0, 0, 1.0}, {0, 7, 1, 0, 0, 0, 1.0}}, 3, 0);
    show_check_spec("compare ignores ncols and further columns", {{0, 4, 9, 2, 77, -5, 1.5}}, 3, 0);
    show_check_spec("ball and window", {{1, 3, 2, 0, 1, 99, 300.0}, {0, 0, 1, 2, 0, 0, -4.0}, {0, 4, 1, 2, 0, 0, 4.0}}, 3, 0);
    show_check_spec("kind 2 with bounds", {{2, 0, 5, 1, 1, 7, 123.0}, {1, 4, 3, 0, 1, 2, 2.5}}, 3, 2);
    show_check_spec("kind 2 among four", {{0, 1, 1, 0, 0, 0, 0.0}, {2, 3, 1, 2, 0, 0, 0.0}, {2, 4, 1, 1, 2, 0, 0.0}, {1, 3, 1, 2, 0, 0, 1.0}}, 3, 3);

    // ---- bin dimensions: a table of 6 columns and 8 rows
    const std::vector<double> c0 = {0.0, 10.0, 2.5, 7.5, 5.0, 1.0, 9.0, 3.0}, c1 = {-4.0, 4.0, 0.0, 1.0, -1.0, 2.0, -2.0, 3.0},
                              c2 = {100.0, 101.0, 102.0, 103.0, 104.0, 105.0, 106.0, 108.0}, c3 = {0.5, 0.25, 0.75, 0.125, 1.0, 0.0, 0.625, 0.375};
    const std::vector<double> constant(8, 3.0), all_nan(8, kNaN);
    std::vector<double> with_inf = c0, with_minf = c0, with_nan = c0;
    with_inf[3] = kInf; with_minf[5] = -kInf; with_nan[0] = kNaN;
    const std::vector<std::vector<double>> tab = {c0, c1, c2, c3, constant, all_nan};
    int rc = 0;
    rc |= show_bin_dims("one-sided compare only", {{0, 0, 1, 2, 0, 0, 101.0}}, tab);
    rc |= show_bin_dims("== and one side", {{0, 2, 1, 2, 0, 0, 101.0}, {0, 3, 1, 1, 0, 0, 2.0}}, tab);
    rc |= show_bin_dims("two-sided window", {{0, 0, 1, 2, 0, 0, 101.0}, {0, 3, 1, 2, 0, 0, 105.0}}, tab);
    rc |= show_bin_dims("two-sided window > <=", {{0, 4, 1, 2, 0, 0, 105.0}, {0, 1, 1, 2, 0, 0, 101.0}}, tab);
    rc |= show_bin_dims("window whose sides are equal", {{0, 0, 1, 2, 0, 0, 103.0}, {0, 4, 1, 2, 0, 0, 103.0}}, tab);
    rc |= show_bin_dims("window on two columns' sides", {{0, 0, 1, 2, 0, 0, 101.0}, {0, 3, 1, 1, 0, 0, 105.0}}, tab);
    rc |= show_bin_dims("ball first, window's column first", {{1, 3, 2, 0, 1, 0, 2.0}, {0, 0, 1, 2, 0, 0, 101.0}, {0, 4, 1, 2, 0, 0, 104.0}}, tab);
    rc |= show_bin_dims("column in ball and window", {{1, 4, 2, 2, 0, 0, 3.0}, {0, 1, 1, 2, 0, 0, 100.0}, {0, 3, 1, 2, 0, 0, 101.0}}, tab);
    rc |= show_bin_dims("column twice in one ball", {{1, 4, 3, 1, 1, 0, 3.0}}, tab);
    rc |= show_bin_dims("four candidates", {{1, 3, 3, 0, 1, 3, 0.5}, {0, 0, 1, 2, 0, 0, 100.0}, {0, 3, 1, 2, 0, 0, 104.0}}, tab);
    rc |= show_bin_dims("two balls, four columns", {{1, 3, 2, 3, 2, 0, 0.25}, {1, 3, 2, 1, 0, 0, 1.0}}, tab);
    rc |= show_bin_dims("constant column", {{1, 3, 2, 4, 0, 0, 1.0}}, tab);
    rc |= show_bin_dims("all-NaN column", {{1, 3, 2, 5, 1, 0, 1.0}}, tab);
    rc |= show_bin_dims("column with +inf", {{1, 3, 1, 0, 0, 0, 1.0}}, {with_inf, c1});
    rc |= show_bin_dims("column with -inf", {{1, 3, 2, 0, 1, 0, 1.0}}, {with_minf, c1});
    rc |= show_bin_dims("column with one NaN", {{1, 3, 1, 0, 0, 0, 1.0}}, {with_nan, c1});
    rc |= show_bin_dims("cell 0", {{1, 3, 2, 0, 1, 0, 0.0}}, tab);
    rc |= show_bin_dims("cell negative", {{1, 3, 2, 0, 1, 0, -1.0}}, tab);
    rc |= show_bin_dims("cell NaN", {{1, 3, 2, 0, 1, 0, kNaN}}, tab);
    rc |= show_bin_dims("cell inf", {{1, 3, 2, 0, 1, 0, kInf}}, tab);
    rc |= show_bin_dims("window of infinite width", {{0, 0, 1, 2, 0, 0, -kInf}, {0, 3, 1, 2, 0, 0, 104.0}}, tab);
    rc |= show_bin_dims("window with a NaN side", {{0, 0, 1, 2, 0, 0, kNaN}, {0, 3, 1, 2, 0, 0, 104.0}}, tab);
    rc |= show_bin_dims("ratio 1024", {{1, 3, 1, 0, 0, 0, 10.0 / 1024.0}}, tab);
    rc |= show_bin_dims("ratio above 1024", {{1, 3, 2, 0, 1, 0, 0.001}}, tab);
    rc |= show_bin_dims("cell wider than the range", {{1, 3, 2, 0, 1, 0, 1e6}}, tab);
    rc |= show_bin_dims("one row", {{1, 3, 2, 0, 1, 0, 1.0}}, {{2.0}, {3.0}});
    if (rc) return rc;

    // ---- expert order
    {
        gpsat::BinSpec b = {};
        b.ndim = 1; b.col[0] = 1; b.origin[0] = 10.0; b.ncell[0] = 4; b.inv_cell[0] = 0.5;      // cells of width 2 over [10, 18]
        //                         below, in 3, last edge, beyond, in 0, below, in 1, in 3, NaN, in 1
        show_order("one dimension", b, {0, 9.0, 0, 16.5, 0, 18.0, 0, 1e300, 0, 10.0, 0, -kInf, 0, 12.0, 0, 17.9, 0, kNaN, 0, 13.9}, 2);
        show_order("equal keys", b, {0, 12.5, 0, 12.0, 0, 13.0, 0, 12.5}, 2);
        show_order("one expert", b, {0, 12.5}, 2);
        gpsat::BinSpec b3 = {};
        b3.ndim = 3;
        b3.col[0] = 2; b3.origin[0] = 0.0; b3.ncell[0] = 2; b3.inv_cell[0] = 1.0;
        b3.col[1] = 0; b3.origin[1] = -1.0; b3.ncell[1] = 3; b3.inv_cell[1] = 1.0;
        b3.col[2] = 1; b3.origin[2] = 5.0; b3.ncell[2] = 1024; b3.inv_cell[2] = 0.0;          // a constant column: every expert in cell 0
        show_order("three dimensions", b3, {1.5, 7.0, 1.5, -0.5, 7.0, 0.5, 0.5, 7.0, 0.5, 9.0, 7.0, 9.0, -9.0, 7.0, -9.0, 0.5, 1e9, 1.5}, 3);
        gpsat::BinSpec wide = {};
        wide.ndim = 3;
        for (int d = 0; d < 3; ++d) { wide.col[d] = d; wide.origin[d] = 0.0; wide.ncell[d] = 1024; wide.inv_cell[d] = 1.0; }
        show_order("1024 cells a side", wide, {1023, 1023, 1023, 0, 0, 0, 1023, 0, 5, 5000, 5000, 5000, 0, 1023, 1023, 1, 0, 0}, 3);
    }

    // ---- scan
    show_scan("empty cells", {0, 3, 0, 0, 0, 0, 2, 0, 1, 0, 0, 0}, 4, 3);
    show_scan("nothing selected", {0, 0, 0, 0}, 2, 2);
    show_scan("T = 1", {5}, 1, 1);
    show_scan("T = 1, four chunks", {1, 0, 2, 4}, 1, 4);
    show_scan("total above 2^31", {1LL << 30, 1LL << 30, 0, 1LL << 30, 2147483647LL, 1}, 3, 2);

    // ---- bin_check: every refusal in the order it is made, then what passes
    { BinCase c; c.R = -1; show_bin_check("R < 0", c); }
    { BinCase c; c.G = -1; show_bin_check("G < 0", c); }
    { BinCase c; c.capacity = -1; show_bin_check("capacity < 0", c); }
    { BinCase c; c.R = 2147483648LL; show_bin_check("2^31 rows", c); }
    { BinCase c; c.R = 2147483648LL; c.stats = 0; show_bin_check("2^31 rows before stats", c); }
    { BinCase c; c.stats = 0; show_bin_check("stats 0", c); }
    { BinCase c; c.stats = 128; show_bin_check("stats 128", c); }
    { BinCase c; c.stats = 127; show_bin_check("every statistic", c); }
    { BinCase c; c.ex = {0.0}; show_bin_check("one x edge", c); }
    { BinCase c; c.null_ex = true; show_bin_check("ex NULL", c); }
    { BinCase c; c.ex = {0.0, kInf}; c.x_hi = kInf; show_bin_check("x edge inf", c); }
    { BinCase c; c.ex = {kNaN, 1.0}; show_bin_check("x edge NaN", c); }
    { BinCase c; c.ex = {0.0, 1.0, 1.0}; show_bin_check("x edges equal", c); }
    { BinCase c; c.ex = {0.0, 2.0, 1.0}; show_bin_check("x edges descending", c); }
    { BinCase c; c.x_hi = 1.5; show_bin_check("x_hi below the last edge", c); }
    { BinCase c; c.x_hi = kNaN; show_bin_check("x_hi NaN", c); }
    { BinCase c; c.ey = {0.0}; show_bin_check("1-D ignores ey", c); }
    { BinCase c; c.has_y = true; c.ey = {0.0}; show_bin_check("one y edge", c); }
    { BinCase c; c.has_y = true; c.null_ey = true; show_bin_check("ey NULL", c); }
    { BinCase c; c.has_y = true; c.ey = {0.0, -kInf}; show_bin_check("y edge -inf", c); }
    { BinCase c; c.has_y = true; c.ey = {1.0, 0.0}; show_bin_check("y edges descending", c); }
    { BinCase c; c.has_y = true; c.y_hi = 0.5; show_bin_check("y_hi below the last edge", c); }
    { BinCase c; c.has_y = true; c.ex = {0.0}; c.ey = {0.0}; show_bin_check("x before y", c); }
    { BinCase c; c.has_x = false; show_bin_check("x NULL", c); }
    { BinCase c; c.has_v = false; show_bin_check("v NULL", c); }
    { BinCase c; c.has_x = false; c.R = 0; show_bin_check("x NULL without rows", c); }
    { BinCase c; c.has_v = false; c.G = 0; c.gid = {5, 5, 5, 5}; show_bin_check("v NULL and gid without groups", c); }
    { BinCase c; c.G = 2; c.gid = {0, 1, -1, 0}; show_bin_check("gid -1", c); }
    { BinCase c; c.G = 2; c.gid = {0, 1, 1, 2}; show_bin_check("gid G", c); }
    { BinCase c; c.G = 2; c.gid = {0, 1, 1, 0}; show_bin_check("gid in range", c); }
    { BinCase c; c.has_y = true; c.G = 3; c.gid = {2, 2, 0, 1}; show_bin_check("2-D with gid", c); }
    { BinCase c; c.ex = {-1.7e308, 1.7e308}; c.x_hi = 1.7e308; show_bin_check("x range overflows", c); }
    {
        // the cells of one group stay below 2^31: 46341^2 is the first square above it (an axis alone cannot reach it: nx is int32)
        BinCase c; c.has_y = true; c.ex = ramp(46342); c.x_hi = 46341.0; c.ey = ramp(46342); c.y_hi = 46341.0;
        show_bin_check("46341 x 46341 cells", c);
        c.ey = ramp(46341); c.y_hi = 46340.0;
        show_bin_check("46341 x 46340 cells", c);
        c.ex = ramp(65537); c.x_hi = 65536.0; c.ey = ramp(32769); c.y_hi = 32768.0;
        show_bin_check("2^31 cells", c);
        // G * cells < 2^63 cannot fail after the first limit (G < 2^31 as well): the largest of both passes
        c.ex = ramp(46342); c.x_hi = 46341.0; c.ey = ramp(46341); c.y_hi = 46340.0; c.G = 2147483647;
        show_bin_check("2^31-1 groups of 46341 x 46340 cells", c);
        c.R = 0;
        show_bin_check("... without rows", c);
    }

    // ---- bin_layout
    for (long long R : {1LL, 255LL, 256LL, 257LL, (long long)long_rows - 1, (long long)long_rows, 2147483647LL})
        for (int two_d = 0; two_d < 2; ++two_d)
            for (int has_gid = 0; has_gid < 2; ++has_gid)
                for (int median = 0; median < 2; ++median) {
                    const int nx = R == 256 ? 33 : 3, ny = R == 256 ? 32 : 4;      // 256: edges that cross a 256-byte boundary in 2-D
                    const gpsat::BinLayout l = gpsat::bin_layout(R, nx, ny, two_d, has_gid, median, long_rows);
                    std::printf("bin_layout R=%lld nx=%d ny=%d two_d=%d gid=%d median=%d: in %zu x %zu v %zu y %zu gid %zu | keys %zu rows %zu vals %zu | "
                                "runs %zu n_cells %zu n_runs %zu n_long %zu flags %zu long_list %zu\n",
                                R, nx, ny, two_d, has_gid, median, l.in_bytes, l.in_x, l.in_v, l.in_y, l.in_gid, l.keys_bytes, l.rows_bytes,
                                l.vals_bytes, l.runs_bytes, l.runs_n_cells, l.runs_n_runs, l.runs_n_long, l.runs_flags, l.runs_long_list);
                }

    // ---- bin_scales
    {
        struct { const char* name; std::vector<double> ex, ey; bool two_d; int G; unsigned stats; } cases[] = {
            {"1-D", {0.0, 0.5, 4.0}, {}, false, 1, GPSAT_BIN_MEAN},
            {"1-D, 7 groups, every statistic", {-3.0, 0.0, 1.0, 7.0}, {}, false, 7, 127u},
            {"2-D", {0.0, 1.0, 2.0, 3.0}, {10.0, 10.25, 10.5}, true, 1, GPSAT_BIN_COUNT | GPSAT_BIN_MEDIAN},
            {"2-D, 5 groups", {0.0, 0.1, 0.3}, {-1e-3, 1e-3}, true, 5, GPSAT_BIN_STD | GPSAT_BIN_MIN | GPSAT_BIN_MAX},
            {"x range overflows", {-1.7e308, 0.0, 1.7e308}, {0.0, 1.0}, true, 2, GPSAT_BIN_SUM},
            {"y range overflows", {0.0, 1.0}, {-1.7e308, 1.7e308}, true, 2, GPSAT_BIN_SUM},
            {"denormal range", {0.0, 5e-324}, {}, false, 1, GPSAT_BIN_SUM},
            {"2^31-1 groups", {0.0, 1.0, 2.0}, {0.0, 1.0, 2.0, 3.0}, true, 2147483647, GPSAT_BIN_MEDIAN},
        };
        for (const auto& c : cases) {
            const gpsat::BinScales s = gpsat::bin_scales((int)c.ex.size(), c.ex.data(), (int)c.ey.size(), c.ey.data(), c.two_d, c.G, c.stats);
            std::printf("bin_scales %s: inv_x %.17g inv_y %.17g sentinel %llu n_stat %d\n", c.name, s.inv_x, s.inv_y, s.sentinel, s.n_stat);
        }
        const std::vector<double> ex = ramp(46342), ey = ramp(46341);
        const gpsat::BinScales s = gpsat::bin_scales(46342, ex.data(), 46341, ey.data(), true, 2147483647, 1u);
        std::printf("bin_scales largest grid: inv_x %.17g inv_y %.17g sentinel %llu n_stat %d\n", s.inv_x, s.inv_y, s.sentinel, s.n_stat);
    }

    return check_cache();
}
