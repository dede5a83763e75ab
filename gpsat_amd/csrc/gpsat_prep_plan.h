// gpsat_prep_plan.h -- host side of gpsat_project_batch and gpsat_track_batch: the argument checks, the constants of the
// projection, the launch geometry and the layout of the handle's buffers.  Plain C++ without a HIP call, in the manner of
// gpsat_bin_plan.h, so that tests/prep_plan_host_check.cpp can run it under the host sanitizers; the two checks are exported
// like gpsat::check_glue_keyed, so that tests drive every refusal without a device.  Part of gpsat_capi.cpp's translation unit.
#ifndef GPSAT_PREP_PLAN_H
#define GPSAT_PREP_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "gpsat_hip.h"
#include "gpsat_key_runs_plan.h"

namespace gpsat {

constexpr int64_t PREP_MAX_ROWS = 2147483647LL;       // the sort carries a 32-bit source row, the scan counts in int32

// ---- projection
// WGS84 and what the kernels need of it, computed once per call in fp64: q(phi) of Snyder 3-12 at phi = 90 degrees is
// q_p = (1 - e^2) (1 / (1 - e^2) - ln((1 - e) / (1 + e)) / (2e)).
// qp + qp_lo is q_p to twice the precision (1.9955310875028367 + 9.345699910345638e-17, mpmath at 50 digits; qp itself is the
// formula's fp64 value, a few ulps off): beyond the equator the inverse takes 2 q_p - (rho / a)^2, whose error decides phi.
struct ProjConst { double a, e, e2, one_m_e2, inv_2e, qp, qp_lo; };

inline ProjConst proj_const() {
    ProjConst c;
    const double f = 1.0 / 298.257223563;
    c.a = 6378137.0;
    c.e2 = f * (2.0 - f);
    c.e = std::sqrt(c.e2);
    c.one_m_e2 = 1.0 - c.e2;
    c.inv_2e = 1.0 / (2.0 * c.e);
    c.qp = c.one_m_e2 * (1.0 / c.one_m_e2 - std::log((1.0 - c.e) / (1.0 + c.e)) * c.inv_2e);
    c.qp_lo = (1.9955310875028367 - c.qp) + 9.345699910345638e-17;
    return c;
}

// Everything gpsat_project_batch can refuse (the handle is the entry point's to check).  GPSAT_OK, or GPSAT_EINVAL with the
// reason in why[why_len].
int check_project(const gpsat_project* p, char* why, size_t why_len) {
    if (why_len > 0) why[0] = 0;
    auto bad = [&](const char* msg) { std::snprintf(why, why_len, "gpsat_project_batch: %s", msg); return GPSAT_EINVAL; };
    if (!p) return bad("gpsat_project is NULL");
    for (int i = 0; i < 8; ++i)
        if (p->reserved[i] != 0) return bad("reserved words must be 0");
    if (p->n < 0) return bad("n must not be negative");
    if (p->n > PREP_MAX_ROWS) return bad("more than 2^31-1 rows in one call");
    if (p->direction != GPSAT_PROJECT_FORWARD && p->direction != GPSAT_PROJECT_INVERSE) return bad("unknown direction (GPSAT_PROJECT_FORWARD or _INVERSE)");
    if (p->memory != GPSAT_MEM_HOST && p->memory != GPSAT_MEM_DEVICE) return bad("bad memory flag");
    if (!(p->lat_0 == 90.0 || p->lat_0 == -90.0)) return bad("lat_0 must be 90 or -90: only the polar aspects are built");
    if (!std::isfinite(p->lon_0)) return bad("lon_0 must be finite");
    if (p->n > 0 && (!p->in0 || !p->in1 || !p->out0 || !p->out1)) return bad("in0 / in1 / out0 / out1 is NULL");
    return GPSAT_OK;
}

// ---- tracks
// Everything gpsat_track_batch can refuse.  In host mode the group codes are read: a code below -1 is refused with its row.
// *sentinel (when the arguments pass): the key that rows in no group get on the device, one above the largest code; in device
// mode, where the codes are not read, 2^31.
int check_track(const gpsat_track* t, unsigned long long* sentinel, char* why, size_t why_len) {
    if (why_len > 0) why[0] = 0;
    if (sentinel) *sentinel = 0;
    auto bad = [&](const char* msg) { std::snprintf(why, why_len, "gpsat_track_batch: %s", msg); return GPSAT_EINVAL; };
    if (!t) return bad("gpsat_track is NULL");
    for (int i = 0; i < 8; ++i)
        if (t->reserved[i] != 0) return bad("reserved words must be 0");
    if (t->n < 0) return bad("n must not be negative");
    if (t->n > PREP_MAX_ROWS) return bad("more than 2^31-1 rows in one call");
    if (t->memory != GPSAT_MEM_HOST && t->memory != GPSAT_MEM_DEVICE) return bad("bad memory flag");
    if (t->mode != GPSAT_TRACK_CUT && t->mode != GPSAT_TRACK_RUNS && t->mode != GPSAT_TRACK_GIVEN) return bad("unknown mode (GPSAT_TRACK_CUT, _RUNS or _GIVEN)");
    if (t->n_cols < 1 || t->n_cols > 3) return bad("n_cols must be 1..3");
    if (t->mode != GPSAT_TRACK_CUT && t->n_cols != 1) return bad("GPSAT_TRACK_RUNS and _GIVEN take one column");
    if (t->mode != GPSAT_TRACK_RUNS) {
        if (!std::isfinite(t->cut_off)) return bad("cut_off must be finite");
        if (t->start_track < 0) return bad("start_track must not be negative");
        if ((int64_t)t->start_track + t->n > PREP_MAX_ROWS) return bad("start_track + n must stay below 2^31: the tracks are int32");
    }
    if (t->n > 0) {
        for (int c = 0; c < t->n_cols; ++c)
            if (!t->cols[c]) return bad("a column of cols is NULL");
        if (!t->out_track || !t->out_order) return bad("out_track / out_order is NULL");
        if (t->mode != GPSAT_TRACK_RUNS && !t->out_delta) return bad("out_delta is NULL");
    }
    unsigned long long s = 1ull << 31;
    if (t->group && t->memory == GPSAT_MEM_HOST) {
        int32_t mx = -1;
        for (int64_t i = 0; i < t->n; ++i) {
            const int32_t g = t->group[i];
            if (g < -1) {
                std::snprintf(why, why_len, "gpsat_track_batch: group[%lld] = %d: codes are >= 0, or -1 for a row in no group", (long long)i, (int)g);
                return GPSAT_EINVAL;
            }
            mx = g > mx ? g : mx;
        }
        s = (unsigned long long)((int64_t)mx + 1);
    }
    if (sentinel) *sentinel = s;
    return GPSAT_OK;
}

// ---- launch geometry
// Blocks of `block` rows that cover n rows (one thread per row): 0 for n = 0; n <= 2^31 - 1 keeps it below 2^31 / block.
inline unsigned prep_blocks(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// The three-pass scan over blocks of B rows: pass 1 leaves one sum per block, pass 2 is ONE workgroup that walks the sums
// `block` at a time with a carry, pass 3 adds a block's offset to its rows.
struct ScanGeometry {
    unsigned blocks;                  // grids of pass 1 and pass 3 = number of block sums
    unsigned rounds;                  // iterations of pass 2's loop
};
inline ScanGeometry prep_scan_geometry(int64_t n, int block) {
    ScanGeometry g;
    g.blocks = prep_blocks(n, block);
    g.rounds = prep_blocks((int64_t)g.blocks, block);
    return g;
}

// Bytes of the handle's buffers and the byte offsets of what lies in them.  Device mode stages nothing: `in` holds the 64-bit
// keys only, `out` the block sums only.  keys, rows and runs are the stage's (KeyRunsLayout; runs_counts: n_groups [2]);
// all 0 without groups.
struct TrackLayout : KeyRunsLayout {
    // `in`: the columns [n_cols][n], the codes [n] int32 rounded to 8 B, the 64-bit keys of the sort [n] (the last two with groups)
    size_t in_bytes, in_cols, in_group, in_key, runs_n_groups;        // runs_n_groups: the stage's runs_counts, by the tracks' name
    // `out`: delta [n] fp64, track [n], order [n] (host mode), the block sums of the scan
    size_t out_bytes, out_track, out_order, out_sums;
};

inline TrackLayout track_layout(int64_t n, int n_cols, bool has_group, bool host_mode, int block) {
    const size_t nN = (size_t)n;
    TrackLayout l = {};
    size_t at = 0;
    if (host_mode) { l.in_cols = at; at += (size_t)n_cols * nN * sizeof(double); }
    if (has_group) {
        if (host_mode) { l.in_group = at; at += (nN * sizeof(int32_t) + 7) & ~size_t(7); }
        l.in_key = at; at += nN * sizeof(int64_t);
    }
    l.in_bytes = at;
    if (has_group) static_cast<KeyRunsLayout&>(l) = key_runs_layout(n);
    l.runs_n_groups = l.runs_counts;
    at = 0;
    if (host_mode) {
        at += nN * sizeof(double);
        l.out_track = at; at += nN * sizeof(int32_t);
        l.out_order = at; at += nN * sizeof(int32_t);
        at = (at + 7) & ~size_t(7);
    }
    l.out_sums = at;
    at += (size_t)prep_blocks(n, block) * sizeof(int32_t);
    l.out_bytes = at;
    return l;
}

}  // namespace gpsat
#endif
