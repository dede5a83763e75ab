// gpsat_kernels.h -- internal interface between the C ABI (gpsat_capi.cpp) and the gfx950 kernels.
#ifndef GPSAT_KERNELS_H
#define GPSAT_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "gpsat_select_types.h"

// Largest tile the C ABI accepts in any dtype (gpsat_max_tile_obs searches down from here), and the block columns (32
// observations each) of the largest fp32 tile: the words of the fp32 sweep flags colrow[] in the workgroup state
// (gpsat_opt.h Shared) and in each cooperative control block (gpsat_coop.h CoopCtl).  phase_pt writes colrow[0 .. NB-1].
#define GPSAT_MAX_TILE_OBS 4096
#define GPSAT_PT_MAXNB 128
static_assert(32 * GPSAT_PT_MAXNB >= GPSAT_MAX_TILE_OBS, "fp32 sweep flags must cover the largest tile gpsat_max_tile_obs allows");

namespace gpsat {

// All pointers are DEVICE pointers.
// per-tile words of multi-start state (gpsat_opt.h ms_end_start)
constexpr int MS_WORDS = 16;
// Per-tile memo of recent evaluations (fp32 tile kernels, KernelArgs::memo), 32-bit words.  Header: [0] entries stored so far,
// [1] entry (+ 1) whose factor, z and scaled coordinates are in the running workgroup's workspace and LDS (0: none), [2] entry
// (+ 1) of the previous evaluation (0: none), [3] evaluations answered from the memo, [4] those that repeated the previous
// evaluation's key, [5] the last line-search evaluation was answered from the memo.  Then MEMO_K entries, replaced round-robin:
// the key (6 floats: scaled inverse length scales, sf2, sn2, as the evaluation forms them), nll (fp64) and the 6 summed
// gradient values in front of the chain to theta (fp64).
constexpr int MEMO_K = 4, MEMO_HDR = 8, MEMO_ENTRY = 6 + 2 + 12;
constexpr int MEMO_WORDS = MEMO_HDR + MEMO_K * MEMO_ENTRY;

struct KernelArgs {
    int T, kernel, optimiser, max_iter, max_ls, NBmax;
    double ftol, gtol, adam_lr;
    double noise_rel;             // relative objective resolution of the arithmetic (line-search failure at the noise floor)
    const long long* obs_off;     // [T+1]
    const long long* pred_off;    // [T+1]
    const double* theta0;         // [T*H], H = gpsat_n_hyper(kernel, D)
    const double* lo;             // [T*H]
    const double* hi;             // [T*H]
    const unsigned char* trainable;  // [H]
    const float* X;               // [sumN*D]
    const float* y;               // [sumN]
    const float* Xs;              // [sumP*D]
    double* theta;                // [T*H]
    double* nll;                  // [T]
    double* grad;                 // [T*H] or nullptr
    int* status;                  // [T]
    int* n_eval;                  // [T]
    int* n_iter;                  // [T] optimiser iterations completed, or nullptr
    float* f_mean;                // [sumP]
    float* f_var;
    float* y_var;
    const int* order;             // [T] tile processing order (largest first)
    int* queue;                   // work-queue head (zeroed before launch)
    float* ws;                    // per-workgroup workspace
    size_t ws_stride;             // floats per workgroup
    unsigned long long* prof;     // [NW*16] cycle counters (diagnostic build only, else nullptr)
    const long long* cov_off;     // [T+1] element offsets into f_cov, or nullptr
    float* f_cov;                 // per tile P x P posterior covariance, or nullptr
    int PCmax;                    // max prediction chunks per tile (only used with f_cov)
    // time slicing of the optimisation (seg_cost = 0: every tile runs to completion from `queue`):
    // tiles are served from a ring; after ~seg_cost / NB^3 evaluations an unfinished tile's optimiser state is saved and the
    // tile goes to the back of the ring, so that all tiles of a homogeneous batch finish together instead of leaving a tail
    unsigned long long* ring;     // [ring_mask + 1] entries (sequence + 1) << 32 | resumed << 31 | tile; first T preset
    int* ring_ctl;                // [0] pop counter, [16] push counter (preset T), [32] unfinished tiles (preset T)
    unsigned* state;              // [T][state_words] saved optimiser state (the kernel's Shared struct)
    int ring_mask, state_words, seg_cost;
    // cooperative tiles (nullptr: off): one CoopCtl per workgroup (gpsat_coop.h), zeroed before the launch; workgroups that
    // find no tile left attach themselves to a running tile and pull groups of its sweep / gradient queues
    void* coop;                   // [grid] CoopCtl
    int* coop_live;               // tiles not finished yet (preset T): the helpers' exit condition
    // teams (fp64 kernels, gpsat_kernels_f64.hip): team_size workgroups run one tile together; [grid / team_size] TeamCtl of
    // 256 bytes, zeroed before the launch
    int team_size;
    void* team_ctl;
    int coop_min_nb;              // smallest tile (block columns) worth helping
    int coop_hdiv;                // helpers wanted per tile: NB / coop_hdiv (1..7)
    int coop_force;               // developer / tests: every evaluation of a helpable tile runs the cooperative code path, helped or not
    // diagnostic builds only (-DGPSAT_DUMP, scripts/e48_dump_compare.py): per tile the factor square, DinvT, z, alpha and the
    // log-determinant of its LAST evaluation, [T][dump_stride] floats in device memory; nullptr in the product
    float* dump;
    size_t dump_stride;
    // deferred predictions (fp32 4-wave build, time-sliced launches without f_cov; pq == nullptr: every prediction inline):
    // a tile that finishes its fit while other tiles wait in the ring leaves a snapshot of what its prediction reads and
    // takes the next tile; workgroups that find the ring empty run the predictions (gpsat_ring.h)
    unsigned long long* pq;       // [pq_slots] published entries (tile + 1; 0: not yet), zeroed before the launch
    int* pq_ctl;                  // [0] snapshot slots taken, [16] entries claimed; zeroed before the launch
    int* cu_busy;                 // [2048] per CU (XCC_ID << 8 | HW_ID[15:8]): workgroups running a tile; zeroed
    float* pq_snap;               // [pq_slots][pq_stride] snapshots
    size_t pq_stride;             // floats per snapshot slot
    int pq_slots;
    // multi-start bounded L-BFGS-B in log space (gpsat_fit_predict_batch_ms; ms_S = 0: off), device pointers (gpsat_opt.h)
    int ms_S = 0;                 // starts per tile
    const double* ms_starts = nullptr;   // [T][ms_S - 1][H]
    double* ms_state = nullptr;   // [T][MS_WORDS]
    double* ms_fout = nullptr;    // [T][ms_S] or nullptr
    // evaluation memo of the fp32 tile kernels (nullptr: every evaluation is computed): a line-search evaluation whose D + 2
    // parameter floats equal those of one of the tile's last MEMO_K distinct evaluations is answered from it (gpsat_kernels.hip)
    unsigned* memo = nullptr;         // [T][MEMO_WORDS]; a tile's header is cleared where the tile starts
    unsigned* memo_stats = nullptr;   // developer, zeroed: [0] evaluations, [1] answered from the memo, [2] of those: the previous key
                                      // again, [3] tiles with such an evaluation, [4] tiles whose last line-search evaluation was one,
                                      // [5] as [1] and [6] tiles, of the tiles with >= 30 evaluations, [7] most evaluations of a tile,
                                      // [8] most computed evaluations of a tile
};

// Held-out predictions of the fp64 tile kernels (gpsat_fit_predict_batch_cv); device pointers.  Folds are numbered through the
// batch in tile order; `pairs` lists, per tile, the 16 x 16 blocks (a << 16 | b, a >= b) of K_y^-1 that hold two rows of one fold.
struct CvArgs {
    const int* pair_off = nullptr;    // [T+1] into pairs
    const int* pairs = nullptr;
    const int* fold_off = nullptr;    // [T+1] folds of a tile
    const int* fold_ptr = nullptr;    // [F+1] into fold_rows
    const int* fold_rows = nullptr;   // rows of every fold (positions inside the tile), in the order of the rows
    const int* fold_a = nullptr;      // [F] doubles in front of the fold's g x g matrix in the tile's scratch
    const int* row_fold = nullptr;    // [sumN] the row's fold, -1: never held out
    const int* row_pos = nullptr;     // [sumN] the row's position inside its fold
    double* mean = nullptr;           // [sumN] outputs
    double* f_var = nullptr;
    double* y_var = nullptr;
    double* fold_lpd = nullptr;       // [F] joint log predictive density of every fold (gpsat_fit_predict_batch_cv_joint), nullptr: off
};
// Known noise variances per observation for the fp64 tile kernels (gpsat_fit_predict_batch_noise); a device pointer.
struct NoiseArgs {
    const double* obs_var = nullptr;  // [sumN] v of K_y = K + sn2 I + diag(v), in the order of y
};
// The gradient of the posterior mean at the prediction points and its variance per component (gpsat_fit_predict_batch_grad);
// device pointers, both [sumP, D] row-major.
struct GradArgs {
    double* f_grad = nullptr;
    double* f_grad_var = nullptr;
};
// The second derivatives of the posterior mean at the prediction points (gpsat_fit_predict_batch_hess); device pointers.  The
// pairs a <= b of the coordinates in `dims` (bit a: coordinate a), a ascending, then b, are the npair columns of f_hess and
// f_hess_var, [sumP, npair] row-major.  f_lap / f_lap_var [sumP]: sum_a lap_w[a] d2f/dx_a^2 and its variance; both null: no
// such pass.  f_grad / f_grad_var [sumP, D]: the grad row's two outputs from the same launch; both null: not asked for.
struct HessArgs {
    double* f_hess = nullptr;
    double* f_hess_var = nullptr;
    double* f_lap = nullptr;
    double* f_lap_var = nullptr;
    double* f_grad = nullptr;
    double* f_grad_var = nullptr;
    double lap_w[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned dims = 0;
    int npair = 0;
};
#define GPSAT_MAX_CV_FOLD 256         // largest fold: sum g^2 <= 256 N doubles fits the prediction scratch of a tile's workspace

size_t shared_bytes(int D, int NBmax);
// fp64 kernels (gpsat_kernels_f64.hip): X, y, Xs, f_* and ws of KernelArgs point at doubles, ws_stride counts doubles
size_t shared_bytes_f64(int D, int NBmax);
size_t workspace_doubles_per_wg_f64(int NBmax, int PCcov);
int state_words_f64();
// 4-wave build (gpsat_kernels_f64.hip -DGPSAT_F64_W4): two workgroups per CU for tiles whose LDS fits twice
size_t shared_bytes_f64_w4(int D, int NBmax);
size_t workspace_doubles_per_wg_f64_w4(int NBmax, int PCcov);
int state_words_f64_w4();
// The variants of the fp64 tile loop (the table at the top of gpsat_kernels_f64.hip), launch_tiles_f64[_variant][_w4], one
// signature: `cv` is null unless the variant is cv, `nz` unless it is noise, `gr` unless it is grad, `hs` unless it is hess.  A (D, a.kernel, a.team_size) a variant does not have: hipErrorInvalidValue.
//   plain  kernels 0..3, D = 1..4, H = D + 2; teams in the 8-wave build
//   cv     the same with the held-out phase (gpsat_fit_predict_batch_cv), one workgroup per tile
//   rq     the RationalQuadratic covariance function: kernel 4, D = 1..3, H = D + 3, one workgroup per tile
//   mean   a trainable constant mean: kernels 0..3, D = 1..3, H = D + 3 with c last, one workgroup per tile
//   noise  known noise variances per observation (NoiseArgs): kernels 0..3, D = 1..4, H = D + 2, one workgroup per tile
//   grad   the gradient of the posterior mean and its variance (GradArgs): kernels 0, 2, 3, D = 1..4, H = D + 2, one workgroup per tile, no f_cov
//   hess   the second derivatives of the posterior mean, their variances and a weighted Laplacian (HessArgs), with the grad
//          row's outputs when asked for: kernels 0, 3, D = 1..4, H = D + 2, one workgroup per tile, no f_cov
// LDS, workspace and state words of every variant are those of the build of the same wave count.
typedef hipError_t F64Launch(int D, const KernelArgs& a, const CvArgs* cv, const NoiseArgs* nz, const GradArgs* gr, const HessArgs* hs,
                             int grid, size_t smem, hipStream_t stream);
F64Launch launch_tiles_f64, launch_tiles_f64_w4, launch_tiles_f64_cv, launch_tiles_f64_cv_w4;
F64Launch launch_tiles_f64_rq, launch_tiles_f64_rq_w4, launch_tiles_f64_mean, launch_tiles_f64_mean_w4;
F64Launch launch_tiles_f64_noise, launch_tiles_f64_noise_w4, launch_tiles_f64_grad, launch_tiles_f64_grad_w4;
F64Launch launch_tiles_f64_hess, launch_tiles_f64_hess_w4;
size_t pq_floats_per_slot(int D, int NBmax);              // deferred-prediction snapshot slot (KernelArgs::pq_stride)
size_t workspace_floats_per_wg(int NBmax, int PCcov);     // PCcov: prediction chunks kept for f_cov (0 = none)
hipError_t launch_tiles(int D, const KernelArgs& a, int grid, size_t smem, hipStream_t stream);
int state_words();                                        // 32-bit words of saved optimiser state per tile (time slicing)
// 8-wave build of the same kernels (gpsat_kernels.hip -DGPSAT_W8): used when a workgroup needs more than half of the LDS
size_t shared_bytes_w8(int D, int NBmax);
size_t workspace_floats_per_wg_w8(int NBmax, int PCcov);
hipError_t launch_tiles_w8(int D, const KernelArgs& a, int grid, size_t smem, hipStream_t stream);
int state_words_w8();

// tile selection (gpsat_select.hip); all pointers are device pointers.  The criteria come first (gpsat_select_types.h).
struct SelectArgs : SelectCriteria {
    long long M;                      // rows of the point table
    int C;                            // columns of the point table / reference table
    int T;                            // experts
    const double* pts;                // [C][M] column-major (SoA)
    const double* refs;               // [T][C] row-major
    int n_chunks;                     // row chunks (grid.y)
    long long chunk_rows;             // rows per chunk (multiple of 64)
    long long* counts;                // [T][n_chunks]   (count pass)
    const long long* off;             // [T][n_chunks] start offsets (fill pass)
    int* idx;                         // [off[T]] (fill pass)
    const double* box;                // [ceil(M / sub)][C][2] per-column [min, max] of every sub-chunk of rows, or nullptr
    const int* eorder;                // [T] order in which the experts are dealt to the waves (neighbours together), or nullptr
    int n_bounds;                     // interval bound pairs per expert (kind 2)
    const double* bounds;             // [T][n_bounds][2] {lo, hi}: lo <= x < hi, or nullptr when n_bounds == 0
};

hipError_t launch_select(const SelectArgs& a, bool fill, hipStream_t stream);
hipError_t launch_select_boxes(long long M, int C, const double* pts, double* box, hipStream_t stream);
int select_sub_rows();      // rows per box; chunk_rows must be a multiple of it

// Spatial binning of the point table (gpsat_select.hip) by a BinSpec (gpsat_select_types.h).
hipError_t select_bin_rows(long long M, int C, const double* pts, const BinSpec& b, unsigned* keys, unsigned* keys_out, int* rows,
                           int* perm, double* pts_perm, void* temp, size_t& temp_bytes, hipStream_t stream);
// selected positions of the binned table -> source rows, every expert's list ascending (the reference's source row order)
hipError_t select_unbin(int T, long long total, const unsigned* seg_off, const int* perm, int* idx, int* idx_out, void* temp,
                        size_t& temp_bytes, hipStream_t stream);

// The keyed sort-and-run-heads stage (gpsat_key_runs.hip); device pointers, carved out of the user's
// buffers as gpsat_key_runs_plan.h lays them out.  The user's key kernel writes keys[i] and rows[i] = i.
struct KeyRuns {
    long long R;                      // rows (< 2^31)
    unsigned long long sentinel;      // the key of rows that take no part: above every other key, so they sort behind every group
    unsigned long long *keys, *keys_sorted;   // [R]
    unsigned *rows, *perm;            // [R] source rows, and the same in sorted order
    unsigned char* flags;             // [R] 1 at the first row of every run of equal keys
    unsigned* starts;                 // [R + 1] first sorted row of every run; starts[counts[0]] = counts[1]
    unsigned* n_runs;                 // [1] runs, the sentinel's included
    long long* counts;                // [2] runs without the sentinel's (cells, groups), rows in them
};
// the head flag of sorted row i
__device__ __forceinline__ unsigned char key_run_head(const unsigned long long* __restrict__ keys_sorted, long long i) {
    return (i == 0 || keys_sorted[i] != keys_sorted[i - 1]) ? 1 : 0;
}
// Launches the kernel that writes k.flags[0 .. R) from k.keys_sorted (key_run_head), and whatever the user does in that pass.
typedef void KeyRunsFlags(const void* ctx, hipStream_t stream);
// Stable sort of (key, row) over the sentinel's bits, head flags (write_flags(ctx, stream); nullptr: the stage's own kernel), run starts,
// the sentinel's run dropped; leaves counts[0..1] on the device.  temp == nullptr: only the scratch size is returned.  `after_sort`: recorded behind the sort.
hipError_t key_runs(const KeyRuns& k, KeyRunsFlags* write_flags, const void* ctx, hipEvent_t after_sort, void* temp,
                    size_t& temp_bytes, hipStream_t stream);

// binning of raw observations (gpsat_bin.hip); device pointers.  The statistic bits are those of include/gpsat_hip.h.
#ifndef GPSAT_BIN_COUNT
#define GPSAT_BIN_COUNT  1u
#define GPSAT_BIN_SUM    2u
#define GPSAT_BIN_MEAN   4u
#define GPSAT_BIN_STD    8u
#define GPSAT_BIN_MIN    16u
#define GPSAT_BIN_MAX    32u
#define GPSAT_BIN_MEDIAN 64u
#endif
struct BinArgs : KeyRuns {            // sentinel: G * cells, the key of rows outside the grid; counts: non-empty cells, rows inside the grid
    int nx, ny;                       // edges per axis (>= 2); ny is not read when y == nullptr (1-D)
    const double *x, *y, *v;          // [R] coordinates and values; y == nullptr: 1-D
    const int* gid;                   // [R] group of every row, or nullptr (all rows in group 0)
    const double *ex, *ey;            // [nx], [ny] increasing bin edges
    double x_hi, y_hi;                // inclusive upper limit of the last bin (>= the last edge)
    double inv_x, inv_y;              // bins / (last edge - first edge): the guess of bin_index
    double* vs;                       // [R] values in sorted order
    double *vcanon, *vsorted;         // [R] median only: vs with one NaN pattern, and every cell's values ascending
    unsigned* n_long;                // [1] cells of bin_long_rows() rows or more (zeroed by bin_cell_stats)
    unsigned* long_list;              // [R / bin_long_rows() + 1] those cells, in no particular order
    unsigned mask;                    // GPSAT_BIN_* statistics wanted
    long long* out_keys;              // [n_cells] ascending
    double* out;                      // [statistics in bit order][n_cells]
};
// key per row, then key_runs with the gather of the values in its flag pass; leaves counts[0..1] on the device
hipError_t bin_sort_rows(const BinArgs& a, void* temp, size_t& temp_bytes, hipStream_t stream);
hipError_t bin_cell_stats(const BinArgs& a, long long n_cells, long long n_valid, void* temp, size_t& temp_bytes, hipStream_t stream);
int bin_long_rows();                  // rows from which a cell's sums are walked by a wave instead of a lane

// refitted cross-validation (gpsat_cvfold.hip); device pointers, tables as gpsat_cvfold.h builds them.  Bulk arrays are float
// or double according to `f64`.
struct CvFoldArgs {
    int F2, D, f64, recentre;         // derived tiles (fitted folds), input dimension, element type, de-mean the remaining rows
    long long sumN;                   // rows of the source batch
    const long long *d_obs_off, *d_pred_off;      // [F2+1] CSR offsets of the derived batch
    const long long* d_src_off;       // [F2] first row of the derived tile's source tile
    const int *d_src_n, *d_fold;      // [F2] rows of the source tile, fold of the derived tile
    const int* d_status;              // [F2] status of the derived tile's fit (scatter only)
    const int *fold_ptr, *fold_rows;  // [F+1], [R] a fold's tile-local rows, ascending
    const int* fold_derived;          // [F] derived tile of a fold, -1: not fitted
    const int *row_fold, *row_pos;    // [sumN] fold of a source row (-1: never held out), position in it
    const void *X, *y;                // source batch [sumN, D], [sumN]
    void *Xd, *yd, *Xsd;              // derived batch [E, D], [E], [P2, D]
    double* delta;                    // [F2] mean of the remaining rows (0 without recentre)
    const void *fm, *fv, *yv;         // [P2] predictions of the derived batch (scatter)
    void *cv_mean, *cv_f_var, *cv_y_var;          // [sumN]; cv_y_var may be nullptr
    // joint log predictive density of every fitted fold (gpsat_fit_predict_batch_cv_refit_joint, fp64 only; cvfold_lpd)
    const long long* cov_off = nullptr;           // [F2+1] into f_cov: g_j^2 elements per derived tile
    double* f_cov = nullptr;                      // the derived batch's posterior covariances; factorised in place
    const double* sn2 = nullptr;                  // [F2] fitted likelihood variance of every derived tile
    double* resid = nullptr;                      // [P2] scratch: y'_G - f*, consumed by the forward substitution
    double* lpd = nullptr;                        // [F2] out
};
hipError_t launch_cvfold_expand(const CvFoldArgs& a, hipStream_t stream);
hipError_t launch_cvfold_scatter(const CvFoldArgs& a, hipStream_t stream);
hipError_t launch_cvfold_lpd(const CvFoldArgs& a, hipStream_t stream);

#define GPSAT_GLUE_MAXVARS 4
// post-processing (gpsat_post.hip); device pointers
hipError_t launch_smooth(int T, const double* x, const double* y, const double* vals, double lx, double ly, double* out,
                         hipStream_t stream);
hipError_t launch_glue(int G, int ndim, int nvars, long long R, const long long* seg, const double* pred, const double* xprt,
                       const double* vals, double sigma, const double* sigma_rows, double* out, hipStream_t stream);
// keyed glue (gpsat_glue_keyed_batch): rows in any order, grouped by an integer key on the device
struct GlueKeyedArgs : KeyRuns {      // sentinel: largest key + 1, the key of ignored rows; counts: distinct keys >= 0, rows that have one
    int ndim, nvars;
    const double *pred, *xprt, *vals, *sigma_rows;   // [ndim][R], [ndim][R], [nvars][R], [R] or nullptr; in SOURCE order
    double sigma;
    double md2;                       // max_dist^2; < 0: no limit
    long long* out_key;               // [G] ascending
    int* out_count;                   // [G] rows that took part
    double* out;                      // [nvars][G]
};
// with what the orders above 0 add (gpsat_glue_keyed_grad_batch, _hess_batch; vals is the one value [R], nvars 1): from order 1
// grad [ndim][R] and out_grad [ndim][G]; order 2 hess [npair][R] and out_hess [npair][G], npair = ndim (ndim + 1) / 2 in the
// order (0,0), (0,1), (1,1); nullptr where the order has none
struct GlueKeyedOrderArgs : GlueKeyedArgs {
    const double *grad, *hess;
    double *out_grad, *out_hess;
};
// key_runs on the keys as a caller gave them: key [R], < 0: the row is ignored.  Also the sort of the grouped tracks.
hipError_t glue_keyed_sort(const KeyRuns& k, const long long* key, void* temp, size_t& temp_bytes, hipEvent_t after_sort, hipStream_t stream);
// one team of `team` lanes per group, gathering through the permutation; team in {1, 4, 8, 16, 32, 64}.  order 0: the glued
// columns; 1: the glued value and the exact slope of the glued map; 2: its second derivatives as well.  What an order shares
// with the one below holds the same bytes.
hipError_t launch_glue_keyed(const GlueKeyedOrderArgs& a, long long G, int team, int order, hipStream_t stream);
int glue_keyed_team();                // the team width of the product

// raw rows to x / y and track numbers (gpsat_prep.hip); device pointers.  The scalars come from gpsat_prep_plan.h.
struct ProjectArgs {
    long long n;                      // rows (< 2^31)
    const double *in0, *in1;          // forward: lon, lat (degrees); inverse: x, y (metres)
    double *out0, *out1;              // forward: x, y; inverse: lon, lat
    double lon_0;                     // degrees
    double a, e, e2, one_m_e2, inv_2e, qp;        // WGS84: semi-major axis, eccentricity, e^2, 1 - e^2, 1 / (2e), q(90 degrees)
    double qp_lo;                     // qp + qp_lo: q(90 degrees) to twice the precision (the inverse beyond the equator)
};
hipError_t launch_project(const ProjectArgs& a, bool forward, bool south, hipStream_t stream);

struct TrackArgs {
    long long n;                      // rows (< 2^31)
    int n_cols, mode;                 // columns of the distance; GPSAT_TRACK_*: 0 cut, 1 runs, 2 given
    const double* cols[3];            // [n] in SOURCE order
    const unsigned* perm;             // [n] source row of every taken row, or nullptr: the rows as they are
    const unsigned char* heads;       // [n] 1 at the first taken row of every group (run heads of the sort), or nullptr: one group
    const long long* n_valid;         // [1] taken rows that are in a group (the others follow them), or nullptr: all
    double cut_off;
    int start_track;
    double* delta;                    // [n] out, or nullptr (runs only)
    int* track;                       // [n] out; between the passes: what the scan adds up
    int* order;                       // [n] out
    int* block_sums;                  // [prep_scan_blocks(n)] scratch of the scan
};
int prep_scan_block();                // B: rows per block of the three-pass scan
// int32 group codes as the 64-bit keys glue_keyed_sort takes (negative: in no group)
hipError_t launch_track_keys(long long n, const int* group, long long* key, hipStream_t stream);
// distances and flags, block sums, their scan, the scan applied: track[] and order[] final
hipError_t launch_track(const TrackArgs& a, hipStream_t stream);

// sparse GP experts (gpsat_sgpr.hip, fp64 only); device pointers.  One workgroup per tile from an atomic queue.
struct SgprArgs {
    int T, kernel, optimiser, max_iter, max_ls, Mmax;
    double ftol, gtol, adam_lr, noise_rel, jitter;
    const long long* obs_off;     // [T+1]
    const long long* pred_off;    // [T+1]
    const long long* z_off;       // [T+1] rows of Z per tile
    const double* theta0;         // [T*H]
    const double* lo;
    const double* hi;
    const unsigned char* trainable;
    const double* X;              // [sumN*D]
    const double* y;              // [sumN]
    const double* Xs;             // [sumP*D]
    const double* Z;              // [sumM*D]
    double* theta;
    double* nll;
    double* grad;                 // or nullptr
    int* status;
    int* n_eval;
    int* n_iter;                  // or nullptr
    double* f_mean;
    double* f_var;
    double* y_var;
    const int* order;             // [T] processing order
    int* queue;                   // zeroed before launch
    double* ws;                   // per-workgroup workspace
    size_t ws_stride;             // doubles per workgroup
};
#define GPSAT_MAX_INDUCING 1024    // largest M per tile (workspace: (7 + D) M^2 doubles per workgroup)
size_t sgpr_shared_bytes(int D, int Mmax);
size_t sgpr_workspace_doubles_per_wg(int D, int Mmax);
int sgpr_threads();
hipError_t launch_sgpr(int D, const SgprArgs& a, int grid, size_t smem, hipStream_t stream);

}  // namespace gpsat
#endif
