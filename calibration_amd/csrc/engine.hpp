// engine.hpp — internal state behind the opaque cba_reproj handle, and the prototypes of the files that work on it.  The buffers and
// streams it is made of are in hip_glue.hpp; the one-shot solvers and the batched pipelines, which never see an Engine, are declared
// in pipelines.hpp.
//
// HBM layout (all fp64, SoA, one allocation per array):
//   u, v              [ld]          pixel observations; every residual block starts at an EVEN padded index
//                                    (so a lane's two observations are one 16-byte load/store) and ld is
//                                    the padded total rounded up to 256 elements
//   X, Y              [ld_xy]       target-plane points, DEDUPLICATED: residual blocks whose object_xy lists are
//                                    bitwise identical (the usual case: every view sees the same physical
//                                    target) share one copy, so the per-observation HBM read drops from 32 B
//                                    towards 16 B and the shared copy stays L2 / Infinity-Cache resident
//   J (Mode A output) [n_tilesA][2 + 2P - 1][128]  tile-blocked: for every 128-observation tile one contiguous
//                                    (2+2P-1) KiB region = u/v residual rows, then the P Jacobian columns of
//                                    the u row, then of the v row (streams like a fill; +6 % over whole-array
//                                    columns r[2][ld], J[2P - 1][ld], which CBA_EVAL_BLOCKED=0 still selects).
//                                    The v row's fy entry equals the u row's skew entry and lives in that one's
//                                    slot (eval_layout.hpp eval_row_slot: every access goes through it).
//                                    Seven of the 2P Jacobian rows are structural constants, written once per
//                                    buffer and not by k_eval (EvalFill below)
//   bc                [n_blocks][36] per-block chain constants (reproj_math.hpp BC_*)
//   sd                [n_cams][36]  Scheimpflug per-camera constants (SD_*)
//   intr/cam/view/target            parameter blocks, current [0] and trial [1] copies
//   tilesA / tilesB                 wave-tile tables: a tile is <=128 (Mode A) / >= TILE_B except a block's last (Mode B, R)
//                                    consecutive observations of ONE block, processed by ONE wavefront
//   partial           [n_tilesB][NACC]  per-tile Mode B sums;  blk_acc [n_blocks][NACC] per-block sums
#pragma once
#include "hip_glue.hpp"  // first: hip_runtime.h, which the math headers' CBA_HD needs
#include "eval_layout.hpp"

#include <deque>
#include <vector>

#include "../../include/calibba.h"

namespace cba {

struct Tile {          // 32 bytes, read with scalar loads (wave-uniform)
    int32_t blk;       // residual block
    int32_t count;     // observations in this tile (Mode A: padded, even; Mode B/R: valid count)
    int64_t start;     // padded observation index of the tile's first observation (u, v, outputs)
    int64_t xy_start;  // index of the tile's first target point in the DEDUPLICATED X, Y arrays
    int64_t reserved;
};

// TILE_A = 128 (Mode A: 64 lanes x 2 adjacent observations) and the row layout of a Mode A output tile: eval_layout.hpp
constexpr int OPL_B = 32;    // Mode B/R: observations per lane of the SHORTEST full tile (2048 observations: the wave reduction and the
                             // tile's partial row are paid once per tile; large problems use longer tiles, capi.cpp)
constexpr int TILE_B = 64 * OPL_B;

// What a Mode A output buffer's constant rows (reproj_math.hpp jac_const) were last filled for.  k_eval does not store those rows,
// so it may run on a buffer only while `valid` and the layout, width and chain / model it is about to use match; anything that
// gives the buffer new memory, or lets another writer at it, clears `valid` (capi.cpp ensure_eval_buffers, the ablation launches).
// Held per handle and per buffer, never per device address: the block cache hands a released block, old contents and all, to
// whichever handle asks next.
struct EvalFill {
    bool valid = false;
    int blocked = -1, PL = 0, chain = -1, model = -1;
    bool matches(int b, int pl, int c, int m) const { return valid && blocked == b && PL == pl && chain == c && model == m; }
    void set(int b, int pl, int c, int m) { valid = true; blocked = b; PL = pl; chain = c; model = m; }
};

struct Engine {
    // ---- problem -----------------------------------------------------------------------------
    int chain = 0, model = 0;
    int n_blocks = 0, n_cams = 0, n_views = 0;
    int64_t first_view_global = 0;
    int64_t n_obs = 0, ld = 0, ld_xy = 0;
    int64_t n_xy_unique_blocks = 0;
    int PI = 10, PL = 16, NACC = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    std::vector<int64_t> blk_offset;  // unpadded CSR (host)
    std::vector<int64_t> pad_offset;  // padded start of every block (host)
    std::vector<int64_t> xy_offset;   // start of every block's target points in the deduplicated X, Y arrays (host)
    std::vector<int32_t> blk_cam, blk_view;
    std::vector<int64_t> blk_tile_off;  // Mode B tiles per block CSR (host)
    int64_t n_tilesA = 0, n_tilesB = 0;
    int32_t max_tileB = 0;  // observations of the largest Mode B tile (small-block problems take the single-group kernel)

    // host copies of the parameters (current accepted state); h_cam / h_target are always sized
    // (7 per camera / 7) and simply unused by chains that have no such block
    std::vector<double> h_intr, h_cam, h_view, h_target;

    // ---- device ------------------------------------------------------------------------------
    DevBuf<double> X, Y, u, v, r, J;
    // A tile-blocked Mode A output above 4 GiB is held as SEGMENTS of whole tiles, each a physically contiguous block of at most
    // 4 GiB (capi.cpp alloc_output: such blocks stream at the rate the memory system was laid out for and cost a millisecond to
    // obtain; one contiguous block of 59 GB costs 1.7 s, a plain one runs 5-8 % slower).  k_eval is launched once per segment with
    // the segment's tile range and base address: the kernel is unchanged.  Empty when the output is one block (J).
    std::deque<DevBuf<double>> Jseg;
    EvalFill J_fill, Jf_fill;          // constant rows of J / Jf
    std::deque<EvalFill> Jseg_fill;    // ... of every segment (same length as Jseg)
    int64_t seg_tiles = 0;  // tiles per segment (the last one may hold fewer)
    double* eval_tile_ptr(int64_t w, int64_t tile_doubles) {  // device address of tile w's output
        return Jseg.empty() ? J.p + w * tile_doubles : Jseg[static_cast<size_t>(w / seg_tiles)].p + (w % seg_tiles) * tile_doubles;
    }
    // fp32 study (BASELINE config 5): rounded copies of the observations / constant tables, fp32 Mode A output
    int scalar = 0;  // 0 = fp64 per-observation arithmetic, 1 = fp32 (accumulators stay fp64)
    DevBuf<float> Xf, Yf, uf, vf, Jf, bcf, sdf, intrf;
    DevBuf<double> bc, sd, aux;  // aux: bundle b_T_g [n_blocks][12]
    // The SHARED parameter blocks of copy k live side by side in shared_pack[k] = [intr | cam poses | target pose | shared step]
    // (intr[k], cam[k], target[k], delta_sh are windows into it): a trial point goes up as ONE copy and is accepted by one
    // small kernel (lm_kernels.hpp k_accept).  Declared before its windows.
    DevBuf<double> shared_pack[2];
    size_t pk_cam = 0, pk_target = 0, pk_delta = 0, pk_size = 0;  // offsets (doubles) of the windows
    DevBuf<double> intr[2], cam[2], view[2], target[2];
    int eval_blocked = 1;  // Mode A output layout: 1 tile-blocked out[tile][2+2P-1][128] (default), 0 whole-array columns
    int eval_done = 0, eval_blocked_last = 0;
    int eval_ablate = 0;  // timing-only ablation of k_eval (CBA_EVAL_ABLATE; outputs are wrong when non-zero)
    int eval_variant = 1;  // k_eval variant: bit 0 = non-temporal stores, bits 1.. = log2(tiles per wave)
    int active = 0;  // parameter copy (0 current / 1 trial) the constants bc, sd were last built from
    const double* gate = nullptr;  // device flag the launches of block constants / Mode B check (0: do nothing); set by the LM driver
                                   // while it queues the head of a step ahead of the controller's decision, nullptr otherwise
    // >= 0: launch_normal_eq() also leaves the blocks' robust weights / |r|^2 (blk_w, blk_s) for this Huber parameter where one
    // of its kernels can take the work along; head_weights says whether the last call did (the caller skips k_weights then)
    double head_huber = -1.0;
    bool head_weights = false;
    DevBuf<int32_t> d_blk_cam, d_blk_view;
    DevBuf<Tile> tilesA, tilesB;
    DevBuf<int64_t> d_blk_tile_off;
    DevBuf<double> partial, blk_acc, blk_s, scalar_out;
    // reprojection diagnostics (residual_stats.hip): buffers of their own, never shared with the cost / LM path
    DevBuf<double> diag_part, diag_blk, diag_tot;   // per-tile rows [n_tilesB][4], per-block rows [n_blocks][4], totals [4]
    DevBuf<double> diag_fpart, diag_ru, diag_rv;    // the fetch form: tile rows and residuals of the requested block range
    DevBuf<uint8_t> diag_keep;
    DevBuf<double> cost_part; // [2 * ceil(n_blocks / 2048)] partial cost pairs (only above 4096 blocks)
    DevBuf<double> blk_mom;   // [n_blocks][MomLayout::N] Mode B moment rows of the two-pose chains (kernels_reproj.hip)
    int modeb_moments = 1;    // 0 = accumulate the 12 pose columns directly (CBA_MODEB_MOMENTS=0, for A/B comparison)
    int modeb_shared = 1;     // 1 = one workgroup per tile, the parts as its wavefronts, rows evaluated once and shared through LDS
                              // (kernels_modeb.hip); 0 = one launch per part, every part re-evaluates the rows (CBA_MODEB_SHARED)
    int modeb_split = -1;     // one-pose chain: 1 = pose rows | intrinsics block (mode_b.hpp SplitPoseIntr), 0 = round-robin halves,
                              // -1 = per camera model as measured (CBA_MODEB_SPLIT)

    // ---- LM / Schur state (backend_hip.hip, resident_lm.hip; the rest lives in HipLMState, lm_state.hpp) ----------
    DevBuf<double> blk_w;       // [n_blocks] Huber weights rho'(s_b)
    DevBuf<double> blk_acc_alt, blk_w_alt;  // the trial point's block sums / weights of a speculative LM step (backend_hip.hip sys_step)
    DevBuf<double> cam_acc;     // [n_cams][NACC] weighted per-camera sums
    DevBuf<double> view_L;      // [n_views][36] Cholesky factor of damped H_pp (lower, row-major)
    DevBuf<double> view_y;      // [n_views][6]
    DevBuf<double> view_D;      // [n_views][6]  damping added to diag(H_pp)
    DevBuf<double> view_gp;     // [n_views][6]  g_p
    DevBuf<double> view_scale2; // [n_views][6]  jacobi scale^2
    DevBuf<double> blk_Z;       // [n_blocks][6][PSH]
    DevBuf<int32_t> view_fixed; // [n_views]
    DevBuf<double> delta_sh;    // [nsh] shared step of the current trial

    // ---- collectives -------------------------------------------------------------------------
    cba_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    void* rccl_comm = nullptr;
    int n_ranks = 1, rank = 0;
    DevBuf<double> coll_buf;
    PinnedBuf<double> coll_pin;  // page-locked staging of the packed all-reduce buffer (both copies are queued, one sync)
    void* lm_state = nullptr;  // HipLMState (backend_hip.hip)

    ~Engine();
};

// kernels_reproj.hip
void ensure_f32_buffers(Engine& e);                      // fp32 copies of the observations + float tables
void launch_block_consts(Engine& e, int which);         // params[which] -> bc, sd
void launch_camera_consts(Engine& e, int which);        // ... the per-camera part alone (sd)
void launch_eval_fill(Engine& e);                       // Mode A: the constant Jacobian rows of the output buffers that lack them
void launch_eval(Engine& e);                            // Mode A: r, J at bc/sd (the live rows; needs launch_eval_fill before it)
void launch_resid(Engine& e);                           // Mode R: blk_s[b] = |r_b|^2
void warm_reproj_kernels();                              // forces the code object of kernels_reproj.hip to load
void launch_normal_eq(Engine& e);                       // Mode B: blk_acc[b] = [H | g | s]
bool launch_normal_eq_shared_rows(Engine& e, double* rows);  // kernels_modeb.hip: the parts of a tile as one workgroup, rows through LDS
void launch_cost(Engine& e, double huber_delta, double* out = nullptr);  // out (default scalar_out) = {1/2 sum rho(blk_s), sum blk_s}

// residual_stats.hip: raw residual statistics (t2: the largest e2 that counts as kept).  blk_stats [n_blocks][4] / total [4] host,
// either may be null: {sum e2, max sqrt(e2), #not kept, #obs}.  The fetch form: r [2n] interleaved and keep [n] of blocks [b0, b1)
void residual_stats_launch(Engine& e, double t2);  // device only: diag_blk, diag_tot
void residual_stats(Engine& e, double t2, double* blk_stats, double* total);
void residuals_fetch_range(Engine& e, int b0, int b1, double t2, double* r, uint8_t* keep);

// backend_hip.hip
void init_lm_state(Engine& e, const cba_reproj_problem& d, bool have_records = false);
void destroy_lm_state(Engine& e);
void warm_lm(Engine& e);
void solve_lm(Engine& e, const cba_options& o, cba_summary* out);
void solve_stats(const Engine& e, int64_t stats8[8]);  // ExchangeStats of the last host-driven solve
void set_lm_mode(Engine& e, int mode);  // 0 host-driven iteration, 1 automatic (default), 2 resident kernel whenever it can run the problem
void compute_covariance(Engine& e, const cba_options& o, double* cov, bool shared_only = false);
void compute_covariance_views(Engine& e, const cba_options& o, const int32_t* views, int n_sel, double* view_cov);
int64_t covariance_dim(const Engine& e);
int64_t shared_covariance_dim(const Engine& e);
// collectives.cpp
void engine_allreduce(Engine& e, double* host_buf, int64_t count);
void rccl_unique_id(uint8_t* id);
void rccl_init(Engine& e, const uint8_t* id, int n_ranks, int rank);
void rccl_destroy(Engine& e);
void rccl_abort(Engine& e);  // ncclCommAbort: this rank leaves a multi-rank solve abnormally; the peers' collectives fail instead of hanging

}  // namespace cba
