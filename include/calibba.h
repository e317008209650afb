/* calibba.h — C ABI of libcalibba.so, the MI355X (gfx950) bundle-adjustment engine that
 * drops in behind VitalyVorobyev/calibration's `calib::estimation_optim` refinement API.
 *
 * Plain C: pointers, sizes, POD structs.  No C++/Eigen/torch types cross this boundary.
 * All floating-point data is IEEE fp64; all matrices row-major unless stated.
 * Every entry point returns a cba_status; cba_last_error() gives the message a C++ adapter
 * re-throws (std::invalid_argument for CBA_ERR_INVALID_ARGUMENT, std::runtime_error for
 * CBA_ERR_RUNTIME — the exception types of the reference, SURVEY.md §8b "Errors").
 *
 * Reference interface each group replaces (paths relative to the reference repo):
 *   cba_options                 include/calib/estimation/optim/optimize.h:24-33 (OptimOptions)
 *                               + intrinsics.h:13-20, extrinsics.h:22-27, bundle.h:30-36
 *   cba_summary                 include/calib/estimation/optim/optimize.h:35-40 (OptimResult)
 *   cba_optimize_intrinsics     include/calib/estimation/optim/intrinsics.h:35-39
 *                               (src/estimation/optim/intrinsics.cpp:98-120)
 *   cba_optimize_extrinsics     include/calib/estimation/optim/extrinsics.h:29-34
 *                               (src/estimation/optim/extrinsics.cpp:174-196)
 *   cba_optimize_bundle         include/calib/estimation/optim/bundle.h:58-63
 *                               (src/estimation/optim/bundle.cpp:147-170)
 *   cba_optimize_handeye        include/calib/estimation/optim/handeye.h:40-43
 *                               (src/estimation/optim/handeye.cpp:60-78)
 *   cba_optimize_planar_pose    include/calib/estimation/optim/planarpose.h:24-26
 *                               (src/estimation/optim/planarpose.cpp:84-127)
 *   cba_optimize_intrinsics_semidlt  include/calib/estimation/optim/intrinsics.h (optimize_intrinsics_semidlt)
 *                               (src/estimation/optim/intrinsicssemidlt.cpp:155-191)
 *   cba_optimize_homography     include/calib/estimation/optim/homography.h:17-18
 *                               (src/estimation/optim/homography.cpp:144-175)
 *   cba_estimate_extrinsic_dlt  include/calib/estimation/linear/extrinsics.h:27-78
 *   cba_estimate_bundle_seed    src/pipeline/detail/bundle_utils.cpp:46-237 (+ estimate_handeye_dlt)
 *   cba_reproj_* (handle API)   the ceres::Problem the reference builds and solves inside those
 *                               functions (intrinsics.cpp:63-90, extrinsics.cpp:86-160,
 *                               bundle.cpp:83-133, detail/ceresutils.h:27-43,69-126); exposed so
 *                               observations can stay resident in HBM across solves and so the
 *                               residual+Jacobian evaluation (ceres::CostFunction::Evaluate of
 *                               residuals/intrinsicresidual.h:20-35, extrinsicsresidual.h:28-46,
 *                               bundleresidual.h:36-56) can be called and timed on its own.
 *
 * Pose convention: a rigid transform is 7 doubles [qw, qx, qy, qz, tx, ty, tz] — exactly the
 * parameter blocks the reference hands to Ceres (observationutils.h:43-48 populate_quat_tran;
 * quaternion storage w,x,y,z, observationutils.h:20-24).  Results come back un-normalised, as in
 * the reference's blocks; the caller applies restore_pose (observationutils.h:50-62).
 * cba_pose_from_matrix / cba_pose_to_matrix restate those two helpers for hosts without Eigen.
 *
 * Camera parameter vectors follow CameraTraits (include/calib/models/pinhole.h:117-133,
 * scheimpflug.h:234-261):
 *   CBA_CAMERA_PINHOLE_BC   10: [fx, fy, cx, cy, skew, k1, k2, k3, p1, p2]
 *   CBA_CAMERA_SCHEIMPFLUG  12: the above + [tau_x, tau_y]
 *
 * Threading: entry points are re-entrant; one handle must not be used from two threads at once.
 */
#ifndef CALIBBA_H
#define CALIBBA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBA_VERSION_STRING "0.1.0"

typedef enum cba_status {
    CBA_OK = 0,
    CBA_ERR_INVALID_ARGUMENT = 1, /* reference throws std::invalid_argument */
    CBA_ERR_RUNTIME = 2,          /* reference throws std::runtime_error */
    CBA_ERR_NO_DEVICE = 3,        /* no usable gfx950 device: the engine has NO CPU fallback */
    CBA_ERR_HIP = 4,              /* HIP / RCCL runtime error */
    CBA_ERR_INTERNAL = 5
} cba_status;

typedef enum cba_chain {
    CBA_CHAIN_INTRINSIC = 0, /* c_T_t = view pose                       (intrinsicresidual.h) */
    CBA_CHAIN_EXTRINSIC = 1, /* c_T_t = c_T_r * r_T_t                   (extrinsicsresidual.h) */
    CBA_CHAIN_BUNDLE = 2     /* c_T_t = g_T_c^-1 * b_T_g^-1 * b_T_t     (bundleresidual.h) */
} cba_chain;

typedef enum cba_camera_model { CBA_CAMERA_PINHOLE_BC = 0, CBA_CAMERA_SCHEIMPFLUG = 1 } cba_camera_model;

typedef enum cba_termination {
    CBA_TERM_CONVERGENCE = 0,    /* ceres::CONVERGENCE  -> success = true (ceresutils.h:42) */
    CBA_TERM_NO_CONVERGENCE = 1, /* max_iterations hit  -> success = false */
    CBA_TERM_FAILURE = 2
} cba_termination;

/* OptimOptions + the per-stage switches.  cba_options_default() gives the reference defaults. */
typedef struct cba_options {
    int32_t optimizer;            /* OptimizerType 0..3; accepted, ignored (one Schur solver) */
    int32_t max_iterations;       /* 1000 */
    double huber_delta;           /* 1.0; <= 0 disables the loss (intrinsics.cpp:70-71) */
    double epsilon;               /* 1e-9: function, gradient and parameter tolerance */
    int32_t compute_covariance;   /* 1 */
    int32_t verbose;              /* 0 */
    int32_t optimize_intrinsics;  /* ExtrinsicOptions (default 1) / BundleOptions (default 0);
                                     ignored (always on) for the intrinsic chain */
    int32_t optimize_skew;        /* 0 */
    int32_t optimize_extrinsics;  /* ExtrinsicOptions::optimize_extrinsics (1) /
                                     BundleOptions::optimize_hand_eye (1) */
    int32_t optimize_target_pose; /* BundleOptions::optimize_target_pose (1) */
} cba_options;

/* OptimResult.  `covariance` is fetched separately (cba_reproj_covariance). */
typedef struct cba_summary {
    int32_t success;     /* termination == CONVERGENCE */
    int32_t termination; /* cba_termination */
    int32_t iterations;
    int32_t successful_steps;
    double initial_cost;
    double final_cost; /* 1/2 sum_blocks rho(|r_block|^2), as ceres::Solver::Summary */
    double solve_seconds;
    char report[192]; /* brief report string (engine's own wording) */
} cba_summary;

/* One reprojection bundle problem.  A "residual block" is one planar view seen by one camera,
 * exactly one ceres residual block of the reference (2*N residuals, one loss per block).
 *
 *   chain INTRINSIC: n_cams = 1; block b has private pose view_pose[blk_view[b]] (c_T_t)
 *   chain EXTRINSIC: cam_pose[c] = c_T_r, view_pose[v] = r_T_t; block b = (view blk_view[b], cam blk_cam[b])
 *   chain BUNDLE:    cam_pose[c] = g_T_c, target_pose = b_T_t, blk_b_T_g[b] = robot pose (data);
 *                    n_views = 0
 * Observations are SoA over all blocks, CSR-indexed by blk_offset.
 */
typedef struct cba_reproj_problem {
    int32_t chain;        /* cba_chain */
    int32_t camera_model; /* cba_camera_model */
    int32_t n_blocks;
    int32_t n_cams;
    int32_t n_views;
    int32_t reserved0;
    int64_t first_view_global; /* index of local view 0 in the whole (multi-GPU) problem; the
                                  gauge rule "first target pose constant" (extrinsics.cpp:123-126)
                                  applies to global view 0 */
    const int64_t* blk_offset; /* [n_blocks + 1] */
    const int32_t* blk_cam;    /* [n_blocks] */
    const int32_t* blk_view;   /* [n_blocks]; ignored for BUNDLE */
    const double* blk_b_T_g;   /* BUNDLE: [n_blocks][12] = rotation row-major (9) + translation (3) */
    const double* X;           /* [n_obs] target-plane x  (PlanarObservation::object_xy) */
    const double* Y;           /* [n_obs] target-plane y */
    const double* u;           /* [n_obs] pixel u         (PlanarObservation::image_uv) */
    const double* v;           /* [n_obs] pixel v */
    double* intr;              /* [n_cams][10|12]  in/out */
    double* cam_pose;          /* [n_cams][7]      in/out (NULL for INTRINSIC) */
    double* view_pose;         /* [n_views][7]     in/out (NULL for BUNDLE) */
    double* target_pose;       /* [7]              in/out (BUNDLE only) */
} cba_reproj_problem;

typedef struct cba_reproj cba_reproj; /* opaque: owns device buffers + one HIP stream */

/* ---- library ------------------------------------------------------------------------------ */
const char* cba_version(void);
const char* cba_last_error(void); /* thread-local, valid until the next call on this thread */
int32_t cba_device_count(void);   /* number of visible HIP devices (0 if none) */
/* Handles and the one-shot calls return their device / page-locked blocks (up to 16 MiB each, 256 MiB per kind and device) and
 * their stream to a process-wide cache instead of the runtime: a pipeline that calls optimize_* stage after stage pays for the
 * allocations once (releasing them was 1.9 ms of a 5 ms call at the reference's test sizes).  This frees what the cache holds. */
void cba_trim_cache(void);
/* The device used by every entry point that takes neither a handle nor a device argument (the one-shot cba_optimize_* calls, the
 * batched per-view solvers and seeds).  Default 0.  With one process per GPU call cba_set_device(LOCAL_RANK) once: the batched
 * solvers have no exchange step, so several GPUs simply take slices of the views. */
cba_status cba_set_device(int32_t device);
int32_t cba_get_device(void);
void cba_options_default(cba_options* o);
int32_t cba_intrinsics_size(int32_t camera_model); /* 10 or 12 */
int32_t cba_local_columns(int32_t chain, int32_t camera_model); /* tangent columns per observation:
                                     INTRINSIC 6+P, otherwise 12+P  [poseA d(3) t(3) | poseB d(3) t(3) | intr] */

/* populate_quat_tran / restore_pose (observationutils.h:43-62) for 4x4 column-major matrices
 * (the memory layout of Eigen::Isometry3d::data()). */
void cba_pose_from_matrix(const double* m44_colmajor, double* pose7);
void cba_pose_to_matrix(const double* pose7, double* m44_colmajor);

/* ---- handle API --------------------------------------------------------------------------- */
/* Validates like the reference (empty block -> INVALID_ARGUMENT "No observations provided",
 * bad indices -> INVALID_ARGUMENT), copies observations into padded SoA device arrays and the
 * parameters into device blocks.  Host buffers may be freed after this returns. */
cba_status cba_reproj_create(const cba_reproj_problem* desc, int32_t device, cba_reproj** out);
/* The same from array-of-structures input, read in place: blk_obs[b] points to block b's observations as interleaved
 * {object_x, object_y, image_u, image_v} records (32 bytes each) — exactly the memory of the reference's
 * std::vector<PlanarObservation> (include/calib/estimation/linear/planarpose.h:22-26: two Eigen::Vector2d), so a binding
 * passes view.data() and never builds X / Y / u / v arrays (desc->X, Y, u, v are ignored and may be NULL; desc->blk_offset
 * still gives the record counts).  SURVEY.md §8(f) rank 4: at 1.6e8 observations the caller-side AoS -> SoA copy alone is
 * 5 GB read + 5 GB written. */
cba_status cba_reproj_create_aos(const cba_reproj_problem* desc, const double* const* blk_obs, int32_t device, cba_reproj** out);
void cba_reproj_destroy(cba_reproj* h);
cba_status cba_reproj_set_params(cba_reproj* h, const double* intr, const double* cam_pose,
                                 const double* view_pose, const double* target_pose);
cba_status cba_reproj_get_params(cba_reproj* h, double* intr, double* cam_pose, double* view_pose,
                                 double* target_pose);
int64_t cba_reproj_num_observations(const cba_reproj* h);

/* Residual + tangent-space Jacobian of every observation at the current parameters ("Mode A").
 * Output stays in HBM as SoA (r: [2][n_pad], J: [2*P][n_pad]); cba_reproj_eval_fetch copies it
 * out in Ceres layout: r[2*n_obs] interleaved (u0,v0,u1,v1,..) per block, J row-major
 * [2*n_obs][P] with the local column order of cba_local_columns().  Quaternion columns are in
 * the tangent space of ceres::QuaternionManifold (ambient 2Nx4 Jacobian times PlusJacobian). */
cba_status cba_reproj_eval(cba_reproj* h);
cba_status cba_reproj_eval_fetch(cba_reproj* h, double* r, double* J);
/* The same for the residual blocks [b0, b1) only: r [2 * n], J [2 * n][P] with n = observations of those blocks, indexed from
 * the first observation of block b0.  For problems whose full Mode A output (59 GB at BASELINE config 3) must not cross PCIe. */
cba_status cba_reproj_eval_fetch_blocks(cba_reproj* h, int32_t b0, int32_t b1, double* r, double* J);
/* Runs `iters` back-to-back evaluations on the handle's stream bracketed by HIP events;
 * returns the average milliseconds per evaluation of the dominant kernel region. */
cba_status cba_reproj_eval_timed(cba_reproj* h, int32_t warmup, int32_t iters, double* ms_per_eval);

/* The same for one Mode B pass (all launches that produce the per-block normal equations of a linearisation). */
cba_status cba_reproj_normal_eq_timed(cba_reproj* h, int32_t warmup, int32_t iters, double* ms_per_pass);

/* Arithmetic type of the per-observation kernels (BASELINE config 5's fp32-vs-fp64 study): 0 = fp64
 * (default), 1 = fp32: observations and per-block constants are rounded to fp32 once, the residual and
 * Jacobian rows are evaluated in fp32, and EVERY accumulator (J^T J, J^T r, |r|^2), the Schur step and the
 * LM stay fp64.  Affects cba_reproj_eval / _eval_timed / _cost / _block_normal_eq / _solve / _covariance.
 * With fp32 the Mode A output is float: fetch it with cba_reproj_eval_fetch_f32 (same layout as
 * cba_reproj_eval_fetch). */
cba_status cba_reproj_set_scalar(cba_reproj* h, int32_t scalar);
cba_status cba_reproj_eval_fetch_f32(cba_reproj* h, float* r, float* J);

/* Cost 1/2 sum rho(|r_b|^2) at the current parameters (residual-only pass). */
cba_status cba_reproj_cost(cba_reproj* h, double huber_delta, double* cost);

/* Reprojection diagnostics at the handle's current parameters: raw residuals r = projection - observation (no loss, no
 * weights), one residual-only pass that leaves Mode A output, LM state and the cost buffers untouched.
 * e2 = r_u^2 + r_v^2 (fp64, no FMA).  blk_stats[b] = {sum e2, max sqrt(e2) (px), #not kept, #observations};
 * total[4] = the same over the handle's blocks.  Either pointer may be NULL.  Multi-rank handles: this rank's blocks, no
 * exchange.  threshold_px: >= 0 or +inf; NaN / negative -> CBA_ERR_INVALID_ARGUMENT.
 * An observation is kept exactly when sqrt(e2) <= threshold_px (correctly rounded square root), so a threshold equal to an
 * observation's own error keeps it; a NaN residual is never kept and counts as over the threshold; the maximum ignores NaN.
 * Sums run in a fixed order (tiles, then blocks): two calls give the same bits. */
cba_status cba_reproj_residual_stats(cba_reproj* h, double threshold_px, double* blk_stats, double* total);
/* Residuals and inlier flags of residual blocks [b0, b1): r[2n] interleaved as cba_reproj_eval_fetch_blocks,
 * keep[n] = (sqrt(e2) <= threshold_px) (0 for NaN).  Either pointer may be NULL.  Needs no prior cba_reproj_eval.
 * Device buffers are sized to the range.  Bad block ranges -> CBA_ERR_INVALID_ARGUMENT. */
cba_status cba_reproj_residuals_fetch_blocks(cba_reproj* h, int32_t b0, int32_t b1, double threshold_px, double* r,
                                             uint8_t* keep);
/* Device time (HIP events) of `iters` diagnostics passes over the whole handle after one untimed call, ms[iters]:
 * fetch = 0 the statistics form, 1 the fetch form's kernel (residuals and flags of every block written on the device). */
cba_status cba_reproj_residual_stats_timed(cba_reproj* h, int32_t fetch, int32_t iters, double* ms);

/* Per-block normal-equation blocks at the current parameters ("Mode B", unweighted):
 * out[b] = [ upper triangle of J_b^T J_b row-major (P(P+1)/2) | J_b^T r_b (P) | |r_b|^2 (1) ]. */
cba_status cba_reproj_block_normal_eq(cba_reproj* h, double* out);
int64_t cba_reproj_block_normal_eq_size(const cba_reproj* h); /* doubles per block */

/* Levenberg-Marquardt solve (what solve_problem + ceres::Solve do, ceresutils.h:27-43). */
cba_status cba_reproj_solve(cba_reproj* h, const cba_options* opts, cba_summary* summary);

/* How cba_reproj_solve runs the iteration.  0: stage by stage (every stage a kernel launch on the handle's stream; the only form
 * for multi-rank handles, verbose solves and the fp32 study).  The reduced system, the step decision, the radius update and the
 * next trial point of the shared blocks are the work of ONE single-workgroup controller kernel right behind the packed exchange
 * (csrc/lm_ctl.hip): the host queues launch sequences and reads a control record, it takes no part in the arithmetic.
 * 2: "resident" - the whole solve in ONE launch of a single-workgroup kernel, for problems too small to fill the chip (the
 * sizes the reference's own tests and pipelines run); falls back to 0 when the kernel cannot take the problem (reduced system
 * wider than 80, > 16 cameras, a transport set).  1 (default): resident below the measured crossover with the staged form
 * (intrinsic chain: n_views + 0.0105 n_obs <= 28, e.g. 10 views x 88 points; 20 x 88 is already faster staged), staged otherwise.
 * 3 (diagnostic, for A/B measurements): as 0, but the reduced solve and the step decision run on the host from a copy of the
 * reduced pack, as they did before the controller existed.
 * All forms follow the same rules, take the same decisions and agree to rounding. */
cba_status cba_reproj_set_lm_mode(cba_reproj* h, int32_t mode);

/* What the last host-driven cba_reproj_solve on this handle exchanged between ranks (one packed
 * sum-all-reduce per linear solve).  A trial point is linearised ahead of the accept decision, so an accepted step whose
 * gain ratio is >= 0.937 (Ceres then grows the radius by its maximum factor 3, which is the radius the elimination was
 * made with) costs exactly ONE collective; stats8 = {all-reduce calls, all-reduced doubles, speculative steps,
 * of those accepted with the predicted radius, accepted with another radius (+1 re-elimination and collective),
 * rejected steps, trust-region steps that went through the projected Armijo line search of bounds-constrained problems,
 * line-search evaluations (one collective each)}.  All zero after a resident-kernel solve.  CBA_LM_SPECULATE=0 selects the
 * two-exchange sequence, CBA_LM_LINE_SEARCH=0 switches the line search off. */
cba_status cba_reproj_solve_stats(const cba_reproj* h, int64_t stats8[8]);

/* Covariance in the reference's layout (ceresutils.h:69-126): dense symmetric, AMBIENT block
 * sizes, block order = get_param_blocks() of the stage (intrinsics.cpp:34-50,
 * extrinsics.cpp:50-67, bundle.cpp:48-68).  Returns CBA_ERR_RUNTIME if rank deficient (the
 * reference then leaves the matrix empty). */
int64_t cba_reproj_covariance_dim(const cba_reproj* h);
cba_status cba_reproj_covariance(cba_reproj* h, const cba_options* opts, double* cov /*[dim*dim]*/);

/* The same matrix restricted to the SHARED blocks — [intr[c]..., camera quats, camera trans] (for BUNDLE: every block) — i.e.
 * the marginal covariance of everything but the per-view poses, from the Schur-reduced system: O(#views) work and a
 * (shared dim)^2 result where the all-block-pairs matrix of ceresutils.h:80-84 is O(#views^2) (393 MB at 1000 views, 6.3 GB
 * at 4000).  Equal to the corresponding rows/columns of cba_reproj_covariance. */
int64_t cba_reproj_covariance_shared_dim(const cba_reproj* h);
cba_status cba_reproj_covariance_shared(cba_reproj* h, const cba_options* opts, double* cov /*[dim*dim]*/);
/* ... and the per-view blocks on demand: the marginal covariance of the poses of the listed views
 * (indices local to this handle), cov7x7 [n_sel][7][7] in ambient coordinates [quaternion (4), translation (3)] - the diagonal
 * blocks cba_reproj_covariance holds for those views, from the same Schur pieces, O(#views + n_sel) work instead of
 * O(#views^2); zeros for a view the gauge holds constant.  Same rank test as cba_reproj_covariance_shared.
 * INTRINSIC / EXTRINSIC chains (the bundle chain has no per-view poses).  ceresutils.h:69-126. */
cba_status cba_reproj_covariance_views(cba_reproj* h, const cba_options* opts, int32_t n_sel, const int32_t* view_idx,
                                       double* cov7x7);

/* ---- multi-GPU: views sharded across ranks, one sum-all-reduce per LM linear solve ---------- */
/* Host-buffer callback (any transport: gloo, MPI, ...): in-place sum of buf[count] over ranks. */
typedef int32_t (*cba_allreduce_fn)(double* buf, int64_t count, void* user);
cba_status cba_reproj_set_allreduce(cba_reproj* h, cba_allreduce_fn fn, void* user, int32_t n_ranks, int32_t rank);
/* RCCL-native: device-buffer ncclAllReduce on the handle's stream (xGMI within a node). */
#define CBA_RCCL_UNIQUE_ID_BYTES 128
cba_status cba_rccl_unique_id(uint8_t id[CBA_RCCL_UNIQUE_ID_BYTES]);
cba_status cba_reproj_init_rccl(cba_reproj* h, const uint8_t id[CBA_RCCL_UNIQUE_ID_BYTES],
                                int32_t n_ranks, int32_t rank);

/* ---- one-shot entry points mirroring the reference's free functions ------------------------- */
/* optimize_intrinsics: >= 4 views else INVALID_ARGUMENT (intrinsics.cpp:92-96).
 * cov may be NULL; otherwise [(P + 7*n_views)^2], order [intr, quats..., trans...]. */
cba_status cba_optimize_intrinsics(int32_t camera_model, int32_t n_views, const int64_t* view_offset,
                                   const double* X, const double* Y, const double* u, const double* v,
                                   double* intr, double* c_T_t /*[n_views][7]*/, const cba_options* opts,
                                   cba_summary* summary, double* cov);
/* optimize_extrinsics: views[v][c] = block; empty (view,cam) pairs are simply absent.
 * cov order: [intr[c]..., cam quats..., cam trans..., view quats..., view trans...]. */
cba_status cba_optimize_extrinsics(int32_t camera_model, int32_t n_cams, int32_t n_views, int32_t n_blocks,
                                   const int64_t* blk_offset, const int32_t* blk_view, const int32_t* blk_cam,
                                   const double* X, const double* Y, const double* u, const double* v,
                                   double* intr, double* c_T_r, double* r_T_t, const cba_options* opts,
                                   cba_summary* summary, double* cov);
/* optimize_bundle: n_cams == 0 / n_blocks == 0 -> INVALID_ARGUMENT (bundle.cpp:139-144).
 * cov order: [intr[c]..., g quats..., g trans..., b quat, b tran]. */
cba_status cba_optimize_bundle(int32_t camera_model, int32_t n_cams, int32_t n_blocks,
                               const int64_t* blk_offset, const int32_t* blk_cam, const double* blk_b_T_g,
                               const double* X, const double* Y, const double* u, const double* v,
                               double* intr, double* g_T_c, double* b_T_t, const cba_options* opts,
                               cba_summary* summary, double* cov);
/* optimize_handeye: AX = XB refinement over all motion pairs (handeye.cpp:60-78; pairs per
 * src/estimation/linear/handeyedlt.cpp:51-81 with min angle 0.5 deg).  Poses are 7-vectors.
 * RUNTIME error for < 2 poses / size mismatch / no valid pairs.  cov: [7*7] or NULL. */
cba_status cba_optimize_handeye(int32_t n_poses, const double* base_T_gripper, const double* cam_T_target,
                                double* g_T_c /*[7] in/out*/, const cba_options* opts, cba_summary* summary,
                                double* cov);

/* estimate_handeye_dlt (include/calib/estimation/linear/handeye.h, src/estimation/linear/handeyedlt.cpp:126-137): the all-pairs
 * Tsai-Lenz seed — rotation from sum skew(alpha+beta) x = beta - alpha, translation from sum (R_A - I) t = R_X t_B - t_A, both
 * ridge 1e-12 — over the pairs that pass the filter at min_angle_deg (:25-49).  O(n^2) pairs are enumerated on the device.
 * g_T_c [7] out.  RUNTIME error for < 2 poses / no valid pairs.
 * estimate_and_optimize_handeye (include/calib/estimation/optim/handeye.h:64-67, handeye.cpp:80-87): that seed, then
 * cba_optimize_handeye. */
cba_status cba_estimate_handeye_dlt(int32_t n_poses, const double* base_T_gripper, const double* cam_T_target,
                                    double min_angle_deg, double* g_T_c /*[7] out*/);
cba_status cba_estimate_and_optimize_handeye(int32_t n_poses, const double* base_T_gripper, const double* cam_T_target,
                                             double min_angle_deg /*reference default 1.0*/, double* g_T_c /*[7] out*/,
                                             const cba_options* opts, cba_summary* summary, double* cov);

/* The same two steps on several GPUs (AX = XB row): every rank passes ALL n poses; rank r evaluates the pairs
 * (i, j > i) whose first pose i lies in its range (ranges balanced by pair count) and the 29 accumulated values
 * [H | g | cost | #pairs] of every evaluation are summed over ranks through `fn` (the callback of cba_reproj_set_allreduce), so
 * every rank runs the same LM on the same sums.  estimate != 0: start from the all-pairs Tsai-Lenz seed (g_T_c out), else refine
 * g_T_c in place.  `device`: this rank's GPU. */
cba_status cba_estimate_and_optimize_handeye_sharded(int32_t n_poses, const double* base_T_gripper, const double* cam_T_target,
                                                     double min_angle_deg, int32_t estimate, double* g_T_c,
                                                     const cba_options* opts, cba_summary* summary, double* cov,
                                                     cba_allreduce_fn fn, void* user, int32_t n_ranks, int32_t rank, int32_t device);

/* ... and with RCCL over xGMI as the transport (BASELINE configs[3]: "8 MI355X"): `id` is the 128-byte unique id of
 * cba_rccl_unique_id(), created by one rank and handed to all of them by the caller; every rank calls this entry point (it is a
 * collective: the communicator is created inside, over the ranks' devices, and torn down at the end).  The 29 sums of every
 * evaluation are reduced IN PLACE in device memory on the evaluation's stream (ncclAllReduce), then copied back once.  A rank
 * that fails aborts the communicator so that its peers fail too instead of waiting. */
cba_status cba_estimate_and_optimize_handeye_rccl(int32_t n_poses, const double* base_T_gripper, const double* cam_T_target,
                                                  double min_angle_deg, int32_t estimate, double* g_T_c,
                                                  const cba_options* opts, cba_summary* summary, double* cov,
                                                  const uint8_t id[CBA_RCCL_UNIQUE_ID_BYTES], int32_t n_ranks, int32_t rank,
                                                  int32_t device);

/* optimize_planar_pose (include/calib/estimation/optim/planarpose.h:24-26, src/estimation/optim/planarpose.cpp:84-127):
 * pose refinement of ONE planar view for fixed K = [fx, fy, cx, cy, skew] by variable projection over the
 * Brown-Conrady coefficients (num_radial radial + 2 tangential, PlanarPoseOptions::num_radial default 2).
 * pose7 in/out; distortion [num_radial + 2] = fitted coefficients; reprojection_error = sqrt(ssr / 2N);
 * cov36 = 6x6 covariance of [angle-axis, t] scaled by ssr / max(1, 2N - 6) (zeros if rank deficient), may be NULL.
 * Fewer than 8 observations: the reference's functor fails to evaluate and Ceres reports FAILURE
 * (success = false), not an exception; same here.
 * The _batch form solves n_views independent views in one launch (one GPU thread per view); arrays are
 * per view: pose7 [n_views][7], summaries [n_views], distortion [n_views][num_radial + 2], etc. */
cba_status cba_optimize_planar_pose(int32_t n, const double* X, const double* Y, const double* u, const double* v,
                                    const double* kmtx5, int32_t num_radial, double* pose7, const cba_options* opts,
                                    cba_summary* summary, double* distortion, double* reprojection_error, double* cov36);
cba_status cba_optimize_planar_pose_batch(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y,
                                          const double* u, const double* v, const double* kmtx5, int32_t num_radial,
                                          double* pose7, const cba_options* opts, cba_summary* summaries, double* distortion,
                                          double* reprojection_error, double* cov36);

/* optimize_homography (include/calib/estimation/optim/homography.h:17-18, src/estimation/optim/homography.cpp:144-175):
 * refinement of the 8 free entries of a plane-to-image homography (H22 = 1), one 2-residual block PER
 * CORRESPONDENCE, each with its own Huber loss (homography.cpp:132-142).  h9 in/out, row-major 3x3: the first 8
 * entries are taken as given (HomographyBlocks::create :79-84), H22 comes back as 1.  Fewer than 4 correspondences:
 * INVALID_ARGUMENT (:146-148).  cov64 = 8x8 covariance scaled by ssr / max(1, 2N - 8), ssr from the loss-corrected
 * residuals (:163-173 evaluate the ceres::Problem with its default EvaluateOptions); zeros if rank deficient; may be
 * NULL.  The _batch form refines n_views independent views in one launch (one wavefront per view). */
cba_status cba_optimize_homography(int32_t n, const double* X, const double* Y, const double* u, const double* v,
                                   double* h9, const cba_options* opts, cba_summary* summary, double* cov64);
cba_status cba_optimize_homography_batch(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y,
                                         const double* u, const double* v, double* h9 /*[n_views][9]*/,
                                         const cba_options* opts, cba_summary* summaries, double* cov64 /*[n_views][64]*/);

/* optimize_intrinsics_semidlt (include/calib/estimation/optim/intrinsics.h, src/estimation/optim/intrinsicssemidlt.cpp:155-191):
 * refinement of K = [fx, fy, cx, cy, skew] and one pose per view with the Brown-Conrady coefficients of ALL views
 * eliminated by linear least squares inside the cost (CalibVPResidual, residuals/intrinsicsemidltresidual.h:19-73): one
 * residual block, one Huber loss, QuaternionManifold per view, skew held by a SubsetManifold unless opts->optimize_skew,
 * optional box bounds on K (CalibrationBounds; both pointers NULL = none).
 * kmtx5 in/out; c_T_t [n_views][7] in/out — the reference seeds these inside the call with calib::estimate_planar_pose
 * (host code of calib::estimation_linear, intrinsicssemidlt.cpp:37-40); the adapter calls it and passes the result.
 * After the solve the coefficients are re-fitted with the listed entries held fixed (solve_full :74-90, distortion.h:296-363):
 * distortion [num_radial + 2] = [k1.., p1, p2]; view_errors [n_views] = per-view RMS (:137-153);
 * cov [(5 + 7 n_views)^2], block order [K, all quaternions, all translations], scaled by ssr / max(1, 2N - (5 + 7 n_views))
 * (:184-188), zeros if rank deficient; may be NULL.  Fewer than 4 views: CBA_OK with summary->success = 0 and nothing written
 * (the reference prints a message and returns a default result, :163-166). */
cba_status cba_optimize_intrinsics_semidlt(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y,
                                           const double* u, const double* v, double* kmtx5, double* c_T_t, int32_t num_radial,
                                           const double* bounds_lo5, const double* bounds_hi5, const int32_t* fixed_distortion_indices,
                                           const double* fixed_distortion_values, int32_t n_fixed, const cba_options* opts,
                                           cba_summary* summary, double* distortion, double* view_errors, double* cov);

/* The same refinement with the VIEWS sharded over ranks (one process per GPU; BASELINE configs[3] names 8): this rank passes the
 * observations of views [first_view, first_view + n_views_local) of n_views_total (view_offset [n_views_local + 1] into its own
 * X, Y, u, v) and the seeds of the whole problem (kmtx5, c_T_t [n_views_total][7], identical on every rank).  The
 * O(#observations) passes run on the local views; per evaluation the ranks exchange the m(m+1)/2 + m sums that determine the
 * eliminated distortion coefficients and the table of per-view sums (78 + 22 m doubles per view, every rank filling its own rows),
 * after which the O(#views) step of the solver runs identically on every rank.  Outputs cover the whole problem and are identical
 * on every rank: kmtx5, c_T_t, distortion, view_errors [n_views_total], cov [(5 + 7 n_views_total)^2].  Agrees with the
 * single-GPU call to rounding (the sums are added in another order).  Transport: the host callback of cba_reproj_set_allreduce
 * (_sharded), or RCCL on device memory with the id from cba_rccl_unique_id on rank 0 (_rccl: a communicator is created for the
 * call; a rank that fails aborts it so that its peers' collectives fail instead of hanging).
 * src/estimation/optim/intrinsicssemidlt.cpp:155-191. */
cba_status cba_optimize_intrinsics_semidlt_sharded(int32_t n_views_local, const int64_t* view_offset, const double* X, const double* Y,
                                                   const double* u, const double* v, int32_t n_views_total, int32_t first_view,
                                                   double* kmtx5, double* c_T_t, int32_t num_radial, const double* bounds_lo5,
                                                   const double* bounds_hi5, const int32_t* fixed_distortion_indices,
                                                   const double* fixed_distortion_values, int32_t n_fixed, const cba_options* opts,
                                                   cba_summary* summary, double* distortion, double* view_errors, double* cov,
                                                   cba_allreduce_fn fn, void* user, int32_t n_ranks, int32_t rank, int32_t device);
cba_status cba_optimize_intrinsics_semidlt_rccl(int32_t n_views_local, const int64_t* view_offset, const double* X, const double* Y,
                                                const double* u, const double* v, int32_t n_views_total, int32_t first_view,
                                                double* kmtx5, double* c_T_t, int32_t num_radial, const double* bounds_lo5,
                                                const double* bounds_hi5, const int32_t* fixed_distortion_indices,
                                                const double* fixed_distortion_values, int32_t n_fixed, const cba_options* opts,
                                                cba_summary* summary, double* distortion, double* view_errors, double* cov,
                                                const uint8_t id[CBA_RCCL_UNIQUE_ID_BYTES], int32_t n_ranks, int32_t rank, int32_t device);

/* estimate_homography, DLT path (include/calib/estimation/linear/homography.h, src/estimation/optim/homography.cpp:31-43 ->
 * HomographyEstimator::fit, src/estimation/linear/homographyestimator.cpp:123-146): Hartley-normalised DLT of every view in one
 * launch.  h9 [n_views][9] row-major = T_dst^-1 Hn T_src with Hn(2,2) = 1, returned WITHOUT a final rescale exactly as the reference
 * does (homographyestimator.cpp:70, 79-87); success [n_views] = 0 where fit fails (< 4 correspondences, non-finite H), h9 is then
 * the identity.  The natural seed of cba_optimize_homography_batch. */
cba_status cba_estimate_homography_batch(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y,
                                         const double* u, const double* v, double* h9, int32_t* success);

/* estimate_planar_pose (include/calib/estimation/linear/planarpose.h:38-110, src/estimation/linear/planarpose_linear.cpp:54-76)
 * for a batch of views in one launch: pixels normalised by K = [fx, fy, cx, cy, skew], Hartley-normalised DLT homography
 * (src/estimation/linear/homographyestimator.cpp:17-87), pose_from_homography_normalized (planarpose_linear.cpp:17-52).
 * pose7 [n_views][7] out; a view with fewer than 4 points gets the identity, as in the reference (:55-57).
 * This is the seed optimize_intrinsics' callers and optimize_intrinsics_semidlt (intrinsicssemidlt.cpp:37-40) start from. */
cba_status cba_estimate_planar_pose_batch(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y,
                                          const double* u, const double* v, const double* kmtx5, double* pose7);

/* ---- laser-plane calibration of a line-scan rig (include/calib/estimation/linear/linescan.h:39-144, planefit.h/.cpp,
 * common/ransac.h; facade src/pipeline/linescan.cpp) ------------------------------------------------------------------
 *
 * cba_plane_fit_options = LineScanPlaneFitOptions (linescan.h:30-33) with its RansacOptions (ransac.h:23-30) inlined.
 * Defaults (cba_plane_fit_options_default): use_ransac 0, max_iters 1000, thresh 2.0, min_inliers 12, confidence 0.99,
 * seed 1234567, refit_on_inliers 1.
 *
 * RANSAC here is data-parallel: all max_iters hypotheses are scored (the reference's adaptive calculate_iterations only ever
 * lowers its iteration count, so this is a superset of its search); iters reports max_iters.  Hypothesis k draws three
 * distinct point indices from splitmix64 of (seed, 3k + j) (linescan_math.hpp), not from std::mt19937_64: the same seed
 * gives a different (equally valid) sample sequence than the reference.  confidence is accepted and unused.
 * The best model has the most inliers, ties broken by lower inlier RMS, then by lower k.  The winner's plane is refit on
 * its inliers exactly (two-pass centred scatter), as the reference's refit_model does, and its inliers recounted.
 *
 * Deliberate departures from the reference:
 *   - Scheimpflug unprojection.  The reference's ScheimpflugCamera::unproject (scheimpflug.h:198-230) cannot be
 *     instantiated (it calls CameraTraits<...>::apply_intrinsics_linear; the trait defines apply_linear_intrinsics,
 *     pinhole.h:149) and would return sensor-plane rather than normalised coordinates.  Here unproject is the exact
 *     inverse of the projection this library implements (scheimpflug.h:139-181): normalise by K, subtract the sensor
 *     offset m0, undistort, add m0, and map the tilted-sensor ray mx a + my b + n back to (x/z, y/z).
 *   - Plane sign.  The reference returns whatever sign its SVD gives.  Every plane returned here has d > 0, or, when
 *     |d| <= 1e-12 max|p|, its largest-magnitude normal component positive.
 */
#define CBA_PLANE_FIT_MAX_ITERS (1 << 20) /* most RANSAC hypotheses of one call (max_iters beyond it: CBA_ERR_INVALID_ARGUMENT) */

typedef struct cba_plane_fit_options {
    int32_t use_ransac;       /* 0: fit_plane_svd ("linear_svd"); 1: fit_plane_ransac ("ransac") */
    int32_t max_iters;        /* 1000; at most CBA_PLANE_FIT_MAX_ITERS */
    double thresh;            /* 2.0: a point is an inlier when |n.p + d| <= thresh */
    int32_t min_inliers;      /* 12 */
    int32_t refit_on_inliers; /* 1 */
    double confidence;        /* 0.99 (unused: every hypothesis is scored) */
    uint64_t seed;            /* 1234567 */
} cba_plane_fit_options;

typedef struct cba_laser_plane_result {
    double plane[4];        /* n (unit), d: n.p + d = 0 in the camera frame */
    double homography[9];   /* build_plane_homography(plane) (linescan.h:49-61), row-major */
    double rms_error;       /* plane_rms over all points (linear_svd) or over the inliers (ransac) */
    int64_t inlier_count;   /* n_points (linear_svd) or the number of inliers (ransac) */
    int64_t n_points;       /* points produced by points_from_view over all views */
    int32_t n_views_used;   /* views whose homography succeeded */
    int32_t iters;          /* ransac: hypotheses scored (= max_iters); linear_svd: 0 */
    char summary[16];       /* "linear_svd" | "ransac" */
} cba_laser_plane_result;

void cba_plane_fit_options_default(cba_plane_fit_options* opts);

/* calibrate_laser_plane (linescan.h:101-144).  The camera: camera_model + intr[10 | 12]; inverse_coeffs == NULL undistorts with
 * the 5-step fixed point of BrownConrady (distortion.h:119-134), non-NULL (n_inverse_coeffs in [2, 16], [k1..k_nr, p1, p2]) with
 * one evaluation of DualDistortion's inverse polynomial (distortion.h:213-217; see cba_invert_brown_conrady).  View i has target
 * correspondences [target_offset[i], target_offset[i+1]) of (X, Y) -> (u, v) and laser pixels [laser_offset[i], laser_offset[i+1]).
 * A view whose homography fails contributes no points (not an error).  Errors: fewer than 2 views, a view with fewer than 4
 * target correspondences, or fewer than 3 points in total -> CBA_ERR_INVALID_ARGUMENT; RANSAC finding no model -> CBA_ERR_RUNTIME.
 * Optional outputs: points_xyz [n_laser][3] = points_from_view of every laser pixel (NaN rows for views whose homography failed);
 * inlier_mask [n_laser] (1 = inlier; every point of a used view for linear_svd, 0 for the pixels of failed views).
 * The result is bitwise reproducible: every reduction runs in a fixed order. */
cba_status cba_calibrate_laser_plane(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                                     int32_t n_views, const int64_t* target_offset, const double* X, const double* Y, const double* u,
                                     const double* v, const int64_t* laser_offset, const double* laser_u, const double* laser_v,
                                     const cba_plane_fit_options* opts, cba_laser_plane_result* result, double* points_xyz,
                                     uint8_t* inlier_mask);

/* fit_plane_svd / fit_plane_ransac (planefit.cpp:68-114) on caller points xyz [n][3] (n >= 3, else CBA_ERR_INVALID_ARGUMENT).
 * opts->use_ransac selects the form; plane [4]; inlier_rms = plane_rms over the inliers (all points for the SVD form);
 * inlier_count; inlier_mask [n] optional.  RANSAC finding no model -> CBA_ERR_RUNTIME. */
cba_status cba_fit_plane(int64_t n, const double* xyz, const cba_plane_fit_options* opts, double* plane, double* inlier_rms,
                         int64_t* inlier_count, uint8_t* inlier_mask);

/* invert_brown_conrady (distortion.h:165-195): least-squares inverse coefficients of forward [k1..k_nr, p1, p2] (n >= 2) on the
 * 21 x 21 grid over [-1, 1]^2 (fit_distortion_full with K = identity, distortion.h:231-291).  inverse [n] out.  Host-only: the one
 * entry point of this group that needs no GPU.  n < 2 -> CBA_ERR_RUNTIME, as the reference throws std::runtime_error. */
cba_status cba_invert_brown_conrady(int32_t n, const double* forward, double* inverse);

/* ---- linear seed of planar intrinsic calibration (include/calib/estimation/linear/homography.h, intrinsics.h, zhang.h,
 * posefromhomography.h; src/estimation/linear/intrinsicsdlt.cpp:101-145, common/ransac.h, common/intrinsics_utils.h) ----------
 *
 * cba_ransac_options = RansacOptions (ransac.h:23-30).  Defaults (cba_ransac_options_default): max_iters 1000, thresh 2.0,
 * min_inliers 12, confidence 0.99, seed 1234567, refit_on_inliers 1.
 *
 * RANSAC over the homography of one view (ransac<HomographyEstimator>, ransac.h:121-194) is data-parallel, with the same two
 * departures as the laser-plane RANSAC above:
 *   - Every one of max_iters hypotheses is scored (the reference's adaptive calculate_iterations only ever lowers its count, so
 *     this is a superset of its search); confidence is accepted and unused.
 *   - Hypothesis k draws four distinct point indices from splitmix64 of (seed, 4k + j) (hom_ransac_math.hpp), not from
 *     std::mt19937_64 + std::sample: the same seed gives a different (equally valid) sample sequence than the reference.  As in
 *     the reference, which runs ransac per view with the same options, a view's samples depend only on its own point count and
 *     the options, never on its position in a batch.
 * A sample whose object points hold a near-collinear triplet (twice the area < 1e-6, homographyestimator.cpp:100-119) is skipped;
 * a model is kept when it has at least min_inliers inliers (symmetric transfer error <= thresh, :80-94); with refit_on_inliers it
 * is refit on those inliers by the Hartley-normalised DLT (refit_model, ransac.h:98-111; a failed refit keeps the raw model and
 * its inliers) and its inliers recounted.  The best model has the most inliers, ties broken by lower inlier RMS, then by lower k.
 * Every reduction runs in a fixed order: two identical calls are bitwise identical, and a view's result does not depend on the
 * other views of the batch.
 *
 * symmetric_rms reproduces the reference's symmetric_rms_px (intrinsicsdlt.cpp:21-30, optim/homography.cpp:19-28), which sums
 * the residuals r_i, not r_i^2: sqrt(sum_i r_i / 2n) over the n inliers (infinity when there are none). */
#define CBA_RANSAC_MAX_ITERS (1 << 16) /* most RANSAC hypotheses per view (max_iters beyond it: CBA_ERR_INVALID_ARGUMENT) */

typedef struct cba_ransac_options {
    int32_t max_iters;        /* 1000; in [0, CBA_RANSAC_MAX_ITERS] (0: no hypothesis, every view fails) */
    double thresh;            /* 2.0: a correspondence is an inlier when its symmetric transfer error is <= thresh (pixels) */
    int32_t min_inliers;      /* 12 */
    int32_t refit_on_inliers; /* 1 */
    double confidence;        /* 0.99 (unused: every hypothesis is scored) */
    uint64_t seed;            /* 1234567 */
} cba_ransac_options;

void cba_ransac_options_default(cba_ransac_options* opts);

/* estimate_homography (include/calib/estimation/linear/homography.h:22-24, src/estimation/optim/homography.cpp:31-60) of every
 * view: view i has correspondences [view_offset[i], view_offset[i+1]) of target (X, Y) -> pixel (u, v).  opts != NULL: RANSAC
 * with those options (estimate_homography_ransac, :45-60); opts == NULL: the all-points Hartley-normalised DLT
 * (estimate_homography_dlt, :31-43).  Per view: h9 [9] row-major, returned WITHOUT an h22 rescale as the reference returns it
 * (the identity where the view fails); success (0 for fewer than 4 points, a failed fit, or RANSAC finding no model);
 * inlier_count; symmetric_rms (see above; 0 where the view fails).  inlier_mask [view_offset[n_views]] optional (1 = inlier; every
 * point of a successful view on the DLT path).  n_views == 0 is no work.  Errors: null pointers, bad offsets, max_iters outside
 * [0, CBA_RANSAC_MAX_ITERS] or thresh < 0 -> CBA_ERR_INVALID_ARGUMENT. */
cba_status cba_estimate_homography_ransac_batch(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y,
                                                const double* u, const double* v, const cba_ransac_options* opts, double* h9,
                                                int32_t* success, int32_t* inlier_count, double* symmetric_rms, uint8_t* inlier_mask);

/* estimate_intrinsics (include/calib/estimation/linear/intrinsics.h:56-58, intrinsicsdlt.cpp:101-145) as one device pipeline:
 * the homography of every view (RANSAC with *ransac when use_ransac, else the all-points DLT), rescaled by h22 where
 * |h22| > 1e-15 (:56-58, 69-71); zhang_intrinsics_from_hs over the successful views in view order; sanitize_intrinsics with the
 * optional bounds (bounds_lo5 / bounds_hi5 = [fx, fy, cx, cy, skew], both NULL: no bounds); pose_from_homography of every
 * successful view with the sanitised K.  use_skew is accepted and unused, as in the reference.
 * Outputs: success (0: no views, or fewer than 4 views with a homography -- not an error); kmtx5 [fx, fy, cx, cy, skew] (zeros when
 * unsuccessful); sanitized (1 when the bounds changed K); and per INPUT view: view_ok (the homography succeeded: the view is one of
 * the reference's result.views, in input order), h9 (rescaled), forward_rms_px (symmetric_rms_px), rt12 = c_T_t as [R (9, row-major) | t (3)]
 * (the identity where it fails) and pose_ok (pose_from_homography succeeded).  Poses are [R | t], not quaternions: where t_z <= 0
 * the reference negates R and t together (posefromhomography.cpp:49-54), which leaves det R = -1, and that is returned as is.  inlier_mask [view_offset[n_views]] optional.
 * A view with fewer than 4 points fails (not an error).  Errors: as cba_estimate_homography_ransac_batch. */
cba_status cba_estimate_intrinsics(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u,
                                   const double* v, int32_t use_ransac, const cba_ransac_options* ransac, const double* bounds_lo5,
                                   const double* bounds_hi5, int32_t use_skew, int32_t* success, double* kmtx5, int32_t* sanitized,
                                   int32_t* view_ok, double* h9, double* forward_rms_px, double* rt12, int32_t* pose_ok,
                                   uint8_t* inlier_mask);

/* zhang_intrinsics_from_hs (zhang.h, zhang.cpp:174-206) on n homographies h9 [n][9] (row-major): kmtx5 = [fx, fy, cx, cy, skew],
 * success = 0 (kmtx5 untouched) where the reference returns nullopt (n < 4, B factors with neither sign).  Host-only. */
cba_status cba_zhang_intrinsics_from_hs(int32_t n, const double* h9, double* kmtx5, int32_t* success);

/* pose_from_homography (posefromhomography.h, posefromhomography.cpp:11-62) with K = kmtx5: rt12 = c_T_t as [R (9, row-major) | t (3)]
 * (see cba_estimate_intrinsics on det R), success, and the reference's diagnostics scale and cond_check (either may be NULL).  Host-only. */
cba_status cba_pose_from_homography(const double* kmtx5, const double* h9, double* rt12, int32_t* success, double* scale,
                                    double* cond_check);

/* sanitize_intrinsics (common/intrinsics_utils.h) with bounds lo5 / hi5 ([fx, fy, cx, cy, skew]; fx_max, fy_max unused, as in the
 * reference): out5, modified.  Host-only. */
cba_status cba_sanitize_intrinsics(const double* kmtx5, const double* bounds_lo5, const double* bounds_hi5, double* out5,
                                   int32_t* modified);

/* ---- linear seed of a multi-camera rig (include/calib/estimation/linear/extrinsics.h:27-78, estimation/common/se3_utils.h:75-95;
 * the seed of the stereo and multi-camera facades, src/pipeline/facades/extrinsics.cpp:91-131, 184-229) --------------------------
 *
 * estimate_extrinsic_dlt on the blocked layout of cba_optimize_extrinsics: block b holds the points [blk_offset[b], blk_offset[b+1])
 * of view blk_view[b] seen by camera blk_cam[b]; an absent (view, camera) pair has no block.  kmtx5 [n_cams][5] = [fx, fy, cx, cy,
 * skew] of each camera.  Outputs feed cba_optimize_extrinsics directly: c_T_r [n_cams][7], r_T_t [n_views][7] (pose7, unit
 * quaternions), and optionally blk_c_T_t [n_blocks][7] (each block's planar pose) and blk_ok [n_blocks].
 *   1. Every block's pose is estimate_planar_pose (planarpose.h:38-110) with its camera's K: pixels normalised by K only, so
 *      DISTORTION IS IGNORED, as in the reference (the facades' dual-distortion cameras are only read for K); then the
 *      Hartley-normalised DLT and pose_from_homography_normalized.  A block's pose is bitwise what cba_estimate_planar_pose_batch
 *      returns for it with the same K.
 *   2. c_T_r[0] = I; c_T_r[c] averages T[v][c] T[v][0]^-1 over the views v, in increasing v, where both blocks exist and have at
 *      least 4 points (the identity when there is none).
 *   3. r_T_t[v] averages c_T_r[c]^-1 T[v][c] over the cameras c, in increasing c, whose block exists and has at least 4 points (the
 *      identity when there is none).
 *   Averaging is average_isometries: the mean translation and a running quaternion sum in which each new quaternion is negated when
 *   its dot product with the sum so far is negative.  That sign rule is sequential and order-dependent and is kept as it is; the
 *   order comes from the (view, camera) indices, so results do not depend on the order of the blocks, a camera's c_T_r does not
 *   depend on the other cameras' blocks, and two identical calls are bitwise identical.
 * Departure: the reference's template estimate_planar_pose has no failure branch.  Here, as in its CameraMatrix overload
 * (planarpose_linear.cpp:54-76), a block of >= 4 points whose homography fit fails (non-finite, or a singular normal matrix) gets
 * the identity pose and blk_ok = 0; the skip rules of steps 2 and 3 count points only, as the reference's do, so such a block still
 * enters the averages with that identity.  blk_ok = 0 also marks blocks of fewer than 4 points.
 * Errors: n_cams < 1 or n_views < 1 -> CBA_ERR_RUNTIME "Empty views or cameras provided" (the reference's runtime_error); null
 * required pointers, n_blocks < 0, offsets not starting at 0 or decreasing, a view or camera index out of range, or two blocks with
 * the same (view, camera) -> CBA_ERR_INVALID_ARGUMENT, all checked before any device work.  n_blocks == 0 gives identities without
 * a device; otherwise no device -> CBA_ERR_NO_DEVICE. */
cba_status cba_estimate_extrinsic_dlt(int32_t n_cams, int32_t n_views, int32_t n_blocks, const int64_t* blk_offset, const int32_t* blk_view,
                                      const int32_t* blk_cam, const double* X, const double* Y, const double* u, const double* v,
                                      const double* kmtx5, double* c_T_r, double* r_T_t, double* blk_c_T_t, int32_t* blk_ok);

/* ---- seed of the hand-eye and bundle stages of a robot-mounted rig (src/pipeline/detail/bundle_utils.cpp:46-237 with
 * estimate_handeye_dlt, src/estimation/linear/handeyedlt.cpp:126-137; stages src/pipeline/stages/handeye_stage.cpp,
 * bundle_stage.cpp) ------------------------------------------------------------------------------------------------------------
 *
 * On the blocked layout of cba_optimize_bundle: block b holds the points [blk_offset[b], blk_offset[b+1]) seen by camera blk_cam[b]
 * from robot pose blk_b_T_g[b] (row-major R (9) then t (3)).  kmtx5 [n_cams][5] = [fx, fy, cx, cy, skew].  The outputs feed
 * cba_optimize_bundle directly: g_T_c [n_cams][7] and b_T_t [7] (pose7).
 *   1. Every block's pose c_T_t is estimate_planar_pose with its camera's K: pixels normalised by K only, so DISTORTION IS IGNORED;
 *      a block's pose is bitwise what cba_estimate_planar_pose_batch returns for it (blk_c_T_t, blk_ok; both may be NULL).
 *   2. Camera c's pose list (the reference's SensorAccumulator, bundle_utils.cpp:126-127) is its blocks of >= 4 points in
 *      increasing block index: collect_bundle_observations appends in view order and observations are listed view-major.
 *   3. compute_handeye_initialization (bundle_utils.cpp:154-200), per camera:
 *        given_mask[c] != 0 -> g_T_c_given[c] is copied, status GIVEN (a successful hand-eye stage result; no DLT is run);
 *        fewer than 2 listed blocks -> the identity, TOO_FEW_VIEWS ("insufficient_observations");
 *        otherwise estimate_handeye_dlt over the list at min_angle_deg: all pairs i < j, the pair filter of build_all_pairs
 *        (axis eps 1e-3), the Tsai-Lenz rotation then translation ridge solves (1e-12).  cam_pairs[c] = pairs that pass the filter.
 *        No pair -> the identity, NO_PAIRS (the reference's "No valid motion pairs after filtering. Increase motion or relax
 *        thresholds."); else DLT.  The per-camera sums are reduced in the order cba_estimate_handeye_dlt reduces one pose list.
 *   4. choose_initial_target (bundle_utils.cpp:202-237): b_T_t_given non-NULL -> copied, CONFIG.  Otherwise the candidates
 *      b_T_g * g_T_c[c] * c_T_t of every listed block, camera-major and then in list order (a camera whose seed failed takes part
 *      with its identity g_T_c, as in the reference), are averaged by average_isometries with its sequential sign rule
 *      (se3_utils.h:75-95): ESTIMATED; no candidate -> the identity, IDENTITY.
 * A camera's g_T_c depends only on its own blocks and their order, b_T_t only on each camera's own order: interleaving different
 * cameras' blocks changes neither, and two identical calls are bitwise identical.
 * Departures: a singular Tsai-Lenz system gives SINGULAR and the identity (the reference's LDLT returns whatever it returns, as
 * cba_estimate_handeye_dlt does); a block of >= 4 points whose fit fails gets the identity pose and blk_ok = 0 but stays in its
 * camera's list, because the reference's skip rule counts points only (as cba_estimate_extrinsic_dlt).
 * Errors (CBA_ERR_INVALID_ARGUMENT, all before any device work): n_cams < 1, n_blocks < 0, offsets not starting at 0 or
 * decreasing, a blk_cam out of range, a negative or non-finite min_angle_deg, a NULL required pointer, given_mask without
 * g_T_c_given.  n_blocks == 0 needs no device; otherwise no device -> CBA_ERR_NO_DEVICE. */
enum {
    CBA_HANDEYE_DLT = 0,           /* estimated here */
    CBA_HANDEYE_GIVEN = 1,         /* copied from g_T_c_given */
    CBA_HANDEYE_TOO_FEW_VIEWS = 2, /* fewer than 2 listed blocks: identity */
    CBA_HANDEYE_NO_PAIRS = 3,      /* no motion pair passes the filter: identity */
    CBA_HANDEYE_SINGULAR = 4       /* a singular Tsai-Lenz system: identity */
};
enum {
    CBA_TARGET_ESTIMATED = 0, /* averaged from the candidates */
    CBA_TARGET_CONFIG = 1,    /* copied from b_T_t_given */
    CBA_TARGET_IDENTITY = 2   /* no candidate */
};
cba_status cba_estimate_bundle_seed(int32_t n_cams, int32_t n_blocks, const int64_t* blk_offset, const int32_t* blk_cam,
                                    const double* blk_b_T_g /*[n_blocks][12]*/, const double* X, const double* Y, const double* u,
                                    const double* v, const double* kmtx5 /*[n_cams][5]*/, double min_angle_deg,
                                    const int32_t* given_mask /*[n_cams] or NULL*/, const double* g_T_c_given /*[n_cams][7] or NULL*/,
                                    const double* b_T_t_given /*[7] or NULL*/, double* g_T_c /*[n_cams][7]*/,
                                    int32_t* cam_status /*[n_cams]*/, int32_t* cam_pairs /*[n_cams]*/, double* b_T_t /*[7]*/,
                                    int32_t* target_source, double* blk_c_T_t /*[n_blocks][7] or NULL*/, int32_t* blk_ok /*or NULL*/);

/* ---- distortion fits and the iterative linear intrinsic seed (include/calib/models/distortion.h:229-406;
 * include/calib/estimation/linear/intrinsics.h:60-70, src/estimation/linear/intrinsicsdlt.cpp:147-368) ----------------------
 *
 * Batched over independent problems: problem p owns the observations [offset[p], offset[p+1]) of x, y (normalised, undistorted)
 * and u, v (pixels), the reference's Observation (distortion.h:69-72).  kmtx5 = [fx, fy, cx, cy, skew]; coefficients are
 * [k1 .. k_nr, p1, p2] (m = num_radial + 2 per problem).  One data pass forms each problem's moments (distortion_fit_math.hpp);
 * the solves and the alternation then run on the moments alone.  Results are bitwise reproducible: a problem's result does not
 * depend on its position in the batch or on the other problems, and two identical calls agree bit for bit.
 *
 * cba_fit_distortion_batch: fit_distortion_full (:231-363) of every problem at its kmtx5, coeffs [P][m], ok [P] (0 where the
 * reference returns nullopt: fewer than 8 observations; coeffs are then 0), residuals [2 N] (optional: design * alpha - rhs, rows
 * 2i and 2i + 1 of observation i; 0 for problems with ok = 0).  dual = 1: fit_distortion_dual (:373-406), whose inverse fit runs on
 * ((u - cx - skew y_d) / fx, (v - cy) / fy) -> the undistorted pixels, with the same fixed set; inverse [P][m] is then required and
 * the residuals are the forward fit's.  Fixed coefficients (fixed_idx [n_fixed], fixed_val [n_fixed] or NULL, the same for every
 * problem): an index outside [0, m - 1] is CBA_ERR_INVALID_ARGUMENT (:315-318); a NULL fixed_val holds every fixed value at 0 (the
 * reference's missing values); fixed entries come back bit-exact; with every coefficient fixed, alpha is the fixed values and the
 * residuals are still computed (:334-337).
 * cba_estimate_intrinsics_linear_batch: estimate_intrinsics_linear (:289-312) with CalibrationBounds bounds_lo5 / bounds_hi5
 * ([fx, fy, cx, cy, skew]; both NULL select CalibrationBounds{}, as nullopt does).  status [P]; fallback [P] = 1 where
 * apply_bounds_and_fallback took its fallback (the reference's stderr warning).  use_skew is honoured.
 * cba_estimate_intrinsics_linear_iterative_batch: estimate_intrinsics_linear_iterative (:319-368).  Kept from the reference:
 *   - every K fit uses the DEFAULT bounds (it passes nullopt, :323, :343), so K outside fx, fy <= 2000, cx <= 1280, cy <= 720,
 *     |skew| <= 0.01 takes the fallback: fx, fy -> clamp(max(500, f)); cx, cy -> clamp(mean(u_corr) / 2), clamp(mean(v_corr) / 2);
 *     skew -> clamp(skew) when use_skew, else 0.  fallback [P] counts the fits of K (the initial one included) that took it;
 *   - the loop breaks when the distortion fit fails (fewer than 8 observations) or the K refit fails, and stops when
 *     Σ|ΔK| < 1e-6, compared against the post-fallback K; iterations [P] counts the K refits adopted;
 *   - the final fit failing (fewer than 8 observations) gives TOO_FEW; use_skew is honoured.
 *   kmtx5 [P][5] and coeffs [P][m] are 0 where status != OK.
 * Departures:
 *   (a) normal equations from fixed-order moments replace JacobiSVD.  The distortion fit's m x m Gram (of the free columns) is
 *       column-equilibrated and eigen-decomposed by cyclic Jacobi; eigenvalues <= 1e-13 lambda_max are dropped and the
 *       minimum-norm solution (in the coefficients' own scale) is returned, which is what svd.solve returns up to the cutoff.
 *       JacobiSVD's own rank cutoff is relative too (about 1e-15 of sigma_max), so the distortion fits differ only for designs whose
 *       equilibrated singular-value ratio lies between about 1e-15 and 3.2e-7, which the Gram cannot resolve.
 *       The K fit's sigma_min < 1e-12 test is ABSOLUTE in the reference, so it depends on the scale of the data; here it becomes
 *       the relative test lambda_min <= 1e-13 lambda_max on the equilibrated 2 x 2 / 3 x 3 Gram.  Both reject identical x (or y)
 *       values.  They differ in two places: this test rejects a spread of x or y below ~4.5e-7 of its mean, which the reference
 *       may accept; and the reference rejects a well-conditioned design whose x or y values are all tiny in magnitude (sigma_min
 *       below 1e-12 in absolute terms), which this test accepts.  Neither arises with normalised coordinates of a real camera.
 *   (b) num_radial must be in [0, 3].
 *   (c) max_iterations is at most CBA_LINEAR_MAX_ITERATIONS; a negative value means 0, as in the reference.
 *   (d) duplicate fixed indices: the first in input order wins (the reference's sort + unique leaves it unspecified).
 * Errors (CBA_ERR_INVALID_ARGUMENT, all checked before any device work): n_problems < 0; NULL required pointers; offsets not
 * starting at 0 or decreasing; num_radial outside [0, 3]; n_fixed < 0 or a fixed index out of range; dual without inverse; one
 * bounds pointer NULL and not the other; max_iterations above CBA_LINEAR_MAX_ITERATIONS.  n_problems == 0 is no work; otherwise
 * no device -> CBA_ERR_NO_DEVICE.
 * Order of checks: the fixed set is one per call, so cba_fit_distortion_batch rejects a fixed index out of range for the whole
 * batch, even when every problem has fewer than 8 observations.  The reference returns nullopt for fewer than 8 observations
 * before it looks at the indices (distortion.h:235-238, 315-318); the single-problem wrappers (Python calibration_amd.distortion,
 * C++ calibba_distortion.hpp) restore that order by returning nullopt / None before they call the batch. */
#define CBA_LINEAR_MAX_ITERATIONS 65536
enum {
    CBA_LINEAR_OK = 0,
    CBA_LINEAR_TOO_FEW = 1,    /* < 2 observations for a K fit, < 8 for a distortion fit (the iterative estimator's final fit) */
    CBA_LINEAR_DEGENERATE = 2  /* a K fit's design is rank-deficient */
};
cba_status cba_fit_distortion_batch(int32_t n_problems, const int64_t* offset, const double* x, const double* y, const double* u,
                                    const double* v, const double* kmtx5 /*[P][5]*/, int32_t num_radial, int32_t n_fixed,
                                    const int32_t* fixed_idx, const double* fixed_val, int32_t dual, double* coeffs /*[P][m]*/,
                                    double* inverse /*[P][m] or NULL*/, int32_t* ok /*[P]*/, double* residuals /*[2 N] or NULL*/);
cba_status cba_estimate_intrinsics_linear_batch(int32_t n_problems, const int64_t* offset, const double* x, const double* y,
                                                const double* u, const double* v, const double* bounds_lo5, const double* bounds_hi5,
                                                int32_t use_skew, double* kmtx5 /*[P][5]*/, int32_t* status, int32_t* fallback);
cba_status cba_estimate_intrinsics_linear_iterative_batch(int32_t n_problems, const int64_t* offset, const double* x, const double* y,
                                                          const double* u, const double* v, int32_t num_radial, int32_t max_iterations,
                                                          int32_t use_skew, double* kmtx5 /*[P][5]*/, double* coeffs /*[P][m]*/,
                                                          int32_t* status, int32_t* iterations, int32_t* fallback);

/* ---- camera models: project, unproject and undistortion / rectification maps (include/calib/models/pinhole.h:96-113,
 * scheimpflug.h:139-181, distortion.h:119-160, 208-218) ----------------------------------------------------------------------
 *
 * A camera is described as for cba_calibrate_laser_plane: camera_model CBA_CAMERA_PINHOLE_BC or CBA_CAMERA_SCHEIMPFLUG, intr [10 | 12];
 * where an inverse is needed, inverse_coeffs [n_inverse_coeffs] (n in [2, 16], [k1 .. k_nr, p1, p2]) select DualDistortion's one-step
 * undistortion and NULL BrownConrady's 5-step fixed point.  All arithmetic is fp64 unless stated.
 *
 * cba_camera_project: uv [n][2] = project(xyz [n][3]) (camera frame), the reference's project(xyz) with its Scheimpflug form, in the
 * expression order of the reprojection residual, with the Horner radial polynomial.  No masking: z <= 0, or a Scheimpflug sensor denominator
 * <= 0, gives whatever the division gives, as in the reference.  xyz = (x, y, 1) is project(norm_xy); with intr = [1, 1, 0, 0, 0,
 * k1, k2, k3, p1, p2] it is the distortion's distort.
 * cba_camera_unproject: xy [n][2] = the normalised coordinates of pixels uv [n][2]: the pinhole's unproject (normalize, then
 * undistort); for Scheimpflug the exact inverse of the projection that cba_calibrate_laser_plane documents and runs.
 *
 * cba_undistort_map: a handle that owns the maps on one device and one stream.  cba_undistort_map_create takes n_cams cameras of one
 * model, intr [n_cams][10 | 12], an optional rectifying rotation per camera R [n_cams][9] (row-major; NULL: identity), an optional
 * new camera matrix per camera new_k5 [n_cams][5] ([fx', fy', cx', cy', skew']; NULL: each camera's own K) and one output size
 * width x height.  For every output pixel centre (u', v') (integer coordinates) of every camera it computes on the device
 *   y = (v' - cy') / fy',  x = (u' - cx' - skew' y) / fx',  P = R^T (x, y, 1),  (map_x, map_y) = project(P) rounded to nearest float32;
 * a ray with z <= 0 (pinhole) or a sensor denominator <= 0 (Scheimpflug) gives NaN in both.  The maps are [n_cams][height][width]
 * float32, the layout of OpenCV's remap.  cba_undistort_map_fetch downloads them (map_x, map_y [n_cams][height][width]).
 * cba_undistort_map_apply resamples n_images source images src [n_images][src_height][src_width][channels] (channels 1..4,
 * interleaved; dtype CBA_DTYPE_U8 or CBA_DTYPE_F32) through the maps of cameras cam [n_images] into dst
 * [n_images][height][width][channels].  Bilinear with a constant border: a tap outside the source reads the border value; a NaN map
 * coordinate, or one beyond +-2^24, gives the border value for the pixel.  The maps never leave the device.  Arithmetic:
 *   uint8    OpenCV's fixed-point rule: X = rintf(32 map_x) (round half to even), x0 = X >> 5, a = X & 31 (the same for y, b);
 *            weights (32-a)(32-b)32, a(32-b)32, (32-a)b32 and ab32 of the taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1),
 *            which sum to 2^15; the result is (sum w p + 2^14) >> 15, saturated: exact integers.  The border is rounded half to
 *            even and clamped to [0, 255] (NaN: 0).
 *   float32  x0 = floorf(map_x), fx = map_x - x0 (the same for y); t = p00 + fx (p01 - p00), b = p10 + fx (p11 - p10),
 *            result = t + fy (b - t) in fp32; the border is converted to float32.
 * Errors (CBA_ERR_INVALID_ARGUMENT, all checked before any device work): NULL required pointers; an unknown model; an inverse count
 * outside [2, 16]; n < 0; n_cams < 1; width, height, src_width or src_height outside [1, 32768]; fx' or fy' equal to 0; n_images < 0;
 * a camera index out of range; channels outside 1..4; an unknown dtype.  n == 0 (n_images == 0) is no work; otherwise no device ->
 * CBA_ERR_NO_DEVICE. */
enum { CBA_DTYPE_U8 = 0, CBA_DTYPE_F32 = 1 };
#define CBA_IMAGE_MAX_SIDE 32768
cba_status cba_camera_project(int32_t camera_model, const double* intr, int64_t n, const double* xyz /*[n][3]*/, double* uv /*[n][2]*/);
cba_status cba_camera_unproject(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs, int64_t n,
                                const double* uv /*[n][2]*/, double* xy /*[n][2]*/);
typedef struct cba_undistort_map cba_undistort_map; /* opaque: owns the maps on the device + one HIP stream */
cba_status cba_undistort_map_create(int32_t camera_model, int32_t n_cams, const double* intr, const double* R /*[n_cams][9] or NULL*/,
                                    const double* new_k5 /*[n_cams][5] or NULL*/, int32_t width, int32_t height, int32_t device,
                                    cba_undistort_map** out);
cba_status cba_undistort_map_fetch(cba_undistort_map* h, float* map_x, float* map_y);
cba_status cba_undistort_map_apply(cba_undistort_map* h, int32_t n_images, const int32_t* cam, int32_t src_width, int32_t src_height,
                                   int32_t channels, int32_t dtype, double border, const void* src, void* dst);
void cba_undistort_map_destroy(cba_undistort_map* h);

/* ---- multi-camera triangulation (no counterpart in the reference) -----------------------------------------------------------
 *
 * cba_triangulate turns matched pixels of n_cams calibrated cameras into 3D points in the reference frame, one independent small
 * nonlinear least-squares problem per point, all on the device in fp64.
 *
 * Inputs: n_cams cameras of one model, 2 <= n_cams <= CBA_TRI_MAX_CAMS; camera_model and intr [n_cams][10 | 12] as above; optional
 * inverse_coeffs [n_cams][n_inverse_coeffs] with the meaning they have in cba_camera_unproject (NULL: the 5-step fixed point);
 * c_T_r [n_cams][7], pose7 rows [qw qx qy qz tx ty tz] mapping the reference frame to each camera, exactly the rows
 * cba_estimate_extrinsic_dlt and cba_optimize_extrinsics return (the rotation is the quaternion's matrix without normalisation); n
 * points with pixels uv [n_cams][n][2], camera-major: each camera's slice has the layout cba_camera_project writes.  A non-finite
 * coordinate means "this camera did not see this point".
 *
 * Outputs: xyz [n][3] (reference frame); rms_px [n] = sqrt(sum over the used cameras of (e_u^2 + e_v^2) / n_used), evaluated with
 * the projection of cba_camera_project at P = R_c X + t_c (each row summed left to right, then + t), so it agrees with a round trip
 * through that entry point; used_mask [n] (bit c: camera c was used); status [n] (cba_tri_status); optional cov6 [n][6] =
 * (J^T J)^-1 at the solution in the order 00 01 02 11 12 22: the covariance of X for unit pixel sigma, the caller scales it.
 * rms_px, used_mask and cov6 may be NULL.
 *
 * Per point:
 * 1. Seed.  For every camera of the set (first: the cameras with a finite pixel), in camera order: (x, y) = the unprojection of
 *    cba_camera_unproject, d = R_c^T (x, y, 1) / |.|, o = -R_c^T t_c; A = sum (I - d d^T), b = sum (I - d d^T) o.  Fewer than
 *    max(min_cams, 2) cameras: CBA_TRI_TOO_FEW, NaN outputs, used_mask 0.  A X = b by the unpivoted 3 x 3 Cholesky; when it fails or
 *    a pivot (a squared diagonal entry of L) is <= 1e-12 n_used (two rays closer than ~2e-6 rad to parallel): CBA_TRI_DEGENERATE,
 *    NaN outputs, used_mask = the set.
 * 2. Refinement.  Levenberg-Marquardt on sum_c |project_c(R_c X + t_c) - uv_c|^2 through the full forward model.  Rows of J are
 *    (du/dP) R_c and (dv/dP) R_c; H = J^T J, g = J^T r; (H + lambda diag H) delta = -g by Cholesky (a failure counts as a rejected
 *    step).  The trial X + delta is accepted when every used camera has a positive denominator there (z for the pinhole, the sensor
 *    denominator for Scheimpflug) and its cost does not exceed the current one by more than the cost's rounding floor
 *    s = 4e-12 px sqrt(n_used cost); then lambda <- max(lambda / 10, 1e-10), otherwise lambda <- 10 lambda.  lambda starts at 1e-4.
 *    The iteration stops with CBA_TRI_OK after the step (accepted or not) whose |delta| <= step_tolerance |X|, or after an accepted
 *    step that lowers the cost by no more than s, and with CBA_TRI_NOT_CONVERGED after max_iterations steps (0: the seed is
 *    returned); outputs are written either way.  (s bounds |sum 2 r e| for pixel roundings e of 1e-12 px.  Below it the sign of a
 *    cost difference is noise, and with two cameras the rounding of J^T r alone keeps |delta| near 3e-12 |X|, so the step rule
 *    cannot end such a point at the default tolerance.)
 * 3. Outlier cameras (max_reproj_px, +inf = off).  When the largest per-camera error sqrt(e_u^2 + e_v^2) at the result exceeds it
 *    and more than max(min_cams, 2) cameras are in the set, that camera (the lowest index among equals) leaves the set and the
 *    point starts again at step 1: the result is, to the bit, that of a call in which that pixel was NaN.
 * 4. A final point with a non-positive denominator in a used camera has status CBA_TRI_BEHIND (outputs written).  cov6 is the
 *    Cholesky inverse of the H of the last accepted linearisation (the seed's when no step was accepted); NaN where H is not
 *    positive definite.
 *
 * A point's result depends on nothing but its own pixels.  Errors (CBA_ERR_INVALID_ARGUMENT, before any device work): an unknown
 * model; n_cams outside [2, 16]; an inverse count outside [2, 16]; fx or fy equal to 0; n < 0; max_iterations < 0; a negative or NaN
 * step_tolerance; max_reproj_px not > 0; NULL intr, c_T_r, opts, or (for n > 0) uv, xyz, status.  n == 0 is no work. */
#define CBA_TRI_MAX_CAMS 16
typedef enum cba_tri_status {
    CBA_TRI_OK = 0,
    CBA_TRI_NOT_CONVERGED = 1, /* max_iterations steps without meeting step_tolerance */
    CBA_TRI_BEHIND = 2,        /* the point is not in front of every used camera */
    CBA_TRI_DEGENERATE = 3,    /* parallel rays: no seed */
    CBA_TRI_TOO_FEW = 4        /* fewer than max(min_cams, 2) cameras saw the point */
} cba_tri_status;
typedef struct cba_triangulate_options {
    int32_t max_iterations; /* LM steps after the seed (default 10) */
    double step_tolerance;  /* relative step size that ends the iteration (default 1e-12) */
    int32_t min_cams;       /* cameras a point needs (default 2; values below 2 mean 2) */
    double max_reproj_px;   /* per-camera error above which the worst camera is dropped (default +inf: off) */
} cba_triangulate_options;
void cba_triangulate_options_default(cba_triangulate_options* o);
cba_status cba_triangulate(int32_t camera_model, int32_t n_cams, const double* intr, int32_t n_inverse_coeffs,
                           const double* inverse_coeffs /*[n_cams][n_inverse_coeffs] or NULL*/, const double* c_T_r /*[n_cams][7]*/,
                           int64_t n, const double* uv /*[n_cams][n][2]*/, const cba_triangulate_options* opts, double* xyz /*[n][3]*/,
                           double* rms_px /*[n] or NULL*/, uint32_t* used_mask /*[n] or NULL*/, int32_t* status /*[n]*/,
                           double* cov6 /*[n][6] or NULL*/);

/* ---- laser profile scanning (no counterpart in the reference) ---------------------------------------------------------------
 *
 * What a line-scan rig does at frame rate with the result of cba_calibrate_laser_plane: find the laser line in each frame with
 * sub-pixel accuracy, turn every line pixel into a ray through the camera and intersect it with the laser plane.  The reference
 * computes the plane and its homography and never applies them.  Camera (camera_model, intr, inverse_coeffs) as for
 * cba_camera_unproject; plane [nx ny nz d] with n.p + d = 0 as cba_calibrate_laser_plane returns it (d > 0).  fp64 unless stated.
 *
 * Pixel to 3D (cba_laser_points, and every line of the scanner).  For a pixel (u, v): (x, y) = the unprojection of
 * cba_camera_unproject, r = (x, y, 1), den = n.r, s = -d / den, P = s r.  den == 0, s <= 0 or a non-finite s (a NaN pixel included)
 * give NaN in all three coordinates.  There is no threshold on den: the plane code divides without one, and s <= 0 rejects every
 * ray that meets the plane behind the camera.  With a frame pose pose7 = [qw qx qy qz tx ty tz], P <- R P + t: R is the quaternion's
 * matrix without normalisation, as in cba_triangulate; each row is summed left to right, then + t.  The products and sums of this
 * paragraph are not contracted into fused multiply-adds.  Optional plane_xy = hnormalized(Hp (x, y, 1)) with
 * Hp = build_plane_homography(plane): the in-plane coordinates that cba_laser_plane_result.homography promises; NaN where P is.
 *
 * cba_laser_points: n caller pixels uv [n][2] -> xyz [n][3] and optionally plane_xy [n][2].  Frames: frame_offset [n_frames + 1],
 * non-decreasing from 0 to n, says which pixels belong to which frame (empty frames allowed); frame_pose7 [n_frames][7] moves each
 * frame's points.  Without frame_pose7 there is no pose (frame_offset, if given, is only checked); frame_pose7 without frame_offset
 * needs n_frames == 1 and applies to every pixel.
 *
 * cba_laser_scanner: a handle that owns the camera, the plane, the options, one stream and device buffers sized at create for
 * max_frames frames of width x height; cba_laser_scanner_process allocates nothing.  Images are single channel, CBA_DTYPE_U8 or
 * CBA_DTYPE_F32 (chosen per call), I[frame][row][column], rows and frames contiguous.  axis 0: one peak per column, searched along
 * the rows (n_lines = width, the pixel of line l is (l, centre)); axis 1: one peak per row, searched along the columns (n_lines =
 * height, the pixel is (centre, l)).  "Position" p is the index along the search direction, inside the ROI [roi_begin, roi_end)
 * (0, 0: the whole side).  For one line:
 * 1. m = the maximum of I over the ROI; p0 = the lowest position with I == m; p1 = the end of the contiguous run of positions equal
 *    to m that starts at p0 (the saturation plateau; normally p1 == p0).  NaN samples (float32) never compare as a maximum, end a
 *    plateau and count as 0 in the sums.
 * 2. The line is invalid when m < min_peak (or the ROI holds no sample that is not NaN): centre = NaN, width_px = NaN, xyz = NaN,
 *    amplitude = m (NaN without a sample).
 * 3. Window [max(p0 - half_window, roi_begin), min(p1 + half_window, roi_end - 1)]; g(p) = max(I(p) - floor_level, 0);
 *    centre = sum g p / sum g.  uint8: floor_level is rounded half to even and clamped to [0, 255]; both sums are exact 64-bit
 *    integers; centre is one fp64 division.  float32: samples are converted to fp64; g p is rounded, then added; both sums run in
 *    ascending p in fp64; centre is one division.  sum g == 0 makes the line invalid as in step 2.
 * 4. Outputs per line, fp64: centre, amplitude = m, width_px = sum g / (m - floor_level) (the equivalent width, with the rounded
 *    floor for uint8), xyz = the pixel's point as above, moved by frame_pose7 [n_frames][7] when given.
 * A line's result depends on nothing but its own samples: not on the other lines or frames of the call, and not on how the device
 * splits the search direction.  Outputs are [n_frames][n_lines] (xyz: [n_frames][n_lines][3]); each may be NULL.
 *
 * Errors (CBA_ERR_INVALID_ARGUMENT, all checked before any device work): NULL required pointers (intr, plane, options, out, the
 * handle; for n > 0 uv and xyz; for n_frames > 0 images); an unknown model or dtype; an inverse count outside [2, 16]; n < 0; width
 * or height outside [1, CBA_IMAGE_MAX_SIDE]; max_frames < 1; an axis other than 0 or 1; an ROI that is empty or outside the image;
 * half_window < 0; n_frames < 0 or n_frames > max_frames; a plane normal that is zero or non-finite, or a non-finite d; a non-finite
 * floor_level or min_peak; frame_pose7 given while frame_offset is NULL and n_frames != 1; frame_offset not non-decreasing from 0
 * to n.  n == 0 and n_frames == 0 are no work; otherwise no device -> CBA_ERR_NO_DEVICE. */
typedef struct cba_laser_scan_options {
    int32_t axis;               /* 0: one peak per column; 1: one peak per row (default 0) */
    int32_t roi_begin, roi_end; /* positions [roi_begin, roi_end) along the search direction; 0, 0 = the whole side (default) */
    int32_t half_window;        /* samples on each side of the peak (plateau) that enter the centre of gravity (default 5) */
    double floor_level;         /* subtracted from every sample of the window (default 0) */
    double min_peak;            /* a line whose maximum is below this is invalid (default 1) */
} cba_laser_scan_options;
void cba_laser_scan_options_default(cba_laser_scan_options* o);
cba_status cba_laser_points(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                            const double plane[4], int64_t n, const double* uv /*[n][2]*/, int32_t n_frames,
                            const int64_t* frame_offset /*[n_frames + 1] or NULL*/, const double* frame_pose7 /*[n_frames][7] or NULL*/,
                            double* xyz /*[n][3]*/, double* plane_xy /*[n][2] or NULL*/);
typedef struct cba_laser_scanner cba_laser_scanner; /* opaque: camera, plane, options, device buffers sized at create, one stream */
cba_status cba_laser_scanner_create(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                                    const double plane[4], int32_t width, int32_t height, int32_t max_frames,
                                    const cba_laser_scan_options* opts, int32_t device, cba_laser_scanner** out);
cba_status cba_laser_scanner_process(cba_laser_scanner* h, int32_t n_frames, int32_t dtype, const void* images,
                                     const double* frame_pose7 /*[n_frames][7] or NULL*/, double* centre /*[n_frames][n_lines] or NULL*/,
                                     double* amplitude /*or NULL*/, double* width_px /*or NULL*/,
                                     double* xyz /*[n_frames][n_lines][3] or NULL*/);
void cba_laser_scanner_destroy(cba_laser_scanner* h);

/* ---- structured-light scanning: Gray-code and phase decode, points (no counterpart in the reference) --------------------------
 *
 * The third 3D front end: a projector and a camera.  A sequence of pattern images, taken by the camera while the projector shows
 * cba_sl_patterns, becomes a projector coordinate for every camera pixel (cba_sl_decoder_process), and with a rig set a point map.
 * A projector is calibrated as an inverse camera through the entry points that exist: decode a board's views, take the projector
 * position of every detected corner (the Python layer's projector_corners: a local homography per corner, fitted to the valid
 * pixels of the square window |du|, |dv| <= radius around rint(corner), by cba_estimate_homography_ransac_batch with opts == NULL,
 * which is the all-points DLT of cba_estimate_homography_batch), and pass them with the board coordinates to the intrinsic and rig
 * solvers.
 *
 * Options.  proj_width, proj_height in [2, CBA_IMAGE_MAX_SIDE]; axes: bit 0 = columns (decodes the projector x), bit 1 = rows (y), at
 * least one; gray_skip_bits s >= 0: the s lowest Gray bits are not projected, a stripe is 2^s projector pixels wide; phase_steps N: 0
 * = no phase patterns, else 3..8; phase_period T in integer projector pixels (used when N > 0, 1 <= T <= CBA_IMAGE_MAX_SIDE and
 * T >= 2^(s+1)); min_contrast and min_bit_diff in 0..255; min_modulation finite and >= 0.  For an axis of P projector pixels
 * nbits = max(1, ceil(log2 P)) - s, which must be >= 1.
 *
 * Sequence.  white, black, then for axis 0 and axis 1 (each only if selected): the nbits Gray planes, MSB first, each followed by
 * its inverse, then the N phase steps k = 0..N-1.  n_images = 2 + sum over the axes of (2 nbits + N) (cba_sl_image_count).
 *
 * Patterns (cba_sl_patterns: host only, no device; out [n_images][proj_height][proj_width] uint8).  Coordinates are pixel indices:
 * index j is the coordinate j.  White is 255, black 0.  Gray plane b at index j: c = j >> s, g = c ^ (c >> 1); 255 when bit
 * nbits-1-b of g is set, else 0; the inverse is 255 minus that.  Phase step k at index j: m = (j N - k T) mod (N T) in [0, N T);
 * c = cos(2 pi m / (N T)) by the C library, and c = 0 exactly when 4 m == N T or 4 m == 3 N T; the pixel is
 * floor(127.5 (1 + c) + 0.5) clamped to [0, 255].  (127.5 (1 + c) + 0.5 is an integer only for rational c; cos of a rational
 * multiple of pi is rational only at 0, +-1/2, +-1, and +-1/2 gives 191.25 and 63.75: with the exact zeros no pixel is a tie.)
 * Column patterns are constant along y, row patterns along x.
 *
 * Decode, per camera pixel, from uint8 images [n_images][height][width]; everything up to the phase sums in exact integers.
 * 1. white - black < min_contrast: status = 1 (bit 0 alone), every coordinate and modulation NaN, nothing else is evaluated.
 * 2. Per selected axis, Gray bits: for each plane with pattern p and inverse q, |p - q| < min_bit_diff sets the axis's "uncertain"
 *    bit: coordinate and modulation NaN, nothing else is evaluated for the axis.  Otherwise the bit is p > q; Gray to binary by the
 *    prefix XOR from the MSB gives c; xg = c 2^s + (2^s - 1) / 2 (exact in fp64).  xg > P - 1 sets the axis's "outside" bit:
 *    coordinate and modulation NaN.
 * 3. N == 0: the coordinate is xg, the modulation NaN.
 * 4. N > 0: ws[k] = sin(2 pi k / N), wc[k] = cos(2 pi k / N), formed once on the host in fp64 by the C library.  S = sum I_k ws[k],
 *    C = sum I_k wc[k], ascending k from 0.0, each product rounded before it is added (no contraction).
 *    modulation = (2 / N) sqrt(S S + C C), written whether or not the next test passes; modulation < min_modulation sets the axis's
 *    "low modulation" bit and the coordinate is NaN.  phi = atan2(S, C), + 2 pi when negative; f = phi T / (2 pi);
 *    kk = rint((xg - f) / T); coordinate = kk T + f.  No clamp to the projector: with T >= 2^(s+1) a stripe's half width is at most
 *    T / 4, which leaves T / 4 of phase error before the unwrap slips.
 * 5. status, one uint8: bit 0 contrast; bits 1..3 axis 0 uncertain, outside, low modulation; bits 4..6 the same for axis 1 (the
 *    bits belong to the projector axis, whichever axes are selected); 0: every selected axis is valid.  An axis's coordinate is
 *    finite exactly when its bits and bit 0 are clear.  A pixel's result depends on nothing but its own samples.
 *
 * Points.  With a rig set (cba_sl_decoder_set_rig) and both axes decoded: n_cams = 2 cameras {camera, projector} of one
 * camera_model, intr [2][10 | 12], optional inverse_coeffs [2][n_inverse_coeffs], c_T_r [2][7], all as for cba_triangulate;
 * uv_0 = (column, row), uv_1 = (x, y) of the decode, NaN where invalid.  xyz, rms_px and tri_status of the pixel are what
 * cba_triangulate's rule gives for that point (the same code): a pixel with either axis NaN has CBA_TRI_TOO_FEW and NaN.  rms_px is
 * the epipolar disagreement of the two axes and is the caller's quality gate.
 *
 * cba_sl_decoder: a handle that owns the options, one stream and device buffers sized at create for max_sequences sequences of
 * width x height images (the point buffers when the rig is first set); cba_sl_decoder_process allocates nothing.  Outputs, each
 * may be NULL: coord and modulation [n_sequences][n_axes][height][width] fp64 (the selected axes in order), status
 * [n_sequences][height][width] uint8, xyz [n_sequences][height][width][3], rms_px [..][height][width], tri_status int32.
 *
 * Errors (CBA_ERR_INVALID_ARGUMENT, all before any device work): an option outside its range; nbits < 1; T < 2^(s+1) with N > 0;
 * width or height outside [1, CBA_IMAGE_MAX_SIDE]; max_sequences < 1; max_sequences n_images width height > 2^31 - 1; n_sequences
 * outside [0, max_sequences]; NULL options, out, handle, images (for n_sequences > 0), intr, c_T_r, tri_opts; point outputs asked
 * for without a rig or with one axis only; what cba_triangulate rejects in the rig.  n_sequences == 0 is no work; otherwise no
 * device -> CBA_ERR_NO_DEVICE. */
typedef struct cba_sl_options {
    int32_t proj_width, proj_height;
    int32_t axes;           /* bit 0: columns (x), bit 1: rows (y) (default 3) */
    int32_t gray_skip_bits; /* s (default 0) */
    int32_t phase_steps;    /* N: 0 or 3..8 (default 0) */
    int32_t phase_period;   /* T (default 16) */
    int32_t min_contrast;   /* default 10 */
    int32_t min_bit_diff;   /* default 4 */
    double min_modulation;  /* default 5 */
} cba_sl_options;
typedef enum cba_sl_status_bits {
    CBA_SL_LOW_CONTRAST = 1,
    CBA_SL_X_UNCERTAIN = 2, CBA_SL_X_OUTSIDE = 4, CBA_SL_X_LOW_MODULATION = 8,
    CBA_SL_Y_UNCERTAIN = 16, CBA_SL_Y_OUTSIDE = 32, CBA_SL_Y_LOW_MODULATION = 64
} cba_sl_status_bits;
void cba_sl_options_default(cba_sl_options* o); /* proj_width and proj_height are left at 0: the caller sets them */
cba_status cba_sl_image_count(const cba_sl_options* opts, int32_t* n_images);
cba_status cba_sl_patterns(const cba_sl_options* opts, uint8_t* out /*[n_images][proj_height][proj_width]*/);
typedef struct cba_sl_decoder cba_sl_decoder; /* opaque: options, device buffers sized at create, one stream */
cba_status cba_sl_decoder_create(const cba_sl_options* opts, int32_t width, int32_t height, int32_t max_sequences, int32_t device,
                                 cba_sl_decoder** out);
cba_status cba_sl_decoder_set_rig(cba_sl_decoder* h, int32_t camera_model, const double* intr /*[2][10 | 12]*/,
                                  int32_t n_inverse_coeffs, const double* inverse_coeffs /*[2][n_inverse_coeffs] or NULL*/,
                                  const double* c_T_r /*[2][7]*/, const cba_triangulate_options* tri_opts);
cba_status cba_sl_decoder_process(cba_sl_decoder* h, int32_t n_sequences, const uint8_t* images /*[n_seq][n_images][H][W]*/,
                                  double* coord /*[n_seq][n_axes][H][W] or NULL*/, double* modulation /*same shape, or NULL*/,
                                  uint8_t* status /*[n_seq][H][W] or NULL*/, double* xyz /*[n_seq][H][W][3] or NULL*/,
                                  double* rms_px /*[n_seq][H][W] or NULL*/, int32_t* tri_status /*[n_seq][H][W] or NULL*/);
void cba_sl_decoder_destroy(cba_sl_decoder* h);

/* ---- scan registration: grid neighbour search, normals, ICP (no counterpart in the reference) ----------------------------------
 *
 * What comes after a 3D front end: the points of one view are brought into the frame of another.  Everything is fp64.  No product
 * or sum named below is contracted into an FMA (as in cba_laser_points), so a restatement in IEEE operations can be held to the
 * bit.  An invalid point is one with a non-finite coordinate, which is how every front end here marks one.
 *
 * 1. cba_point_normals: normals of organised point maps xyz [n_maps][height][width][3] (what the stereo, SGM and structured-light
 *    handles write) -> normals of the same shape.  viewpoint [3], NULL = the origin; max_jump > 0, +inf allowed.  Per pixel with a
 *    valid centre P; a neighbour "qualifies" when it is inside the map, valid and ((ex ex + ey ey) + ez ez) <= max_jump max_jump with
 *    e = neighbour - P.
 *    Horizontal difference dx: P(x+1) - P(x-1) when both qualify; else P(x+1) - P when the right one does; else P - P(x-1) when the
 *    left one does; else there is no normal.  Vertical difference dy: the same with the row below (y+1) in the place of the right
 *    neighbour and the row above in the place of the left one.
 *    n = dx x dy, each component a b - c d with both products rounded: (dx_y dy_z - dx_z dy_y, dx_z dy_x - dx_x dy_z,
 *    dx_x dy_y - dx_y dy_x); len = sqrt((nx nx + ny ny) + nz nz); a len that is zero or non-finite gives no normal; n = n / len
 *    (three divisions).  Orientation: v = viewpoint - P, s = (nx vx + ny vy) + nz vz; n is negated when s < 0 and left as it is
 *    when s >= 0.  No normal: NaN in all three coordinates.  A pixel's result depends only on its own 5-point cross.
 *
 * 2. cba_cloud_index: a uniform grid over a target cloud xyz [n][3] (1 <= n <= 2^31 - 1, at least one valid point) with optional
 *    normals [n][3], built once on the device by cba_cloud_index_create; the handle owns one stream and all device buffers.  Invalid
 *    points are skipped but keep their indices.  lo, hi: the exact minima and maxima of the valid points; cells along axis k:
 *    n_k = floor((hi_k - lo_k) / cell_size) + 1; n_x n_y n_z may not exceed CBA_CLOUD_MAX_CELLS: beyond that create fails with a
 *    message that names a cell size that fits (there is no silent coarsening).  The cell of a coordinate is
 *    c_k = min(n_k - 1, (int)floor((p_k - lo_k) / cell_size)): one subtraction, one division.  Cells are numbered x fastest.  Build:
 *    a count per cell (integer atomics, independent of arrival order), an exclusive scan over the cells, a scatter of 32-byte records
 *    {x, y, z, original index} into cell order, the normals into a parallel array.  The order of the points inside a cell may
 *    depend on arrival; no result does (the tie rule below).  Float atomics are used nowhere.
 *
 * 3. cba_cloud_nearest: for each query [m][3] the nearest valid target point within max_distance, 0 < max_distance <=
 *    0.999 cell_size (the product rounded).  The result is, to the bit, brute force over all valid target points y: d = q - y per
 *    coordinate, d2 = ((dx dx + dy dy) + dz dz); the smallest d2 with d2 <= max_distance max_distance wins, equal d2 goes to the
 *    lowest original index; index [m] int64 receives the original index and dist2 [m] (optional) d2.  None, or an invalid query:
 *    index -1 and dist2 NaN.  A query with lo_k - q_k > max_distance or q_k - hi_k > max_distance on an axis (the differences
 *    rounded) returns -1 without touching the grid: every d2 is then above the bar, and the test keeps the cell arithmetic of the
 *    others inside [-1, n_k].  Otherwise the cells c_k - 1 .. c_k + 1 of the query's unclamped c_k, cut to the grid, are searched:
 *    9 runs of the sorted records.  The 0.1 % covers the rounding of the two quotients (at most about 2^-28 of a cell at the largest
 *    grid), so this neighbourhood holds every point within the radius.
 *
 * 4. cba_cloud_register: ICP of n_sources point sets onto the index.  Source i is source_xyz[source_offset[i] ..
 *    source_offset[i+1]); init_pose7 [n_sources][7] = [qw qx qy qz tx ty tz] maps source to target, NULL = identities; its quaternion
 *    is normalised once on entry: |q| = sqrt(((w w + x x) + y y) + z z), four divisions; zero or non-finite is an argument error.
 *    R of a unit q: xx = x x, ... wz = w z; R00 = 1 - 2 (yy + zz), R01 = 2 (xy - wz), R02 = 2 (xz + wy), R10 = 2 (xy + wz),
 *    R11 = 1 - 2 (xx + zz), R12 = 2 (yz - wx), R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = 1 - 2 (xx + yy).
 *    The system at a pose (q, t): for every valid source point p, in index order: Q_i = ((R_i0 p_0 + R_i1 p_1) + R_i2 p_2) + t_i;
 *    j = the neighbour of Q by rule 3 with opts->max_distance; none: no pair; metric 0 and a NaN normal at j: no pair.
 *    Metric 0 (point to plane): e = Q - y_j, r = (n_0 e_0 + n_1 e_1) + n_2 e_2, J = [Q_1 n_2 - Q_2 n_1, Q_2 n_0 - Q_0 n_2,
 *    Q_0 n_1 - Q_1 n_0, n_0, n_1, n_2].  Metric 1 (point to point): three rows, r = Q_0 - y_0 with J = [0, Q_2, -Q_1, 1, 0, 0], then
 *    r = Q_1 - y_1 with [-Q_2, 0, Q_0, 0, 1, 0], then r = Q_2 - y_2 with [Q_1, -Q_0, 0, 0, 0, 1].  H = sum J^T J (21 distinct
 *    entries, mirrored into H[36], row-major), g = sum J^T r, ss = sum r r, n_pairs counts pairs (not rows).
 *    Iteration: form the system.  n_pairs < min_pairs ends with CBA_ICP_TOO_FEW (values of min_pairs below 6 for metric 0 or 3 for
 *    metric 1 mean 6 or 3).  iterations == max_iterations ends with CBA_ICP_NOT_CONVERGED (so max_iterations = 0 gives the statistics
 *    at the initial pose).  Solve H xi = -g by unpivoted 6 x 6 Cholesky, xi = (omega, v): row k has d = H_kk - sum_j<k L_kj L_kj; the
 *    solve fails unless d > 1e-12 H_kk (scale-free; a single plane under metric 0 ends here), and a failed solve ends with
 *    CBA_ICP_DEGENERATE.  Update: th = |omega| = sqrt((w0 w0 + w1 w1) + w2 w2); dq = [cos(th/2), (sin(th/2) / th) omega], the identity
 *    when th == 0; q <- (dq (x) q) / |dq (x) q| (Hamilton product, each component summed left to right in w, x, y, z order of dq);
 *    t <- R(dq) t + v by the forms of R and Q above.  iterations counts the updates.  The update with th <= step_tolerance and
 *    |v| <= step_tolerance extent (extent: the length of the index's box diagonal, ((ex ex + ey ey) + ez ez) under the root) is the
 *    last one and gives CBA_ICP_OK; otherwise the max_iterations-th update is the last one and gives CBA_ICP_NOT_CONVERGED.  After
 *    the last update the system is formed once more, for the statistics alone.  In every case rms = sqrt(ss / n_pairs) (NaN when
 *    n_pairs == 0), n_pairs, H and g are those of the system at the returned pose.
 *    A source's result depends on nothing but its own points and pose: not on the other sources of the call, not on how the device
 *    splits the work; two calls give the same bits.  (Sums are added in a fixed order: per lane in index order with a fixed stride,
 *    a fixed tree inside the wave and the workgroup, then the workgroups of a source in order.)  The sine and cosine of the update
 *    are the device's.
 *
 * Errors (CBA_ERR_INVALID_ARGUMENT, all before any device work): NULL xyz, normals (the output of cba_point_normals), out, handle,
 * query, index, source_offset, source_xyz, opts, results where one is needed; n_maps < 0, width or height outside
 * [1, CBA_IMAGE_MAX_SIDE], n_maps width height > 2^31 - 1; max_jump not > 0; n outside [1, 2^31 - 1]; cell_size not finite and > 0;
 * no valid target point; too many cells; m < 0; max_distance not finite, not > 0 or above 0.999 cell_size; n_sources < 0; offsets
 * that decrease, do not start at 0 or give a source more than 2^31 - 1 points; a metric other than 0 or 1; metric 0 on an index
 * without normals; max_iterations outside [0, CBA_ICP_MAX_ITERATIONS]; step_tolerance not finite or < 0; a bad initial quaternion.
 * n_maps == 0, m == 0 and n_sources == 0 are no work; otherwise no device -> CBA_ERR_NO_DEVICE. */
#define CBA_CLOUD_MAX_CELLS (1 << 24)
#define CBA_ICP_MAX_ITERATIONS 10000
typedef struct cba_icp_options {
    int32_t metric;         /* 0: point-to-plane (the index must hold normals), 1: point-to-point (default 0) */
    double max_distance;    /* correspondence gate, as in cba_cloud_nearest (no default: the caller sets it) */
    int32_t max_iterations; /* default 30; 0: only the statistics at the initial pose */
    double step_tolerance;  /* default 1e-9 */
    int32_t min_pairs;      /* default 6; values below 6 (plane) or 3 (point) mean 6 or 3 */
} cba_icp_options;
typedef enum cba_icp_status { CBA_ICP_OK = 0, CBA_ICP_NOT_CONVERGED = 1, CBA_ICP_TOO_FEW = 2, CBA_ICP_DEGENERATE = 3 } cba_icp_status;
typedef struct cba_icp_result {
    double pose7[7];
    double rms;
    double H[36];
    double g[6];
    int64_t n_pairs;
    int32_t iterations;
    int32_t status; /* cba_icp_status */
} cba_icp_result;
cba_status cba_point_normals(int32_t n_maps, int32_t height, int32_t width, const double* xyz /*[n_maps][height][width][3]*/,
                             const double* viewpoint /*[3] or NULL*/, double max_jump, double* normals /*[n_maps][height][width][3]*/);
typedef struct cba_cloud_index cba_cloud_index; /* opaque: the grid, the sorted target, the buffers of its calls, one stream */
cba_status cba_cloud_index_create(int64_t n, const double* xyz /*[n][3]*/, const double* normals /*[n][3] or NULL*/, double cell_size,
                                  int32_t device, cba_cloud_index** out);
cba_status cba_cloud_nearest(cba_cloud_index* h, int64_t m, const double* query /*[m][3]*/, double max_distance, int64_t* index /*[m]*/,
                             double* dist2 /*[m] or NULL*/);
void cba_icp_options_default(cba_icp_options* o); /* max_distance is left at 0: the caller sets it */
cba_status cba_cloud_register(cba_cloud_index* h, int32_t n_sources, const int64_t* source_offset /*[n_sources + 1]*/,
                              const double* source_xyz /*[m][3]*/, const double* init_pose7 /*[n_sources][7] or NULL*/,
                              const cba_icp_options* opts, cba_icp_result* results /*[n_sources]*/);
void cba_cloud_index_destroy(cba_cloud_index* h);

/* ---- alignment of many scans: ICP over a graph of scans (no counterpart in the reference) ---------------------------------------
 *
 * What comes between registration and fusion: the poses of N scans are made consistent with each other over a caller's list of
 * overlapping pairs, all at once, with one pose held.  It is a bundle adjustment whose observations are ICP pairs.  "Rule 2, 3, 4"
 * below are those of the registration block above; everything is fp64 and nothing is contracted into an FMA.
 *
 * The set (cba_cloud_set_create): 2 <= n_scans <= CBA_ALIGN_MAX_SCANS; scan k is xyz[offset[k] .. offset[k+1]) with optional normals
 * of the same layout.  Every scan gets a grid of its own by rule 2 (its own lo, hi and cell counts; one cell_size for all), built on
 * the device by the kernels of cba_cloud_index; every scan needs a valid point and at most CBA_CLOUD_MAX_CELLS cells (the message
 * names a cell size that fits).  The set also keeps each scan's points in their original order: they are the sources.  One stream,
 * one device, all buffers owned by the handle.  extent: the largest box diagonal of the scans, each by rule 4's form.
 *
 * cba_cloud_align: pose7 [n_scans][7] receives poses that map each scan into the common frame.  init_pose7 [n_scans][7], NULL =
 * identities, quaternions normalised once on entry by rule 4.  edges [n_edges][2] = (source a, target b), a != b; duplicates and
 * both directions are allowed and count separately.  The pose of scan opts->fixed never changes.
 *
 * A round at poses T_k = (q_k, t_k), R_k by rule 4:
 * 1. Per edge (a, b): R_ab[i][k] = (R_b[0][i] R_a[0][k] + R_b[1][i] R_a[1][k]) + R_b[2][i] R_a[2][k]; d = t_a - t_b;
 *    t_ab[i] = (R_b[0][i] d_0 + R_b[1][i] d_1) + R_b[2][i] d_2 (with T_b the identity these are R_a and t_a).  The edge's system is
 *    rule 4's system of scan a's valid points, in index order, at (R_ab, t_ab) against scan b's grid and normals with
 *    icp.max_distance and icp.metric: H_e [36], g_e [6], ss_e, n_pairs_e.  Its sums are added in exactly cba_cloud_register's order,
 *    so with T_b the identity they are, to the bit, what that call returns for scan a on an index of scan b at max_iterations = 0 from
 *    T_a.  The edge is used when n_pairs_e >= min_pairs (rule 4's floor of 6 or 3).
 * 2. Totals over the used edges in list order: ss, n_pairs, n_used_edges.  No used edge ends with CBA_ICP_TOO_FEW.
 *    iterations == max_iterations ends with CBA_ICP_NOT_CONVERGED.
 * 3. Assembly.  Under the left updates of rule 4 the relative pose moves by A_b (xi_a - xi_b), A_b = Ad(T_b^-1) on (omega, v), 6 x 6
 *    row-major with R = R_b, t = t_b: A[i][k] = A[3+i][3+k] = R[k][i]; A[i][3+k] = 0; A[3+i][0] = R[2][i] t_1 - R[1][i] t_2;
 *    A[3+i][1] = R[0][i] t_2 - R[2][i] t_0; A[3+i][2] = R[1][i] t_0 - R[0][i] t_1 (i, k = 0..2; each product rounded).
 *    B = H_e A, M = A^T B, c = A^T g_e: B[k][j] = sum_l H_e[k][l] A[l][j], M[i][j] = sum_k A[k][i] B[k][j], c[i] = sum_k A[k][i]
 *    g_e[k], every sum left to right over 0..5 from its first product (so A = I gives M = H_e and c = g_e exactly).  Per used edge,
 *    in list order: +M onto the blocks (a, a) and (b, b), -M onto (a, b) and -M^T onto (b, a), +c onto g_a, -c onto g_b of the
 *    6 n_scans wide system.  Every entry receives its contributions in edge order.
 * 4. Solve.  The rows and columns of `fixed` are deleted; the width is n = 6 (n_scans - 1) <= 378.  H xi = -g by rule 4's unpivoted
 *    Cholesky at width n: row k has d = H_kk - sum_j<k L_kj L_kj, every chain sequential in j from 0, forward and back substitution
 *    in rule 4's order; the solve fails unless every d > 1e-12 H_kk, and a failed solve ends with CBA_ICP_DEGENERATE (no pose is
 *    touched).  This is how a scan that no used edge connects to `fixed` is reported.
 * 5. Update: every scan but `fixed` by rule 4's update with its own xi (the device's sine and cosine).  iterations counts the rounds
 *    with an update.  The round after which every scan has th <= step_tolerance and |v| <= step_tolerance extent is the last and
 *    gives CBA_ICP_OK; otherwise the max_iterations-th is the last and gives CBA_ICP_NOT_CONVERGED.  The iteration can enter a
 *    two-cycle in which one pair flips between two neighbours for ever, so CBA_ICP_NOT_CONVERGED at the cap is a normal ending.
 * 6. After the last update the edge systems are formed once more: edge_out [n_edges] (optional: H, g, ss, n_pairs, used of every
 *    edge), rms = sqrt(ss / n_pairs) (NaN without pairs), n_pairs and n_used_edges are those of the returned poses, in every status.
 * A result depends on the scans, the edge list in its order, the poses and the options, not on how the device splits the work; two
 * calls give the same bits; an edge's edge_out does not depend on the other edges of the call.
 *
 * Errors (CBA_ERR_INVALID_ARGUMENT, all before any device work): NULL out, offset, xyz, handle, opts, pose7, result, edges (with
 * n_edges > 0); n_scans outside [2, CBA_ALIGN_MAX_SCANS]; offsets that decrease, do not start at 0 or give a scan more than
 * 2^31 - 1 points; cell_size not finite and > 0; a scan without a valid point; a scan with too many cells; n_edges outside
 * [0, CBA_ALIGN_MAX_EDGES]; a scan number out of range; a == b; fixed out of range; the icp checks of rule 4 (metric 0 on a set
 * without normals among them; max_distance against the set's cell_size); a bad initial quaternion.  n_edges == 0 is no work: the
 * (normalised) poses are copied, the status is CBA_ICP_TOO_FEW, rms is NaN. */
#define CBA_ALIGN_MAX_SCANS 64
#define CBA_ALIGN_MAX_EDGES 1024
typedef struct cba_cloud_set cba_cloud_set; /* opaque: the scans, their grids, the buffers of its calls, one stream */
cba_status cba_cloud_set_create(int32_t n_scans, const int64_t* offset /*[n_scans + 1]*/, const double* xyz /*[m][3]*/,
                                const double* normals /*[m][3] or NULL*/, double cell_size, int32_t device, cba_cloud_set** out);
typedef struct cba_align_options {
    cba_icp_options icp;
    int32_t fixed; /* the scan whose pose is held (default 0) */
} cba_align_options;
typedef struct cba_align_edge {
    double H[36];
    double g[6];
    double ss;
    int64_t n_pairs;
    int32_t used;
} cba_align_edge;
typedef struct cba_align_result {
    double rms;
    int64_t n_pairs;
    int32_t n_used_edges;
    int32_t iterations; /* rounds with an update */
    int32_t status;     /* cba_icp_status */
} cba_align_result;
void cba_align_options_default(cba_align_options* o); /* cba_icp_options_default and fixed = 0 */
cba_status cba_cloud_align(cba_cloud_set* h, int32_t n_edges, const int32_t* edges /*[n_edges][2]: source, target*/,
                           const double* init_pose7 /*[n_scans][7] or NULL*/, const cba_align_options* opts,
                           double* pose7 /*[n_scans][7]*/, cba_align_edge* edge_out /*[n_edges] or NULL*/, cba_align_result* result);
void cba_cloud_set_destroy(cba_cloud_set* h);

/* ---- scan fusion: a truncated signed distance volume from depth maps, surface points (no counterpart in the reference) ---------
 *
 * What comes after registration: the views of one object, each with its pose, are merged into one surface.  Storage is float32;
 * every decision and every arithmetic step is fp64, rounded once on store; no product or sum named below is contracted into an
 * FMA, so a restatement in IEEE operations can be held to the bit.
 *
 * 1. The volume: nx, ny, nz, each in [2, 1024], nx ny nz <= CBA_TSDF_MAX_VOXELS.  Lattice point (i, j, k) lies at
 *    X = (ox + i vs, oy + j vs, oz + k vs) with origin o and vs = voxel_size: the product rounded, then the sum.  A voxel holds D
 *    (float32, starts at 1) and W (float32, starts at 0).  The linear order is x fastest: l = (k ny + j) nx + i.
 *
 * 2. cba_tsdf_integrate: one camera (camera_model and intr [10 | 12] as cba_camera_project takes them), n_maps depth maps
 *    depth [n_maps][height][width], fp64, holding z in the camera frame (a value that is non-finite or <= 0 is invalid), and
 *    c_T_v [n_maps][7], pose7 rows = [qw qx qy qz tx ty tz] that map the volume frame to the camera; R of a row is built as
 *    cba_triangulate builds it (the quaternion as it is, no normalisation).  Maps are applied in order m = 0, 1, ...; each voxel goes
 *    through these steps for each map:
 *      1. P_r = ((R_r0 X_0 + R_r1 X_1) + R_r2 X_2) + t_r.
 *      2. Skip unless P_2 > 0 and the model's denominator is > 0 (P_2 for the pinhole, n_sensor . P for Scheimpflug).
 *      3. (u, v) by cba_camera_project's arithmetic; px = floor(u + 0.5), py = floor(v + 0.5), in fp64.  Skip unless
 *         0 <= px <= width - 1 and 0 <= py <= height - 1 (comparisons that are false for NaN).
 *      4. d = depth[m][py][px].  Skip unless d is finite, d > 0 and d <= max_depth.
 *      5. s = d - P_2.  Skip when s < -truncation.  f = s / truncation, and f = 1 when f > 1.
 *      6. D <- float32((double(W) double(D) + f) / (double(W) + 1)); W <- float32(min(double(W) + 1, max_weight)).
 *    A voxel's result depends only on its own position and the maps, taken in order: not on the batch (one call with seven maps
 *    gives the bits of seven calls with one map each), not on how the device splits the work, not on the other voxels.
 *
 * 3. cba_tsdf_extract(h, min_weight, &n_points): the zero crossings on lattice edges.  Voxels are visited in ascending l; at each
 *    voxel the +x, +y and +z edges in that order; an edge is absent on the grid's last plane along its axis.  With a the voxel and
 *    b the neighbour at the other end: the edge qualifies when W_a >= min_weight, W_b >= min_weight and (D_a < 0) != (D_b < 0)
 *    (so -0.0 counts as non-negative).  t = D_a / (D_a - D_b) in fp64; the point is X_a with t vs (the product rounded) added along
 *    the axis.  The normal: for v in {a, b}, g_c(v) = D(v + e_c) - D(v - e_c) for c = x, y, z, where every neighbour used must be
 *    inside the grid and have W > 0; n_c = g_c(a) + t (g_c(b) - g_c(a)); len = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2); n / len by three
 *    divisions.  There is no normal (NaN in all three components, the point is kept) when a neighbour is missing or len is zero or
 *    non-finite.  D is positive in observed free space, so the normal points from the surface into it: the side cba_point_normals
 *    orients towards.  The output order is the visiting order.  The points and normals stay on the device until
 *    cba_tsdf_extract_fetch(h, xyz [n_points][3], normals [n_points][3] or NULL) copies those of the last extract out.
 *
 * 4. cba_tsdf_mesh(h, min_weight, &n_points, &n_triangles): rule 3's extract with min_weight, then triangles over its points.  The
 *    vertices of the mesh are exactly the points of the extract, so the mesh is an index list: no second vertex set, no welding.
 *    No table of cases is typed in anywhere: the triangles of a cell follow from the rule below, which a few lines of code evaluate
 *    for all 256 sign patterns (tsdf_mesh_math.hpp does so at compile time).  Every output is an integer.
 *
 *    Cell.  Cell (i, j, k), 0 <= i < nx - 1, 0 <= j < ny - 1, 0 <= k < nz - 1, has corners q = dx + 2 dy + 4 dz at lattice point
 *    (i + dx, j + dy, k + dz).  A cell is live when all eight corners have W >= min_weight; every sign-changing edge of a live cell
 *    is therefore a point of rule 3's extract at the same min_weight.  case = sum_q (D_q < 0) 2^q: rule 3's sign test, so -0.0 is
 *    non-negative.  Cases 0 and 255 give nothing.
 *
 *    Local edges.  e = 4 axis + u + 2 v, where (u, v) are the offsets of the edge's lower end along the other two axes in ascending
 *    axis order: x edges 0..3 have (u, v) = (dy, dz), y edges 4..7 have (dx, dz), z edges 8..11 have (dx, dy).  Local edge e of
 *    cell (i, j, k) is the extract's point (voxel at its lower end, axis).
 *
 *    Faces.  The face across axis a on side s (the plane where coordinate a of the corners is s) has its four corners taken in the
 *    cycle (b, c) = (0,0), (1,0), (1,1), (0,1) with b = (a + 1) mod 3 and c = (a + 2) mod 3.  For s = 1 this cycle is
 *    counter-clockwise seen from outside the cell; for s = 0 the cycle is reversed.  Every maximal run of negative corners in a
 *    face's cycle gives one directed segment, FROM the edge on which the cycle enters the run (positive -> negative) TO the edge on
 *    which it leaves the run (negative -> positive).  A face whose two diagonal corners are negative has two runs and so two
 *    segments: negative corners are cut off separately.  The rule reads only the face's four signs, so the two cells that share a
 *    face draw the same segments in opposite directions.
 *
 *    Loops and triangles.  In a cell every crossing edge is the tail of exactly one segment and the head of exactly one, so the
 *    segments form disjoint closed loops.  Loops are taken in ascending order of their lowest local edge; each loop starts at its
 *    lowest edge and is followed along the segments: e_0, e_1, ..., e_(n-1).  Its triangles are (e_0, e_i, e_(i+1)) for
 *    i = 1 .. n - 2.  With this direction (p_1 - p_0) x (p_2 - p_0) points into positive D: the side rule 3's normals point to.
 *
 *    Output.  Cells are visited in ascending l of corner 0, the triangles of a cell in the order above.  A triangle is three int32
 *    indices into the extract's point list (n_points <= 3 2^28 and n_triangles <= 5 2^28, both < 2^31).  The order is a property
 *    of the volume and min_weight: it does not depend on the launch, and no atomic is used.  Afterwards cba_tsdf_extract_fetch
 *    returns the mesh's vertices and normals and cba_tsdf_mesh_fetch(h, triangles [n_triangles][3]) its triangles.  A later
 *    cba_tsdf_extract, cba_tsdf_integrate, cba_tsdf_upload or cba_tsdf_reset does not touch arrays already fetched, but
 *    invalidates the handle's mesh: cba_tsdf_mesh_fetch then fails until the next cba_tsdf_mesh.  n_triangles == 0 is a valid
 *    result.  An allocation failure leaves the handle usable and without a mesh.
 *
 *    What the rule gives, for all 256 cases: closed loops in each of the 254 non-trivial ones; at most 4 loops in a cell, at most
 *    7 edges in a loop, at most 5 triangles in a cell; 820 triangles in all, {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32} cases per
 *    triangle count.  Case 1 -> (0, 4, 8); case 5 -> (0, 1, 10), (0, 10, 8); case 0x69 -> (0,4,8), (1,5,11), (2,7,9), (3,6,10);
 *    case 0x96 -> (0,9,5), (1,10,4), (2,8,6), (3,11,7).  A case fits one 64-bit word (15 four-bit edge numbers and a count), the
 *    whole table 2 KiB.
 *
 *    Guarantees.  Over live cells the directed half-edges balance, count(u -> v) = count(v -> u), except on faces shared with a
 *    cell that is not live or lies outside the grid, where the mesh has a boundary; on a random sign field this balance holds with
 *    half-edge multiplicity up to 2.  The surface can be non-manifold along a fan diagonal, as with classic marching cubes.  On
 *    smooth fields (a sphere, a torus of a few voxels' radius) it is a closed oriented 2-manifold.  A corner with D exactly +-0
 *    against negative neighbours gives t = 0 and zero-area triangles (a sphere of radius 6 voxels centred on a lattice point: 96
 *    of its 1304); they are kept.  Points of the extract that no live cell touches stay in the point list, unreferenced.
 *
 * 5. cba_tsdf_raycast(h, camera_model, intr, n_views, height, width, poses [n_views][7], opts): what a camera at each pose sees of
 *    the model: depth, camera-frame points and normals per pixel, organised as the front ends write their maps.  Only + - * /
 *    sqrt floor and comparisons are used, each rounded once in the order written; min(a, b) is a < b ? a : b and max(a, b) is
 *    a > b ? a : b.
 *
 *    Options {step, skip, near_depth, far_depth, min_weight}, defaults {0, 0.5, 0, +inf, 1}.  step_eff = step > 0 ? step :
 *    0.5 voxel_size.  Argument errors: step not 0 and not in [voxel_size / 16, +inf), or non-finite; skip not in [0, 1];
 *    near_depth not >= 0 or non-finite; far_depth not > near_depth (NaN included); min_weight not >= 1.  The lower bound on step
 *    and the guards of the march are what make every ray end.
 *
 *    Rays.  Pixel (col, row) of a height x width view has the ray (x, y) = cba_camera_unproject's arithmetic at u = col, v = row
 *    (the iterative undistortion; no inverse coefficients).  It is computed once per pixel and call and kept as a table
 *    rays [height][width][2] that can be fetched; the unprojection is not reproducible to the bit between compilers, so
 *    everything below is a function of the table's stored values.  A pixel whose x or y is non-finite has status 3 (NO_RAY).
 *
 *    View.  R and t of a pose as rule 2 takes them (volume frame -> camera).  Centre c_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2);
 *    direction d_r = (R_0r x + R_1r y) + R_2r.  The point at parameter z is p_r = c_r + z d_r (the product rounded, then the sum):
 *    z is the camera-frame depth.
 *
 *    Range.  z0 = near_depth, z1 = far_depth.  For each axis a with lo = o_a and hi = o_a + (n_a - 1) vs (rule 1's position): if
 *    d_a == 0 the ray is a miss when c_a < lo or c_a > hi, and otherwise the axis sets no bound; else ta = (lo - c_a) / d_a,
 *    tb = (hi - c_a) / d_a, z0 = max(z0, min(ta, tb)), z1 = min(z1, max(ta, tb)).  The ray is a miss unless z0 <= z1 (false for NaN).
 *
 *    Sample at z.  g_a = (p_a - o_a) / vs.  The sample is invalid unless 0 <= g_a <= n_a - 1 for every axis (false for NaN; decided
 *    before any conversion to an integer).  i_a = min(floor(g_a), n_a - 2), f_a = g_a - i_a.  The sample is invalid unless all eight
 *    voxels of cell i have W >= min_weight.  F is the trilinear value with lerp(a, b, t) = a + t (b - a): four lerps along x for
 *    (y, z) = (0,0), (1,0), (0,1), (1,1), two along y, one along z.  No address outside the stored volume is formed.
 *
 *    March.  z = z0, "previous" = invalid, count = 0.  Loop:
 *      1. Sample at z; count += 1.
 *      2. If the sample is valid and F < 0: previous valid with F_prev >= 0 -> HIT (1) with
 *         z_hit = z_prev + (z - z_prev) (F_prev / (F_prev - F)), end; previous invalid -> BEHIND (2), end (the ray enters observed
 *         space inside a surface).
 *      3. If the sample is valid, F >= 0, and the previous sample was valid with F_prev < 0 -> BEHIND, end.
 *      4. adv = step_eff for an invalid sample, max(step_eff, (skip F) truncation) otherwise (step_eff when that product is NaN).
 *      5. z_next = z + adv.
 *      6. The ray ends as MISS (0) when not z_next <= z1, or not z_next > z (no progress at a large z), or
 *         count == CBA_TSDF_RAY_MAX_SAMPLES.
 *      7. The current sample becomes "previous"; z = z_next.
 *    "Negative" is F < 0 throughout: -0.0 and 0 count as positive, as in rule 3.
 *
 *    Outputs of a hit.  depth = z_hit; xyz = (x z_hit, y z_hit, z_hit) in the camera frame.  Normal: F sampled at p_hit +- vs e_a
 *    for the three axes (six samples by the rule above, the same min_weight); n_a = F(+) - F(-); len = sqrt((n_0 n_0 + n_1 n_1) +
 *    n_2 n_2).  If any of the six is invalid, or len is not > 0 or not finite, the normal is NaN in all three components and the
 *    hit stays a hit.  Otherwise m = n / len by three divisions and the camera-frame normal is (R_r0 m_0 + R_r1 m_1) + R_r2 m_2:
 *    it points into positive D, as rule 3's normals do.  Every pixel that is no hit has NaN in depth, xyz and normals.
 *
 *    Every output is a function of the volume, the rays table, the pose and the options alone: not of the launch, the batch (n
 *    views in one call give the bits of n calls), or what ran before.  The results stay in the handle until
 *    cba_tsdf_raycast_fetch(h, depth [n_views][height][width], xyz [..][3], normals [..][3], status uint8 [..],
 *    rays [height][width][2]) copies them out; each pointer may be NULL.  The ray cast reads the volume and writes only its own
 *    buffers: it does not invalidate the handle's extract or mesh, and a later integrate, upload, reset, extract or mesh does not
 *    invalidate its results.  n_views == 0 is no work and leaves earlier results as they are, as does every argument error.
 *
 * Colour.  Every voxel has a second record {R, G, B, Wc}: four float32, all zeros at first, in a volume of its own that the first
 * cba_tsdf_integrate_colour or cba_tsdf_colour_upload on a handle allocates.  A handle that makes neither call allocates nothing for
 * colour and behaves in every call as stated above; an allocation failure leaves the handle usable and without colour.  Channels
 * are kept as running means of byte values, so a mean of mixed exposures stays a mean: no gamma, no clamping before the output.
 *
 * 6. cba_tsdf_integrate_colour(h, camera_model, intr, n_maps, height, width, depth, rgba, c_T_v): rule 2 with the camera's image
 *    behind each depth map.  rgba is uint8 [n_maps][height][width][4] = {R, G, B, A} on the depth map's pixel grid; A == 0 means
 *    "this pixel has no colour" (every other A counts alike).  Steps 1 to 6 of rule 2 run unchanged: D and W after the call are,
 *    to the bit, those of cba_tsdf_integrate with the same depth and poses.  Then, only for a voxel that step 6 updated through
 *    map m:
 *      7. Skip unless s <= truncation (the s of step 5) and A(m, py, px) != 0.  Otherwise, with c = double(byte) per channel and
 *         the Wc from before this step, C <- float32((double(Wc) double(C) + c) / (double(Wc) + 1)) for R, G and B; then
 *         Wc <- float32(min(double(Wc) + 1, max_weight)).
 *    s <= truncation keeps the colour of a voxel that lies in observed free space in front of the band: what a pixel shows there
 *    is the surface behind the voxel, seen from one side only.  Voxels with s < -truncation never reach step 7.  Inside the band
 *    the mean is the plain one up to max_weight samples and a moving one after, as D's is.  A voxel's colour depends only on its
 *    position and the maps in order: not on the batch, the launch or the other voxels.  cba_tsdf_integrate on a handle with
 *    colour leaves the colour volume as it is.
 *
 * 7. The colour of an extract's point: cba_tsdf_extract and cba_tsdf_mesh on a handle that has colour at the time of the call also
 *    give every point a colour, uint8 [n_points][4] in the order of the points.  With a, b and t of rule 3: when Wc_a > 0 and
 *    Wc_b > 0, C = C_a + t (C_b - C_a) per channel (the product rounded, then the sum); when one end alone has Wc > 0, that end's
 *    C; otherwise the point has no colour.  A channel's byte is q = floor(C + 0.5), 0 when q < 0 or C is NaN, 255 when q > 255.
 *    A = 255 where there is a colour; where there is none, R = G = B = A = 0.  cba_tsdf_extract_fetch_colour(h, rgba) copies them
 *    out; it fails when the last extract or mesh ran on a handle without colour.
 *
 * 8. The colour of a ray cast's hit: cba_tsdf_raycast on a handle that has colour at the time of the call also gives every pixel
 *    a colour, uint8 [n_views][height][width][4].  For a pixel with status HIT: p_hit = c + z_hit d from the stored depth, the
 *    rays table and the pose by rule 5's "View" arithmetic; g_a, i_a and f_a of p_hit by rule 5's "Sample at z".  There is a colour
 *    only when every g_a is in range and all eight voxels of cell i have Wc > 0 (the weight W is not asked again); then each
 *    channel is the trilinear value in rule 5's lerp order, made a byte as in rule 7, and A = 255.  Every other pixel is
 *    {0, 0, 0, 0}.  The result is a function of the ray cast's stored outputs and the colour volume alone.
 *    cba_tsdf_raycast_fetch_colour(h, rgba) copies it out; it fails when the last ray cast ran on a handle without colour.
 *
 * cba_tsdf_has_colour(h, &out) gives 1 or 0.  cba_tsdf_colour_fetch(h, colour [nz][ny][nx][4]) copies the records out (an error on a
 * handle without colour) and cba_tsdf_colour_upload writes them, allocating the colour volume where there is none (a saved volume
 * restored; the values are taken as they are); like cba_tsdf_upload it invalidates the handle's mesh.  cba_tsdf_reset also zeroes
 * an existing colour volume.  cba_tsdf_integrate_colour has the argument errors of cba_tsdf_integrate and NULL rgba for n_maps > 0;
 * n_maps == 0 is no work and allocates nothing.
 *
 * cba_tsdf_fetch copies the dense [nz][ny][nx] planes of D and W out and cba_tsdf_upload writes them (a saved volume restored; the
 * values are taken as they are); either pointer may be NULL.  cba_tsdf_reset restores D = 1 and W = 0.  The handle owns one stream
 * and all of its device buffers; every call ends synchronised.  Float atomics are used nowhere.
 *
 * Errors (CBA_ERR_INVALID_ARGUMENT, all before any device work): NULL origin, opts, out, handle, intr, n_points, depth or c_T_v for
 * n_maps > 0, xyz for n_points > 0; a side outside [2, 1024] or nx ny nz > CBA_TSDF_MAX_VOXELS; voxel_size, truncation or origin not
 * finite, voxel_size or truncation not > 0; max_weight outside [1, 2^24] or not an integer value; max_depth not > 0; an unknown
 * camera model, fx or fy equal to 0; n_maps < 0; width or height outside [1, CBA_IMAGE_MAX_SIDE]; a zero or non-finite quaternion;
 * min_weight not >= 1; cba_tsdf_extract_fetch before any extract; NULL n_triangles; NULL triangles for n_triangles > 0;
 * cba_tsdf_mesh_fetch without a valid mesh; for cba_tsdf_raycast the camera, side and pose errors of cba_tsdf_integrate, n_views < 0,
 * n_views height width > CBA_TSDF_MAX_RAYS and rule 5's option errors; cba_tsdf_raycast_fetch before any ray cast.  n_maps == 0 is
 * no work; create without a device -> CBA_ERR_NO_DEVICE. */
#define CBA_TSDF_MAX_VOXELS (1 << 28)
#define CBA_TSDF_MAX_RAYS (1 << 26)
#define CBA_TSDF_RAY_MAX_SAMPLES 65536
#define CBA_TSDF_RAY_MISS 0
#define CBA_TSDF_RAY_HIT 1
#define CBA_TSDF_RAY_BEHIND 2
#define CBA_TSDF_RAY_NO_RAY 3
typedef struct cba_tsdf_options {
    double voxel_size; /* lattice spacing (no default: the caller sets it) */
    double truncation; /* the band, in the volume's unit (no default: the caller sets it; a few voxel sizes) */
    double max_weight; /* an integer value in [1, 2^24] (default 64) */
    double max_depth;  /* depths beyond it are not used (default +inf) */
} cba_tsdf_options;
void cba_tsdf_options_default(cba_tsdf_options* o); /* voxel_size and truncation are left at 0: the caller sets them */
typedef struct cba_tsdf_volume cba_tsdf_volume; /* opaque: the volume, the buffers of its calls, the last extract's points, the mesh, the last ray cast, one stream */
cba_status cba_tsdf_volume_create(int32_t nx, int32_t ny, int32_t nz, const double* origin /*[3]*/, const cba_tsdf_options* opts,
                                  int32_t device, cba_tsdf_volume** out);
cba_status cba_tsdf_integrate(cba_tsdf_volume* h, int32_t camera_model, const double* intr /*[10 | 12]*/, int32_t n_maps, int32_t height,
                              int32_t width, const double* depth /*[n_maps][height][width]*/, const double* c_T_v /*[n_maps][7]*/);
cba_status cba_tsdf_fetch(cba_tsdf_volume* h, float* tsdf /*[nz][ny][nx] or NULL*/, float* weight /*[nz][ny][nx] or NULL*/);
cba_status cba_tsdf_upload(cba_tsdf_volume* h, const float* tsdf /*[nz][ny][nx] or NULL*/, const float* weight /*[nz][ny][nx] or NULL*/);
cba_status cba_tsdf_reset(cba_tsdf_volume* h);
cba_status cba_tsdf_extract(cba_tsdf_volume* h, double min_weight, int64_t* n_points);
cba_status cba_tsdf_extract_fetch(cba_tsdf_volume* h, double* xyz /*[n_points][3]*/, double* normals /*[n_points][3] or NULL*/);
cba_status cba_tsdf_mesh(cba_tsdf_volume* h, double min_weight, int64_t* n_points, int64_t* n_triangles);
cba_status cba_tsdf_mesh_fetch(cba_tsdf_volume* h, int32_t* triangles /*[n_triangles][3]*/);
typedef struct cba_tsdf_raycast_options {
    double step;       /* the march's step; 0: half a voxel (default 0) */
    double skip;       /* the share of F truncation a valid sample may advance by, in [0, 1] (default 0.5) */
    double near_depth; /* rays start here (default 0) */
    double far_depth;  /* and end here (default +inf) */
    double min_weight; /* a sample needs W >= min_weight in all eight voxels of its cell (default 1) */
} cba_tsdf_raycast_options;
void cba_tsdf_raycast_options_default(cba_tsdf_raycast_options* o);
cba_status cba_tsdf_raycast(cba_tsdf_volume* h, int32_t camera_model, const double* intr /*[10 | 12]*/, int32_t n_views, int32_t height,
                            int32_t width, const double* poses /*[n_views][7]*/, const cba_tsdf_raycast_options* opts /*NULL: defaults*/);
cba_status cba_tsdf_raycast_fetch(cba_tsdf_volume* h, double* depth /*[n_views][height][width]*/, double* xyz /*[..][3]*/,
                                  double* normals /*[..][3]*/, uint8_t* status /*[..]*/, double* rays /*[height][width][2]*/);
cba_status cba_tsdf_integrate_colour(cba_tsdf_volume* h, int32_t camera_model, const double* intr /*[10 | 12]*/, int32_t n_maps, int32_t height,
                                     int32_t width, const double* depth /*[n_maps][height][width]*/,
                                     const uint8_t* rgba /*[n_maps][height][width][4]*/, const double* c_T_v /*[n_maps][7]*/);
cba_status cba_tsdf_has_colour(cba_tsdf_volume* h, int32_t* out);
cba_status cba_tsdf_colour_fetch(cba_tsdf_volume* h, float* colour /*[nz][ny][nx][4]*/);
cba_status cba_tsdf_colour_upload(cba_tsdf_volume* h, const float* colour /*[nz][ny][nx][4]*/);
cba_status cba_tsdf_extract_fetch_colour(cba_tsdf_volume* h, uint8_t* rgba /*[n_points][4]*/);
cba_status cba_tsdf_raycast_fetch_colour(cba_tsdf_volume* h, uint8_t* rgba /*[n_views][height][width][4]*/);
void cba_tsdf_volume_destroy(cba_tsdf_volume* h);

/* ---- stereo depth: rectification, block matching, disparity to 3D (no counterpart in the reference) -------------------------
 *
 * What a calibrated two-camera rig is used for: calibrated pair -> rectified pair -> dense disparity -> 3D points.
 *
 * cba_stereo_rectify (host, fp64, closed form; needs no device).  Inputs: camera_model, intr [2][10 | 12], c_T_r [2][7] (the pose7
 * rows cba_estimate_extrinsic_dlt and cba_optimize_extrinsics return, reference frame -> camera), the output size width x height and
 * options {focal, cx, cy}, each 0 or NaN for its default.  Rule: each quaternion is normalised (unlike cba_triangulate: the rotations
 * must be orthonormal here); R_i is its matrix, o_i = -R_i^T t_i the camera centre, B = |o_1 - o_0| the baseline;
 *   e1 = (o_1 - o_0) / B,   zbar = R_0^T e_z + R_1^T e_z (the sum of the optical axes in the reference frame),
 *   e2 = (zbar x e1) / |zbar x e1|,   e3 = e1 x e2,   rect_R_r = the matrix with rows e1, e2, e3.
 * Outputs: R [2][9] = rect_R_r R_i^T (row-major), exactly what cba_undistort_map_create takes (its P = R^T (x, y, 1) maps a rectified
 * ray to a camera ray); new_k5 [2][5], two identical rows [f', f', cx', cy', 0] with f' = (fx_0 + fy_0 + fx_1 + fy_1) / 4,
 * cx' = (width - 1) / 2, cy' = (height - 1) / 2 by default; baseline = B; r_T_rect [7], the pose7 that maps the rectified frame of
 * camera 0 to the reference frame: rotation rect_R_r^T as a unit quaternion with w >= 0, translation o_0.
 * Camera 1 lies at +x of camera 0 by construction, so camera 0 is the LEFT image and a point in front of both cameras has disparity
 * u_0 - u_1 = f' B / Z > 0 (Z in the rectified frame).  If the cameras are mounted the other way round the rectified images come out
 * rotated by 180 degrees (the rule still holds; swap the two cameras to get upright images).  Mixed camera models and an output
 * orientation for vertical baselines are out of scope.
 * Errors (CBA_ERR_INVALID_ARGUMENT): NULL pointers; an unknown model; fx or fy equal to 0; width or height outside
 * [1, CBA_IMAGE_MAX_SIDE]; a zero or non-finite quaternion; B <= 1e-12 (|o_0| + |o_1| + 1); |zbar x e1| <= 1e-6 (the optical axes lie
 * along the baseline); a focal that is negative or infinite.
 *
 * cba_stereo_matcher: a handle that owns the options, an optional geometry, one stream and device buffers sized at create for
 * max_pairs pairs of width x height; cba_stereo_matcher_process allocates nothing.  Images are RECTIFIED, single channel uint8,
 * left and right [n_pairs][height][width], rows and pairs contiguous; float32 and multi-channel input are out of scope.  Options:
 *   min_disparity       any int32 with |.| <= 32768       lowest disparity searched
 *   num_disparities     1..256                            D
 *   half_window         1..10                             r: the window is (2r + 1) x (2r + 1)
 *   uniqueness_percent  0..100                            0 = off
 *   lr_max_diff         >= -1                             -1 = off
 *   subpixel            0 / 1                             the parabola step
 * Rule for one left pixel (x, y), W = width, H = height; every cost is an exact integer:
 * 1. Candidate d in [min_disparity, min_disparity + D) is admissible when r <= y <= H-1-r, r <= x <= W-1-r, x - r - d >= 0 and
 *    x + r - d <= W-1.  Then C(x, y, d) = sum over |i|, |j| <= r of |L(x+i, y+j) - R(x+i-d, y+j)| (at most 255 * 441).
 * 2. No admissible candidate: the disparity is NaN (cost -1).  Otherwise d* is the admissible candidate of lowest cost, the lowest d
 *    among equals.
 * 3. Uniqueness (u = uniqueness_percent > 0): the pixel is NaN when some admissible d with |d - d*| > 1 has
 *    100 C(d) <= (100 + u) C(d*).
 * 4. Left-right check (lr_max_diff >= 0): for a right pixel x', d_R(x', y) is the lowest-cost d (the lowest d among equals) over the
 *    d for which (x'+d, y, d) is admissible, its cost being C(x'+d, y, d).  The left pixel is NaN when d_R(x - d*, y) does not exist
 *    or differs from d* by more than lr_max_diff.
 * 5. Sub-pixel step (subpixel != 0): when d*-1 and d*+1 are both admissible and den = C(d*-1) - 2 C(d*) + C(d*+1) > 0,
 *    disparity = d* + (C(d*-1) - C(d*+1)) / (2 den): integer numerator and denominator, one fp64 division, one addition; otherwise
 *    d*.  The result is rounded once to float32.
 * Outputs of process, each may be NULL: disparity float32 [n][H][W]; cost int32 [n][H][W] = C(d*), or -1 where step 2 gives NaN
 * (steps 3 and 4 leave it); xyz float32 [n][H][W][3], only when a geometry was given at create (otherwise passing it is an error):
 * the point of cba_stereo_points for (x, y, float64(disparity)), rounded once to float32.  A pixel's result depends only on its own
 * pair: not on the other pairs of the call, and not on how the device tiles the image.
 *
 * cba_stereo_points: n caller triples uvd [n][3] (u, v, disparity; fp64) -> xyz [n][3] (fp64) by the geometry {f', cx', cy',
 * baseline} that cba_stereo_rectify returns: s = B / d, X = (u - cx') s, Y = (v - cy') s, Z = f' s.  d <= 0 or a non-finite input
 * gives NaN in all three coordinates.  With pose7 (r_T_rect, say), P <- R P + t as in cba_laser_points: the quaternion's matrix
 * without normalisation, each row summed left to right, then + t.  Nothing is contracted into fused multiply-adds.
 *
 * Errors of the matcher and of cba_stereo_points (CBA_ERR_INVALID_ARGUMENT, all checked before any device work): NULL required
 * pointers (options, out, the handle, the geometry of cba_stereo_points; for n_pairs > 0 left and right; for n > 0 uvd and xyz);
 * width or height outside [1, CBA_IMAGE_MAX_SIDE]; max_pairs < 1 or max_pairs width height > 2^31 - 1; an option outside its range;
 * a geometry or pose with a non-finite entry, focal <= 0 or baseline <= 0; a pose at create without a geometry; n_pairs < 0 or
 * n_pairs > max_pairs; xyz on a handle without geometry; n < 0.  n == 0 and n_pairs == 0 are no work; otherwise no device ->
 * CBA_ERR_NO_DEVICE. */
typedef struct cba_stereo_rectify_options {
    double focal; /* f' (0 or NaN: the mean of the four focal lengths) */
    double cx;    /* cx' (0 or NaN: (width - 1) / 2) */
    double cy;    /* cy' (0 or NaN: (height - 1) / 2) */
} cba_stereo_rectify_options;
typedef struct cba_stereo_match_options {
    int32_t min_disparity;      /* lowest disparity searched (default 0) */
    int32_t num_disparities;    /* D, 1..256 (default 64) */
    int32_t half_window;        /* r, 1..10 (default 4) */
    int32_t uniqueness_percent; /* 0..100, 0 = off (default 10) */
    int32_t lr_max_diff;        /* >= -1, -1 = off (default 1) */
    int32_t subpixel;           /* 0 / 1 (default 1) */
} cba_stereo_match_options;
typedef struct cba_stereo_geometry {
    double focal, cx, cy; /* f', cx', cy' of the rectified pair */
    double baseline;      /* B */
} cba_stereo_geometry;
void cba_stereo_match_options_default(cba_stereo_match_options* o);
cba_status cba_stereo_rectify(int32_t camera_model, const double* intr /*[2][10 | 12]*/, const double* c_T_r /*[2][7]*/, int32_t width,
                              int32_t height, const cba_stereo_rectify_options* opts, double* R /*[2][9]*/, double* new_k5 /*[2][5]*/,
                              double* baseline, double* r_T_rect /*[7]*/);
typedef struct cba_stereo_matcher cba_stereo_matcher; /* opaque: options, geometry, device buffers sized at create, one stream */
cba_status cba_stereo_matcher_create(int32_t width, int32_t height, int32_t max_pairs, const cba_stereo_match_options* opts,
                                     const cba_stereo_geometry* geometry /*or NULL*/, const double* pose7 /*[7] or NULL*/,
                                     int32_t device, cba_stereo_matcher** out);
cba_status cba_stereo_matcher_process(cba_stereo_matcher* h, int32_t n_pairs, const uint8_t* left, const uint8_t* right,
                                      float* disparity /*[n][H][W] or NULL*/, int32_t* cost /*[n][H][W] or NULL*/,
                                      float* xyz /*[n][H][W][3] or NULL*/);
void cba_stereo_matcher_destroy(cba_stereo_matcher* h);
cba_status cba_stereo_points(const cba_stereo_geometry* geometry, const double* pose7 /*[7] or NULL*/, int64_t n,
                             const double* uvd /*[n][3]*/, double* xyz /*[n][3]*/);

/* ---- semi-global matching: census cost, path sums, the selection of the block matcher (no counterpart in the reference) ---------
 *
 * cba_sgm_matcher: a second matcher beside cba_stereo_matcher, for the scenes where a window SAD fails (low texture, depth edges).
 * Images, geometry, pose, the three outputs and the xyz rule are exactly those of cba_stereo_matcher; the handle owns the options, an
 * optional geometry, one stream and every device buffer, sized at create; cba_sgm_matcher_process allocates nothing.  Options:
 *   min_disparity       any int32 with |.| <= 32768       dmin, the lowest disparity searched
 *   num_disparities     1..256                            D
 *   p1                  0..p2                             the penalty of a step of one candidate along a path
 *   p2                  0..1023                           the penalty of a larger step
 *   paths               4 or 8
 *   uniqueness_percent  0..100                            0 = off
 *   lr_max_diff         >= -1                             -1 = off
 *   subpixel            0 / 1                             the parabola step
 *   workspace_mb        0..CBA_SGM_MAX_WORKSPACE_MB       the budget of the volumes in MiB, 0 = 2048: the cost and sum volumes are held
 *                                                         for g = max(1, min(max_pairs, budget / bytes per pair)) pairs at a time
 * Rule, W = width, H = height, candidates d in [dmin, dmin + D); every quantity is an exact integer:
 * 1. Census.  Pixels outside an image read 0.  For an image I and a pixel (x, y) the bit of the offset (i, j) is
 *    b_I(x, y; i, j) = [I(x+i, y+j) < I(x, y)], over the window |i| <= 4, |j| <= 3, (i, j) != (0, 0): 62 bits.  How the bits are packed
 *    is the implementation's business; only their set matters.
 * 2. Cost, for every pixel and every candidate: C(x, y, d) = the number of (i, j) with b_L(x, y; i, j) != b_R(x-d, y; i, j); when x - d
 *    lies outside [0, W-1] all 62 bits of b_R are 0.  0 <= C <= 62.
 * 3. Paths.  The directions r are (1,0), (-1,0), (0,1), (0,-1) for paths = 4; paths = 8 adds (1,1), (-1,1), (1,-1), (-1,-1).  With
 *    q = p - r: when q lies outside the image L_r(p, d) = C(p, d); otherwise
 *      L_r(p, d) = C(p, d) + min( L_r(q, d), L_r(q, d-1) + p1, L_r(q, d+1) + p1, M + p2 ) - M,   M = min over all D candidates k of L_r(q, k),
 *    the terms d-1 and d+1 taken only when they are candidates.  Hence 0 <= L_r <= 62 + p2, and S = the sum of L_r over the directions
 *    is at most 8 * 1085 and fits 16 bits.
 * 4. Selection.  Candidate d is admissible for the left pixel (x, y) when 0 <= x - d <= W-1: no window margin, the census is defined
 *    everywhere.  Steps 2 to 5 of the rule of cba_stereo_matcher then apply word for word with S for C and this admissibility: no
 *    admissible candidate gives NaN with cost -1, otherwise d* is the admissible candidate of lowest S, the lowest d among equals;
 *    uniqueness compares 100 S(d) <= (100 + u) S(d*) over the admissible d with |d - d*| > 1; the right map d_R(x', y) is the d of
 *    lowest S, the lowest among equals, over the d with 0 <= x' + d <= W-1, its cost being S(x'+d, y, d), and the left pixel is NaN when
 *    d_R(x - d*, y) differs from d* by more than lr_max_diff; the parabola takes S(d*-1) and S(d*+1) when both are admissible, one
 *    fp64 division, and the result is rounded once to float32.  The cost output is S(d*), or -1 without an admissible candidate.
 * 5. A pixel's result depends on its own pair only: not on the other pairs of the call, on workspace_mb or on any tiling.
 * Errors (CBA_ERR_INVALID_ARGUMENT, all checked before any device work): those of cba_stereo_matcher, an option outside its range,
 * p1 > p2, paths other than 4 or 8, and width height D > CBA_SGM_MAX_VOLUME.  n_pairs == 0 is no work; otherwise no device ->
 * CBA_ERR_NO_DEVICE. */
#define CBA_SGM_MAX_VOLUME ((int64_t)1 << 31) /* largest width * height * num_disparities */
#define CBA_SGM_MAX_WORKSPACE_MB 1048576
typedef struct cba_sgm_options {
    int32_t min_disparity;      /* |.| <= 32768 (default 0) */
    int32_t num_disparities;    /* D, 1..256 (default 64) */
    int32_t p1;                 /* 0..p2 (default 4) */
    int32_t p2;                 /* 0..1023 (default 32) */
    int32_t paths;              /* 4 or 8 (default 8) */
    int32_t uniqueness_percent; /* 0..100, 0 = off (default 10) */
    int32_t lr_max_diff;        /* >= -1, -1 = off (default 1) */
    int32_t subpixel;           /* 0 / 1 (default 1) */
    int32_t workspace_mb;       /* budget for the volumes; 0 = 2048 (default 0) */
} cba_sgm_options;
void cba_sgm_options_default(cba_sgm_options* o);
typedef struct cba_sgm_matcher cba_sgm_matcher; /* opaque: options, geometry, device buffers sized at create, one stream */
cba_status cba_sgm_matcher_create(int32_t width, int32_t height, int32_t max_pairs, const cba_sgm_options* opts,
                                  const cba_stereo_geometry* geometry /*or NULL*/, const double* pose7 /*[7] or NULL*/, int32_t device,
                                  cba_sgm_matcher** out);
cba_status cba_sgm_matcher_process(cba_sgm_matcher* h, int32_t n_pairs, const uint8_t* left, const uint8_t* right,
                                   float* disparity /*[n][H][W] or NULL*/, int32_t* cost /*[n][H][W] or NULL*/,
                                   float* xyz /*[n][H][W][3] or NULL*/);
void cba_sgm_matcher_destroy(cba_sgm_matcher* h);

/* ---- disparity filters: median and speckle removal by connected components (no counterpart in the reference) ----------------------
 *
 * cba_disparity_filter: what follows a dense matcher.  Uniqueness and the left-right check remove single pixels; what survives them in
 * occluded and low-texture regions is small islands of wrong disparity.  The handle owns the options, one stream and every device
 * buffer, sized at create for max_images maps of width x height; cba_disparity_filter_process allocates nothing and ends with its
 * stream synchronised.  Input and output are float32 [n][height][width], rows and maps contiguous, NaN = "no disparity"; out == in is
 * allowed.  Every map is filtered on its own.  Options:
 *   median_half         0..2          m: the window is (2m+1) x (2m+1); 0 skips step 1
 *   speckle_max_size    >= 0          S: a component of at most S pixels is removed; 0 skips step 2
 *   speckle_max_diff    finite, >= 0  two neighbours are joined when their disparities differ by at most this
 * Rule:
 * 0. Reading.  A non-finite input is invalid (NaN); -0.0 is read as +0.0, so every output is a bit pattern this rule defines.
 * 1. Median (m > 0).  An invalid pixel stays NaN: holes are not filled.  For a valid pixel take the valid values of the window clipped
 *    to the image, k >= 1 of them (the centre counts), sorted ascending: the output is the element of index (k - 1) / 2 (integer
 *    division), the lower median.  The step selects and never averages: the output is one of the inputs.
 * 2. Speckle removal (S > 0), on the result of step 1.  The nodes are the valid pixels of one map.  Pixels p and q are joined when they
 *    are 4-neighbours in the same map and |double(d_p) - double(d_q)| <= speckle_max_diff: one fp64 subtraction, one comparison.
 *    Diagonal neighbours are never joined, nor are the last pixel of a row and the first of the next row, nor the last row of map i and
 *    the first row of map i + 1.  A connected component of at most S pixels becomes NaN as a whole.  The relation is symmetric, so the
 *    components, and with them the result, depend on no traversal, tiling or arrival order.
 * 3. Stats, optional: int64 [n][3] = {valid pixels after step 0, components removed, pixels removed}.
 * cba_stereo_matcher_set_filter / cba_sgm_matcher_set_filter attach such a filter to a matcher (NULL: none, the default).  Its
 * workspace is allocated in that call.  With a filter set, process computes the disparity as before, filters it, and writes xyz from
 * the filtered map: xyz is NaN exactly where the filtered disparity is.  cost stays as the matcher's rule leaves it.
 * Errors (CBA_ERR_INVALID_ARGUMENT, all checked before any device work): NULL required pointers, sizes outside
 * [1, CBA_IMAGE_MAX_SIDE], max_images < 1 or max_images width height > 2^31 - 1, an option outside its range, n < 0 or n > max_images.
 * n == 0 is no work; otherwise no device -> CBA_ERR_NO_DEVICE. */
typedef struct cba_disparity_filter_options {
    int32_t median_half;      /* 0..2 (default 1) */
    int32_t speckle_max_size; /* >= 0 (default 100) */
    double speckle_max_diff;  /* finite, >= 0 (default 1.0) */
} cba_disparity_filter_options;
void cba_disparity_filter_options_default(cba_disparity_filter_options* o);
typedef struct cba_disparity_filter cba_disparity_filter; /* opaque: options, device buffers sized at create, one stream */
cba_status cba_disparity_filter_create(int32_t width, int32_t height, int32_t max_images, const cba_disparity_filter_options* opts,
                                       int32_t device, cba_disparity_filter** out);
cba_status cba_disparity_filter_process(cba_disparity_filter* h, int32_t n, const float* in /*[n][H][W]*/, float* out /*[n][H][W]*/,
                                        int64_t* stats /*[n][3] or NULL*/);
void cba_disparity_filter_destroy(cba_disparity_filter* h);
cba_status cba_stereo_matcher_set_filter(cba_stereo_matcher* h, const cba_disparity_filter_options* opts /*or NULL: no filter*/);
cba_status cba_sgm_matcher_set_filter(cba_sgm_matcher* h, const cba_disparity_filter_options* opts /*or NULL: no filter*/);

/* ---- chessboard detection: corners, sub-pixel fit, grid order (no counterpart in the reference, which reads corners from files) ---
 *
 * Pictures of a plain chessboard -> the (object_xy, image_uv) lists every other entry point starts from.
 *
 * cba_corner_detector: a handle that owns the options, one stream and device buffers sized at create for max_images images of
 * width x height with up to max_corners corners each; cba_corner_detector_process allocates nothing.  Images are single channel
 * uint8, [n_images][height][width], rows and images contiguous; float32, colour and a blur before the response are out of scope.
 * Options:
 *   min_response        1..10200     lowest response of a peak (>= 1, so a constant image has none)
 *   nms_radius          1..10        the suppression window is (2 nms_radius + 1)^2
 *   cog_radius          1..5         the centre-of-gravity window is (2 cog_radius + 1)^2
 *   refine              CBA_CORNER_REFINE_NONE / _COG / _GRADIENT (GRADIENT starts from the COG result)
 *   refine_half_window  1..10        w: GRADIENT's window is (2w + 1)^2
 *   refine_iterations   1..100       GRADIENT's rounds
 * Rule for one image, W = width, H = height, I(x, y) the pixels:
 * 1. Response (exact integers).  The ring offsets (dx, dy), n = 0..15, are (0,-5) (2,-5) (3,-3) (5,-2) (5,0) (5,2) (3,3) (2,5) (0,5)
 *    (-2,5) (-3,3) (-5,2) (-5,0) (-5,-2) (-3,-3) (-2,-5), I_n = I(x + dx_n, y + dy_n).  SR = sum_{n<4} |I_n + I_{n+8} - I_{n+4} -
 *    I_{n+12}|, DR = sum_{n<8} |I_n - I_{n+8}|, S16 = sum I_n, S5 = I(x, y) + I(x-1, y) + I(x+1, y) + I(x, y-1) + I(x, y+1),
 *    R = 5 SR - 5 DR - |5 S16 - 16 S5|, in [-30600, 10200].  R is defined for 5 <= x <= W-6, 5 <= y <= H-6 and is 0 elsewhere.
 * 2. Peaks.  A pixel is a peak when R >= min_response, it lies at least 5 + nms_radius from every border, and inside its
 *    (2 nms_radius + 1)^2 window R is greater than every response earlier in row-major order and not less than every later one
 *    (among equal responses the lowest index wins).  The peaks of an image are listed in row-major order.  With more than
 *    max_corners peaks the first max_corners are kept, status has CBA_CORNER_STATUS_OVERFLOW and count is the true number.
 * 3. Angle = 0.5 atan2(sum_{n<8} (I_n + I_{n+8}) s_n, sum_{n<8} (I_n + I_{n+8}) c_n) at the peak's pixel, c_n = (dx^2 - dy^2) / (dx^2 +
 *    dy^2) and s_n = 2 dx dy / (dx^2 + dy^2) (cos and sin of twice the offset's direction; rational, hence the same doubles on every
 *    host), each sum in fp64 with n ascending and nothing contracted; the device makes the sums, the host the atan2.  The angle is
 *    the bisector of one quadrant pair modulo pi, x to the right and y down: the edges lie near angle +- pi/4, grid neighbours differ
 *    by about pi/2 and diagonal neighbours are equal.
 * 4. Position.  NONE: the peak's pixel.  COG: x = px + sum R+ dx / sum R+ over the (2 cog_radius + 1)^2 window (R+ = max(R, 0);
 *    exact integer sums, one fp64 division per axis), the same for y.  GRADIENT (the cornerSubPix condition), from the COG result,
 *    exactly refine_iterations rounds without a convergence test: with (cx, cy) the position, ix = floor(cx), fx = cx - ix (and y
 *    alike), P(a, b) is the image interpolated at (ix + a + fx, iy + b + fy): top = p00 + fx (p01 - p00), bot = p10 + fx (p11 - p10),
 *    P = top + fy (bot - top).  For (dx, dy) in the window, row-major: gx = (P(dx+1, dy) - P(dx-1, dy)) / 2, gy alike, weight
 *    m = exp(-(dx^2 + dy^2) / (2 (w/2)^2)) (made once on the host), gxx = (gx m) gx, gxy = (gx m) gy, gyy = (gy m) gy;
 *    a += gxx, b += gxy, c += gyy, b1 += gxx dx + gxy dy, b2 += gxy dx + gyy dy; det = a c - b b; the position moves by
 *    ((c b1 - b b2) / det, (a b2 - b b1) / det).  All in fp64, in this order, nothing contracted.  The rounds end early, the corner
 *    keeping its last good position, with CBA_CORNER_FLAG_WINDOW when the position or the moved position is closer than w + 2 to a
 *    border, and with CBA_CORNER_FLAG_DET when not det > 1e-6 (a + c)^2 (further rounds would repeat the same numbers).  A corner
 *    that ends further than cog_radius + 1 from its peak along x or y gets CBA_CORNER_FLAG_DRIFT.
 * Outputs of process, each may be NULL: out_count [n] (true number of peaks), out_status [n], out_xy [n][max_corners][2],
 * out_angle [n][max_corners], out_response [n][max_corners] (R at the peak's pixel), out_flags [n][max_corners].  Entries past the
 * kept corners are NaN (xy, angle) and 0 (response, flags).  An image's result does not depend on the other images of the call.
 *
 * cba_chessboard_order (host, fp64; needs no device): one image's corners xy [n][2], angle [n] and the board's rows x cols INNER
 * corners -> out_index [rows cols] into the corner list, row-major over (j, i), so that object point (i square, j square) pairs with
 * corner out_index[j cols + i]; all -1 when the board is not found.
 *   Neighbours: for a corner the candidates are the corners of opposite polarity, |wrap_pi(angle difference)| > pi/4, within 1.7 x
 *   the distance of the nearest such corner; slot k = 0..3 takes the nearest candidate whose displacement lies within 35 degrees of
 *   the direction angle + pi/4 + k pi/2; only mutual links are kept.
 *   Labels: breadth-first growth assigns integer (i, j); the slot of a neighbour that points back defines the neighbour's frame.
 *   Components are tried from the corner nearest the centroid of all corners outwards.
 *   Acceptance: the component has exactly rows cols corners, no corner gets two labels, every cell is filled exactly once and the
 *   extents are cols x rows after an optional transpose.  Partial boards are out of scope.
 *   Canonical labelling: i runs along the cols side; the frame is right-handed in image coordinates, cross(mean i-step, mean
 *   j-step) > 0 with x right and y down; among the labellings that remain (a half turn, or four quarter turns if rows == cols) the
 *   one whose mean i-step has the largest x component is chosen, ties going to the larger y component.
 *
 * Errors (CBA_ERR_INVALID_ARGUMENT, all checked before any device work): NULL options, out, handle, out_index, images for
 * n_images > 0, xy or angle for n > 0; width or height below 11 or above CBA_IMAGE_MAX_SIDE; max_images < 1 or max_images width
 * height > 2^31 - 1; max_corners < 1 or max_images max_corners > 2^28; an option outside its range; n_images < 0 or > max_images;
 * n < 0 or n > 65536; rows or cols < 2 or rows cols > 65536; a non-finite corner.  n_images == 0 is no work; otherwise no device ->
 * CBA_ERR_NO_DEVICE. */
#define CBA_CORNER_REFINE_NONE 0
#define CBA_CORNER_REFINE_COG 1
#define CBA_CORNER_REFINE_GRADIENT 2
#define CBA_CORNER_STATUS_OVERFLOW 1 /* more than max_corners peaks: the first max_corners were kept */
#define CBA_CORNER_FLAG_WINDOW 1     /* GRADIENT: the window would leave the image */
#define CBA_CORNER_FLAG_DET 2        /* GRADIENT: determinant too small */
#define CBA_CORNER_FLAG_DRIFT 4      /* GRADIENT: ended further than cog_radius + 1 from the peak */
typedef struct cba_corner_options {
    int32_t min_response;       /* 1..10200 (default 400) */
    int32_t nms_radius;         /* 1..10 (default 3) */
    int32_t cog_radius;         /* 1..5 (default 2) */
    int32_t refine;             /* CBA_CORNER_REFINE_* (default GRADIENT) */
    int32_t refine_half_window; /* w, 1..10 (default 5) */
    int32_t refine_iterations;  /* 1..100 (default 5) */
} cba_corner_options;
void cba_corner_options_default(cba_corner_options* o);
typedef struct cba_corner_detector cba_corner_detector; /* opaque: options, device buffers sized at create, one stream */
cba_status cba_corner_detector_create(int32_t width, int32_t height, int32_t max_images, int32_t max_corners,
                                      const cba_corner_options* opts, int32_t device, cba_corner_detector** out);
cba_status cba_corner_detector_process(cba_corner_detector* h, int32_t n_images, const uint8_t* images,
                                       int32_t* out_count /*[n] or NULL*/, int32_t* out_status /*[n] or NULL*/,
                                       double* out_xy /*[n][max_corners][2] or NULL*/, double* out_angle /*[n][max_corners] or NULL*/,
                                       int32_t* out_response /*[n][max_corners] or NULL*/, int32_t* out_flags /*[n][max_corners] or NULL*/);
void cba_corner_detector_destroy(cba_corner_detector* h);
cba_status cba_chessboard_order(int32_t n, const double* xy /*[n][2]*/, const double* angle /*[n]*/, int32_t rows, int32_t cols,
                                int32_t* out_index /*[rows cols]*/);

/* ---- circle-grid detection: blobs, ellipse centres, grid order (no counterpart in the reference, which reads features from files) --
 *
 * Pictures of a symmetric or asymmetric circle grid -> the (object_xy, image_uv) lists every other entry point starts from.
 *
 * cba_blob_detector: a handle that owns the options, one stream and device buffers sized at create for max_images images of
 * width x height with up to max_blobs blobs each; cba_blob_detector_process allocates nothing.  Images are single channel uint8,
 * [n_images][height][width], rows and images contiguous.
 * Options:
 *   polarity        CBA_BLOB_DARK (dark blobs on a bright ground) / CBA_BLOB_BRIGHT
 *   inner_half      1..7               a: the inner box is (2a + 1)^2
 *   outer_half      a+1..15            b: the outer box is (2b + 1)^2, the ring is the outer box without the inner one
 *   min_contrast    1..255             lowest difference of the ring's and the inner box's means, in grey levels
 *   nms_radius      1..10              the suppression window is (2 nms_radius + 1)^2
 *   max_radius      2..32              the longest ray, in pixels
 *   rounds          1..8               centroid rounds
 *   max_fit_error   > 0                CBA_BLOB_FLAG_SHAPE above it
 *   max_axis_ratio  >= 1               CBA_BLOB_FLAG_RATIO above it
 *   min_radius      >= 0               CBA_BLOB_FLAG_SIZE below it
 * Rule for one image, W = width, H = height, I(x, y) the pixels, taken as 0 outside the image:
 * 1. Response (exact integers).  S_in = the sum of I over the (2a + 1)^2 box centred on the pixel, S_ring = the sum over the
 *    (2b + 1)^2 box minus S_in, n_in = (2a + 1)^2, n_ring = (2b + 1)^2 - n_in.  DARK: R = n_in S_ring - n_ring S_in = n_in n_ring (mean
 *    ring - mean inner); BRIGHT: the negative.  R is 0 closer than b to a border; |R| < 2^31.  The detector keeps R as int32 and S_in
 *    as uint16 (<= 57375) next to it, so S_ring = (R + n_ring S_in) / n_in (DARK; BRIGHT: (n_ring S_in - R) / n_in) is exact.
 * 2. Peaks: the rule of cba_corner_detector with the border b.  A pixel is a peak when R >= min_contrast n_in n_ring, it lies at
 *    least b + nms_radius from every border, and inside its (2 nms_radius + 1)^2 window R is greater than every response earlier in
 *    row-major order and not less than every later one.  Peaks are listed in row-major order; with more than max_blobs peaks the
 *    first max_blobs are kept, status has CBA_BLOB_STATUS_OVERFLOW and count is the true number.
 * 3. Refinement of one peak, in fp64, in this order, nothing contracted; the device uses only + - x /.  Levels, fixed for all
 *    rounds: lo = S_in / n_in and hi = S_ring / n_ring at the peak, thr = (lo + hi) / 2.  The image at a real position (x, y) with
 *    0 <= x < W - 1, 0 <= y < H - 1 is bilinear: ix = floor(x), fx = x - ix (y alike), top = p00 + fx (p01 - p00), bot = p10 +
 *    fx (p11 - p10), I = top + fy (bot - top); a position outside that range sets CBA_BLOB_FLAG_WINDOW.  The directions are d_k =
 *    (cos 2 pi k / 32, sin 2 pi k / 32), k = 0..31, from a table made on the host.  A round, from the centre c (round 0: the
 *    peak's pixel): I0 = I(c); if I0 is not on the blob's side of thr (DARK: I0 < thr, BRIGHT: I0 > thr) CBA_BLOB_FLAG_NO_EDGE.  For
 *    k = 0..31 sample I(c + t d_k), t = 1..max_radius; the edge is the first t whose sample reaches thr (DARK: >=, BRIGHT: <=) and
 *    lies at r_k = (t - 1) + (thr - I(t-1)) / (I(t) - I(t-1)) (BRIGHT: both differences negated), I(0) = I0; no such t:
 *    CBA_BLOB_FLAG_NO_EDGE.  The edge points e_k = r_k d_k (relative to c) form a polygon; with cr = x_k y_k+1 - x_k+1 y_k summed over
 *    k = 0..31 (e_32 = e_0): s2 = sum cr, sx = sum (x_k + x_k+1) cr, sy alike, sxx = sum (x_k^2 + x_k x_k+1 + x_k+1^2) cr, syy alike,
 *    sxy = sum (x_k y_k+1 + 2 x_k y_k + 2 x_k+1 y_k+1 + x_k+1 y_k) cr.  Not s2 > 0: CBA_BLOB_FLAG_DEGENERATE.  The centroid is g =
 *    (sx, sy) / (3 s2) and c moves to c + g.  After the last round M = 4 x the central second moments per area: m_xx = 4 (sxx / (6 s2)
 *    - g_x^2), m_yy alike, m_xy = 4 (sxy / (12 s2) - g_x g_y); not det M > 0: CBA_BLOB_FLAG_DEGENERATE.  {d : d^T M^-1 d = 1} is the
 *    ellipse with the polygon's moments, and fit_error = max_k |(e_k - g)^T M^-1 (e_k - g) - 1| (a square has 0.5).  Any of the three
 *    flags ends the blob at its last good centre with NaN shape and fit_error.
 * 4. Flags from the numbers (set on the host of the library): CBA_BLOB_FLAG_SHAPE when fit_error > max_fit_error; with the semi-axes
 *    major >= minor, the square roots of M's eigenvalues, CBA_BLOB_FLAG_RATIO when major > max_axis_ratio minor and CBA_BLOB_FLAG_SIZE
 *    when minor < min_radius; CBA_BLOB_FLAG_DUPLICATE when an earlier blob of the image without any flag has its centre within this
 *    blob's minor semi-axis (a disc wider than the outer box gives several peaks on its rim that refine to one centre: the first
 *    stays).
 * Outputs of process, each may be NULL: out_count [n] (true number of peaks), out_status [n], out_xy [n][max_blobs][2], out_shape
 * [n][max_blobs][3] = (m_xx, m_xy, m_yy), out_fit_error [n][max_blobs], out_response [n][max_blobs] (R at the peak's pixel),
 * out_flags [n][max_blobs].  Entries past the kept blobs are NaN (xy, shape, fit_error) and 0 (response, flags).  An image's result
 * does not depend on the other images of the call.
 *
 * cba_circle_grid_order (host, fp64; needs no device): one image's blobs xy [n][2], their shapes [n][3] (NULL: the identity) and the
 * pattern's rows x cols -> out_index [rows cols] into the blob list, row-major over (j, i); all -1 when the grid is not found.
 * CBA_CIRCLES_SYMMETRIC places point (j, i) at (i, j) d, CBA_CIRCLES_ASYMMETRIC at ((2 i + j mod 2) d, j d).  Both are square
 * lattices (pitch d; pitch d sqrt 2 turned by 45 degrees), so one rule links both.
 *   Metric: from blob c, q_c(v) = v^T M_c^-1 v and cos_c(v, w) = v^T M_c^-1 w / sqrt(q_c(v) q_c(w)): the board's metric to first order.
 *   Links: blob c's candidates are its up to four nearest blobs by q_c (ties to the lower index) with q_c <= 1.44 x the nearest's
 *   (1.2 x in distance); a link stays when each blob is a candidate of the other.
 *   Labels: components are grown breadth first from the blob nearest the centroid of all blobs outwards.  The start's basis is e1 =
 *   its first link, e2 = its link with the smallest |cos| to e1.  A blob taken from the queue first refreshes its basis: each axis
 *   is replaced by the link with the largest |cos| to it, signed to point the axis's way, if that exceeds cos 30 degrees.  Then
 *   every link is a step of +-e1 or +-e2 by the larger |cos|, which must exceed cos 30 degrees or the component is rejected; the
 *   neighbour gets label + step and inherits the basis.  A blob reached with two different labels rejects the component.
 *   Acceptance: a component of exactly rows cols blobs; for each of the lattice's eight symmetries (transpose, flip p, flip q) of the
 *   labels (p, q), mapped to (p - q, p + q) for the asymmetric pattern and shifted to start at 0, the occupied cells must equal the
 *   pattern's, and the labelling must be right-handed: cross(mean i-step, mean j-step) > 0 with x right and y down.  Exactly one such
 *   labelling: unique = 1 (the asymmetric pattern with odd rows).  Otherwise the one whose mean i-step has the largest x, then y,
 *   and unique = 0.
 *
 * Errors (CBA_ERR_INVALID_ARGUMENT, all checked before any device work): NULL options, out, handle, out_index, images for n_images > 0
 * or xy for n > 0; an option outside its range; width or height below 2 (outer_half + nms_radius) + 1 or above CBA_IMAGE_MAX_SIDE;
 * max_images < 1 or max_images width height > 2^31 - 1; max_blobs < 1 or max_images max_blobs > 2^28; n_images < 0 or > max_images;
 * n < 0 or > 65536; an unknown pattern; rows or cols < 2 or rows cols > 65536; a non-finite blob or a shape that is not positive
 * definite.  n_images == 0 is no work; otherwise no device -> CBA_ERR_NO_DEVICE. */
#define CBA_BLOB_DARK 0
#define CBA_BLOB_BRIGHT 1
#define CBA_BLOB_STATUS_OVERFLOW 1 /* more than max_blobs peaks: the first max_blobs were kept */
#define CBA_BLOB_FLAG_WINDOW 1     /* a sample would leave the image */
#define CBA_BLOB_FLAG_NO_EDGE 2    /* the centre is not inside the blob, or a ray met no edge by max_radius */
#define CBA_BLOB_FLAG_DEGENERATE 4 /* polygon area or moment determinant not positive */
#define CBA_BLOB_FLAG_SHAPE 8      /* fit_error > max_fit_error */
#define CBA_BLOB_FLAG_RATIO 16     /* major > max_axis_ratio minor */
#define CBA_BLOB_FLAG_SIZE 32      /* minor < min_radius */
#define CBA_BLOB_FLAG_DUPLICATE 64 /* an earlier unflagged blob has its centre within the minor semi-axis */
#define CBA_CIRCLES_SYMMETRIC 0
#define CBA_CIRCLES_ASYMMETRIC 1
typedef struct cba_blob_options {
    int32_t polarity;      /* CBA_BLOB_DARK (default) / CBA_BLOB_BRIGHT */
    int32_t inner_half;    /* a, 1..7 (default 2) */
    int32_t outer_half;    /* b, a+1..15 (default 12) */
    int32_t min_contrast;  /* 1..255 (default 30) */
    int32_t nms_radius;    /* 1..10 (default 4) */
    int32_t max_radius;    /* 2..32 (default 20) */
    int32_t rounds;        /* 1..8 (default 3) */
    int32_t reserved;      /* keeps the doubles aligned; ignored */
    double max_fit_error;  /* (default 0.2) */
    double max_axis_ratio; /* (default 3) */
    double min_radius;     /* (default 1.5) */
} cba_blob_options;
void cba_blob_options_default(cba_blob_options* o);
typedef struct cba_blob_detector cba_blob_detector; /* opaque: options, device buffers sized at create, one stream */
cba_status cba_blob_detector_create(int32_t width, int32_t height, int32_t max_images, int32_t max_blobs, const cba_blob_options* opts,
                                    int32_t device, cba_blob_detector** out);
cba_status cba_blob_detector_process(cba_blob_detector* h, int32_t n_images, const uint8_t* images, int32_t* out_count /*[n] or NULL*/,
                                     int32_t* out_status /*[n] or NULL*/, double* out_xy /*[n][max_blobs][2] or NULL*/,
                                     double* out_shape /*[n][max_blobs][3] or NULL*/, double* out_fit_error /*[n][max_blobs] or NULL*/,
                                     int32_t* out_response /*[n][max_blobs] or NULL*/, int32_t* out_flags /*[n][max_blobs] or NULL*/);
void cba_blob_detector_destroy(cba_blob_detector* h);
cba_status cba_circle_grid_order(int32_t n, const double* xy /*[n][2]*/, const double* shape /*[n][3] or NULL*/, int32_t pattern,
                                 int32_t rows, int32_t cols, int32_t* out_index /*[rows cols]*/, int32_t* out_unique /*or NULL*/);

/* ---- ChArUco boards: corner arms, marker reads, partial views (no counterpart in the reference, which reads corners from files) ----
 *
 * Pictures of a ChArUco board, which may hang over the image's edge -> per image the visible inner corners with their BOARD INDEX and
 * sub-pixel position.  Corners come from cba_corner_detector's rule unchanged; an arm test removes the X-junctions inside the
 * markers; the host labels the partial lattices; the markers of the complete lattice cells are read on the resident images; the host
 * assigns board indices by the markers' votes.
 *
 * Board (cba_charuco_board): squares_x x squares_y squares (each >= 3) of side `square`; square (sx, sy) is dark when sx + sy is
 * even, so square (0, 0) is dark.  Every bright square carries, centred, a marker of marker_bits^2 bits (3..7) inside a dark border
 * one cell wide: (marker_bits + 2)^2 cells on a side of marker_ratio x square, marker_ratio in [0.4, 0.8].  Marker ids ascend
 * row-major (sy, then sx) over the bright squares, the layout of OpenCV's CharucoBoard.  Inner corner (i, j), 0 <= i < squares_x - 1,
 * 0 <= j < squares_y - 1, has board index j (squares_x - 1) + i and object point ((i + 1) square, (j + 1) square): the origin is the
 * outer corner of square (0, 0).  n_markers codes are given (1..16384); a board with more bright squares than codes is legal, its
 * squares past the dictionary are never read as theirs.
 *
 * Dictionary: codes [n_markers] uint64, the marker_bits^2 inner cells row-major (y down, then x right), the first cell the most
 * significant of the marker_bits^2 low bits, bright = 1.  A quarter-turn clockwise, rot(c), has cell (y, x) = c's cell
 * (marker_bits - 1 - x, y).  cba_marker_dictionary_generate (host) draws candidates from splitmix64 with state s = seed: s +=
 * 0x9E3779B97F4A7C15; z = s; z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) 0x94D049BB133111EB; z ^= z >> 31 (mod
 * 2^64); the candidate is z >> (64 - bits^2).  A candidate is kept when its Hamming distance to each of its own three rotations and to
 * all four rotations of every kept code is >= min_distance.  At most 200000 candidates are drawn; *out_found is the number of codes
 * found, which may be less than count.
 *
 * Options (cba_charuco_options):
 *   arm_lengths [2]      (0, 64]       the two distances L along an edge (defaults 7, 10)
 *   arm_offset           (0, 16]       the distance of the two samples from the edge (default 2)
 *   arm_fan_deg          [0, 30]       the fan's half opening in degrees (default 14)
 *   min_arm_contrast     >= 0          lowest arm score of a corner, grey levels (default 112)
 *   min_component        >= 1          smallest lattice component (default 4)
 *   cell_samples         1..5          S: sub-samples per marker cell and axis (default 3)
 *   min_marker_contrast  >= 0          lowest max - min of a reading's cell means, grey levels (default 40)
 *   max_border_errors    >= 0          bright border cells allowed (default 1)
 *   max_correction       >= 0          wrong bits allowed; keep it at most (the dictionary's min_distance - 1) / 2 (default 1)
 *   min_markers          >= 1          readings a component's winning vote needs (default 2)
 *
 * 1. Arm test, one fp64 score per kept corner at its position (x, y) (cba_corner_detector's out_xy) and angle.  Direction 3 k + f, arm
 *    k = 0..3, fan f = 0..2, has phi = angle + pi/4 + k pi/2 + (f - 1) arm_fan_deg pi / 180 and the unit vector (c, s) = (cos phi,
 *    sin phi), made on the host.  On the device only + - x / and floor, in the order written, nothing contracted.  For a length L:
 *    px = x + L c, py = y + L s; a = (px - off s, py + off c), b = (px + off s, py - off c), off = arm_offset; d = B(a) - B(b) with
 *    B(x, y) the bilinear sample: x0 = floor(x), fx = x - x0 (y alike), top = p00 + fx (p01 - p00), bot = p10 + fx (p11 - p10),
 *    B = top + fy (bot - top).  A sample is legal when 1 <= x <= W - 2 and 1 <= y <= H - 2.  An arm with an illegal sample in any of its
 *    three directions is not counted at that length.  For a counted arm, P_k = max_f (-1)^k d and M_k = max_f -(-1)^k d; the score at
 *    L is max(min_k P_k, min_k M_k) over the counted arms, and 0 when fewer than two arms are counted.  The corner's score is the
 *    smaller of the scores at arm_lengths[0] and arm_lengths[1].  A corner passes with score >= min_arm_contrast.
 * 2. Lattice of a partial view (host, fp64; cba_chessboard_lattice).  Input: the corners that passed and carry no refine flag, in the
 *    order of the corner list.  Links: the neighbour rule of cba_chessboard_order (polarity, reach 1.7, 35 degree cone, mutual
 *    links).  Labels: corners are visited in index order; an unlabelled corner starts a component at (0, 0) with quarter-turn count
 *    o = 0 and the component grows breadth-first, slots k = 0..3 in order: slot k of a corner with count o steps by t = (k + o) mod 4,
 *    (1,0) (0,1) (-1,0) (0,-1), and the neighbour, whose slot `back` points back, gets count (k + o + 2 - back) mod 4.  A link to a
 *    corner that already has a different label or count is dropped (both directions) and nothing else changes.  After the pass, if
 *    any label (component, i, j) is claimed by more than one corner, all its claimants lose all their links and leave, and the labels
 *    are made once more from the remaining links; claimants of a label claimed twice in that second pass leave without another pass.
 *    Then every labelled corner that has fewer than two links left leaves (all judged before any leaves).  Components with fewer than
 *    min_component corners are discarded.  Handedness: with the mean i-step the mean of xy(i+1, j) - xy(i, j) over the labelled pairs,
 *    the mean j-step alike, a component whose cross(mean i-step, mean j-step) is negative gets i negated; one with no i-pair, no
 *    j-pair or a zero cross product is discarded.  Labels are shifted so that each component's smallest i and j are 0.  Components are
 *    numbered by size, the largest first, ties by the lowest corner index.  Output per corner: component (-1: none) and (i, j).
 *    After this only a quarter-turn and a shift of each component are unknown.
 * 3. Marker read, one reading per lattice cell (component, i, j) whose corners (i, j) (i+1, j) (i+1, j+1) (i, j+1) are all labelled;
 *    the cells of an image are listed by component, then j, then i.  The quad (x0, y0) .. (x3, y3), in that order, is the image of the
 *    unit square (0,0) (1,0) (1,1) (0,1) under x = (a u + b v + c) / (g u + h v + 1), y = (d u + e v + f) / (g u + h v + 1)
 *    (Heckbert): sx = x0 - x1 + x2 - x3, dx1 = x1 - x2, dx2 = x3 - x2 (y alike), den = dx1 dy2 - dy1 dx2, g = (sx dy2 - sy dx2) / den,
 *    h = (dx1 sy - dy1 sx) / den, a = x1 - x0 + g x1, b = x3 - x0 + h x3, c = x0, d = y1 - y0 + g y1, e = y3 - y0 + h y3, f = y0.
 *    The quad is DEGENERATE when |den|, or the like cross product of the two sides at any other corner (at corner k: (P_{k+1} - P_k) x
 *    (P_{k-1} - P_k), indices modulo 4; den is the one at corner 2), is not greater than 1e-12 x the square of the longest side: two
 *    equal points and three collinear points are both caught.  Marker cell (cx, cy), 0 <= cx, cy
 *    < marker_bits + 2, sub-sample (kx, ky): u = m0 + ms (cx + (0.25 + 0.5 (kx + 0.5) / S)), v alike with cy and ky, m0 = 0.5 (1 -
 *    marker_ratio), ms = marker_ratio / (marker_bits + 2); w = g u + h v + 1, x = (a u + b v + c) / w, y = (d u + e v + f) / w,
 *    products summed left to right.  The cell's mean is the sum of B(x, y) over ky, then kx (row-major), divided once by S^2.  If any
 *    sample of any cell is illegal (rule 1) the reading is WINDOW and nothing is read.  t = (min + max) / 2 over the cell means; a
 *    cell is bright when mean > t.  LOW_CONTRAST: max - min < min_marker_contrast.  BORDER: more than max_border_errors bright border
 *    cells.  The inner cells, row-major, the first the most significant, form the code.  Match: over the table entry 4 id + r =
 *    rot^r(codes[id]) the smallest key = distance 2^16 + 4 id + r wins (distance: Hamming distance to the code), so ties go to the
 *    lowest id, then the lowest rotation; NO_MATCH when the winner's distance > max_correction.  second_distance is the smallest
 *    distance over the entries of every other id (-1 when there is none).  The flags are independent; a reading is accepted when it
 *    has none.  A DEGENERATE or WINDOW reading has id -1, distances -1 and zeros elsewhere.
 * 4. Board index (host; cba_charuco_match).  With T(a, b) = (b, -a), an accepted reading of cell (i, j) with marker id in square
 *    (qx, qy) and rotation r votes for (r, shift) with 2 shift = (2 qx - 1, 2 qy - 1) - T^r(2 i + 1, 2 j + 1): the labelling
 *    board (i, j) = T^r(lattice (i, j)) + shift.  Readings whose id the board does not carry do not vote.  Per component the vote with
 *    the most readings wins when it has at least min_markers and strictly more than every other vote.  Components are then taken by
 *    their winning votes, most first (ties: lower component number): its corners get board indices, corners outside the board are
 *    dropped, and a component one of whose indices is already taken is dropped whole.  Output per image: out_count, out_ids ascending
 *    with out_xy (entries past the count -1 and NaN), out_n_markers (the votes of the winning labellings that were used).
 *
 * cba_charuco_detector: the handle owns a cba_corner_detector's state for max_images images of width x height with up to max_corners
 * corners each, and room for max_cells lattice cells per call; process allocates no device memory.  out_ids [n][nb], out_xy
 * [n][nb][2] with nb = (squares_x - 1)(squares_y - 1).  out_status: CBA_CHARUCO_STATUS_CORNER_OVERFLOW as the corner detector's, and
 * CBA_CHARUCO_STATUS_CELL_OVERFLOW on the images whose cells did not all fit: the first max_cells cells of the call are kept and
 * *out_n_cells stays the true number.  For diagnosis: out_n_corners [n] (peaks), out_cells [max_cells][4] (image, component, i, j)
 * and out_readings [max_cells], the first min(*out_n_cells, max_cells) filled.  Every output may be NULL.  An image's result does not
 * depend on the other images of the call unless cells overflow.  Two mid-level calls act on the images, positions and counts of the
 * last process: cba_charuco_detector_arms (dirs [n][max_corners][12][2] -> scores [n][max_corners], NaN past the kept corners; n must
 * be the last process's) and cba_charuco_detector_read (n_cells <= max_cells cells: the image index and the quad of each ->
 * readings).
 *
 * Errors (CBA_ERR_INVALID_ARGUMENT, checked before any device work): NULL pointers where one is needed; the size limits of
 * cba_corner_detector_create; max_cells < 1 or > 2^24; a board or option value outside the ranges above; a code with bits above
 * marker_bits^2; n_images or n outside its range; an image index outside the last process's; for the host calls n < 0 or > 65536, a
 * non-finite corner, a component or cell label outside [-1, 65536].  No device -> CBA_ERR_NO_DEVICE (the three host calls need none).
 * Not built: the markers of the rim squares (two inner corners only), plain ArUco boards, occlusion inside a square. */
#define CBA_CHARUCO_STATUS_CORNER_OVERFLOW 1
#define CBA_CHARUCO_STATUS_CELL_OVERFLOW 2
#define CBA_MARKER_FLAG_DEGENERATE 1
#define CBA_MARKER_FLAG_WINDOW 2
#define CBA_MARKER_FLAG_LOW_CONTRAST 4
#define CBA_MARKER_FLAG_BORDER 8
#define CBA_MARKER_FLAG_NO_MATCH 16
typedef struct cba_charuco_board {
    int32_t squares_x, squares_y; /* >= 3 */
    int32_t marker_bits;          /* 3..7 */
    int32_t n_markers;            /* codes given */
    double square;                /* side of a square, > 0 */
    double marker_ratio;          /* marker side / square side, [0.4, 0.8] */
} cba_charuco_board;
typedef struct cba_charuco_options {
    double arm_lengths[2];
    double arm_offset;
    double arm_fan_deg;
    double min_arm_contrast;
    double min_marker_contrast;
    int32_t min_component;
    int32_t cell_samples;
    int32_t max_border_errors;
    int32_t max_correction;
    int32_t min_markers;
    int32_t reserved; /* 0 */
} cba_charuco_options;
typedef struct cba_marker_reading {
    uint64_t code;
    double level_min, level_max; /* smallest and largest cell mean */
    int32_t flags;               /* CBA_MARKER_FLAG_* */
    int32_t id, rotation, distance, second_distance, border_errors;
} cba_marker_reading;
void cba_charuco_options_default(cba_charuco_options* o);
typedef struct cba_charuco_detector cba_charuco_detector; /* opaque */
cba_status cba_charuco_detector_create(int32_t width, int32_t height, int32_t max_images, int32_t max_corners, int32_t max_cells,
                                       const cba_corner_options* corner_opts, const cba_charuco_options* charuco_opts,
                                       const cba_charuco_board* board, const uint64_t* codes /*[n_markers]*/, int32_t device,
                                       cba_charuco_detector** out);
cba_status cba_charuco_detector_process(cba_charuco_detector* h, int32_t n_images, const uint8_t* images, int32_t* out_count /*[n]*/,
                                        int32_t* out_status /*[n]*/, int32_t* out_ids /*[n][nb]*/, double* out_xy /*[n][nb][2]*/,
                                        int32_t* out_n_markers /*[n]*/, int32_t* out_n_corners /*[n]*/, int32_t* out_n_cells /*[1]*/,
                                        int32_t* out_cells /*[max_cells][4]*/, cba_marker_reading* out_readings /*[max_cells]*/);
cba_status cba_charuco_detector_arms(cba_charuco_detector* h, int32_t n_images, const double* dirs /*[n][max_corners][12][2]*/,
                                     double* out_score /*[n][max_corners]*/);
cba_status cba_charuco_detector_read(cba_charuco_detector* h, int32_t n_cells, const int32_t* cell_image /*[n_cells]*/,
                                     const double* quads /*[n_cells][4][2]*/, cba_marker_reading* out_readings /*[n_cells]*/);
void cba_charuco_detector_destroy(cba_charuco_detector* h);
cba_status cba_marker_dictionary_generate(int32_t bits, int32_t count, int32_t min_distance, uint64_t seed, uint64_t* codes /*[count]*/,
                                          int32_t* out_found);
cba_status cba_chessboard_lattice(int32_t n, const double* xy /*[n][2]*/, const double* angle /*[n]*/, int32_t min_component,
                                  int32_t* out_component /*[n]*/, int32_t* out_ij /*[n][2]*/, int32_t* out_n_components /*[1] or NULL*/);
cba_status cba_charuco_match(const cba_charuco_board* board, int32_t min_markers, int32_t n, const int32_t* component /*[n]*/,
                             const int32_t* ij /*[n][2]*/, const double* xy /*[n][2]*/, int32_t n_cells,
                             const int32_t* cells /*[n_cells][3]: component, i, j*/, const int32_t* flags /*[n_cells]*/,
                             const int32_t* id /*[n_cells]*/, const int32_t* rotation /*[n_cells]*/, int32_t* out_count /*[1]*/,
                             int32_t* out_ids /*[nb]*/, double* out_xy /*[nb][2]*/, int32_t* out_n_markers /*[1] or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* CALIBBA_H */
