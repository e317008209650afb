// capi_pipelines.cpp — the extern "C" entry points of the batched pipelines (include/calibba.h): laser-plane calibration, the linear
// seeds, the distortion fits, the camera models, triangulation, laser scanning, structured-light decoding, scan registration, scan fusion, stereo depth (block and
// semi-global matching) and chessboard detection.  Host-side duties only, as in capi.cpp: validate the arguments, find the device, call
// the pipeline (pipelines.hpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "capi_common.hpp"
#include "corner_grid.hpp"
#include "corner_math.hpp"
#include "blob_math.hpp"
#include "circle_grid.hpp"
#include "hom_ransac_math.hpp"
#include "linescan_math.hpp"
#include "marker_board.hpp"
#include "pipelines.hpp"
#include "stereo_math.hpp"
#include "structured_light_math.hpp"

using namespace cba;

#ifdef CBA_EXPERIMENTS
// a _timed entry point: its stage_ms must not be NULL
template <typename F>
static cba_status timed(const double* stage_ms, F&& call) {
    if (!stage_ms) { g_err = "null argument"; return CBA_ERR_INVALID_ARGUMENT; }
    return call();
}
#endif

extern "C" {

// ---- checks shared by the sections below --------------------------------------------------------------------------------------
// a camera argument: model, intrinsics, optional inverse coefficients
static void check_camera(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs) {
    if (camera_model != CBA_CAMERA_PINHOLE_BC && camera_model != CBA_CAMERA_SCHEIMPFLUG) throw std::invalid_argument("bad camera model");
    if (!intr) throw std::invalid_argument("null argument");
    if (inverse_coeffs && (n_inverse_coeffs < 2 || n_inverse_coeffs > LS_MAX_INV)) throw std::invalid_argument("n_inverse_coeffs must be in [2, 16]");
}
static void check_sides(int32_t w, int32_t h) {
    if (std::min(w, h) < 1 || std::max(w, h) > CBA_IMAGE_MAX_SIDE) throw std::invalid_argument("image width and height must be in [1, 32768]");
}

// the sizes of a handle for batches of images; name: "max_images" / "max_pairs".  The detectors check their sides first and their
// options before the rest, so they call check_sides themselves as well: here it then passes.
static void check_image_batch(int32_t width, int32_t height, int32_t max_n, const char* name) {
    check_sides(width, height);
    if (max_n < 1) throw std::invalid_argument(std::string(name) + " must be >= 1");
    if (static_cast<int64_t>(max_n) * width * height > 0x7fffffff) throw std::invalid_argument(std::string(name) + " is too large");
}

// the peak list of a detector; name: "max_corners" / "max_blobs"
static void check_peak_capacity(int32_t max_images, int32_t max_items, const char* name) {
    if (max_items < 1 || static_cast<int64_t>(max_images) * max_items > (1 << 28))
        throw std::invalid_argument(std::string(name) + " must be >= 1 and max_images " + name + " <= 2^28");
}

// The start of a handle's process call, after the null-handle test: n in [0, max_n] (what: "frames" / "pairs" / "images"), then the
// call's own check (other: its message when it fails, else nullptr), then false when n == 0 leaves nothing to do, then the images.
static bool check_batch_call(int32_t n, int32_t max_n, const char* what, const char* other, bool have_images) {
    if (n < 0 || n > max_n) throw std::invalid_argument(std::string("n_") + what + " must be in [0, max_" + what + "]");
    if (other) throw std::invalid_argument(other);
    if (n == 0) return false;
    if (!have_images) throw std::invalid_argument("null argument");
    return true;
}

// ---- laser-plane calibration (linescan.hip) --------------------------------------------------------------------------------
void cba_plane_fit_options_default(cba_plane_fit_options* o) {
    if (!o) return;
    o->use_ransac = 0;  // LineScanPlaneFitOptions (linescan.h:30-33), RansacOptions (ransac.h:23-30)
    o->max_iters = 1000;
    o->thresh = 2.0;
    o->min_inliers = 12;
    o->refit_on_inliers = 1;
    o->confidence = 0.99;
    o->seed = 1234567;
}

static void check_plane_fit_options(const cba_plane_fit_options* o) {
    if (!o) throw std::invalid_argument("null options");
    // max_iters: one lane and 10 partial sums per chunk for each hypothesis (the scoring grid is max_iters / 256 workgroups wide)
    if (o->use_ransac && (o->max_iters <= 0 || o->max_iters > CBA_PLANE_FIT_MAX_ITERS || !(o->thresh >= 0.0)))
        throw std::invalid_argument("bad RANSAC options (max_iters must be in [1, CBA_PLANE_FIT_MAX_ITERS], thresh >= 0)");
}

static cba_status laser_plane_impl(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                                   int32_t n_views, const int64_t* target_offset, const double* X, const double* Y, const double* u,
                                   const double* v, const int64_t* laser_offset, const double* laser_u, const double* laser_v,
                                   const cba_plane_fit_options* opts, cba_laser_plane_result* result, double* points_xyz,
                                   uint8_t* inlier_mask, double* stage_ms) {
    return guarded([&] {
        if (camera_model != CBA_CAMERA_PINHOLE_BC && camera_model != CBA_CAMERA_SCHEIMPFLUG) throw std::invalid_argument("bad camera model");
        if (!intr || !target_offset || !laser_offset || !result || (n_views > 0 && (!X || !Y || !u || !v)))
            throw std::invalid_argument("null argument");
        if (inverse_coeffs && (n_inverse_coeffs < 2 || n_inverse_coeffs > LS_MAX_INV)) throw std::invalid_argument("n_inverse_coeffs must be in [2, 16]");
        check_plane_fit_options(opts);
        // validate_observations (linescan.h:39-47)
        if (n_views < 2) throw std::invalid_argument("At least 2 views are required");
        if (target_offset[0] != 0 || laser_offset[0] != 0) throw std::invalid_argument("offsets must start at 0");
        // both tables start at 0; int32 groups of target points, laser pixels unlimited.  A loop of its own: the two tables and the
        // reference's count check are tested view by view, and the first failing view names the error
        for (int i = 0; i < n_views; ++i) {
            if (bad_offset_step(target_offset, i, OFF_INT32_GROUPS) || bad_offset_step(laser_offset, i, 0))
                throw std::invalid_argument("bad view offsets");
            if (target_offset[i + 1] - target_offset[i] < 4) throw std::invalid_argument("Each view requires >=4 target correspondences");
        }
        if (laser_offset[n_views] > 0 && (!laser_u || !laser_v)) throw std::invalid_argument("null argument");
        require_device();
        laser_plane_calibrate(camera_model, intr, n_inverse_coeffs, inverse_coeffs, n_views, target_offset, X, Y, u, v, laser_offset, laser_u,
                              laser_v, *opts, result, points_xyz, inlier_mask, stage_ms, default_device());
    });
}

cba_status cba_calibrate_laser_plane(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                                     int32_t n_views, const int64_t* target_offset, const double* X, const double* Y, const double* u,
                                     const double* v, const int64_t* laser_offset, const double* laser_u, const double* laser_v,
                                     const cba_plane_fit_options* opts, cba_laser_plane_result* result, double* points_xyz,
                                     uint8_t* inlier_mask) {
    return laser_plane_impl(camera_model, intr, n_inverse_coeffs, inverse_coeffs, n_views, target_offset, X, Y, u, v, laser_offset, laser_u,
                            laser_v, opts, result, points_xyz, inlier_mask, nullptr);
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_linescan.py): cba_calibrate_laser_plane without the optional outputs, timing its stages on
// the device: stage_ms [5] = per-view geometry, laser-point back-projection, the whole plane fit, RANSAC scoring pass 1
// (moments), RANSAC scoring pass 2 (recount).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_calibrate_laser_plane_timed(
    int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs, int32_t n_views, const int64_t* target_offset,
    const double* X, const double* Y, const double* u, const double* v, const int64_t* laser_offset, const double* laser_u, const double* laser_v,
    const cba_plane_fit_options* opts, cba_laser_plane_result* result, double* stage_ms) {
    return timed(stage_ms, [&] { return laser_plane_impl(camera_model, intr, n_inverse_coeffs, inverse_coeffs, n_views, target_offset, X, Y, u, v,
                                                         laser_offset, laser_u, laser_v, opts, result, nullptr, nullptr, stage_ms); });
}
#endif

cba_status cba_fit_plane(int64_t n, const double* xyz, const cba_plane_fit_options* opts, double* plane, double* inlier_rms,
                         int64_t* inlier_count, uint8_t* inlier_mask) {
    return guarded([&] {
        if (!xyz || !plane || !inlier_rms || !inlier_count) throw std::invalid_argument("null argument");
        check_plane_fit_options(opts);
        if (n < 3) throw std::invalid_argument("Not enough points to fit a plane");
        require_device();
        plane_fit(n, xyz, *opts, plane, inlier_rms, inlier_count, inlier_mask, default_device());
    });
}

// invert_brown_conrady (distortion.h:165-195) -> fit_distortion_full (:231-291) with K = identity: the 882 x n least-squares
// problem, solved by Householder QR (the reference's JacobiSVD solve; the design has full column rank).
cba_status cba_invert_brown_conrady(int32_t n, const double* forward, double* inverse) {
    return guarded([&] {
        if (!forward || !inverse) throw std::invalid_argument("null argument");
        if (n < 2) throw std::runtime_error("Insufficient distortion coefficients");
        const int nr = n - 2, grid = 21, m = 2 * grid * grid;
        std::vector<double> A(static_cast<size_t>(m) * n), b(m);
        auto distort = [&](double x, double y, double* xd, double* yd) {
            const double r2 = x * x + y * y;
            double radial = 1.0, rpow = r2;
            for (int i = 0; i < nr; ++i) { radial += forward[i] * rpow; rpow *= r2; }
            *xd = x * radial + 2.0 * forward[nr] * x * y + forward[nr + 1] * (r2 + 2.0 * x * x);
            *yd = y * radial + forward[nr] * (r2 + 2.0 * y * y) + 2.0 * forward[nr + 1] * x * y;
        };
        int row = 0;
        for (int i = 0; i < grid; ++i) {
            const double xu = -1.0 + 2.0 * static_cast<double>(i) / static_cast<double>(grid - 1);
            for (int j = 0; j < grid; ++j) {
                const double yu = -1.0 + 2.0 * static_cast<double>(j) / static_cast<double>(grid - 1);
                double x, y;  // observation: (x, y) = distorted, (u, v) = undistorted
                distort(xu, yu, &x, &y);
                const double r2 = x * x + y * y;
                double* au = &A[static_cast<size_t>(row) * n];
                double* av = &A[static_cast<size_t>(row + 1) * n];
                double rpow = r2;
                for (int k = 0; k < nr; ++k) { au[k] = x * rpow; av[k] = y * rpow; rpow *= r2; }
                au[nr] = 2.0 * x * y; au[nr + 1] = r2 + 2.0 * x * x;
                av[nr] = r2 + 2.0 * y * y; av[nr + 1] = 2.0 * x * y;
                b[row] = xu - x;
                b[row + 1] = yu - y;
                row += 2;
            }
        }
        // Householder QR of A (m x n, row-major), applied to b as it goes
        for (int k = 0; k < n; ++k) {
            double nrm = 0.0;
            for (int i = k; i < m; ++i) nrm += A[static_cast<size_t>(i) * n + k] * A[static_cast<size_t>(i) * n + k];
            nrm = std::sqrt(nrm);
            if (nrm == 0.0) throw std::runtime_error("rank-deficient distortion fit");
            const double akk = A[static_cast<size_t>(k) * n + k];
            const double alpha = akk > 0.0 ? -nrm : nrm;
            std::vector<double> w(m - k);
            for (int i = k; i < m; ++i) w[i - k] = A[static_cast<size_t>(i) * n + k];
            w[0] -= alpha;
            double ww = 0.0;
            for (double t : w) ww += t * t;
            for (int j = k; j < n; ++j) {
                double d = 0.0;
                for (int i = k; i < m; ++i) d += w[i - k] * A[static_cast<size_t>(i) * n + j];
                d = 2.0 * d / ww;
                for (int i = k; i < m; ++i) A[static_cast<size_t>(i) * n + j] -= d * w[i - k];
            }
            double d = 0.0;
            for (int i = k; i < m; ++i) d += w[i - k] * b[i];
            d = 2.0 * d / ww;
            for (int i = k; i < m; ++i) b[i] -= d * w[i - k];
        }
        for (int k = n - 1; k >= 0; --k) {
            double s = b[k];
            for (int j = k + 1; j < n; ++j) s -= A[static_cast<size_t>(k) * n + j] * inverse[j];
            inverse[k] = s / A[static_cast<size_t>(k) * n + k];
        }
    });
}

// ---- linear seed of planar intrinsic calibration (hom_ransac.hip, hom_ransac_math.hpp) ----------------------------------------
void cba_ransac_options_default(cba_ransac_options* o) {
    if (!o) return;
    o->max_iters = 1000;  // RansacOptions (ransac.h:23-30)
    o->thresh = 2.0;
    o->min_inliers = 12;
    o->refit_on_inliers = 1;
    o->confidence = 0.99;
    o->seed = 1234567;
}

static void check_views(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v) {
    if (n_views < 0 || !view_offset) throw std::invalid_argument("null argument");
    if (n_views > 0 && (!X || !Y || !u || !v)) throw std::invalid_argument("null argument");
    check_offsets(view_offset, n_views, "view ", OFF_FROM_ZERO | OFF_INT32_GROUPS);  // from 0, int32 groups
}

static void check_ransac_options(const cba_ransac_options* o) {
    // max_iters: one lane per hypothesis; the scoring grid is max_iters / 256 workgroups per view, each writing one candidate record
    if (o->max_iters < 0 || o->max_iters > CBA_RANSAC_MAX_ITERS || !(o->thresh >= 0.0))
        throw std::invalid_argument("bad RANSAC options (max_iters must be in [0, CBA_RANSAC_MAX_ITERS], thresh >= 0)");
}

// estimate_homography (optim/homography.cpp:45-60 with RansacOptions, :31-43 without)
cba_status cba_estimate_homography_ransac_batch(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y,
                                                const double* u, const double* v, const cba_ransac_options* opts, double* h9,
                                                int32_t* success, int32_t* inlier_count, double* symmetric_rms, uint8_t* inlier_mask) {
    return guarded([&] {
        check_views(n_views, view_offset, X, Y, u, v);
        if (!h9 || !success || !inlier_count || !symmetric_rms) throw std::invalid_argument("null argument");
        if (opts) check_ransac_options(opts);
        if (n_views == 0) return;
        require_device();
        homography_ransac_batch(n_views, view_offset, X, Y, u, v, opts, h9, success, inlier_count, symmetric_rms, inlier_mask,
                                default_device());
    });
}

static cba_status estimate_intrinsics_impl(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u,
                                           const double* v, int32_t use_ransac, const cba_ransac_options* ransac, const double* bounds_lo5,
                                           const double* bounds_hi5, int32_t* success, double* kmtx5, int32_t* sanitized,
                                           int32_t* view_ok, double* h9, double* forward_rms_px, double* rt12, int32_t* pose_ok,
                                           uint8_t* inlier_mask, double* stage_ms) {
    return guarded([&] {
        check_views(n_views, view_offset, X, Y, u, v);
        if (!success || !kmtx5 || !sanitized) throw std::invalid_argument("null argument");
        if (n_views > 0 && (!view_ok || !h9 || !forward_rms_px || !rt12 || !pose_ok)) throw std::invalid_argument("null argument");
        if (!bounds_lo5 != !bounds_hi5) throw std::invalid_argument("bounds_lo5 and bounds_hi5 must both be given or both be NULL");
        if (use_ransac) {
            if (!ransac) throw std::invalid_argument("null argument");
            check_ransac_options(ransac);
        }
        *success = 0;
        *sanitized = 0;
        for (int k = 0; k < 5; ++k) kmtx5[k] = 0.0;
        if (n_views == 0) return;  // intrinsicsdlt.cpp:104-106
        require_device();
        estimate_intrinsics_gpu(n_views, view_offset, X, Y, u, v, use_ransac ? ransac : nullptr, bounds_lo5, bounds_hi5, success, kmtx5,
                                sanitized, view_ok, h9, forward_rms_px, rt12, pose_ok, inlier_mask, stage_ms, default_device());
    });
}

cba_status cba_estimate_intrinsics(int32_t n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u,
                                   const double* v, int32_t use_ransac, const cba_ransac_options* ransac, const double* bounds_lo5,
                                   const double* bounds_hi5, int32_t use_skew, int32_t* success, double* kmtx5, int32_t* sanitized,
                                   int32_t* view_ok, double* h9, double* forward_rms_px, double* rt12, int32_t* pose_ok,
                                   uint8_t* inlier_mask) {
    (void)use_skew;  // IntrinsicsEstimOptions::use_skew is not read by estimate_intrinsics
    return estimate_intrinsics_impl(n_views, view_offset, X, Y, u, v, use_ransac, ransac, bounds_lo5, bounds_hi5, success, kmtx5, sanitized,
                                    view_ok, h9, forward_rms_px, rt12, pose_ok, inlier_mask, nullptr);
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_intrinsics_seed.py): cba_estimate_intrinsics timing its stages on the device: stage_ms [5] =
// homographies (the scoring kernel, or the DLT), homographies (selection, h22 rescale, symmetric rms), Zhang + sanitize, poses,
// total.  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_estimate_intrinsics_timed(
    int32_t n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v, int32_t use_ransac,
    const cba_ransac_options* ransac, int32_t* success, double* kmtx5, int32_t* view_ok, double* h9, double* forward_rms_px, double* rt12,
    int32_t* pose_ok, double* stage_ms) {
    int32_t sanitized = 0;
    return timed(stage_ms, [&] { return estimate_intrinsics_impl(n_views, view_offset, X, Y, u, v, use_ransac, ransac, nullptr, nullptr, success, kmtx5,
                                                                 &sanitized, view_ok, h9, forward_rms_px, rt12, pose_ok, nullptr, stage_ms); });
}
#endif

// zhang_intrinsics_from_hs (zhang.cpp:174-206), compiled for the host from the device header
cba_status cba_zhang_intrinsics_from_hs(int32_t n, const double* h9, double* kmtx5, int32_t* success) {
    return guarded([&] {
        if (n < 0 || (n > 0 && !h9) || !kmtx5 || !success) throw std::invalid_argument("null argument");
        double G[36] = {};
        for (int i = 0; i < n; ++i) hr_zhang_accumulate(h9 + 9 * static_cast<int64_t>(i), G);
        double k5[5];
        *success = hr_zhang_solve(n, G, k5) ? 1 : 0;
        if (*success)
            for (int k = 0; k < 5; ++k) kmtx5[k] = k5[k];
    });
}

cba_status cba_pose_from_homography(const double* kmtx5, const double* h9, double* rt12, int32_t* success, double* scale,
                                    double* cond_check) {
    return guarded([&] {
        if (!kmtx5 || !h9 || !rt12 || !success) throw std::invalid_argument("null argument");
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 0.0, c = 0.0;
        *success = hr_pose_from_homography(kmtx5, h9, R, t, &s, &c) ? 1 : 0;
        if (!*success) {
            const double id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            for (int a = 0; a < 9; ++a) R[a] = id[a];
            t[0] = t[1] = t[2] = 0.0;
        }
        for (int a = 0; a < 9; ++a) rt12[a] = R[a];
        for (int k = 0; k < 3; ++k) rt12[9 + k] = t[k];
        if (scale) *scale = s;
        if (cond_check) *cond_check = c;
    });
}

cba_status cba_sanitize_intrinsics(const double* kmtx5, const double* bounds_lo5, const double* bounds_hi5, double* out5,
                                   int32_t* modified) {
    return guarded([&] {
        if (!kmtx5 || !bounds_lo5 || !bounds_hi5 || !out5 || !modified) throw std::invalid_argument("null argument");
        *modified = hr_sanitize(kmtx5, bounds_lo5, bounds_hi5, out5) ? 1 : 0;
    });
}

// ---- linear seed of a multi-camera rig (extrinsic_dlt.hip, extrinsic_dlt_math.hpp) -------------------------------------------
static cba_status extrinsic_dlt_impl(int32_t n_cams, int32_t n_views, int32_t n_blocks, const int64_t* blk_offset, const int32_t* blk_view,
                                     const int32_t* blk_cam, const double* X, const double* Y, const double* u, const double* v,
                                     const double* kmtx5, double* c_T_r, double* r_T_t, double* blk_c_T_t, int32_t* blk_ok,
                                     double* stage_ms) {
    return guarded([&] {
        if (n_cams < 1 || n_views < 1) throw std::runtime_error("Empty views or cameras provided");  // extrinsics.h:31-33
        if (n_blocks < 0) throw std::invalid_argument("n_blocks must be >= 0");
        if (!blk_offset || !kmtx5 || !c_T_r || !r_T_t || (n_blocks > 0 && (!blk_view || !blk_cam))) throw std::invalid_argument("null argument");
        check_offsets(blk_offset, n_blocks, "block ", OFF_FROM_ZERO | OFF_INT32_GROUPS);  // from 0, int32 groups
        if (blk_offset[n_blocks] > 0 && (!X || !Y || !u || !v)) throw std::invalid_argument("null argument");
        // the (view, camera) -> block table: the averaging order of the device stages comes from it, never from the block order
        std::vector<int32_t> table(static_cast<size_t>(n_views) * static_cast<size_t>(n_cams), -1);
        for (int b = 0; b < n_blocks; ++b) {
            if (blk_view[b] < 0 || blk_view[b] >= n_views) throw std::invalid_argument("block " + std::to_string(b) + ": view index out of range");
            if (blk_cam[b] < 0 || blk_cam[b] >= n_cams) throw std::invalid_argument("block " + std::to_string(b) + ": camera index out of range");
            int32_t& slot = table[static_cast<size_t>(blk_view[b]) * static_cast<size_t>(n_cams) + static_cast<size_t>(blk_cam[b])];
            if (slot >= 0)
                throw std::invalid_argument("blocks " + std::to_string(slot) + " and " + std::to_string(b) + " share view " +
                                            std::to_string(blk_view[b]) + " and camera " + std::to_string(blk_cam[b]));
            slot = b;
        }
        if (n_blocks == 0) {  // every pose is the identity (extrinsics.h:55, 65)
            for (int64_t i = 0; i < n_cams; ++i)
                for (int k = 0; k < 7; ++k) c_T_r[7 * i + k] = k == 0 ? 1.0 : 0.0;
            for (int64_t i = 0; i < n_views; ++i)
                for (int k = 0; k < 7; ++k) r_T_t[7 * i + k] = k == 0 ? 1.0 : 0.0;
            if (stage_ms)
                for (int k = 0; k < 4; ++k) stage_ms[k] = 0.0;
            return;
        }
        require_device();
        extrinsic_dlt_gpu(n_cams, n_views, n_blocks, blk_offset, blk_cam, table.data(), X, Y, u, v, kmtx5, c_T_r, r_T_t, blk_c_T_t, blk_ok,
                          stage_ms, default_device());
    });
}

cba_status cba_estimate_extrinsic_dlt(int32_t n_cams, int32_t n_views, int32_t n_blocks, const int64_t* blk_offset, const int32_t* blk_view,
                                      const int32_t* blk_cam, const double* X, const double* Y, const double* u, const double* v,
                                      const double* kmtx5, double* c_T_r, double* r_T_t, double* blk_c_T_t, int32_t* blk_ok) {
    return extrinsic_dlt_impl(n_cams, n_views, n_blocks, blk_offset, blk_view, blk_cam, X, Y, u, v, kmtx5, c_T_r, r_T_t, blk_c_T_t, blk_ok,
                              nullptr);
}

// ---- seed of the hand-eye and bundle stages (bundle_seed.hip, bundle_seed_math.hpp) ------------------------------------------
static cba_status bundle_seed_impl(int32_t n_cams, int32_t n_blocks, const int64_t* blk_offset, const int32_t* blk_cam, const double* blk_b_T_g,
                                   const double* X, const double* Y, const double* u, const double* v, const double* kmtx5,
                                   double min_angle_deg, const int32_t* given_mask, const double* g_T_c_given, const double* b_T_t_given,
                                   double* g_T_c, int32_t* cam_status, int32_t* cam_pairs, double* b_T_t, int32_t* target_source,
                                   double* blk_c_T_t, int32_t* blk_ok, double* stage_ms) {
    return guarded([&] {
        if (n_cams < 1) throw std::invalid_argument("n_cams must be >= 1");
        if (n_blocks < 0) throw std::invalid_argument("n_blocks must be >= 0");
        if (!(min_angle_deg >= 0.0) || !std::isfinite(min_angle_deg)) throw std::invalid_argument("min_angle_deg must be finite and >= 0");
        if (!blk_offset || !kmtx5 || !g_T_c || !cam_status || !cam_pairs || !b_T_t || !target_source ||
            (n_blocks > 0 && (!blk_cam || !blk_b_T_g)))
            throw std::invalid_argument("null argument");
        if (given_mask && !g_T_c_given) throw std::invalid_argument("given_mask needs g_T_c_given");
        check_offsets(blk_offset, n_blocks, "block ", OFF_FROM_ZERO | OFF_INT32_GROUPS);  // from 0, int32 groups
        if (blk_offset[n_blocks] > 0 && (!X || !Y || !u || !v)) throw std::invalid_argument("null argument");
        for (int b = 0; b < n_blocks; ++b)
            if (blk_cam[b] < 0 || blk_cam[b] >= n_cams) throw std::invalid_argument("block " + std::to_string(b) + ": camera index out of range");
        // each camera's pose list: its blocks of >= 4 points in increasing block index (the reference's SensorAccumulator)
        std::vector<int32_t> cam_start(static_cast<size_t>(n_cams) + 1, 0), cam_blk;
        for (int b = 0; b < n_blocks; ++b)
            if (blk_offset[b + 1] - blk_offset[b] >= 4) ++cam_start[static_cast<size_t>(blk_cam[b]) + 1];
        for (int c = 0; c < n_cams; ++c) cam_start[c + 1] += cam_start[c];
        cam_blk.resize(static_cast<size_t>(cam_start[n_cams]));
        {
            std::vector<int32_t> fill(cam_start.begin(), cam_start.end() - 1);
            for (int b = 0; b < n_blocks; ++b)
                if (blk_offset[b + 1] - blk_offset[b] >= 4) cam_blk[fill[blk_cam[b]]++] = b;
        }
        // statuses the host decides; the device overwrites the DLT cameras'
        for (int c = 0; c < n_cams; ++c) {
            double* g = g_T_c + 7 * static_cast<int64_t>(c);
            cam_pairs[c] = 0;
            if (given_mask && given_mask[c]) {
                for (int k = 0; k < 7; ++k) g[k] = g_T_c_given[7 * static_cast<int64_t>(c) + k];
                cam_status[c] = CBA_HANDEYE_GIVEN;
                continue;
            }
            for (int k = 0; k < 7; ++k) g[k] = k == 0 ? 1.0 : 0.0;
            cam_status[c] = cam_start[c + 1] - cam_start[c] >= 2 ? CBA_HANDEYE_DLT : CBA_HANDEYE_TOO_FEW_VIEWS;
        }
        if (b_T_t_given) {
            for (int k = 0; k < 7; ++k) b_T_t[k] = b_T_t_given[k];
            *target_source = CBA_TARGET_CONFIG;
        } else {
            for (int k = 0; k < 7; ++k) b_T_t[k] = k == 0 ? 1.0 : 0.0;
            *target_source = cam_start[n_cams] > 0 ? CBA_TARGET_ESTIMATED : CBA_TARGET_IDENTITY;
        }
        if (stage_ms)
            for (int k = 0; k < 6; ++k) stage_ms[k] = 0.0;
        if (n_blocks == 0) return;  // nothing for a device to do
        require_device();
        bundle_seed_gpu(n_cams, n_blocks, blk_offset, blk_cam, blk_b_T_g, X, Y, u, v, kmtx5, min_angle_deg, cam_start.data(), cam_blk.data(),
                        g_T_c, cam_status, cam_pairs, b_T_t_given, b_T_t, blk_c_T_t, blk_ok, stage_ms, default_device());
    });
}

cba_status cba_estimate_bundle_seed(int32_t n_cams, int32_t n_blocks, const int64_t* blk_offset, const int32_t* blk_cam, const double* blk_b_T_g,
                                    const double* X, const double* Y, const double* u, const double* v, const double* kmtx5,
                                    double min_angle_deg, const int32_t* given_mask, const double* g_T_c_given, const double* b_T_t_given,
                                    double* g_T_c, int32_t* cam_status, int32_t* cam_pairs, double* b_T_t, int32_t* target_source,
                                    double* blk_c_T_t, int32_t* blk_ok) {
    return bundle_seed_impl(n_cams, n_blocks, blk_offset, blk_cam, blk_b_T_g, X, Y, u, v, kmtx5, min_angle_deg, given_mask, g_T_c_given,
                            b_T_t_given, g_T_c, cam_status, cam_pairs, b_T_t, target_source, blk_c_T_t, blk_ok, nullptr);
}

// ---- distortion fits and the linear intrinsic estimators (distortion_fit.hip, distortion_fit_math.hpp) ----------------------
static void check_problems(int32_t n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v) {
    if (n_problems < 0) throw std::invalid_argument("n_problems must be >= 0");
    if (n_problems == 0) return;
    if (!offset) throw std::invalid_argument("null argument");
    check_offsets(offset, n_problems, "", OFF_FROM_ZERO);  // from 0, groups of any size (the chunked kernels index in int64)
    if (offset[n_problems] > 0 && (!x || !y || !u || !v)) throw std::invalid_argument("null argument");
}

static void check_num_radial(int32_t num_radial) {
    if (num_radial < 0 || num_radial > 3) throw std::invalid_argument("num_radial must be in [0, 3]");
}

static cba_status fit_distortion_impl(int32_t n_problems, const int64_t* offset, const double* x, const double* y, const double* u,
                                      const double* v, const double* kmtx5, int32_t num_radial, int32_t n_fixed, const int32_t* fixed_idx,
                                      const double* fixed_val, int32_t dual, double* coeffs, double* inverse, int32_t* ok,
                                      double* residuals, double* stage_ms) {
    return guarded([&] {
        check_problems(n_problems, offset, x, y, u, v);
        check_num_radial(num_radial);
        const int m = num_radial + 2;
        if (n_fixed < 0) throw std::invalid_argument("n_fixed must be >= 0");
        if (n_fixed > 0 && !fixed_idx) throw std::invalid_argument("null argument");
        int mask = 0;
        double val[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < n_fixed; ++i) {
            const int idx = fixed_idx[i];
            if (idx < 0 || idx >= m) throw std::invalid_argument("Fixed distortion index out of range");
            if (mask >> idx & 1) continue;  // the first in input order wins
            mask |= 1 << idx;
            val[idx] = fixed_val ? fixed_val[i] : 0.0;
        }
        if (dual && !inverse) throw std::invalid_argument("dual needs inverse");
        if (stage_ms)
            for (int k = 0; k < 6; ++k) stage_ms[k] = 0.0;
        if (n_problems == 0) return;
        if (!kmtx5 || !coeffs || !ok) throw std::invalid_argument("null argument");
        require_device();
        distortion_fit_gpu(n_problems, offset, x, y, u, v, kmtx5, num_radial, mask, val, dual != 0, coeffs, inverse, ok, residuals, stage_ms,
                           default_device());
    });
}

cba_status cba_fit_distortion_batch(int32_t n_problems, const int64_t* offset, const double* x, const double* y, const double* u,
                                    const double* v, const double* kmtx5, int32_t num_radial, int32_t n_fixed, const int32_t* fixed_idx,
                                    const double* fixed_val, int32_t dual, double* coeffs, double* inverse, int32_t* ok, double* residuals) {
    return fit_distortion_impl(n_problems, offset, x, y, u, v, kmtx5, num_radial, n_fixed, fixed_idx, fixed_val, dual, coeffs, inverse, ok,
                               residuals, nullptr);
}

cba_status cba_estimate_intrinsics_linear_batch(int32_t n_problems, const int64_t* offset, const double* x, const double* y,
                                                const double* u, const double* v, const double* bounds_lo5, const double* bounds_hi5,
                                                int32_t use_skew, double* kmtx5, int32_t* status, int32_t* fallback) {
    return guarded([&] {
        check_problems(n_problems, offset, x, y, u, v);
        if (!bounds_lo5 != !bounds_hi5) throw std::invalid_argument("bounds_lo5 and bounds_hi5 go together");
        if (n_problems == 0) return;
        if (!kmtx5 || !status || !fallback) throw std::invalid_argument("null argument");
        const double dlo[5] = {0.0, 0.0, 0.0, 0.0, -0.01}, dhi[5] = {2000.0, 2000.0, 1280.0, 720.0, 0.01};  // CalibrationBounds{}
        require_device();
        intrinsics_linear_gpu(n_problems, offset, x, y, u, v, bounds_lo5 ? bounds_lo5 : dlo, bounds_hi5 ? bounds_hi5 : dhi, use_skew != 0,
                              kmtx5, status, fallback, default_device());
    });
}

static cba_status linear_iterative_impl(int32_t n_problems, const int64_t* offset, const double* x, const double* y, const double* u,
                                        const double* v, int32_t num_radial, int32_t max_iterations, int32_t use_skew, double* kmtx5,
                                        double* coeffs, int32_t* status, int32_t* iterations, int32_t* fallback, double* stage_ms) {
    return guarded([&] {
        check_problems(n_problems, offset, x, y, u, v);
        check_num_radial(num_radial);
        if (max_iterations > CBA_LINEAR_MAX_ITERATIONS) throw std::invalid_argument("max_iterations above CBA_LINEAR_MAX_ITERATIONS");
        if (stage_ms)
            for (int k = 0; k < 6; ++k) stage_ms[k] = 0.0;
        if (n_problems == 0) return;
        if (!kmtx5 || !coeffs || !status || !iterations || !fallback) throw std::invalid_argument("null argument");
        require_device();
        intrinsics_linear_iterative_gpu(n_problems, offset, x, y, u, v, num_radial, std::max(max_iterations, 0), use_skew != 0, kmtx5, coeffs,
                                        status, iterations, fallback, stage_ms, default_device());
    });
}

cba_status cba_estimate_intrinsics_linear_iterative_batch(int32_t n_problems, const int64_t* offset, const double* x, const double* y,
                                                          const double* u, const double* v, int32_t num_radial, int32_t max_iterations,
                                                          int32_t use_skew, double* kmtx5, double* coeffs, int32_t* status,
                                                          int32_t* iterations, int32_t* fallback) {
    return linear_iterative_impl(n_problems, offset, x, y, u, v, num_radial, max_iterations, use_skew, kmtx5, coeffs, status, iterations,
                                 fallback, nullptr);
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_extrinsic_seed.py): cba_estimate_extrinsic_dlt timing its stages on the device: stage_ms [4] =
// block poses, camera averages, target averages, total (uploads excluded).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_estimate_extrinsic_dlt_timed(
    int32_t n_cams, int32_t n_views, int32_t n_blocks, const int64_t* blk_offset, const int32_t* blk_view, const int32_t* blk_cam,
    const double* X, const double* Y, const double* u, const double* v, const double* kmtx5, double* c_T_r, double* r_T_t, double* stage_ms) {
    return timed(stage_ms, [&] { return extrinsic_dlt_impl(n_cams, n_views, n_blocks, blk_offset, blk_view, blk_cam, X, Y, u, v, kmtx5, c_T_r, r_T_t,
                                                           nullptr, nullptr, stage_ms); });
}

// Experiment builds only (tools/bench_bundle_seed.py): cba_estimate_bundle_seed timing its stages on the device: stage_ms [6] =
// block poses, pass 1 + rotation solve, pass 2 + translation solve, candidates + scan, total, scan alone (uploads excluded).
// Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_estimate_bundle_seed_timed(
    int32_t n_cams, int32_t n_blocks, const int64_t* blk_offset, const int32_t* blk_cam, const double* blk_b_T_g, const double* X,
    const double* Y, const double* u, const double* v, const double* kmtx5, double min_angle_deg, double* g_T_c, int32_t* cam_status,
    int32_t* cam_pairs, double* b_T_t, int32_t* target_source, double* stage_ms) {
    return timed(stage_ms, [&] { return bundle_seed_impl(n_cams, n_blocks, blk_offset, blk_cam, blk_b_T_g, X, Y, u, v, kmtx5, min_angle_deg, nullptr, nullptr,
                                                         nullptr, g_T_c, cam_status, cam_pairs, b_T_t, target_source, nullptr, nullptr, stage_ms); });
}
// Experiment builds only (tools/bench_distortion.py): the distortion fit and the iterative estimator timing their stages on the
// device: stage_ms [6] = moment passes, chunk sums, uploads, tail, residuals, total without uploads.  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_fit_distortion_batch_timed(
    int32_t n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v, const double* kmtx5,
    int32_t num_radial, int32_t dual, double* coeffs, double* inverse, int32_t* ok, double* residuals, double* stage_ms) {
    return timed(stage_ms, [&] { return fit_distortion_impl(n_problems, offset, x, y, u, v, kmtx5, num_radial, 0, nullptr, nullptr, dual, coeffs, inverse,
                                                            ok, residuals, stage_ms); });
}

__attribute__((visibility("default"))) cba_status cba_estimate_intrinsics_linear_iterative_batch_timed(
    int32_t n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v, int32_t num_radial,
    int32_t max_iterations, int32_t use_skew, double* kmtx5, double* coeffs, int32_t* status, int32_t* iterations, int32_t* fallback,
    double* stage_ms) {
    return timed(stage_ms, [&] { return linear_iterative_impl(n_problems, offset, x, y, u, v, num_radial, max_iterations, use_skew, kmtx5, coeffs, status,
                                                              iterations, fallback, stage_ms); });
}
#endif

// ---- camera models (camera.hip, camera_math.hpp) ----------------------------------------------------------------------------
static cba_status camera_project_impl(int32_t camera_model, const double* intr, int64_t n, const double* xyz, double* uv, double* stage_ms) {
    return guarded([&] {
        check_camera(camera_model, intr, 0, nullptr);
        if (n < 0) throw std::invalid_argument("n must be >= 0");
        if (n == 0) return;
        if (!xyz || !uv) throw std::invalid_argument("null argument");
        require_device();
        camera_project_gpu(camera_model, intr, n, xyz, uv, stage_ms, default_device());
    });
}

static cba_status camera_unproject_impl(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                                        int64_t n, const double* uv, double* xy, double* stage_ms) {
    return guarded([&] {
        check_camera(camera_model, intr, n_inverse_coeffs, inverse_coeffs);
        if (n < 0) throw std::invalid_argument("n must be >= 0");
        if (n == 0) return;
        if (!uv || !xy) throw std::invalid_argument("null argument");
        require_device();
        camera_unproject_gpu(camera_model, intr, inverse_coeffs ? n_inverse_coeffs : 0, inverse_coeffs, n, uv, xy, stage_ms, default_device());
    });
}

cba_status cba_camera_project(int32_t camera_model, const double* intr, int64_t n, const double* xyz, double* uv) {
    return camera_project_impl(camera_model, intr, n, xyz, uv, nullptr);
}

cba_status cba_camera_unproject(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs, int64_t n,
                                const double* uv, double* xy) {
    return camera_unproject_impl(camera_model, intr, n_inverse_coeffs, inverse_coeffs, n, uv, xy, nullptr);
}

static cba_status undistort_map_create_impl(int32_t camera_model, int32_t n_cams, const double* intr, const double* R, const double* new_k5,
                                            int32_t width, int32_t height, int32_t device, cba_undistort_map** out, double* stage_ms) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        check_camera(camera_model, intr, 0, nullptr);
        if (n_cams < 1) throw std::invalid_argument("n_cams must be >= 1");
        check_sides(width, height);
        const int ni = cam_intr_size(camera_model);
        for (int c = 0; c < n_cams; ++c) {
            const double* k = new_k5 ? new_k5 + 5 * static_cast<size_t>(c) : intr + static_cast<size_t>(c) * ni;
            if (k[0] == 0.0 || k[1] == 0.0) throw std::invalid_argument("fx' and fy' must not be 0");
        }
        require_device(device);
        *out = reinterpret_cast<cba_undistort_map*>(undistort_map_create(camera_model, n_cams, intr, R, new_k5, width, height, stage_ms, device));
    });
}

cba_status cba_undistort_map_create(int32_t camera_model, int32_t n_cams, const double* intr, const double* R, const double* new_k5,
                                    int32_t width, int32_t height, int32_t device, cba_undistort_map** out) {
    return undistort_map_create_impl(camera_model, n_cams, intr, R, new_k5, width, height, device, out, nullptr);
}

cba_status cba_undistort_map_fetch(cba_undistort_map* h, float* map_x, float* map_y) {
    return guarded([&] {
        if (!h || !map_x || !map_y) throw std::invalid_argument("null argument");
        undistort_map_fetch(reinterpret_cast<UndistortMap*>(h), map_x, map_y);
    });
}

static cba_status undistort_map_apply_impl(cba_undistort_map* h, int32_t n_images, const int32_t* cam, int32_t src_width, int32_t src_height,
                                           int32_t channels, int32_t dtype, double border, const void* src, void* dst, double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        if (n_images < 0) throw std::invalid_argument("n_images must be >= 0");
        check_sides(src_width, src_height);
        if (channels < 1 || channels > 4) throw std::invalid_argument("channels must be in 1..4");
        if (dtype != CBA_DTYPE_U8 && dtype != CBA_DTYPE_F32) throw std::invalid_argument("unknown dtype");
        if (n_images == 0) return;
        if (!cam || !src || !dst) throw std::invalid_argument("null argument");
        UndistortMap* m = reinterpret_cast<UndistortMap*>(h);
        const int n_cams = undistort_map_cams(m);
        for (int i = 0; i < n_images; ++i)
            if (cam[i] < 0 || cam[i] >= n_cams) throw std::invalid_argument("camera index out of range");
        undistort_map_apply(m, n_images, cam, src_width, src_height, channels, dtype, border, src, dst, stage_ms);
    });
}

cba_status cba_undistort_map_apply(cba_undistort_map* h, int32_t n_images, const int32_t* cam, int32_t src_width, int32_t src_height,
                                   int32_t channels, int32_t dtype, double border, const void* src, void* dst) {
    return undistort_map_apply_impl(h, n_images, cam, src_width, src_height, channels, dtype, border, src, dst, nullptr);
}

void cba_undistort_map_destroy(cba_undistort_map* h) { undistort_map_destroy(reinterpret_cast<UndistortMap*>(h)); }

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_camera.py): the camera entry points timing their stages on the device: stage_ms [3] = upload,
// kernel, download.  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_camera_project_timed(int32_t camera_model, const double* intr, int64_t n,
                                                                           const double* xyz, double* uv, double* stage_ms) {
    return timed(stage_ms, [&] { return camera_project_impl(camera_model, intr, n, xyz, uv, stage_ms); });
}
__attribute__((visibility("default"))) cba_status cba_camera_unproject_timed(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs,
                                                                             const double* inverse_coeffs, int64_t n, const double* uv,
                                                                             double* xy, double* stage_ms) {
    return timed(stage_ms, [&] { return camera_unproject_impl(camera_model, intr, n_inverse_coeffs, inverse_coeffs, n, uv, xy, stage_ms); });
}
__attribute__((visibility("default"))) cba_status cba_undistort_map_create_timed(int32_t camera_model, int32_t n_cams, const double* intr,
                                                                                 const double* R, const double* new_k5, int32_t width,
                                                                                 int32_t height, int32_t device, cba_undistort_map** out,
                                                                                 double* stage_ms) {
    return timed(stage_ms, [&] { return undistort_map_create_impl(camera_model, n_cams, intr, R, new_k5, width, height, device, out, stage_ms); });
}
__attribute__((visibility("default"))) cba_status cba_undistort_map_apply_timed(cba_undistort_map* h, int32_t n_images, const int32_t* cam,
                                                                                int32_t src_width, int32_t src_height, int32_t channels,
                                                                                int32_t dtype, double border, const void* src, void* dst,
                                                                                double* stage_ms) {
    return timed(stage_ms, [&] { return undistort_map_apply_impl(h, n_images, cam, src_width, src_height, channels, dtype, border, src, dst, stage_ms); });
}
#endif

// ---- multi-camera triangulation (triangulate.hip, tri_math.hpp) ---------------------------------------------------------------
void cba_triangulate_options_default(cba_triangulate_options* o) {
    if (!o) return;
    o->max_iterations = 10;
    o->step_tolerance = 1e-12;
    o->min_cams = 2;
    o->max_reproj_px = std::numeric_limits<double>::infinity();
}

// the cameras and the options of a triangulation (shared with cba_sl_decoder_set_rig), in the order cba_triangulate checks them
static void check_tri_cameras(int32_t camera_model, int32_t n_cams, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                              const double* c_T_r, const cba_triangulate_options* opts) {
    check_camera(camera_model, intr, n_inverse_coeffs, inverse_coeffs);
    if (n_cams < 2 || n_cams > CBA_TRI_MAX_CAMS) throw std::invalid_argument("n_cams must be in [2, 16]");
    if (!c_T_r || !opts) throw std::invalid_argument("null argument");
    const int ni = cam_intr_size(camera_model);
    for (int c = 0; c < n_cams; ++c)
        if (intr[static_cast<size_t>(c) * ni] == 0.0 || intr[static_cast<size_t>(c) * ni + 1] == 0.0)
            throw std::invalid_argument("fx and fy must not be 0");
}
static void check_tri_options(const cba_triangulate_options* opts) {
    if (opts->max_iterations < 0) throw std::invalid_argument("max_iterations must be >= 0");
    if (!(opts->step_tolerance >= 0.0)) throw std::invalid_argument("step_tolerance must be >= 0");
    if (!(opts->max_reproj_px > 0.0)) throw std::invalid_argument("max_reproj_px must be > 0");
}

static cba_status triangulate_impl(int32_t camera_model, int32_t n_cams, const double* intr, int32_t n_inverse_coeffs,
                                   const double* inverse_coeffs, const double* c_T_r, int64_t n, const double* uv,
                                   const cba_triangulate_options* opts, double* xyz, double* rms_px, uint32_t* used_mask, int32_t* status,
                                   double* cov6, int32_t* linearisations, double* stage_ms) {
    return guarded([&] {
        check_tri_cameras(camera_model, n_cams, intr, n_inverse_coeffs, inverse_coeffs, c_T_r, opts);
        if (n < 0) throw std::invalid_argument("n must be >= 0");
        check_tri_options(opts);
        if (n == 0) return;
        if (!uv || !xyz || !status) throw std::invalid_argument("null argument");
        require_device();
        triangulate_gpu(camera_model, n_cams, intr, inverse_coeffs ? n_inverse_coeffs : 0, inverse_coeffs, c_T_r, n, uv, *opts, xyz, rms_px,
                        used_mask, status, cov6, linearisations, stage_ms, default_device());
    });
}

cba_status cba_triangulate(int32_t camera_model, int32_t n_cams, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                           const double* c_T_r, int64_t n, const double* uv, const cba_triangulate_options* opts, double* xyz,
                           double* rms_px, uint32_t* used_mask, int32_t* status, double* cov6) {
    return triangulate_impl(camera_model, n_cams, intr, n_inverse_coeffs, inverse_coeffs, c_T_r, n, uv, opts, xyz, rms_px, used_mask, status,
                            cov6, nullptr, nullptr);
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_triangulate.py): cba_triangulate timing its stages on the device (stage_ms [3] = upload,
// kernel, download) and returning each point's number of linearisations.  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_triangulate_timed(int32_t camera_model, int32_t n_cams, const double* intr,
                                                                        int32_t n_inverse_coeffs, const double* inverse_coeffs,
                                                                        const double* c_T_r, int64_t n, const double* uv,
                                                                        const cba_triangulate_options* opts, double* xyz, double* rms_px,
                                                                        uint32_t* used_mask, int32_t* status, double* cov6,
                                                                        int32_t* linearisations, double* stage_ms) {
    return timed(stage_ms, [&] { return triangulate_impl(camera_model, n_cams, intr, n_inverse_coeffs, inverse_coeffs, c_T_r, n, uv, opts, xyz, rms_px,
                                                         used_mask, status, cov6, linearisations, stage_ms); });
}
#endif

// ---- laser profile scanning (laser_scan.hip, laser_scan_math.hpp) ---------------------------------------------------------------
void cba_laser_scan_options_default(cba_laser_scan_options* o) {
    if (!o) return;
    o->axis = 0;
    o->roi_begin = 0;
    o->roi_end = 0;
    o->half_window = 5;
    o->floor_level = 0.0;
    o->min_peak = 1.0;
}

static void check_laser_plane(const double* plane) {
    if (!plane) throw std::invalid_argument("null argument");
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(plane[k])) throw std::invalid_argument("the plane must be finite");
    if (plane[0] == 0.0 && plane[1] == 0.0 && plane[2] == 0.0) throw std::invalid_argument("the plane normal must not be zero");
}

cba_status cba_laser_points(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                            const double plane[4], int64_t n, const double* uv, int32_t n_frames, const int64_t* frame_offset,
                            const double* frame_pose7, double* xyz, double* plane_xy) {
    return guarded([&] {
        check_camera(camera_model, intr, n_inverse_coeffs, inverse_coeffs);
        check_laser_plane(plane);
        if (n < 0) throw std::invalid_argument("n must be >= 0");
        if (n_frames < 0) throw std::invalid_argument("n_frames must be >= 0");
        if (frame_pose7 && !frame_offset && n_frames != 1) throw std::invalid_argument("frame_pose7 without frame_offset needs n_frames == 1");
        if (frame_offset) {
            check_offsets(frame_offset, n_frames, "frame ", OFF_FROM_ZERO);
            if (frame_offset[n_frames] != n) throw std::invalid_argument("frame offsets must end at n");
        }
        if (n == 0) return;
        if (!uv || !xyz) throw std::invalid_argument("null argument");
        require_device();
        const int64_t single[2] = {0, n};  // one posed frame without a table
        laser_points_gpu(camera_model, intr, inverse_coeffs ? n_inverse_coeffs : 0, inverse_coeffs, plane, n, uv, n_frames,
                         frame_pose7 ? (frame_offset ? frame_offset : single) : nullptr, frame_pose7, xyz, plane_xy, default_device());
    });
}

cba_status cba_laser_scanner_create(int32_t camera_model, const double* intr, int32_t n_inverse_coeffs, const double* inverse_coeffs,
                                    const double plane[4], int32_t width, int32_t height, int32_t max_frames,
                                    const cba_laser_scan_options* opts, int32_t device, cba_laser_scanner** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        check_camera(camera_model, intr, n_inverse_coeffs, inverse_coeffs);
        check_laser_plane(plane);
        if (!opts) throw std::invalid_argument("null argument");
        check_sides(width, height);
        if (max_frames < 1) throw std::invalid_argument("max_frames must be >= 1");
        if (opts->axis != 0 && opts->axis != 1) throw std::invalid_argument("axis must be 0 or 1");
        const int32_t side = opts->axis == 0 ? height : width;
        if (!(opts->roi_begin == 0 && opts->roi_end == 0) && (opts->roi_begin < 0 || opts->roi_end > side || opts->roi_begin >= opts->roi_end))
            throw std::invalid_argument("the ROI must be a non-empty range inside the image");
        if (opts->half_window < 0) throw std::invalid_argument("half_window must be >= 0");
        if (!std::isfinite(opts->floor_level) || !std::isfinite(opts->min_peak))
            throw std::invalid_argument("floor_level and min_peak must be finite");
        if (static_cast<int64_t>(max_frames) * std::max(width, height) > 0x7fffffff) throw std::invalid_argument("max_frames is too large");
        require_device(device);
        *out = reinterpret_cast<cba_laser_scanner*>(laser_scanner_create(camera_model, intr, inverse_coeffs ? n_inverse_coeffs : 0,
                                                                          inverse_coeffs, plane, width, height, max_frames, *opts, device));
    });
}

static cba_status laser_scanner_process_impl(cba_laser_scanner* h, int32_t n_frames, int32_t dtype, const void* images,
                                             const double* frame_pose7, double* centre, double* amplitude, double* width_px, double* xyz,
                                             double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        LaserScanner* sc = reinterpret_cast<LaserScanner*>(h);
        const char* bad_dtype = dtype != CBA_DTYPE_U8 && dtype != CBA_DTYPE_F32 ? "unknown dtype" : nullptr;
        if (!check_batch_call(n_frames, laser_scanner_max_frames(sc), "frames", bad_dtype, images != nullptr)) return;
        laser_scanner_process(sc, n_frames, dtype, images, frame_pose7, centre, amplitude, width_px, xyz, stage_ms);
    });
}

cba_status cba_laser_scanner_process(cba_laser_scanner* h, int32_t n_frames, int32_t dtype, const void* images, const double* frame_pose7,
                                     double* centre, double* amplitude, double* width_px, double* xyz) {
    return laser_scanner_process_impl(h, n_frames, dtype, images, frame_pose7, centre, amplitude, width_px, xyz, nullptr);
}

void cba_laser_scanner_destroy(cba_laser_scanner* h) { laser_scanner_destroy(reinterpret_cast<LaserScanner*>(h)); }

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_laser_scan.py): cba_laser_scanner_process timing its stages on the device (stage_ms [3] = upload,
// kernel, download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_laser_scanner_process_timed(cba_laser_scanner* h, int32_t n_frames, int32_t dtype,
                                                                                  const void* images, const double* frame_pose7,
                                                                                  double* centre, double* amplitude, double* width_px,
                                                                                  double* xyz, double* stage_ms) {
    return timed(stage_ms, [&] { return laser_scanner_process_impl(h, n_frames, dtype, images, frame_pose7, centre, amplitude, width_px, xyz, stage_ms); });
}
#endif

// ---- structured-light scanning (structured_light.hip, structured_light_math.hpp) ------------------------------------------------
void cba_sl_options_default(cba_sl_options* o) {
    if (!o) return;
    o->proj_width = 0;
    o->proj_height = 0;
    o->axes = 3;
    o->gray_skip_bits = 0;
    o->phase_steps = 0;
    o->phase_period = 16;
    o->min_contrast = 10;
    o->min_bit_diff = 4;
    o->min_modulation = 5.0;
}

static void check_sl_options(const cba_sl_options* o) {
    if (!o) throw std::invalid_argument("null argument");
    if (std::min(o->proj_width, o->proj_height) < 2 || std::max(o->proj_width, o->proj_height) > CBA_IMAGE_MAX_SIDE)
        throw std::invalid_argument("proj_width and proj_height must be in [2, 32768]");
    if (o->axes < 1 || o->axes > 3) throw std::invalid_argument("axes must be 1, 2 or 3");
    if (o->gray_skip_bits < 0) throw std::invalid_argument("gray_skip_bits must be >= 0");
    if (o->phase_steps != 0 && (o->phase_steps < 3 || o->phase_steps > SL_MAX_STEPS)) throw std::invalid_argument("phase_steps must be 0 or in 3..8");
    if (o->min_contrast < 0 || o->min_contrast > 255 || o->min_bit_diff < 0 || o->min_bit_diff > 255)
        throw std::invalid_argument("min_contrast and min_bit_diff must be in 0..255");
    if (!std::isfinite(o->min_modulation) || !(o->min_modulation >= 0.0)) throw std::invalid_argument("min_modulation must be finite and >= 0");
    for (int a = 0; a < 2; ++a)
        if ((o->axes >> a & 1) && (o->gray_skip_bits > 15 || sl_nbits(a == 0 ? o->proj_width : o->proj_height, o->gray_skip_bits) < 1))
            throw std::invalid_argument("gray_skip_bits leaves no Gray plane");
    if (o->phase_steps > 0 && (o->phase_period < 1 || o->phase_period > CBA_IMAGE_MAX_SIDE || o->phase_period < (2 << o->gray_skip_bits)))
        throw std::invalid_argument("phase_period must be in [2^(gray_skip_bits + 1), 32768]");
}

cba_status cba_sl_image_count(const cba_sl_options* opts, int32_t* n_images) {
    return guarded([&] {
        check_sl_options(opts);
        if (!n_images) throw std::invalid_argument("null argument");
        *n_images = sl_options_image_count(*opts);
    });
}

cba_status cba_sl_patterns(const cba_sl_options* opts, uint8_t* out) {
    return guarded([&] {
        check_sl_options(opts);
        if (!out) throw std::invalid_argument("null argument");
        sl_patterns_host(*opts, out);
    });
}

cba_status cba_sl_decoder_create(const cba_sl_options* opts, int32_t width, int32_t height, int32_t max_sequences, int32_t device,
                                 cba_sl_decoder** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        check_sl_options(opts);
        check_image_batch(width, height, max_sequences, "max_sequences");
        if (static_cast<double>(max_sequences) * sl_options_image_count(*opts) * width * height > 2147483647.0)
            throw std::invalid_argument("max_sequences n_images width height must be <= 2^31 - 1");
        require_device(device);
        *out = reinterpret_cast<cba_sl_decoder*>(sl_decoder_create(*opts, width, height, max_sequences, device));
    });
}

cba_status cba_sl_decoder_set_rig(cba_sl_decoder* h, int32_t camera_model, const double* intr, int32_t n_inverse_coeffs,
                                  const double* inverse_coeffs, const double* c_T_r, const cba_triangulate_options* tri_opts) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        check_tri_cameras(camera_model, 2, intr, n_inverse_coeffs, inverse_coeffs, c_T_r, tri_opts);
        check_tri_options(tri_opts);
        sl_decoder_set_rig(reinterpret_cast<SlDecoder*>(h), camera_model, intr, inverse_coeffs ? n_inverse_coeffs : 0, inverse_coeffs, c_T_r,
                           *tri_opts);
    });
}

static cba_status sl_decoder_process_impl(cba_sl_decoder* h, int32_t n_sequences, const uint8_t* images, double* coord, double* modulation,
                                          uint8_t* status, double* xyz, double* rms_px, int32_t* tri_status, double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        SlDecoder* d = reinterpret_cast<SlDecoder*>(h);
        const char* no_points = (xyz || rms_px || tri_status) && !sl_decoder_can_point(d) ? "points need a rig and both axes" : nullptr;
        if (!check_batch_call(n_sequences, sl_decoder_max_sequences(d), "sequences", no_points, images != nullptr)) return;
        sl_decoder_process(d, n_sequences, images, coord, modulation, status, xyz, rms_px, tri_status, stage_ms);
    });
}

cba_status cba_sl_decoder_process(cba_sl_decoder* h, int32_t n_sequences, const uint8_t* images, double* coord, double* modulation,
                                  uint8_t* status, double* xyz, double* rms_px, int32_t* tri_status) {
    return sl_decoder_process_impl(h, n_sequences, images, coord, modulation, status, xyz, rms_px, tri_status, nullptr);
}

void cba_sl_decoder_destroy(cba_sl_decoder* h) { sl_decoder_destroy(reinterpret_cast<SlDecoder*>(h)); }

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_structured_light.py): cba_sl_decoder_process timing its stages on the device (stage_ms [4] =
// upload, decode, points, download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_sl_decoder_process_timed(cba_sl_decoder* h, int32_t n_sequences, const uint8_t* images,
                                                                               double* coord, double* modulation, uint8_t* status,
                                                                               double* xyz, double* rms_px, int32_t* tri_status,
                                                                               double* stage_ms) {
    return timed(stage_ms, [&] { return sl_decoder_process_impl(h, n_sequences, images, coord, modulation, status, xyz, rms_px, tri_status, stage_ms); });
}
#endif

// ---- scan registration (cloud_register.hip, cloud_math.hpp) -------------------------------------------------------------------
cba_status cba_point_normals(int32_t n_maps, int32_t height, int32_t width, const double* xyz, const double* viewpoint, double max_jump,
                             double* normals) {
    return guarded([&] {
        if (n_maps < 0) throw std::invalid_argument("n_maps must be >= 0");
        check_sides(width, height);
        if (static_cast<int64_t>(n_maps) * width * height > 0x7fffffff) throw std::invalid_argument("n_maps width height must be <= 2^31 - 1");
        if (!(max_jump > 0.0)) throw std::invalid_argument("max_jump must be > 0");
        if (n_maps == 0) return;
        if (!xyz || !normals) throw std::invalid_argument("null argument");
        require_device();
        point_normals_gpu(n_maps, height, width, xyz, viewpoint, max_jump, normals, default_device());
    });
}

static void check_cell_size(double c) { if (!std::isfinite(c) || !(c > 0.0)) throw std::invalid_argument("cell_size must be finite and > 0"); }
// the text of a grid plan's answer 2: whom ("" or "scan k ") the cell size gives too many cells, and the one that fits
static std::string too_many_cells(const std::string& whom, double fit, const char* tail) {
    char fits[32];
    std::snprintf(fits, sizeof fits, "%.6g", fit);
    return "cell_size gives " + whom + "more than 2^24 cells; a cell_size of " + fits + tail;
}

// the n poses of pose7 [n][7] have non-zero finite quaternions, or invalid_argument(message) -> the last one's norm, nothing contracted
static double check_pose_quaternions(const double* pose7, int64_t n, const char* message) {
#pragma clang fp contract(off)
    double nq = 0.0;
    for (int64_t m = 0; m < n; ++m) {
        const double* q = pose7 + 7 * static_cast<size_t>(m);
        nq = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        if (!(nq > 0.0) || !std::isfinite(nq)) throw std::invalid_argument(message);
    }
    return nq;
}

cba_status cba_cloud_index_create(int64_t n, const double* xyz, const double* normals, double cell_size, int32_t device, cba_cloud_index** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        if (n < 1 || n > 0x7fffffff) throw std::invalid_argument("n must be in [1, 2^31 - 1]");
        if (!xyz) throw std::invalid_argument("null argument");
        check_cell_size(cell_size);
        double fit = 0.0;
        const int plan = cloud_plan(n, xyz, cell_size, &fit);
        if (plan == 1) throw std::invalid_argument("the target has no valid point");
        if (plan == 2) throw std::invalid_argument(too_many_cells("", fit, " or more fits"));
        require_device(device);
        *out = reinterpret_cast<cba_cloud_index*>(cloud_index_create(n, xyz, normals, cell_size, device));
    });
}

static void check_cloud_distance(double cell_size, double max_distance) {
    if (!std::isfinite(max_distance) || !(max_distance > 0.0) || max_distance > 0.999 * cell_size)
        throw std::invalid_argument("max_distance must be > 0 and <= 0.999 cell_size");
}
static void check_cloud_distance(const CloudIndex* h, double max_distance) { check_cloud_distance(cloud_index_cell_size(h), max_distance); }

// the checks of cba_icp_options against a grid (what: "an index", "a set")
static void check_icp_options(const cba_icp_options& o, bool has_normals, double cell_size, const char* what) {
    if (o.metric != 0 && o.metric != 1) throw std::invalid_argument("metric must be 0 or 1");
    if (o.metric == 0 && !has_normals) throw std::invalid_argument(std::string("metric 0 needs ") + what + " with normals");
    check_cloud_distance(cell_size, o.max_distance);
    if (o.max_iterations < 0 || o.max_iterations > CBA_ICP_MAX_ITERATIONS) throw std::invalid_argument("max_iterations must be in [0, 10000]");
    if (!std::isfinite(o.step_tolerance) || o.step_tolerance < 0.0) throw std::invalid_argument("step_tolerance must be finite and >= 0");
}

// out [7] = in [7] with its quaternion normalised by the rule of cba_cloud_register
static void normalised_pose(const double* in, double* out) {
    const char* message = "init_pose7 needs a non-zero finite quaternion and a finite translation";
    const double nq = check_pose_quaternions(in, 1, message);
    if (!std::isfinite(in[4]) || !std::isfinite(in[5]) || !std::isfinite(in[6])) throw std::invalid_argument(message);
    for (int k = 0; k < 4; ++k) out[k] = in[k] / nq;
    for (int k = 4; k < 7; ++k) out[k] = in[k];
}

cba_status cba_cloud_nearest(cba_cloud_index* h, int64_t m, const double* query, double max_distance, int64_t* index, double* dist2) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        CloudIndex* c = reinterpret_cast<CloudIndex*>(h);
        if (m < 0 || m > 0x7fffffff) throw std::invalid_argument("m must be in [0, 2^31 - 1]");
        check_cloud_distance(c, max_distance);
        if (m == 0) return;
        if (!query || !index) throw std::invalid_argument("null argument");
        cloud_index_nearest(c, m, query, max_distance, index, dist2);
    });
}

void cba_icp_options_default(cba_icp_options* o) {
    if (!o) return;
    o->metric = 0;
    o->max_distance = 0.0;
    o->max_iterations = 30;
    o->step_tolerance = 1e-9;
    o->min_pairs = 6;
}

static cba_status cloud_register_impl(cba_cloud_index* h, int32_t n_sources, const int64_t* source_offset, const double* source_xyz,
                                      const double* init_pose7, const cba_icp_options* opts, cba_icp_result* results, double* stage_ms) {
    return guarded([&] {
        if (!h || !opts) throw std::invalid_argument("null argument");
        CloudIndex* c = reinterpret_cast<CloudIndex*>(h);
        if (n_sources < 0) throw std::invalid_argument("n_sources must be >= 0");
        check_icp_options(*opts, cloud_index_has_normals(c), cloud_index_cell_size(c), "an index");
        if (n_sources == 0) return;
        if (!source_offset || !results) throw std::invalid_argument("null argument");
        check_offsets(source_offset, n_sources, "source ", OFF_FROM_ZERO | OFF_INT32_GROUPS);
        if (source_offset[n_sources] > 0 && !source_xyz) throw std::invalid_argument("null argument");
        for (int32_t i = 0; i < n_sources; ++i) {
            cba_icp_result& r = results[i];
            r = cba_icp_result{};
            r.pose7[0] = 1.0;
            if (init_pose7) normalised_pose(init_pose7 + 7 * i, r.pose7);
            r.status = CBA_ICP_NOT_CONVERGED;
        }
        cloud_index_register(c, n_sources, source_offset, source_xyz, *opts, results, stage_ms);
    });
}

cba_status cba_cloud_register(cba_cloud_index* h, int32_t n_sources, const int64_t* source_offset, const double* source_xyz,
                              const double* init_pose7, const cba_icp_options* opts, cba_icp_result* results) {
    return cloud_register_impl(h, n_sources, source_offset, source_xyz, init_pose7, opts, results, nullptr);
}

void cba_cloud_index_destroy(cba_cloud_index* h) { cloud_index_destroy(reinterpret_cast<CloudIndex*>(h)); }

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_registration.py): cba_cloud_register timing its stages on the device (stage_ms [3] = upload,
// rounds, download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_cloud_register_timed(cba_cloud_index* h, int32_t n_sources, const int64_t* source_offset,
                                                                           const double* source_xyz, const double* init_pose7,
                                                                           const cba_icp_options* opts, cba_icp_result* results,
                                                                           double* stage_ms) {
    return timed(stage_ms, [&] { return cloud_register_impl(h, n_sources, source_offset, source_xyz, init_pose7, opts, results, stage_ms); });
}
#endif

// ---- alignment of many scans (cloud_register.hip, cloud_math.hpp) -----------------------------------------------------------------
cba_status cba_cloud_set_create(int32_t n_scans, const int64_t* offset, const double* xyz, const double* normals, double cell_size,
                                int32_t device, cba_cloud_set** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        if (n_scans < 2 || n_scans > CBA_ALIGN_MAX_SCANS) throw std::invalid_argument("n_scans must be in [2, 64]");
        if (!offset || !xyz) throw std::invalid_argument("null argument");
        check_offsets(offset, n_scans, "scan ", OFF_FROM_ZERO | OFF_INT32_GROUPS);
        check_cell_size(cell_size);
        for (int32_t k = 0; k < n_scans; ++k)
            if (offset[k + 1] == offset[k]) throw std::invalid_argument("scan " + std::to_string(k) + " has no valid point");
        double fit = 0.0;
        int scan = 0;
        const int plan = cloud_set_plan(n_scans, offset, xyz, cell_size, &scan, &fit);
        if (plan == 1) throw std::invalid_argument("scan " + std::to_string(scan) + " has no valid point");
        if (plan == 2) throw std::invalid_argument(too_many_cells("scan " + std::to_string(scan) + " ", fit, " or more fits it"));
        require_device(device);
        *out = reinterpret_cast<cba_cloud_set*>(cloud_set_create(n_scans, offset, xyz, normals, cell_size, device));
    });
}

void cba_align_options_default(cba_align_options* o) {
    if (!o) return;
    cba_icp_options_default(&o->icp);
    o->fixed = 0;
}

static cba_status cloud_align_impl(cba_cloud_set* h, int32_t n_edges, const int32_t* edges, const double* init_pose7,
                                   const cba_align_options* opts, double* pose7, cba_align_edge* edge_out, cba_align_result* result,
                                   double* stage_ms) {
    return guarded([&] {
        if (!h || !opts || !pose7 || !result) throw std::invalid_argument("null argument");
        CloudSet* c = reinterpret_cast<CloudSet*>(h);
        const int32_t n_scans = cloud_set_scans(c);
        if (n_edges < 0 || n_edges > CBA_ALIGN_MAX_EDGES) throw std::invalid_argument("n_edges must be in [0, 1024]");
        if (n_edges > 0 && !edges) throw std::invalid_argument("null argument");
        for (int32_t e = 0; e < n_edges; ++e) {
            const int32_t a = edges[2 * e], b = edges[2 * e + 1];
            if (a < 0 || a >= n_scans || b < 0 || b >= n_scans)
                throw std::invalid_argument("edge " + std::to_string(e) + " names a scan outside [0, n_scans)");
            if (a == b) throw std::invalid_argument("edge " + std::to_string(e) + " joins a scan to itself");
        }
        if (opts->fixed < 0 || opts->fixed >= n_scans) throw std::invalid_argument("fixed must be in [0, n_scans)");
        check_icp_options(opts->icp, cloud_set_has_normals(c), cloud_set_cell_size(c), "a set");
        std::vector<double> pose(7 * static_cast<size_t>(n_scans), 0.0);
        for (int32_t k = 0; k < n_scans; ++k) {
            pose[7 * static_cast<size_t>(k)] = 1.0;
            if (init_pose7) normalised_pose(init_pose7 + 7 * k, &pose[7 * static_cast<size_t>(k)]);
        }
        if (n_edges == 0) {  // no work
            std::copy(pose.begin(), pose.end(), pose7);
            *result = cba_align_result{};
            result->rms = std::numeric_limits<double>::quiet_NaN();
            result->status = CBA_ICP_TOO_FEW;
            return;
        }
        cloud_set_align(c, n_edges, edges, opts->icp, opts->fixed, pose.data(), edge_out, result, stage_ms);
        std::copy(pose.begin(), pose.end(), pose7);
    });
}

cba_status cba_cloud_align(cba_cloud_set* h, int32_t n_edges, const int32_t* edges, const double* init_pose7, const cba_align_options* opts,
                           double* pose7, cba_align_edge* edge_out, cba_align_result* result) {
    return cloud_align_impl(h, n_edges, edges, init_pose7, opts, pose7, edge_out, result, nullptr);
}

void cba_cloud_set_destroy(cba_cloud_set* h) { cloud_set_destroy(reinterpret_cast<CloudSet*>(h)); }

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_align.py): cba_cloud_align timing its stages on the device (stage_ms [3] = upload, rounds,
// download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_cloud_align_timed(cba_cloud_set* h, int32_t n_edges, const int32_t* edges,
                                                                        const double* init_pose7, const cba_align_options* opts,
                                                                        double* pose7, cba_align_edge* edge_out, cba_align_result* result,
                                                                        double* stage_ms) {
    return timed(stage_ms, [&] { return cloud_align_impl(h, n_edges, edges, init_pose7, opts, pose7, edge_out, result, stage_ms); });
}
#endif

// ---- scan fusion (tsdf_fusion.hip, tsdf_math.hpp) ------------------------------------------------------------------------------
void cba_tsdf_options_default(cba_tsdf_options* o) {
    if (!o) return;
    o->voxel_size = 0.0;
    o->truncation = 0.0;
    o->max_weight = 64.0;
    o->max_depth = std::numeric_limits<double>::infinity();
}

cba_status cba_tsdf_volume_create(int32_t nx, int32_t ny, int32_t nz, const double* origin, const cba_tsdf_options* opts, int32_t device,
                                  cba_tsdf_volume** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        if (!origin || !opts) throw std::invalid_argument("null argument");
        if (std::min({nx, ny, nz}) < 2 || std::max({nx, ny, nz}) > 1024) throw std::invalid_argument("nx, ny and nz must be in [2, 1024]");
        if (static_cast<int64_t>(nx) * ny * nz > CBA_TSDF_MAX_VOXELS) throw std::invalid_argument("nx ny nz must be <= 2^28");
        if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2])) throw std::invalid_argument("origin must be finite");
        if (!std::isfinite(opts->voxel_size) || !(opts->voxel_size > 0.0)) throw std::invalid_argument("voxel_size must be finite and > 0");
        if (!std::isfinite(opts->truncation) || !(opts->truncation > 0.0)) throw std::invalid_argument("truncation must be finite and > 0");
        if (!(opts->max_weight >= 1.0 && opts->max_weight <= 16777216.0) || opts->max_weight != std::floor(opts->max_weight))
            throw std::invalid_argument("max_weight must be an integer value in [1, 2^24]");
        if (!(opts->max_depth > 0.0)) throw std::invalid_argument("max_depth must be > 0");
        require_device(device);
        *out = reinterpret_cast<cba_tsdf_volume*>(tsdf_volume_create(nx, ny, nz, origin, *opts, device));
    });
}

// colour: cba_tsdf_integrate_colour, which needs rgba; eager: the experiment builds' kernel that loads every colour word
static cba_status tsdf_integrate_impl(cba_tsdf_volume* h, int32_t camera_model, const double* intr, int32_t n_maps, int32_t height, int32_t width,
                                      const double* depth, const uint8_t* rgba, bool colour, const double* c_T_v, bool eager, double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        check_camera(camera_model, intr, 0, nullptr);
        if (intr[0] == 0.0 || intr[1] == 0.0) throw std::invalid_argument("fx and fy must not be 0");
        if (n_maps < 0) throw std::invalid_argument("n_maps must be >= 0");
        check_sides(width, height);
        if (n_maps == 0) return;
        if (!depth || !c_T_v || (colour && !rgba)) throw std::invalid_argument("null argument");
        check_pose_quaternions(c_T_v, n_maps, "c_T_v needs a non-zero finite quaternion");
        tsdf_volume_integrate(reinterpret_cast<TsdfVolume*>(h), camera_model, intr, n_maps, height, width, depth, colour ? rgba : nullptr, c_T_v, eager,
                              stage_ms);
    });
}

cba_status cba_tsdf_integrate(cba_tsdf_volume* h, int32_t camera_model, const double* intr, int32_t n_maps, int32_t height, int32_t width,
                              const double* depth, const double* c_T_v) {
    return tsdf_integrate_impl(h, camera_model, intr, n_maps, height, width, depth, nullptr, false, c_T_v, false, nullptr);
}

cba_status cba_tsdf_integrate_colour(cba_tsdf_volume* h, int32_t camera_model, const double* intr, int32_t n_maps, int32_t height, int32_t width,
                                     const double* depth, const uint8_t* rgba, const double* c_T_v) {
    return tsdf_integrate_impl(h, camera_model, intr, n_maps, height, width, depth, rgba, true, c_T_v, false, nullptr);
}

cba_status cba_tsdf_has_colour(cba_tsdf_volume* h, int32_t* out) {
    return guarded([&] {
        if (!h || !out) throw std::invalid_argument("null argument");
        *out = tsdf_volume_has_colour(reinterpret_cast<TsdfVolume*>(h)) ? 1 : 0;
    });
}

cba_status cba_tsdf_colour_fetch(cba_tsdf_volume* h, float* colour) {
    return guarded([&] {
        if (!h || !colour) throw std::invalid_argument("null argument");
        TsdfVolume* v = reinterpret_cast<TsdfVolume*>(h);
        if (!tsdf_volume_has_colour(v)) throw std::invalid_argument("this volume has no colour");
        tsdf_volume_colour_fetch(v, colour);
    });
}

cba_status cba_tsdf_colour_upload(cba_tsdf_volume* h, const float* colour) {
    return guarded([&] {
        if (!h || !colour) throw std::invalid_argument("null argument");
        tsdf_volume_colour_upload(reinterpret_cast<TsdfVolume*>(h), colour);
    });
}

cba_status cba_tsdf_fetch(cba_tsdf_volume* h, float* tsdf, float* weight) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        if (tsdf || weight) tsdf_volume_fetch(reinterpret_cast<TsdfVolume*>(h), tsdf, weight);
    });
}

cba_status cba_tsdf_upload(cba_tsdf_volume* h, const float* tsdf, const float* weight) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        if (tsdf || weight) tsdf_volume_upload(reinterpret_cast<TsdfVolume*>(h), tsdf, weight);
    });
}

cba_status cba_tsdf_reset(cba_tsdf_volume* h) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        tsdf_volume_reset(reinterpret_cast<TsdfVolume*>(h));
    });
}

static cba_status tsdf_extract_impl(cba_tsdf_volume* h, double min_weight, int64_t* n_points, double* stage_ms) {
    return guarded([&] {
        if (!h || !n_points) throw std::invalid_argument("null argument");
        if (!(min_weight >= 1.0)) throw std::invalid_argument("min_weight must be >= 1");
        tsdf_volume_extract(reinterpret_cast<TsdfVolume*>(h), min_weight, n_points, stage_ms);
    });
}

cba_status cba_tsdf_extract(cba_tsdf_volume* h, double min_weight, int64_t* n_points) { return tsdf_extract_impl(h, min_weight, n_points, nullptr); }

cba_status cba_tsdf_extract_fetch(cba_tsdf_volume* h, double* xyz, double* normals) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        TsdfVolume* v = reinterpret_cast<TsdfVolume*>(h);
        if (tsdf_volume_points(v) < 0) throw std::invalid_argument("no extract has run on this volume");
        if (tsdf_volume_points(v) == 0) return;
        if (!xyz) throw std::invalid_argument("null argument");
        tsdf_volume_extract_fetch(v, xyz, normals);
    });
}

cba_status cba_tsdf_extract_fetch_colour(cba_tsdf_volume* h, uint8_t* rgba) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        TsdfVolume* v = reinterpret_cast<TsdfVolume*>(h);
        if (tsdf_volume_points(v) < 0) throw std::invalid_argument("no extract has run on this volume");
        if (!tsdf_volume_points_coloured(v)) throw std::invalid_argument("the last extract ran without colour");
        if (tsdf_volume_points(v) == 0) return;
        if (!rgba) throw std::invalid_argument("null argument");
        tsdf_volume_extract_fetch_colour(v, rgba);
    });
}

static cba_status tsdf_mesh_impl(cba_tsdf_volume* h, double min_weight, int64_t* n_points, int64_t* n_triangles, double* stage_ms) {
    return guarded([&] {
        if (!h || !n_points || !n_triangles) throw std::invalid_argument("null argument");
        if (!(min_weight >= 1.0)) throw std::invalid_argument("min_weight must be >= 1");
        tsdf_volume_mesh(reinterpret_cast<TsdfVolume*>(h), min_weight, n_points, n_triangles, stage_ms);
    });
}

cba_status cba_tsdf_mesh(cba_tsdf_volume* h, double min_weight, int64_t* n_points, int64_t* n_triangles) {
    return tsdf_mesh_impl(h, min_weight, n_points, n_triangles, nullptr);
}

cba_status cba_tsdf_mesh_fetch(cba_tsdf_volume* h, int32_t* triangles) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        TsdfVolume* v = reinterpret_cast<TsdfVolume*>(h);
        if (tsdf_volume_triangles(v) < 0) throw std::invalid_argument("this volume has no valid mesh: call cba_tsdf_mesh");
        if (tsdf_volume_triangles(v) == 0) return;
        if (!triangles) throw std::invalid_argument("null argument");
        tsdf_volume_mesh_fetch(v, triangles);
    });
}

void cba_tsdf_raycast_options_default(cba_tsdf_raycast_options* o) {
    if (!o) return;
    o->step = 0.0;
    o->skip = 0.5;
    o->near_depth = 0.0;
    o->far_depth = std::numeric_limits<double>::infinity();
    o->min_weight = 1.0;
}

// wave_w: the width of a wavefront's pixel block (8; the experiment builds compare 64)
static cba_status tsdf_raycast_impl(cba_tsdf_volume* h, int32_t camera_model, const double* intr, int32_t n_views, int32_t height, int32_t width,
                                    const double* poses, const cba_tsdf_raycast_options* opts, int wave_w, double* stage_ms,
                                    double* colour_ms = nullptr) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        check_camera(camera_model, intr, 0, nullptr);
        if (intr[0] == 0.0 || intr[1] == 0.0) throw std::invalid_argument("fx and fy must not be 0");
        if (n_views < 0) throw std::invalid_argument("n_views must be >= 0");
        check_sides(width, height);
        if (static_cast<int64_t>(n_views) * height * width > CBA_TSDF_MAX_RAYS) throw std::invalid_argument("n_views height width must be <= 2^26");
        cba_tsdf_raycast_options o;
        cba_tsdf_raycast_options_default(&o);
        if (opts) o = *opts;
        TsdfVolume* v = reinterpret_cast<TsdfVolume*>(h);
        const double vs = tsdf_volume_voxel_size(v);
        if (o.step != 0.0 && !(std::isfinite(o.step) && o.step >= vs / 16.0)) throw std::invalid_argument("step must be 0 or finite and >= voxel_size / 16");
        if (!(o.skip >= 0.0 && o.skip <= 1.0)) throw std::invalid_argument("skip must be in [0, 1]");
        if (!(o.near_depth >= 0.0) || !std::isfinite(o.near_depth)) throw std::invalid_argument("near_depth must be finite and >= 0");
        if (!(o.far_depth > o.near_depth)) throw std::invalid_argument("far_depth must be > near_depth");
        if (!(o.min_weight >= 1.0)) throw std::invalid_argument("min_weight must be >= 1");
        if (n_views == 0) return;
        if (!poses) throw std::invalid_argument("null argument");
        check_pose_quaternions(poses, n_views, "poses needs a non-zero finite quaternion");
        tsdf_volume_raycast(v, camera_model, intr, n_views, height, width, poses, o, wave_w, stage_ms, colour_ms);
    });
}

cba_status cba_tsdf_raycast(cba_tsdf_volume* h, int32_t camera_model, const double* intr, int32_t n_views, int32_t height, int32_t width,
                            const double* poses, const cba_tsdf_raycast_options* opts) {
    return tsdf_raycast_impl(h, camera_model, intr, n_views, height, width, poses, opts, 8, nullptr);
}

cba_status cba_tsdf_raycast_fetch(cba_tsdf_volume* h, double* depth, double* xyz, double* normals, uint8_t* status, double* rays) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        TsdfVolume* v = reinterpret_cast<TsdfVolume*>(h);
        if (tsdf_volume_ray_views(v) < 0) throw std::invalid_argument("no ray cast has run on this volume");
        if (depth || xyz || normals || status || rays) tsdf_volume_raycast_fetch(v, depth, xyz, normals, status, rays);
    });
}

cba_status cba_tsdf_raycast_fetch_colour(cba_tsdf_volume* h, uint8_t* rgba) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        TsdfVolume* v = reinterpret_cast<TsdfVolume*>(h);
        if (tsdf_volume_ray_views(v) < 0) throw std::invalid_argument("no ray cast has run on this volume");
        if (!tsdf_volume_rays_coloured(v)) throw std::invalid_argument("the last ray cast ran without colour");
        if (!rgba) throw std::invalid_argument("null argument");
        tsdf_volume_raycast_fetch_colour(v, rgba);
    });
}

void cba_tsdf_volume_destroy(cba_tsdf_volume* h) { tsdf_volume_destroy(reinterpret_cast<TsdfVolume*>(h)); }

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_fusion.py): integrate and extract timing their stages on the device (stage_ms [2] = upload,
// kernel; count and scan, place).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_tsdf_integrate_timed(cba_tsdf_volume* h, int32_t camera_model, const double* intr,
                                                                           int32_t n_maps, int32_t height, int32_t width, const double* depth,
                                                                           const double* c_T_v, double* stage_ms) {
    return timed(stage_ms, [&] { return tsdf_integrate_impl(h, camera_model, intr, n_maps, height, width, depth, nullptr, false, c_T_v, false, stage_ms); });
}
// tools/bench_colour.py: the colour integrate with its stages; eager != 0: the kernel that loads every colour word up front
__attribute__((visibility("default"))) cba_status cba_tsdf_integrate_colour_timed(cba_tsdf_volume* h, int32_t camera_model, const double* intr,
                                                                                  int32_t n_maps, int32_t height, int32_t width, const double* depth,
                                                                                  const uint8_t* rgba, const double* c_T_v, int32_t eager,
                                                                                  double* stage_ms) {
    return timed(stage_ms, [&] { return tsdf_integrate_impl(h, camera_model, intr, n_maps, height, width, depth, rgba, true, c_T_v, eager != 0, stage_ms); });
}
__attribute__((visibility("default"))) cba_status cba_tsdf_extract_timed(cba_tsdf_volume* h, double min_weight, int64_t* n_points,
                                                                         double* stage_ms) {
    return timed(stage_ms, [&] { return tsdf_extract_impl(h, min_weight, n_points, stage_ms); });
}
// stage_ms [4] = the extract's count and scan, its place with the records, the triangles' count and scan, their place
__attribute__((visibility("default"))) cba_status cba_tsdf_mesh_timed(cba_tsdf_volume* h, double min_weight, int64_t* n_points,
                                                                      int64_t* n_triangles, double* stage_ms) {
    return timed(stage_ms, [&] { return tsdf_mesh_impl(h, min_weight, n_points, n_triangles, stage_ms); });
}
// stage_ms [2] = upload and the rays table, the cast; wave_w: 8 or 64 (tools/bench_raycast.py compares the two pixel blocks)
__attribute__((visibility("default"))) cba_status cba_tsdf_raycast_timed(cba_tsdf_volume* h, int32_t camera_model, const double* intr,
                                                                         int32_t n_views, int32_t height, int32_t width, const double* poses,
                                                                         const cba_tsdf_raycast_options* opts, int32_t wave_w, double* stage_ms) {
    if (wave_w != 8 && wave_w != 64) return CBA_ERR_INVALID_ARGUMENT;
    return timed(stage_ms, [&] { return tsdf_raycast_impl(h, camera_model, intr, n_views, height, width, poses, opts, wave_w, stage_ms); });
}
// tools/bench_colour.py: stage_ms [3] = upload and the rays table, the cast, the colour pass
__attribute__((visibility("default"))) cba_status cba_tsdf_raycast_colour_timed(cba_tsdf_volume* h, int32_t camera_model, const double* intr,
                                                                                int32_t n_views, int32_t height, int32_t width, const double* poses,
                                                                                const cba_tsdf_raycast_options* opts, double* stage_ms) {
    return timed(stage_ms, [&] { return tsdf_raycast_impl(h, camera_model, intr, n_views, height, width, poses, opts, 8, stage_ms, stage_ms + 2); });
}
#endif

// ---- stereo depth (stereo_match.hip, stereo_math.hpp) ---------------------------------------------------------------------------
void cba_stereo_match_options_default(cba_stereo_match_options* o) {
    if (!o) return;
    o->min_disparity = 0;
    o->num_disparities = 64;
    o->half_window = 4;
    o->uniqueness_percent = 10;
    o->lr_max_diff = 1;
    o->subpixel = 1;
}

cba_status cba_stereo_rectify(int32_t camera_model, const double* intr, const double* c_T_r, int32_t width, int32_t height,
                              const cba_stereo_rectify_options* opts, double* R, double* new_k5, double* baseline, double* r_T_rect) {
    return guarded([&] {
        check_camera(camera_model, intr, 0, nullptr);
        if (!c_T_r || !opts || !R || !new_k5 || !baseline || !r_T_rect) throw std::invalid_argument("null argument");
        check_sides(width, height);
        const char* err = stereo_rectify(intr, cam_intr_size(camera_model), c_T_r, width, height, opts->focal, opts->cx,
                                         opts->cy, R, new_k5, baseline, r_T_rect);
        if (err) throw std::invalid_argument(err);
    });
}

// g == NULL: no geometry, which a pose cannot go with (the matchers; cba_stereo_points requires g before it calls)
static void check_stereo_geometry(const cba_stereo_geometry* g, const double* pose7) {
    if (!g) {
        if (pose7) throw std::invalid_argument("a pose needs a geometry");
        return;
    }
    if (!std::isfinite(g->focal) || !std::isfinite(g->cx) || !std::isfinite(g->cy) || !std::isfinite(g->baseline))
        throw std::invalid_argument("the stereo geometry must be finite");
    if (!(g->focal > 0.0) || !(g->baseline > 0.0)) throw std::invalid_argument("focal and baseline must be > 0");
    if (pose7)
        for (int k = 0; k < 7; ++k)
            if (!std::isfinite(pose7[k])) throw std::invalid_argument("the pose must be finite");
}

// the disparity options both matchers have, in two parts: each matcher checks options of its own between them, in the order it shipped
static void check_disparity_range(int32_t min_disparity, int32_t num_disparities) {
    if (min_disparity < -32768 || min_disparity > 32768) throw std::invalid_argument("|min_disparity| must be <= 32768");
    if (num_disparities < 1 || num_disparities > 256) throw std::invalid_argument("num_disparities must be in 1..256");
}
static void check_disparity_selection(int32_t uniqueness_percent, int32_t lr_max_diff, int32_t subpixel) {
    if (uniqueness_percent < 0 || uniqueness_percent > 100) throw std::invalid_argument("uniqueness_percent must be in 0..100");
    if (lr_max_diff < -1) throw std::invalid_argument("lr_max_diff must be >= -1");
    if (subpixel != 0 && subpixel != 1) throw std::invalid_argument("subpixel must be 0 or 1");
}
static const char NO_GEOMETRY[] = "xyz needs a matcher created with a geometry";

cba_status cba_stereo_matcher_create(int32_t width, int32_t height, int32_t max_pairs, const cba_stereo_match_options* opts,
                                     const cba_stereo_geometry* geometry, const double* pose7, int32_t device, cba_stereo_matcher** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        if (!opts) throw std::invalid_argument("null argument");
        check_image_batch(width, height, max_pairs, "max_pairs");
        check_disparity_range(opts->min_disparity, opts->num_disparities);
        if (opts->half_window < 1 || opts->half_window > 10) throw std::invalid_argument("half_window must be in 1..10");
        check_disparity_selection(opts->uniqueness_percent, opts->lr_max_diff, opts->subpixel);
        check_stereo_geometry(geometry, pose7);
        require_device(device);
        *out = reinterpret_cast<cba_stereo_matcher*>(stereo_matcher_create(width, height, max_pairs, *opts, geometry, pose7, device));
    });
}

static cba_status stereo_matcher_process_impl(cba_stereo_matcher* h, int32_t n_pairs, const uint8_t* left, const uint8_t* right,
                                              float* disparity, int32_t* cost, float* xyz, double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        StereoMatcher* m = reinterpret_cast<StereoMatcher*>(h);
        const char* no_geometry = xyz && !stereo_matcher_has_geometry(m) ? NO_GEOMETRY : nullptr;
        if (!check_batch_call(n_pairs, stereo_matcher_max_pairs(m), "pairs", no_geometry, left && right)) return;
        stereo_matcher_process(m, n_pairs, left, right, disparity, cost, xyz, stage_ms);
    });
}

cba_status cba_stereo_matcher_process(cba_stereo_matcher* h, int32_t n_pairs, const uint8_t* left, const uint8_t* right, float* disparity,
                                      int32_t* cost, float* xyz) {
    return stereo_matcher_process_impl(h, n_pairs, left, right, disparity, cost, xyz, nullptr);
}

void cba_stereo_matcher_destroy(cba_stereo_matcher* h) { stereo_matcher_destroy(reinterpret_cast<StereoMatcher*>(h)); }

cba_status cba_stereo_points(const cba_stereo_geometry* geometry, const double* pose7, int64_t n, const double* uvd, double* xyz) {
    return guarded([&] {
        if (!geometry) throw std::invalid_argument("null argument");
        check_stereo_geometry(geometry, pose7);
        if (n < 0) throw std::invalid_argument("n must be >= 0");
        if (n == 0) return;
        if (!uvd || !xyz) throw std::invalid_argument("null argument");
        require_device();
        stereo_points_gpu(*geometry, pose7, n, uvd, xyz, default_device());
    });
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_stereo.py): cba_stereo_matcher_process timing its stages on the device (stage_ms [3] = upload,
// kernels, download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_stereo_matcher_process_timed(cba_stereo_matcher* h, int32_t n_pairs,
                                                                                   const uint8_t* left, const uint8_t* right,
                                                                                   float* disparity, int32_t* cost, float* xyz,
                                                                                   double* stage_ms) {
    return timed(stage_ms, [&] { return stereo_matcher_process_impl(h, n_pairs, left, right, disparity, cost, xyz, stage_ms); });
}
#endif

// ---- semi-global matching (stereo_sgm.hip, sgm_math.hpp) ------------------------------------------------------------------------------
void cba_sgm_options_default(cba_sgm_options* o) {
    if (!o) return;
    o->min_disparity = 0;
    o->num_disparities = 64;
    o->p1 = 4;
    o->p2 = 32;
    o->paths = 8;
    o->uniqueness_percent = 10;
    o->lr_max_diff = 1;
    o->subpixel = 1;
    o->workspace_mb = 0;
}

cba_status cba_sgm_matcher_create(int32_t width, int32_t height, int32_t max_pairs, const cba_sgm_options* opts,
                                  const cba_stereo_geometry* geometry, const double* pose7, int32_t device, cba_sgm_matcher** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        if (!opts) throw std::invalid_argument("null argument");
        check_image_batch(width, height, max_pairs, "max_pairs");
        check_disparity_range(opts->min_disparity, opts->num_disparities);
        if (opts->p2 < 0 || opts->p2 > 1023) throw std::invalid_argument("p2 must be in 0..1023");
        if (opts->p1 < 0 || opts->p1 > opts->p2) throw std::invalid_argument("p1 must be in 0..p2");
        if (opts->paths != 4 && opts->paths != 8) throw std::invalid_argument("paths must be 4 or 8");
        check_disparity_selection(opts->uniqueness_percent, opts->lr_max_diff, opts->subpixel);
        if (opts->workspace_mb < 0 || opts->workspace_mb > CBA_SGM_MAX_WORKSPACE_MB) throw std::invalid_argument("workspace_mb must be in 0..1048576");
        if (static_cast<int64_t>(width) * height * opts->num_disparities > CBA_SGM_MAX_VOLUME)
            throw std::invalid_argument("width height num_disparities must be <= 2^31");
        check_stereo_geometry(geometry, pose7);
        require_device(device);
        *out = reinterpret_cast<cba_sgm_matcher*>(sgm_matcher_create(width, height, max_pairs, *opts, geometry, pose7, device));
    });
}

static cba_status sgm_matcher_process_impl(cba_sgm_matcher* h, int32_t n_pairs, const uint8_t* left, const uint8_t* right, float* disparity,
                                           int32_t* cost, float* xyz, double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        SgmMatcher* m = reinterpret_cast<SgmMatcher*>(h);
        const char* no_geometry = xyz && !sgm_matcher_has_geometry(m) ? NO_GEOMETRY : nullptr;
        if (!check_batch_call(n_pairs, sgm_matcher_max_pairs(m), "pairs", no_geometry, left && right)) return;
        sgm_matcher_process(m, n_pairs, left, right, disparity, cost, xyz, stage_ms);
    });
}

cba_status cba_sgm_matcher_process(cba_sgm_matcher* h, int32_t n_pairs, const uint8_t* left, const uint8_t* right, float* disparity,
                                   int32_t* cost, float* xyz) {
    return sgm_matcher_process_impl(h, n_pairs, left, right, disparity, cost, xyz, nullptr);
}

void cba_sgm_matcher_destroy(cba_sgm_matcher* h) { sgm_matcher_destroy(reinterpret_cast<SgmMatcher*>(h)); }

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_sgm.py): cba_sgm_matcher_process timing its stages on the device (stage_ms [13] = upload, census,
// cost, the 8 path launches in the order of the rule, selection, download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_sgm_matcher_process_timed(cba_sgm_matcher* h, int32_t n_pairs, const uint8_t* left,
                                                                                const uint8_t* right, float* disparity, int32_t* cost,
                                                                                float* xyz, double* stage_ms) {
    return timed(stage_ms, [&] { return sgm_matcher_process_impl(h, n_pairs, left, right, disparity, cost, xyz, stage_ms); });
}
#endif

// ---- disparity filters (disparity_filter.hip, disparity_filter_math.hpp) -----------------------------------------------------------
void cba_disparity_filter_options_default(cba_disparity_filter_options* o) {
    if (!o) return;
    o->median_half = 1;
    o->speckle_max_size = 100;
    o->speckle_max_diff = 1.0;
}

static void check_disparity_filter_options(const cba_disparity_filter_options* o) {
    if (o->median_half < 0 || o->median_half > 2) throw std::invalid_argument("median_half must be in 0..2");
    if (o->speckle_max_size < 0) throw std::invalid_argument("speckle_max_size must be >= 0");
    if (!std::isfinite(o->speckle_max_diff) || !(o->speckle_max_diff >= 0.0)) throw std::invalid_argument("speckle_max_diff must be finite and >= 0");
}

cba_status cba_disparity_filter_create(int32_t width, int32_t height, int32_t max_images, const cba_disparity_filter_options* opts,
                                       int32_t device, cba_disparity_filter** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        if (!opts) throw std::invalid_argument("null argument");
        check_image_batch(width, height, max_images, "max_images");
        check_disparity_filter_options(opts);
        require_device(device);
        *out = reinterpret_cast<cba_disparity_filter*>(disparity_filter_create(width, height, max_images, *opts, device));
    });
}

static cba_status disparity_filter_process_impl(cba_disparity_filter* h, int32_t n, const float* in, float* out, int64_t* stats,
                                                double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        DisparityFilter* f = reinterpret_cast<DisparityFilter*>(h);
        if (!check_batch_call(n, disparity_filter_max_images(f), "images", nullptr, in && out)) return;
        disparity_filter_process(f, n, in, out, stats, stage_ms);
    });
}

cba_status cba_disparity_filter_process(cba_disparity_filter* h, int32_t n, const float* in, float* out, int64_t* stats) {
    return disparity_filter_process_impl(h, n, in, out, stats, nullptr);
}

void cba_disparity_filter_destroy(cba_disparity_filter* h) { disparity_filter_destroy(reinterpret_cast<DisparityFilter*>(h)); }

cba_status cba_stereo_matcher_set_filter(cba_stereo_matcher* h, const cba_disparity_filter_options* opts) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        if (opts) check_disparity_filter_options(opts);
        stereo_matcher_set_filter(reinterpret_cast<StereoMatcher*>(h), opts);
    });
}

cba_status cba_sgm_matcher_set_filter(cba_sgm_matcher* h, const cba_disparity_filter_options* opts) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        if (opts) check_disparity_filter_options(opts);
        sgm_matcher_set_filter(reinterpret_cast<SgmMatcher*>(h), opts);
    });
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_disparity_filter.py): cba_disparity_filter_process timing its kernels on the device (stage_ms [6] =
// median, local labels, merge, flatten, sizes, apply).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_disparity_filter_process_timed(cba_disparity_filter* h, int32_t n, const float* in,
                                                                                     float* out, int64_t* stats, double* stage_ms) {
    return timed(stage_ms, [&] { return disparity_filter_process_impl(h, n, in, out, stats, stage_ms); });
}
#endif

// ---- chessboard detection (corner_detect.hip, corner_math.hpp, corner_grid.hpp) ---------------------------------------------------
void cba_corner_options_default(cba_corner_options* o) {
    if (!o) return;
    o->min_response = 400;
    o->nms_radius = 3;
    o->cog_radius = 2;
    o->refine = CBA_CORNER_REFINE_GRADIENT;
    o->refine_half_window = 5;
    o->refine_iterations = 5;
}

// the sizes and options of a corner detector (shared with cba_charuco_detector_create)
static void check_corner_create(int32_t width, int32_t height, int32_t max_images, int32_t max_corners, const cba_corner_options* opts) {
    if (!opts) throw std::invalid_argument("null argument");
    check_sides(width, height);
    if (width < 11 || height < 11) throw std::invalid_argument("width and height must be >= 11");
    check_image_batch(width, height, max_images, "max_images");
    check_peak_capacity(max_images, max_corners, "max_corners");
    if (opts->min_response < 1 || opts->min_response > 10200) throw std::invalid_argument("min_response must be in 1..10200");
    if (opts->nms_radius < 1 || opts->nms_radius > 10) throw std::invalid_argument("nms_radius must be in 1..10");
    if (opts->cog_radius < 1 || opts->cog_radius > 5) throw std::invalid_argument("cog_radius must be in 1..5");
    if (opts->refine < CBA_CORNER_REFINE_NONE || opts->refine > CBA_CORNER_REFINE_GRADIENT)
        throw std::invalid_argument("refine must be NONE, COG or GRADIENT");
    if (opts->refine_half_window < 1 || opts->refine_half_window > 10) throw std::invalid_argument("refine_half_window must be in 1..10");
    if (opts->refine_iterations < 1 || opts->refine_iterations > 100) throw std::invalid_argument("refine_iterations must be in 1..100");
}

cba_status cba_corner_detector_create(int32_t width, int32_t height, int32_t max_images, int32_t max_corners, const cba_corner_options* opts,
                                      int32_t device, cba_corner_detector** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        check_corner_create(width, height, max_images, max_corners, opts);
        require_device(device);
        *out = reinterpret_cast<cba_corner_detector*>(corner_detector_create(width, height, max_images, max_corners, *opts, device));
    });
}

static cba_status corner_detector_process_impl(cba_corner_detector* h, int32_t n_images, const uint8_t* images, int32_t* out_count,
                                               int32_t* out_status, double* out_xy, double* out_angle, int32_t* out_response,
                                               int32_t* out_flags, double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        CornerDetector* d = reinterpret_cast<CornerDetector*>(h);
        if (!check_batch_call(n_images, corner_detector_max_images(d), "images", nullptr, images != nullptr)) return;
        corner_detector_process(d, n_images, images, out_count, out_status, out_xy, out_angle, out_response, out_flags, stage_ms);
    });
}

cba_status cba_corner_detector_process(cba_corner_detector* h, int32_t n_images, const uint8_t* images, int32_t* out_count,
                                       int32_t* out_status, double* out_xy, double* out_angle, int32_t* out_response, int32_t* out_flags) {
    return corner_detector_process_impl(h, n_images, images, out_count, out_status, out_xy, out_angle, out_response, out_flags, nullptr);
}

void cba_corner_detector_destroy(cba_corner_detector* h) { corner_detector_destroy(reinterpret_cast<CornerDetector*>(h)); }

cba_status cba_chessboard_order(int32_t n, const double* xy, const double* angle, int32_t rows, int32_t cols, int32_t* out_index) {
    return guarded([&] {
        if (!out_index) throw std::invalid_argument("null argument");
        if (n < 0) throw std::invalid_argument("n must be >= 0");
        if (rows < 2 || cols < 2 || static_cast<int64_t>(rows) * cols > 65536) throw std::invalid_argument("rows and cols must be >= 2, rows cols <= 65536");
        if (n > 0 && (!xy || !angle)) throw std::invalid_argument("null argument");
        if (n > 65536) throw std::invalid_argument("n must be <= 65536");
        for (int32_t i = 0; i < n; ++i)
            if (!std::isfinite(xy[2 * i]) || !std::isfinite(xy[2 * i + 1]) || !std::isfinite(angle[i]))
                throw std::invalid_argument("corners must be finite");
        if (!chessboard_order(n, xy, angle, rows, cols, out_index))
            for (int32_t i = 0; i < rows * cols; ++i) out_index[i] = -1;  // not found
    });
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_corners.py): cba_corner_detector_process timing its stages on the device (stage_ms [5] = upload,
// response, peaks, refine, download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_corner_detector_process_timed(cba_corner_detector* h, int32_t n_images,
                                                                                    const uint8_t* images, int32_t* out_count,
                                                                                    int32_t* out_status, double* out_xy, double* out_angle,
                                                                                    int32_t* out_response, int32_t* out_flags,
                                                                                    double* stage_ms) {
    return timed(stage_ms, [&] { return corner_detector_process_impl(h, n_images, images, out_count, out_status, out_xy, out_angle, out_response,
                                                                     out_flags, stage_ms); });
}
#endif

// ---- circle-grid detection (blob_detect.hip, blob_math.hpp, circle_grid.hpp) --------------------------------------------------------
void cba_blob_options_default(cba_blob_options* o) {
    if (!o) return;
    o->polarity = CBA_BLOB_DARK;
    o->inner_half = 2;
    o->outer_half = 12;
    o->min_contrast = 30;
    o->nms_radius = 4;
    o->max_radius = 20;
    o->rounds = 3;
    o->max_fit_error = 0.2;
    o->max_axis_ratio = 3.0;
    o->min_radius = 1.5;
    o->reserved = 0;
}

cba_status cba_blob_detector_create(int32_t width, int32_t height, int32_t max_images, int32_t max_blobs, const cba_blob_options* opts,
                                    int32_t device, cba_blob_detector** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        if (!opts) throw std::invalid_argument("null argument");
        check_sides(width, height);
        if (opts->polarity != CBA_BLOB_DARK && opts->polarity != CBA_BLOB_BRIGHT) throw std::invalid_argument("polarity must be DARK or BRIGHT");
        if (opts->inner_half < 1 || opts->inner_half > 7) throw std::invalid_argument("inner_half must be in 1..7");
        if (opts->outer_half <= opts->inner_half || opts->outer_half > 15) throw std::invalid_argument("outer_half must be in inner_half + 1..15");
        if (opts->min_contrast < 1 || opts->min_contrast > 255) throw std::invalid_argument("min_contrast must be in 1..255");
        if (opts->nms_radius < 1 || opts->nms_radius > 10) throw std::invalid_argument("nms_radius must be in 1..10");
        if (opts->max_radius < 2 || opts->max_radius > 32) throw std::invalid_argument("max_radius must be in 2..32");
        if (opts->rounds < 1 || opts->rounds > 8) throw std::invalid_argument("rounds must be in 1..8");
        if (!(opts->max_fit_error > 0.0) || !(opts->max_axis_ratio >= 1.0) || !(opts->min_radius >= 0.0))
            throw std::invalid_argument("max_fit_error must be > 0, max_axis_ratio >= 1 and min_radius >= 0");
        const int side = 2 * (opts->outer_half + opts->nms_radius) + 1;
        if (width < side || height < side) throw std::invalid_argument("width and height must be >= 2 (outer_half + nms_radius) + 1");
        check_image_batch(width, height, max_images, "max_images");
        check_peak_capacity(max_images, max_blobs, "max_blobs");
        require_device(device);
        *out = reinterpret_cast<cba_blob_detector*>(blob_detector_create(width, height, max_images, max_blobs, *opts, device));
    });
}

static cba_status blob_detector_process_impl(cba_blob_detector* h, int32_t n_images, const uint8_t* images, int32_t* out_count,
                                             int32_t* out_status, double* out_xy, double* out_shape, double* out_fit_error,
                                             int32_t* out_response, int32_t* out_flags, double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        BlobDetector* d = reinterpret_cast<BlobDetector*>(h);
        if (!check_batch_call(n_images, blob_detector_max_images(d), "images", nullptr, images != nullptr)) return;
        blob_detector_process(d, n_images, images, out_count, out_status, out_xy, out_shape, out_fit_error, out_response, out_flags, stage_ms);
    });
}

cba_status cba_blob_detector_process(cba_blob_detector* h, int32_t n_images, const uint8_t* images, int32_t* out_count, int32_t* out_status,
                                     double* out_xy, double* out_shape, double* out_fit_error, int32_t* out_response, int32_t* out_flags) {
    return blob_detector_process_impl(h, n_images, images, out_count, out_status, out_xy, out_shape, out_fit_error, out_response, out_flags,
                                      nullptr);
}

void cba_blob_detector_destroy(cba_blob_detector* h) { blob_detector_destroy(reinterpret_cast<BlobDetector*>(h)); }

cba_status cba_circle_grid_order(int32_t n, const double* xy, const double* shape, int32_t pattern, int32_t rows, int32_t cols,
                                 int32_t* out_index, int32_t* out_unique) {
    return guarded([&] {
        if (!out_index) throw std::invalid_argument("null argument");
        if (n < 0) throw std::invalid_argument("n must be >= 0");
        if (pattern != CBA_CIRCLES_SYMMETRIC && pattern != CBA_CIRCLES_ASYMMETRIC) throw std::invalid_argument("pattern must be SYMMETRIC or ASYMMETRIC");
        if (rows < 2 || cols < 2 || static_cast<int64_t>(rows) * cols > 65536) throw std::invalid_argument("rows and cols must be >= 2, rows cols <= 65536");
        if (n > 0 && !xy) throw std::invalid_argument("null argument");
        if (n > 65536) throw std::invalid_argument("n must be <= 65536");
        for (int32_t i = 0; i < n; ++i) {
            if (!std::isfinite(xy[2 * i]) || !std::isfinite(xy[2 * i + 1])) throw std::invalid_argument("blobs must be finite");
            if (!shape) continue;
            const double* m = shape + 3 * i;
            if (!std::isfinite(m[0]) || !std::isfinite(m[1]) || !std::isfinite(m[2]) || !(m[0] > 0.0) || !(m[0] * m[2] - m[1] * m[1] > 0.0))
                throw std::invalid_argument("shapes must be finite and positive definite");
        }
        int unique = 0;
        if (!circle_grid_order(n, xy, shape, pattern, rows, cols, out_index, &unique))
            for (int32_t i = 0; i < rows * cols; ++i) out_index[i] = -1;  // not found
        if (out_unique) *out_unique = unique;
    });
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_blobs.py): cba_blob_detector_process timing its stages on the device (stage_ms [5] = upload,
// response, peaks, refine, download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_blob_detector_process_timed(cba_blob_detector* h, int32_t n_images,
                                                                                  const uint8_t* images, int32_t* out_count,
                                                                                  int32_t* out_status, double* out_xy, double* out_shape,
                                                                                  double* out_fit_error, int32_t* out_response,
                                                                                  int32_t* out_flags, double* stage_ms) {
    return timed(stage_ms, [&] { return blob_detector_process_impl(h, n_images, images, out_count, out_status, out_xy, out_shape, out_fit_error,
                                                                   out_response, out_flags, stage_ms); });
}
#endif

// ---- ChArUco boards (marker_read.hip, marker_math.hpp, marker_board.hpp) -----------------------------------------------------------
void cba_charuco_options_default(cba_charuco_options* o) {
    if (!o) return;
    o->arm_lengths[0] = 7.0;
    o->arm_lengths[1] = 10.0;
    o->arm_offset = 2.0;
    o->arm_fan_deg = 14.0;
    o->min_arm_contrast = 112.0;
    o->min_marker_contrast = 40.0;
    o->min_component = 4;
    o->cell_samples = 3;
    o->max_border_errors = 1;
    o->max_correction = 1;
    o->min_markers = 2;
    o->reserved = 0;
}

static void check_charuco_board(const cba_charuco_board* b) {
    if (!b) throw std::invalid_argument("null argument");
    if (b->squares_x < 3 || b->squares_y < 3 || b->squares_x > 256 || b->squares_y > 256) throw std::invalid_argument("squares_x and squares_y must be in 3..256");
    if (b->marker_bits < 3 || b->marker_bits > MARKER_MAX_BITS) throw std::invalid_argument("marker_bits must be in 3..7");
    if (b->n_markers < 1 || b->n_markers > MARKER_MAX_CODES) throw std::invalid_argument("n_markers must be in 1..16384");
    if (!(b->square > 0.0) || !std::isfinite(b->square)) throw std::invalid_argument("square must be > 0");
    if (!(b->marker_ratio >= 0.4 && b->marker_ratio <= 0.8)) throw std::invalid_argument("marker_ratio must be in [0.4, 0.8]");
}

cba_status cba_charuco_detector_create(int32_t width, int32_t height, int32_t max_images, int32_t max_corners, int32_t max_cells,
                                       const cba_corner_options* corner_opts, const cba_charuco_options* o, const cba_charuco_board* board,
                                       const uint64_t* codes, int32_t device, cba_charuco_detector** out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        *out = nullptr;
        if (!o || !codes) throw std::invalid_argument("null argument");
        check_corner_create(width, height, max_images, max_corners, corner_opts);
        if (max_cells < 1 || max_cells > (1 << 24)) throw std::invalid_argument("max_cells must be in 1..2^24");
        check_charuco_board(board);
        for (int k = 0; k < 2; ++k)
            if (!(o->arm_lengths[k] > 0.0 && o->arm_lengths[k] <= 64.0)) throw std::invalid_argument("arm_lengths must be in (0, 64]");
        if (!(o->arm_offset > 0.0 && o->arm_offset <= 16.0)) throw std::invalid_argument("arm_offset must be in (0, 16]");
        if (!(o->arm_fan_deg >= 0.0 && o->arm_fan_deg <= 30.0)) throw std::invalid_argument("arm_fan_deg must be in [0, 30]");
        if (!(o->min_arm_contrast >= 0.0) || !(o->min_marker_contrast >= 0.0) || !std::isfinite(o->min_arm_contrast) || !std::isfinite(o->min_marker_contrast))
            throw std::invalid_argument("min_arm_contrast and min_marker_contrast must be finite and >= 0");
        if (o->min_component < 1) throw std::invalid_argument("min_component must be >= 1");
        if (o->cell_samples < 1 || o->cell_samples > 5) throw std::invalid_argument("cell_samples must be in 1..5");
        if (o->max_border_errors < 0 || o->max_correction < 0) throw std::invalid_argument("max_border_errors and max_correction must be >= 0");
        if (o->min_markers < 1) throw std::invalid_argument("min_markers must be >= 1");
        const int nbits = board->marker_bits * board->marker_bits;
        for (int32_t i = 0; i < board->n_markers; ++i)
            if (codes[i] >> nbits) throw std::invalid_argument("a code has bits above marker_bits^2");
        require_device(device);
        *out = reinterpret_cast<cba_charuco_detector*>(
            charuco_detector_create(width, height, max_images, max_corners, max_cells, *corner_opts, *o, *board, codes, device));
    });
}

static cba_status charuco_detector_process_impl(cba_charuco_detector* h, int32_t n_images, const uint8_t* images, int32_t* out_count,
                                                int32_t* out_status, int32_t* out_ids, double* out_xy, int32_t* out_n_markers,
                                                int32_t* out_n_corners, int32_t* out_n_cells, int32_t* out_cells,
                                                cba_marker_reading* out_readings, double* stage_ms) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        CharucoDetector* d = reinterpret_cast<CharucoDetector*>(h);
        if (out_n_cells) *out_n_cells = 0;
        if (!check_batch_call(n_images, charuco_detector_max_images(d), "images", nullptr, images != nullptr)) return;
        charuco_detector_process(d, n_images, images, out_count, out_status, out_ids, out_xy, out_n_markers, out_n_corners, out_n_cells,
                                 out_cells, out_readings, stage_ms);
    });
}

cba_status cba_charuco_detector_process(cba_charuco_detector* h, int32_t n_images, const uint8_t* images, int32_t* out_count,
                                        int32_t* out_status, int32_t* out_ids, double* out_xy, int32_t* out_n_markers, int32_t* out_n_corners,
                                        int32_t* out_n_cells, int32_t* out_cells, cba_marker_reading* out_readings) {
    return charuco_detector_process_impl(h, n_images, images, out_count, out_status, out_ids, out_xy, out_n_markers, out_n_corners, out_n_cells,
                                         out_cells, out_readings, nullptr);
}

#ifdef CBA_EXPERIMENTS
// Experiment builds only (tools/bench_charuco.py): cba_charuco_detector_process timing its stages (stage_ms [9] = upload, response,
// peaks, refine, arms, host lattice, read, host match, download).  Not part of calibba.h.
__attribute__((visibility("default"))) cba_status cba_charuco_detector_process_timed(cba_charuco_detector* h, int32_t n_images,
                                                                                     const uint8_t* images, int32_t* out_count,
                                                                                     int32_t* out_n_markers, int32_t* out_n_cells,
                                                                                     double* stage_ms) {
    return timed(stage_ms, [&] { return charuco_detector_process_impl(h, n_images, images, out_count, nullptr, nullptr, nullptr, out_n_markers,
                                                                      nullptr, out_n_cells, nullptr, nullptr, stage_ms); });
}
#endif

cba_status cba_charuco_detector_arms(cba_charuco_detector* h, int32_t n_images, const double* dirs, double* out_score) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        CharucoDetector* d = reinterpret_cast<CharucoDetector*>(h);
        const char* other = n_images != charuco_detector_last_images(d) ? "n_images must be that of the last process" : nullptr;
        if (!check_batch_call(n_images, charuco_detector_max_images(d), "images", other, dirs != nullptr && out_score != nullptr)) return;
        charuco_detector_arms(d, n_images, dirs, out_score);
    });
}

cba_status cba_charuco_detector_read(cba_charuco_detector* h, int32_t n_cells, const int32_t* cell_image, const double* quads,
                                     cba_marker_reading* out_readings) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("null argument");
        CharucoDetector* d = reinterpret_cast<CharucoDetector*>(h);
        if (!check_batch_call(n_cells, charuco_detector_max_cells(d), "cells", nullptr, cell_image && quads && out_readings)) return;
        for (int32_t i = 0; i < n_cells; ++i)
            if (cell_image[i] < 0 || cell_image[i] >= charuco_detector_last_images(d))
                throw std::invalid_argument("a cell's image index lies outside the last process");
        charuco_detector_read(d, n_cells, cell_image, quads, out_readings);
    });
}

void cba_charuco_detector_destroy(cba_charuco_detector* h) { charuco_detector_destroy(reinterpret_cast<CharucoDetector*>(h)); }

cba_status cba_marker_dictionary_generate(int32_t bits, int32_t count, int32_t min_distance, uint64_t seed, uint64_t* codes,
                                          int32_t* out_found) {
    return guarded([&] {
        if (!codes || !out_found) throw std::invalid_argument("null argument");
        *out_found = 0;
        if (bits < 3 || bits > MARKER_MAX_BITS) throw std::invalid_argument("bits must be in 3..7");
        if (count < 1 || count > MARKER_MAX_CODES) throw std::invalid_argument("count must be in 1..16384");
        if (min_distance < 0 || min_distance > bits * bits) throw std::invalid_argument("min_distance must be in 0..bits^2");
        *out_found = marker_dictionary_generate(bits, count, min_distance, seed, codes);
    });
}

static void check_corner_list(int32_t n, const double* xy, const double* angle) {
    if (n < 0 || n > 65536) throw std::invalid_argument("n must be in 0..65536");
    if (n > 0 && !xy) throw std::invalid_argument("null argument");
    for (int32_t i = 0; i < n; ++i)
        if (!std::isfinite(xy[2 * i]) || !std::isfinite(xy[2 * i + 1]) || (angle && !std::isfinite(angle[i])))
            throw std::invalid_argument("corners must be finite");
}

cba_status cba_chessboard_lattice(int32_t n, const double* xy, const double* angle, int32_t min_component, int32_t* out_component,
                                  int32_t* out_ij, int32_t* out_n_components) {
    return guarded([&] {
        if (out_n_components) *out_n_components = 0;
        if (n > 0 && (!angle || !out_component || !out_ij)) throw std::invalid_argument("null argument");
        check_corner_list(n, xy, angle);
        if (min_component < 1) throw std::invalid_argument("min_component must be >= 1");
        const int k = chessboard_lattice(n, xy, angle, min_component, out_component, out_ij);
        if (out_n_components) *out_n_components = k;
    });
}

cba_status cba_charuco_match(const cba_charuco_board* board, int32_t min_markers, int32_t n, const int32_t* component, const int32_t* ij,
                             const double* xy, int32_t n_cells, const int32_t* cells, const int32_t* flags, const int32_t* id,
                             const int32_t* rotation, int32_t* out_count, int32_t* out_ids, double* out_xy, int32_t* out_n_markers) {
    return guarded([&] {
        if (!out_count || !out_ids || !out_xy) throw std::invalid_argument("null argument");
        *out_count = 0;
        check_charuco_board(board);
        if (min_markers < 1) throw std::invalid_argument("min_markers must be >= 1");
        if (n < 0 || n > 65536 || n_cells < 0 || n_cells > 65536) throw std::invalid_argument("n and n_cells must be in 0..65536");
        if ((n > 0 && (!component || !ij || !xy)) || (n_cells > 0 && (!cells || !flags || !id || !rotation))) throw std::invalid_argument("null argument");
        for (int32_t c = 0; c < n; ++c) {
            if (component[c] < -1 || component[c] > 65536 || ij[2 * c] < -65536 || ij[2 * c] > 65536 || ij[2 * c + 1] < -65536 || ij[2 * c + 1] > 65536)
                throw std::invalid_argument("a corner's component or label is out of range");
            if (component[c] >= 0 && (!std::isfinite(xy[2 * c]) || !std::isfinite(xy[2 * c + 1]))) throw std::invalid_argument("corners must be finite");
        }
        for (int32_t t = 0; t < 3 * n_cells; ++t)
            if (cells[t] < -65536 || cells[t] > 65536) throw std::invalid_argument("a cell's component or label is out of range");
        int32_t nm = 0;
        *out_count = charuco_match(CharucoBoard{board->squares_x, board->squares_y}, min_markers, n, component, ij, xy, n_cells, cells, flags, id,
                                   rotation, out_ids, out_xy, &nm);
        if (out_n_markers) *out_n_markers = nm;
    });
}

}  // extern "C"
