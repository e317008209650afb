// calibba_linear.hpp — header-only C++ adapter of the linear seed of planar intrinsic calibration: the reference's
// estimate_homography, estimate_intrinsics, zhang_intrinsics_from_hs and pose_from_homography with their signatures, on top of the
// C ABI of include/calibba.h (cba_estimate_homography_ransac_batch, cba_estimate_intrinsics, cba_zhang_intrinsics_from_hs,
// cba_pose_from_homography).  Like calibba_adapter.hpp it is compiled in the reference's tree (it needs Eigen and the
// reference's headers) and only flattens containers and maps status codes back to the reference's exception types.  It is a
// separate header so that calibba_adapter.hpp does not pull in the linear-estimation headers.
//
//   replaces                                   (reference file:line)
//   calib::estimate_homography                 include/calib/estimation/linear/homography.h:22-24 (optim/homography.cpp:31-60)
//   calib::estimate_intrinsics                 include/calib/estimation/linear/intrinsics.h:56-58 (linear/intrinsicsdlt.cpp:101-145)
//   calib::zhang_intrinsics_from_hs            include/calib/estimation/linear/zhang.h:13-14 (linear/zhang.cpp:174-206)
//   calib::pose_from_homography                include/calib/estimation/linear/posefromhomography.h:52 (posefromhomography.cpp:11-62)
//
// The functions live in namespace calibba_adapter, as the ones of calibba_adapter.hpp do, so a caller switches by namespace.
// Departures from the reference (RANSAC scores every hypothesis and draws its samples from a counter-based stream) are listed in
// calibba.h.  The diagnostic messages the reference prints are not reproduced; PoseFromHResult::message names the failed check.
#pragma once
#include <cmath>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "calib/estimation/common/ransac.h"
#include "calib/estimation/linear/homography.h"
#include "calib/estimation/linear/intrinsics.h"
#include "calib/estimation/linear/posefromhomography.h"
#include "calib/estimation/linear/zhang.h"
#include "calibba.h"

namespace calibba_adapter {
namespace linear_detail {

inline void check(cba_status st) {
    if (st == CBA_OK) return;
    if (st == CBA_ERR_INVALID_ARGUMENT) throw std::invalid_argument(cba_last_error());
    throw std::runtime_error(cba_last_error());
}

struct FlatViews {
    std::vector<int64_t> off{0};
    std::vector<double> X, Y, u, v;
    explicit FlatViews(const std::vector<calib::PlanarView>& views) {
        for (const auto& view : views) {
            for (const auto& o : view) {
                X.push_back(o.object_xy.x()); Y.push_back(o.object_xy.y());
                u.push_back(o.image_uv.x()); v.push_back(o.image_uv.y());
            }
            off.push_back(static_cast<int64_t>(X.size()));
        }
    }
    int32_t n_views() const { return static_cast<int32_t>(off.size() - 1); }
};

inline cba_ransac_options ransac_options(const calib::RansacOptions& r) {
    cba_ransac_options o;
    o.max_iters = r.max_iters;
    o.thresh = r.thresh;
    o.min_inliers = r.min_inliers;
    o.refit_on_inliers = r.refit_on_inliers ? 1 : 0;
    o.confidence = r.confidence;
    o.seed = r.seed;
    return o;
}

inline Eigen::Matrix3d matrix3(const double* h) {
    Eigen::Matrix3d m;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) m(r, c) = h[3 * r + c];
    return m;
}

inline void put_matrix3(const Eigen::Matrix3d& m, double* h) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) h[3 * r + c] = m(r, c);
}

inline Eigen::Isometry3d isometry(const double* rt12) {
    Eigen::Isometry3d T = Eigen::Isometry3d::Identity();
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T.linear()(r, c) = rt12[3 * r + c];
        T.translation()[r] = rt12[9 + r];
    }
    return T;
}

inline std::vector<int> inliers_of(const std::vector<uint8_t>& mask, int64_t b, int64_t e) {
    std::vector<int> out;
    for (int64_t i = b; i < e; ++i)
        if (mask[static_cast<size_t>(i)]) out.push_back(static_cast<int>(i - b));
    return out;
}

}  // namespace linear_detail

// estimate_homography (homography.h:22-24): RANSAC with ransac_opts, the all-points DLT without.  H is not rescaled by h22.
inline auto estimate_homography(const calib::PlanarView& data, std::optional<calib::RansacOptions> ransac_opts = std::nullopt)
    -> calib::HomographyResult {
    const linear_detail::FlatViews f({data});
    const size_t n = f.X.size();
    double h9[9];
    int32_t ok = 0, cnt = 0;
    double rms = 0.0;
    std::vector<uint8_t> mask(n > 0 ? n : 1);
    cba_ransac_options o{};
    if (ransac_opts) o = linear_detail::ransac_options(*ransac_opts);
    linear_detail::check(cba_estimate_homography_ransac_batch(1, f.off.data(), f.X.data(), f.Y.data(), f.u.data(), f.v.data(),
                                                              ransac_opts ? &o : nullptr, h9, &ok, &cnt, &rms, mask.data()));
    calib::HomographyResult r;
    r.success = ok != 0;
    if (r.success) {
        r.hmtx = linear_detail::matrix3(h9);
        r.inliers = linear_detail::inliers_of(mask, 0, static_cast<int64_t>(n));
        r.symmetric_rms_px = rms;
    }
    return r;
}

// estimate_intrinsics (intrinsics.h:56-58): result.views holds the views whose homography succeeded, each with its view_index
inline auto estimate_intrinsics(const std::vector<calib::PlanarView>& views, const calib::IntrinsicsEstimOptions& opts = {})
    -> calib::IntrinsicsEstimateResult {
    const linear_detail::FlatViews f(views);
    const int32_t nv = f.n_views();
    const size_t m = nv > 0 ? static_cast<size_t>(nv) : 1;
    std::vector<int32_t> ok(m), pok(m);
    std::vector<double> h9(9 * m), rms(m), rt(12 * m);
    std::vector<uint8_t> mask(f.X.empty() ? 1 : f.X.size());
    double k5[5];
    int32_t success = 0, sanitized = 0;
    cba_ransac_options o{};
    if (opts.homography_ransac) o = linear_detail::ransac_options(*opts.homography_ransac);
    double lo[5], hi[5];
    if (opts.bounds) {
        const auto& b = *opts.bounds;
        const double l[5] = {b.fx_min, b.fy_min, b.cx_min, b.cy_min, b.skew_min}, h[5] = {b.fx_max, b.fy_max, b.cx_max, b.cy_max, b.skew_max};
        for (int k = 0; k < 5; ++k) { lo[k] = l[k]; hi[k] = h[k]; }
    }
    linear_detail::check(cba_estimate_intrinsics(nv, f.off.data(), f.X.data(), f.Y.data(), f.u.data(), f.v.data(),
                                                 opts.homography_ransac ? 1 : 0, opts.homography_ransac ? &o : nullptr,
                                                 opts.bounds ? lo : nullptr, opts.bounds ? hi : nullptr, opts.use_skew ? 1 : 0, &success, k5,
                                                 &sanitized, ok.data(), h9.data(), rms.data(), rt.data(), pok.data(), mask.data()));
    calib::IntrinsicsEstimateResult result;
    if (!success) return result;
    result.success = true;
    result.kmtx.fx = k5[0]; result.kmtx.fy = k5[1]; result.kmtx.cx = k5[2]; result.kmtx.cy = k5[3]; result.kmtx.skew = k5[4];
    if (sanitized) result.log = "Intrinsics sanitized by bounds.";
    for (int32_t i = 0; i < nv; ++i) {
        if (!ok[static_cast<size_t>(i)]) continue;
        calib::ViewEstimateData ved;
        ved.view_index = static_cast<size_t>(i);
        ved.homography.success = true;
        ved.homography.hmtx = linear_detail::matrix3(&h9[9 * static_cast<size_t>(i)]);
        ved.homography.inliers = linear_detail::inliers_of(mask, f.off[static_cast<size_t>(i)], f.off[static_cast<size_t>(i) + 1]);
        ved.homography.symmetric_rms_px = rms[static_cast<size_t>(i)];
        ved.forward_rms_px = rms[static_cast<size_t>(i)];
        if (pok[static_cast<size_t>(i)]) ved.c_se3_t = linear_detail::isometry(&rt[12 * static_cast<size_t>(i)]);
        result.views.push_back(ved);
    }
    return result;
}

// zhang_intrinsics_from_hs (zhang.h:13-14)
inline auto zhang_intrinsics_from_hs(const std::vector<calib::HomographyResult>& hs) -> std::optional<calib::CameraMatrix> {
    std::vector<double> h9(9 * (hs.empty() ? 1 : hs.size()));
    for (size_t i = 0; i < hs.size(); ++i) linear_detail::put_matrix3(hs[i].hmtx, &h9[9 * i]);
    double k5[5];
    int32_t ok = 0;
    linear_detail::check(cba_zhang_intrinsics_from_hs(static_cast<int32_t>(hs.size()), h9.data(), k5, &ok));
    if (!ok) return std::nullopt;
    calib::CameraMatrix k;
    k.fx = k5[0]; k.fy = k5[1]; k.cx = k5[2]; k.cy = k5[3]; k.skew = k5[4];
    return k;
}

// pose_from_homography (posefromhomography.h:52)
inline auto pose_from_homography(const calib::CameraMatrix& kmtx, const Eigen::Matrix3d& hmtx) -> calib::PoseFromHResult {
    const double k5[5] = {kmtx.fx, kmtx.fy, kmtx.cx, kmtx.cy, kmtx.skew};
    double h9[9], rt[12], scale = 0.0, cond = 0.0;
    linear_detail::put_matrix3(hmtx, h9);
    int32_t ok = 0;
    linear_detail::check(cba_pose_from_homography(k5, h9, rt, &ok, &scale, &cond));
    calib::PoseFromHResult out;
    if (!ok) {  // the check that failed (posefromhomography.cpp:16-35)
        if (!std::isfinite(kmtx.fx) || !std::isfinite(kmtx.fy) || kmtx.cx <= 0 || kmtx.cy <= 0) out.message = "Invalid camera matrix K";
        else if (!std::isfinite(hmtx(2, 2))) out.message = "Invalid homography H.";
        else out.message = "Degenerate H: zero column norm.";
        return out;
    }
    out.success = true;
    out.c_se3_t = linear_detail::isometry(rt);
    out.scale = scale;
    out.cond_check = cond;
    out.message = "OK";
    return out;
}

}  // namespace calibba_adapter
