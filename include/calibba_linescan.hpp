// calibba_linescan.hpp — header-only C++ adapter of the laser-plane calibration: the reference's line-scan entry points with
// their signatures, on top of the C ABI of include/calibba.h (cba_calibrate_laser_plane, cba_fit_plane,
// cba_invert_brown_conrady).  Like calibba_adapter.hpp it is compiled in the reference's tree (it needs Eigen and the
// reference's headers) and only flattens containers and maps status codes back to the reference's exception types.  It is
// a separate header so that calibba_adapter.hpp does not pull in the line-scan headers.
//
//   replaces                                                  (reference file:line)
//   calib::calibrate_laser_plane<CameraT>                     include/calib/estimation/linear/linescan.h:101-144
//   calib::points_from_view<CameraT>                          include/calib/estimation/linear/linescan.h:63-91
//   calib::fit_plane_svd, calib::fit_plane_ransac             src/estimation/linear/planefit.cpp:68-114
//   calib::invert_brown_conrady                               include/calib/models/distortion.h:165-195
//   calib::pipeline::LinescanCalibrationFacade::calibrate     src/pipeline/linescan.cpp
//
// The functions live in namespace calibba_adapter, as the ones of calibba_adapter.hpp do: calibrate_laser_plane and
// points_from_view are inline templates of the reference's own header, so a caller switches by namespace (or the facade
// class below), not by relinking.
//
// Cameras: PinholeCamera<BrownConradyd> (undistortion by the 5-step fixed point; at most 3 radial terms),
// PinholeCamera<DualDistortion> (undistortion by the inverse coefficients, 2..16 of them), and ScheimpflugCamera of either.
// Departures from the reference (Scheimpflug unprojection, the plane's sign, RANSAC's sample generator) are listed in
// calibba.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "calib/estimation/common/ransac.h"
#include "calib/estimation/linear/linescan.h"
#include "calib/estimation/linear/planefit.h"
#include "calib/models/distortion.h"
#include "calib/models/pinhole.h"
#include "calib/models/scheimpflug.h"
#include "calib/pipeline/facades/linescan.h"
#include "calibba.h"

namespace calibba_adapter {
namespace linescan_detail {

inline void check(cba_status st) {
    if (st == CBA_OK) return;
    if (st == CBA_ERR_INVALID_ARGUMENT) throw std::invalid_argument(cba_last_error());
    throw std::runtime_error(cba_last_error());
}

struct FlatCamera {
    int32_t model = CBA_CAMERA_PINHOLE_BC;
    double intr[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<double> inverse;  // empty: iterative undistortion
};

inline void put_kmtx(const calib::CameraMatrix& k, FlatCamera& c) {
    c.intr[0] = k.fx; c.intr[1] = k.fy; c.intr[2] = k.cx; c.intr[3] = k.cy; c.intr[4] = k.skew;
}

// [k1 .. k_nr, p1, p2] -> intr[5..9] = [k1 k2 k3 p1 p2]
inline void put_forward(const Eigen::VectorXd& coeffs, FlatCamera& c) {
    const Eigen::Index n = coeffs.size();
    if (n < 2) throw std::runtime_error("Insufficient distortion coefficients");
    if (n - 2 > 3) throw std::invalid_argument("calibba: at most 3 radial distortion terms are supported");
    for (Eigen::Index i = 0; i < n - 2; ++i) c.intr[5 + i] = coeffs[i];
    c.intr[8] = coeffs[n - 2];
    c.intr[9] = coeffs[n - 1];
}

inline FlatCamera flatten(const calib::PinholeCamera<calib::BrownConradyd>& cam) {
    FlatCamera c;
    put_kmtx(cam.kmtx, c);
    put_forward(cam.distortion.coeffs, c);
    return c;
}

inline FlatCamera flatten(const calib::PinholeCamera<calib::DualDistortion>& cam) {
    FlatCamera c;
    put_kmtx(cam.kmtx, c);
    c.inverse.assign(cam.distortion.inverse.data(), cam.distortion.inverse.data() + cam.distortion.inverse.size());
    if (c.inverse.size() < 2) throw std::runtime_error("Insufficient distortion coefficients");
    return c;
}

template <class Inner>
FlatCamera flatten(const calib::ScheimpflugCamera<Inner>& cam) {
    FlatCamera c = flatten(cam.camera);
    c.model = CBA_CAMERA_SCHEIMPFLUG;
    c.intr[10] = cam.tau_x;
    c.intr[11] = cam.tau_y;
    return c;
}

inline cba_plane_fit_options options(bool use_ransac, const calib::RansacOptions& r) {
    cba_plane_fit_options o;
    cba_plane_fit_options_default(&o);
    o.use_ransac = use_ransac ? 1 : 0;
    o.max_iters = r.max_iters;
    o.thresh = r.thresh;
    o.min_inliers = r.min_inliers;
    o.refit_on_inliers = r.refit_on_inliers ? 1 : 0;
    o.confidence = r.confidence;
    o.seed = r.seed;
    return o;
}

struct FlatViews {
    std::vector<int64_t> toff{0}, loff{0};
    std::vector<double> X, Y, u, v, lu, lv;
    void push(const calib::LineScanView& view) {
        for (const auto& o : view.target_view) {
            X.push_back(o.object_xy.x()); Y.push_back(o.object_xy.y());
            u.push_back(o.image_uv.x()); v.push_back(o.image_uv.y());
        }
        for (const auto& p : view.laser_uv) { lu.push_back(p.x()); lv.push_back(p.y()); }
        toff.push_back(static_cast<int64_t>(X.size()));
        loff.push_back(static_cast<int64_t>(lu.size()));
    }
};

inline cba_status run(const FlatCamera& c, const FlatViews& f, const cba_plane_fit_options& o, cba_laser_plane_result* r, double* xyz) {
    return cba_calibrate_laser_plane(c.model, c.intr, static_cast<int32_t>(c.inverse.size()), c.inverse.empty() ? nullptr : c.inverse.data(),
                                     static_cast<int32_t>(f.toff.size() - 1), f.toff.data(), f.X.data(), f.Y.data(), f.u.data(), f.v.data(),
                                     f.loff.data(), f.lu.data(), f.lv.data(), &o, r, xyz, nullptr);
}

inline std::vector<Eigen::Vector3d> to_points(const std::vector<double>& xyz, std::size_t n) {
    std::vector<Eigen::Vector3d> p(n);
    for (std::size_t i = 0; i < n; ++i) p[i] = Eigen::Vector3d(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    return p;
}

}  // namespace linescan_detail

template <class CameraT>
auto calibrate_laser_plane(const std::vector<calib::LineScanView>& views, const CameraT& camera, const calib::LineScanPlaneFitOptions& opts = {})
    -> calib::LineScanCalibrationResult {
    namespace d = linescan_detail;
    const d::FlatCamera c = d::flatten(camera);
    d::FlatViews f;
    for (const auto& v : views) f.push(v);
    cba_laser_plane_result r;
    d::check(d::run(c, f, d::options(opts.use_ransac, opts.ransac_options), &r, nullptr));
    calib::LineScanCalibrationResult out;
    for (int k = 0; k < 4; ++k) out.plane[k] = r.plane[k];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out.homography(i, j) = r.homography[3 * i + j];
    out.covariance.setZero();
    out.rms_error = r.rms_error;
    out.summary = r.summary;
    out.inlier_count = static_cast<std::size_t>(r.inlier_count);
    return out;
}

// points_from_view of one view: empty when its homography fails.  Runs through cba_calibrate_laser_plane (two views and three
// points at least): the view is paired with a copy whose laser pixels are its target pixels.
template <class CameraT>
auto points_from_view(const calib::LineScanView& view, const CameraT& camera) -> std::vector<Eigen::Vector3d> {
    namespace d = linescan_detail;
    const d::FlatCamera c = d::flatten(camera);
    if (view.target_view.size() < 4) throw std::invalid_argument("Each view requires >=4 target correspondences");
    calib::LineScanView helper;
    helper.target_view = view.target_view;
    for (const auto& o : view.target_view) helper.laser_uv.push_back(o.image_uv);
    d::FlatViews f;
    f.push(view);
    f.push(helper);
    std::vector<double> xyz(3 * std::max<std::size_t>(f.lu.size(), 1));
    cba_laser_plane_result r;
    const cba_status st = d::run(c, f, d::options(false, {}), &r, xyz.data());
    if (st == CBA_ERR_INVALID_ARGUMENT && std::string(cba_last_error()) == "Not enough laser points to fit a plane") return {};
    d::check(st);
    if (r.n_views_used == 0) return {};
    return d::to_points(xyz, view.laser_uv.size());
}

inline auto fit_plane_svd(const std::vector<Eigen::Vector3d>& pts) -> Eigen::Vector4d {
    std::vector<double> xyz;
    for (const auto& p : pts) { xyz.push_back(p[0]); xyz.push_back(p[1]); xyz.push_back(p[2]); }
    const cba_plane_fit_options o = linescan_detail::options(false, {});
    double plane[4], rms;
    int64_t cnt;
    linescan_detail::check(cba_fit_plane(static_cast<int64_t>(pts.size()), xyz.data(), &o, plane, &rms, &cnt, nullptr));
    Eigen::Vector4d out;
    for (int k = 0; k < 4; ++k) out[k] = plane[k];
    return out;
}

inline auto fit_plane_ransac(const std::vector<Eigen::Vector3d>& pts, const calib::RansacOptions& opts = {}) -> calib::PlaneRansacResult {
    calib::PlaneRansacResult res;
    if (pts.size() < 3) return res;
    std::vector<double> xyz;
    for (const auto& p : pts) { xyz.push_back(p[0]); xyz.push_back(p[1]); xyz.push_back(p[2]); }
    const cba_plane_fit_options o = linescan_detail::options(true, opts);
    double plane[4], rms;
    int64_t cnt;
    std::vector<uint8_t> mask(pts.size());
    const cba_status st = cba_fit_plane(static_cast<int64_t>(pts.size()), xyz.data(), &o, plane, &rms, &cnt, mask.data());
    if (st == CBA_ERR_RUNTIME) return res;  // no model: the reference returns an unsuccessful result
    linescan_detail::check(st);
    res.success = true;
    for (int k = 0; k < 4; ++k) res.plane[k] = plane[k];
    for (std::size_t i = 0; i < pts.size(); ++i)
        if (mask[i]) res.inliers.push_back(static_cast<int>(i));
    res.inlier_rms = rms;
    return res;
}

inline auto invert_brown_conrady(const Eigen::VectorXd& forward) -> Eigen::VectorXd {
    Eigen::VectorXd inv(forward.size());
    linescan_detail::check(cba_invert_brown_conrady(static_cast<int32_t>(forward.size()), forward.data(), inv.data()));
    return inv;
}

// LinescanCalibrationFacade::calibrate (src/pipeline/linescan.cpp): the camera becomes a DualDistortion camera through
// invert_brown_conrady, then calibrate_laser_plane; any failure gives success = false.
class LinescanCalibrationFacade final {
  public:
    [[nodiscard]] auto calibrate(const calib::PinholeCamera<calib::BrownConradyd>& camera, const std::vector<calib::LineScanView>& views,
                                 const calib::pipeline::LinescanCalibrationOptions& opts = {}) const -> calib::pipeline::LinescanCalibrationRunResult {
        calib::pipeline::LinescanCalibrationRunResult out;
        out.used_views = views.size();
        try {
            calib::DualDistortion dual;
            dual.forward = camera.distortion.coeffs;
            dual.inverse = invert_brown_conrady(camera.distortion.coeffs);
            out.result = calibrate_laser_plane(views, calib::PinholeCamera<calib::DualDistortion>(camera.kmtx, dual), opts.plane_fit);
            out.success = true;
        } catch (...) {
            out.success = false;
        }
        return out;
    }
};

}  // namespace calibba_adapter
