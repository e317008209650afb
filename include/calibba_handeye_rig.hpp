// calibba_handeye_rig.hpp — header-only C++ adapter of the hand-eye / bundle seed: the reference's compute_handeye_initialization
// and choose_initial_target (src/pipeline/detail/bundle_utils.cpp:154-237) over BundleObservation records, on top of
// cba_estimate_bundle_seed (include/calibba.h).  Like calibba_extrinsics.hpp it is compiled in the reference's tree (it needs Eigen
// and the reference's headers), only flattens containers and maps status codes back to the reference's exception types.
//
//   replaces                                              (reference file:line)
//   calib::pipeline::detail::compute_handeye_initialization   src/pipeline/detail/bundle_utils.cpp:154-200
//   calib::pipeline::detail::choose_initial_target            src/pipeline/detail/bundle_utils.cpp:202-237
//
// The observations are listed view-major, as collect_bundle_observations lists them; blocks of fewer than 4 points are skipped.
// Only each camera's K is read (camera.kmtx, or the inner camera's for a Scheimpflug camera): distortion is ignored.  The JSON
// reports of the reference are replaced by per-camera status codes (CBA_HANDEYE_*) and the target source; the departures are listed
// in calibba.h.
#pragma once
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "calib/estimation/optim/bundle.h"
#include "calibba.h"

namespace calibba_adapter {

struct BundleSeedResult {
    std::vector<Eigen::Isometry3d> g_se3_c;  // HandeyeInitializationResult::transforms
    std::vector<int32_t> status;             // CBA_HANDEYE_* per camera
    std::vector<int32_t> pairs;              // motion pairs that passed the filter, per camera
    bool failed = false;                     // HandeyeInitializationResult::failed
    Eigen::Isometry3d b_se3_t = Eigen::Isometry3d::Identity();  // TargetInitializationResult::pose
    std::string target_source;               // "estimated" / "config" / "identity"
};

namespace handeye_rig_detail {

inline void check(cba_status st) {
    if (st == CBA_OK) return;
    if (st == CBA_ERR_INVALID_ARGUMENT) throw std::invalid_argument(cba_last_error());
    throw std::runtime_error(cba_last_error());
}

template <class CameraT>
const auto& kmtx_of(const CameraT& cam) {
    if constexpr (requires { cam.kmtx; })
        return cam.kmtx;
    else
        return kmtx_of(cam.camera);
}

// Eigen::Quaterniond(Matrix3d) restated (same as cba_pose_from_matrix), storage [w x y z] then t
inline void pose7_of(const Eigen::Isometry3d& T, double* p) {
    const auto& m = T.linear();
    double t = m(0, 0) + m(1, 1) + m(2, 2);
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        p[0] = 0.5 * t;
        t = 0.5 / t;
        p[1] = (m(2, 1) - m(1, 2)) * t;
        p[2] = (m(0, 2) - m(2, 0)) * t;
        p[3] = (m(1, 0) - m(0, 1)) * t;
    } else {
        int i = 0;
        if (m(1, 1) > m(0, 0)) i = 1;
        if (m(2, 2) > m(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0);
        p[1 + i] = 0.5 * t;
        t = 0.5 / t;
        p[0] = (m(k, j) - m(j, k)) * t;
        p[1 + j] = (m(j, i) + m(i, j)) * t;
        p[1 + k] = (m(k, i) + m(i, k)) * t;
    }
    for (int a = 0; a < 3; ++a) p[4 + a] = T.translation()[a];
}

// pose7 -> isometry; the quaternion (unit, from the seed) is converted without renormalising
inline Eigen::Isometry3d isometry(const double* p) {
    const double w = p[0], x = p[1], y = p[2], z = p[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)};
    Eigen::Isometry3d T = Eigen::Isometry3d::Identity();
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T.linear()(r, c) = R[3 * r + c];
    for (int k = 0; k < 3; ++k) T.translation()[k] = p[4 + k];
    return T;
}

}  // namespace handeye_rig_detail

// handeye[c]: a successful hand-eye stage result for camera c (the "handeye" source), or empty; initial_target: the configured
// target pose, or empty to estimate it.  handeye may be empty (no camera has one) or hold one entry per camera.
template <class CameraT>
auto estimate_bundle_seed(const std::vector<calib::BundleObservation>& observations, const std::vector<CameraT>& cameras,
                          double min_angle_deg = 1.0, const std::vector<std::optional<Eigen::Isometry3d>>& handeye = {},
                          const std::optional<Eigen::Isometry3d>& initial_target = std::nullopt) -> BundleSeedResult {
    namespace d = handeye_rig_detail;
    const size_t n_cams = cameras.size();
    if (!handeye.empty() && handeye.size() != n_cams) throw std::invalid_argument("one hand-eye entry per camera");
    std::vector<int64_t> off{0};
    std::vector<int32_t> bcam;
    std::vector<double> btg, X, Y, u, v, K;
    for (const auto& o : observations) {
        for (const auto& p : o.view) {
            X.push_back(p.object_xy.x()); Y.push_back(p.object_xy.y());
            u.push_back(p.image_uv.x()); v.push_back(p.image_uv.y());
        }
        off.push_back(static_cast<int64_t>(X.size()));
        bcam.push_back(static_cast<int32_t>(o.camera_index));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) btg.push_back(o.b_se3_g.linear()(r, c));
        for (int k = 0; k < 3; ++k) btg.push_back(o.b_se3_g.translation()[k]);
    }
    for (const auto& cam : cameras) {
        const auto& k = d::kmtx_of(cam);
        K.insert(K.end(), {static_cast<double>(k.fx), static_cast<double>(k.fy), static_cast<double>(k.cx), static_cast<double>(k.cy),
                           static_cast<double>(k.skew)});
    }
    std::vector<int32_t> mask;
    std::vector<double> given;
    if (!handeye.empty()) {
        mask.assign(n_cams, 0);
        given.assign(7 * n_cams, 0.0);
        for (size_t c = 0; c < n_cams; ++c) {
            given[7 * c] = 1.0;
            if (handeye[c]) {
                mask[c] = 1;
                d::pose7_of(*handeye[c], given.data() + 7 * c);
            }
        }
    }
    double bt_given[7];
    if (initial_target) d::pose7_of(*initial_target, bt_given);
    std::vector<double> g(7 * (n_cams ? n_cams : 1));
    BundleSeedResult out;
    out.status.assign(n_cams ? n_cams : 1, 0);
    out.pairs.assign(n_cams ? n_cams : 1, 0);
    double bt[7];
    int32_t src = 0;
    d::check(cba_estimate_bundle_seed(static_cast<int32_t>(n_cams), static_cast<int32_t>(bcam.size()), off.data(), bcam.data(), btg.data(),
                                      X.data(), Y.data(), u.data(), v.data(), K.data(), min_angle_deg, mask.empty() ? nullptr : mask.data(),
                                      given.empty() ? nullptr : given.data(), initial_target ? bt_given : nullptr, g.data(),
                                      out.status.data(), out.pairs.data(), bt, &src, nullptr, nullptr));
    out.status.resize(n_cams);
    out.pairs.resize(n_cams);
    for (size_t c = 0; c < n_cams; ++c) {
        out.g_se3_c.push_back(d::isometry(g.data() + 7 * c));
        out.failed = out.failed || (out.status[c] != CBA_HANDEYE_DLT && out.status[c] != CBA_HANDEYE_GIVEN);
    }
    out.b_se3_t = d::isometry(bt);
    out.target_source = src == CBA_TARGET_CONFIG ? "config" : (src == CBA_TARGET_IDENTITY ? "identity" : "estimated");
    return out;
}

}  // namespace calibba_adapter
