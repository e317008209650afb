// calibba_extrinsics.hpp — header-only C++ adapter of the linear seed of a multi-camera rig: the reference's estimate_extrinsic_dlt
// with its signature, on top of cba_estimate_extrinsic_dlt (include/calibba.h).  Like calibba_adapter.hpp it is compiled in the
// reference's tree (it needs Eigen and the reference's headers) and only flattens containers and maps status codes back to the
// reference's exception types.  It is a separate header so that calibba_adapter.hpp does not pull in the linear-estimation headers.
//
//   replaces                                   (reference file:line)
//   calib::estimate_extrinsic_dlt<CameraT>     include/calib/estimation/linear/extrinsics.h:27-78
//
// The function lives in namespace calibba_adapter, as the ones of calibba_adapter.hpp do, so a caller switches by namespace.
// Only each camera's K is read (camera.kmtx, or the inner camera's for a Scheimpflug camera): distortion is ignored, as in the
// reference.  An empty PlanarView is an absent block.  The departure on failed fits is listed in calibba.h.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "calib/estimation/linear/extrinsics.h"
#include "calibba.h"

namespace calibba_adapter {
namespace extrinsics_detail {

inline void check(cba_status st) {
    if (st == CBA_OK) return;
    if (st == CBA_ERR_INVALID_ARGUMENT) throw std::invalid_argument(cba_last_error());
    throw std::runtime_error(cba_last_error());
}

// the camera matrix apply_intrinsics uses: PinholeCamera::kmtx, or ScheimpflugCamera::camera's (scheimpflug.h:105-106)
template <class CameraT>
const auto& kmtx_of(const CameraT& cam) {
    if constexpr (requires { cam.kmtx; })
        return cam.kmtx;
    else
        return kmtx_of(cam.camera);
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

}  // namespace extrinsics_detail

template <class CameraT>
auto estimate_extrinsic_dlt(const std::vector<calib::MulticamPlanarView>& views, const std::vector<CameraT>& cameras) -> calib::ExtrinsicPoses {
    if (views.empty() || cameras.empty()) throw std::runtime_error("Empty views or cameras provided");
    const size_t n_cams = cameras.size(), n_views = views.size();
    for (size_t v = 0; v < n_views; ++v)
        if (views[v].size() != n_cams)
            throw std::runtime_error("View " + std::to_string(v) + " has wrong number of cameras: expected " + std::to_string(n_cams) +
                                     ", got " + std::to_string(views[v].size()));
    std::vector<int64_t> off{0};
    std::vector<int32_t> bview, bcam;
    std::vector<double> X, Y, u, v, K;
    for (size_t vi = 0; vi < n_views; ++vi)
        for (size_t c = 0; c < n_cams; ++c) {
            const auto& pv = views[vi][c];
            if (pv.empty()) continue;
            for (const auto& o : pv) {
                X.push_back(o.object_xy.x()); Y.push_back(o.object_xy.y());
                u.push_back(o.image_uv.x()); v.push_back(o.image_uv.y());
            }
            off.push_back(static_cast<int64_t>(X.size()));
            bview.push_back(static_cast<int32_t>(vi));
            bcam.push_back(static_cast<int32_t>(c));
        }
    for (const auto& cam : cameras) {
        const auto& k = extrinsics_detail::kmtx_of(cam);
        K.insert(K.end(), {static_cast<double>(k.fx), static_cast<double>(k.fy), static_cast<double>(k.cx), static_cast<double>(k.cy),
                           static_cast<double>(k.skew)});
    }
    std::vector<double> cr(7 * n_cams), rt(7 * n_views);
    extrinsics_detail::check(cba_estimate_extrinsic_dlt(static_cast<int32_t>(n_cams), static_cast<int32_t>(n_views),
                                                        static_cast<int32_t>(bview.size()), off.data(), bview.data(), bcam.data(), X.data(),
                                                        Y.data(), u.data(), v.data(), K.data(), cr.data(), rt.data(), nullptr, nullptr));
    calib::ExtrinsicPoses out;
    for (size_t c = 0; c < n_cams; ++c) out.c_se3_r.push_back(extrinsics_detail::isometry(cr.data() + 7 * c));
    for (size_t i = 0; i < n_views; ++i) out.r_se3_t.push_back(extrinsics_detail::isometry(rt.data() + 7 * i));
    return out;
}

}  // namespace calibba_adapter
