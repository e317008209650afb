// calibba_camera.hpp — header-only C++ adapter of the camera models: batch project / unproject / distort / undistort over the
// reference's PinholeCamera<BrownConradyd>, PinholeCamera<DualDistortion> and ScheimpflugCamera<PinholeCamera<...>> with Eigen
// vectors, and an RAII undistortion map, on top of the C ABI of include/calibba.h (cba_camera_project, cba_camera_unproject,
// cba_undistort_map_*).  Like calibba_distortion.hpp it is compiled in the reference's tree (it needs Eigen and the reference's
// headers), only flattens containers and maps status codes to exceptions; neither calibba_adapter.hpp nor calibba_linear.hpp
// includes it.
//
//   replaces (batched)                               (reference file:line)
//   PinholeCamera::project / unproject               include/calib/models/pinhole.h:96-113
//   ScheimpflugCamera::project                       include/calib/models/scheimpflug.h:139-181
//   BrownConrady::distort / undistort                include/calib/models/distortion.h:119-160
//   DualDistortion::undistort                        include/calib/models/distortion.h:208-218
//
// The device runs the Brown-Conrady model with three radial terms: forward coefficients [k1, k2, p1, p2] are taken as
// [k1, k2, 0, p1, p2]; any other count than 4 or 5 is std::invalid_argument.  ScheimpflugCamera's unproject here is the exact
// inverse documented in calibba.h (the reference's own cannot be instantiated).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "calib/models/distortion.h"
#include "calib/models/pinhole.h"
#include "calib/models/scheimpflug.h"
#include "calibba.h"

namespace calibba_adapter {
namespace camera_detail {

inline void check(cba_status st) {
    if (st == CBA_OK) return;
    if (st == CBA_ERR_INVALID_ARGUMENT) throw std::invalid_argument(cba_last_error());
    throw std::runtime_error(cba_last_error());
}

template <typename V>
inline void dist5(const V& c, double* out) {
    if (c.size() == 4) {
        out[0] = c[0]; out[1] = c[1]; out[2] = 0.0; out[3] = c[2]; out[4] = c[3];
    } else if (c.size() == 5) {
        for (int k = 0; k < 5; ++k) out[k] = c[k];
    } else {
        throw std::invalid_argument("the device model takes 4 or 5 Brown-Conrady coefficients");
    }
}

// A camera as the C ABI takes it: model, intr [10 | 12], the inverse coefficients of a DualDistortion (empty otherwise)
struct Flat {
    int32_t model = CBA_CAMERA_PINHOLE_BC;
    double intr[12] = {};
    std::vector<double> inv;
};

template <typename K>
inline void kmtx(const K& k, double* intr) {
    intr[0] = k.fx; intr[1] = k.fy; intr[2] = k.cx; intr[3] = k.cy; intr[4] = k.skew;
}

inline Flat flat(const calib::PinholeCamera<calib::BrownConradyd>& c) {
    Flat f;
    kmtx(c.kmtx, f.intr);
    dist5(c.distortion.coeffs, f.intr + 5);
    return f;
}

inline Flat flat(const calib::PinholeCamera<calib::DualDistortion>& c) {
    Flat f;
    kmtx(c.kmtx, f.intr);
    dist5(c.distortion.forward, f.intr + 5);
    f.inv.assign(c.distortion.inverse.data(), c.distortion.inverse.data() + c.distortion.inverse.size());
    return f;
}

template <typename CameraT>
inline Flat flat(const calib::ScheimpflugCamera<CameraT>& c) {
    Flat f = flat(c.camera);
    f.model = CBA_CAMERA_SCHEIMPFLUG;
    f.intr[10] = c.tau_x;
    f.intr[11] = c.tau_y;
    return f;
}

inline std::vector<Eigen::Matrix<double, 2, 1>> unpack2(const std::vector<double>& a) {
    std::vector<Eigen::Matrix<double, 2, 1>> out(a.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = Eigen::Matrix<double, 2, 1>(a[2 * i], a[2 * i + 1]);
    return out;
}

inline std::vector<double> project_flat(const Flat& f, const std::vector<double>& xyz) {
    std::vector<double> uv(xyz.size() / 3 * 2);
    check(cba_camera_project(f.model, f.intr, static_cast<int64_t>(xyz.size() / 3), xyz.data(), uv.data()));
    return uv;
}

inline std::vector<double> unproject_flat(const Flat& f, const std::vector<double>& uv) {
    std::vector<double> xy(uv.size());
    check(cba_camera_unproject(f.model, f.intr, static_cast<int32_t>(f.inv.size()), f.inv.empty() ? nullptr : f.inv.data(),
                               static_cast<int64_t>(uv.size() / 2), uv.data(), xy.data()));
    return xy;
}

inline Flat identity_k(const Flat& c) {
    Flat f = c;
    f.model = CBA_CAMERA_PINHOLE_BC;
    f.intr[0] = 1.0; f.intr[1] = 1.0; f.intr[2] = 0.0; f.intr[3] = 0.0; f.intr[4] = 0.0;
    return f;
}

}  // namespace camera_detail

// camera.project(xyz) of every camera-frame point
template <typename CameraT>
inline std::vector<Eigen::Matrix<double, 2, 1>> project(const CameraT& camera, const std::vector<Eigen::Matrix<double, 3, 1>>& xyz) {
    std::vector<double> a;
    a.reserve(3 * xyz.size());
    for (const auto& p : xyz) { a.push_back(p.x()); a.push_back(p.y()); a.push_back(p.z()); }
    return camera_detail::unpack2(camera_detail::project_flat(camera_detail::flat(camera), a));
}

// camera.project(norm_xy) of every normalised point
template <typename CameraT>
inline std::vector<Eigen::Matrix<double, 2, 1>> project(const CameraT& camera, const std::vector<Eigen::Matrix<double, 2, 1>>& norm_xy) {
    std::vector<double> a;
    a.reserve(3 * norm_xy.size());
    for (const auto& p : norm_xy) { a.push_back(p.x()); a.push_back(p.y()); a.push_back(1.0); }
    return camera_detail::unpack2(camera_detail::project_flat(camera_detail::flat(camera), a));
}

// camera.unproject(pixel) of every pixel (Scheimpflug: the exact inverse of project, calibba.h)
template <typename CameraT>
inline std::vector<Eigen::Matrix<double, 2, 1>> unproject(const CameraT& camera, const std::vector<Eigen::Matrix<double, 2, 1>>& pixels) {
    std::vector<double> a;
    a.reserve(2 * pixels.size());
    for (const auto& p : pixels) { a.push_back(p.x()); a.push_back(p.y()); }
    return camera_detail::unpack2(camera_detail::unproject_flat(camera_detail::flat(camera), a));
}

// camera.distort / camera.undistort of normalised points (pinhole cameras: the distortion model alone)
template <typename DistortionT>
inline std::vector<Eigen::Matrix<double, 2, 1>> distort(const calib::PinholeCamera<DistortionT>& camera,
                                                        const std::vector<Eigen::Matrix<double, 2, 1>>& norm_xy) {
    std::vector<double> a;
    a.reserve(3 * norm_xy.size());
    for (const auto& p : norm_xy) { a.push_back(p.x()); a.push_back(p.y()); a.push_back(1.0); }
    return camera_detail::unpack2(camera_detail::project_flat(camera_detail::identity_k(camera_detail::flat(camera)), a));
}

template <typename DistortionT>
inline std::vector<Eigen::Matrix<double, 2, 1>> undistort(const calib::PinholeCamera<DistortionT>& camera,
                                                          const std::vector<Eigen::Matrix<double, 2, 1>>& distorted_xy) {
    std::vector<double> a;
    a.reserve(2 * distorted_xy.size());
    for (const auto& p : distorted_xy) { a.push_back(p.x()); a.push_back(p.y()); }
    return camera_detail::unpack2(camera_detail::unproject_flat(camera_detail::identity_k(camera_detail::flat(camera)), a));
}

// The undistortion / rectification maps of cameras of one model, kept on a device (calibba.h: cba_undistort_map_*).  R: row-major
// rotations [n][9] (empty: identity), new_k5: [n][5] = [fx', fy', cx', cy', skew'] (empty: each camera's own K).
class UndistortMap {
  public:
    template <typename CameraT>
    UndistortMap(const std::vector<CameraT>& cameras, int width, int height, const std::vector<double>& R = {},
                 const std::vector<double>& new_k5 = {}, int device = 0)
        : n_(static_cast<int>(cameras.size())), w_(width), h_(height) {
        std::vector<double> intr;
        int32_t model = CBA_CAMERA_PINHOLE_BC;
        for (const auto& c : cameras) {
            const camera_detail::Flat f = camera_detail::flat(c);
            model = f.model;
            intr.insert(intr.end(), f.intr, f.intr + (model == CBA_CAMERA_SCHEIMPFLUG ? 12 : 10));
        }
        camera_detail::check(cba_undistort_map_create(model, n_, intr.empty() ? nullptr : intr.data(), R.empty() ? nullptr : R.data(),
                                                      new_k5.empty() ? nullptr : new_k5.data(), width, height, device, &h_map_));
    }
    UndistortMap(const UndistortMap&) = delete;
    UndistortMap& operator=(const UndistortMap&) = delete;
    ~UndistortMap() { cba_undistort_map_destroy(h_map_); }

    // map_x, map_y [n_cams][height][width]
    void maps(std::vector<float>& map_x, std::vector<float>& map_y) const {
        const size_t n = static_cast<size_t>(n_) * w_ * h_;
        map_x.resize(n);
        map_y.resize(n);
        camera_detail::check(cba_undistort_map_fetch(h_map_, map_x.data(), map_y.data()));
    }

    // images [n][src_height][src_width][channels] of uint8_t or float -> [n][height][width][channels]
    template <typename T>
    std::vector<T> apply(const std::vector<T>& images, const std::vector<int32_t>& cams, int src_width, int src_height, int channels,
                         double border = 0.0) const {
        static_assert(sizeof(T) == 1 || sizeof(T) == 4, "uint8_t or float images");
        std::vector<T> out(cams.size() * static_cast<size_t>(w_) * h_ * static_cast<size_t>(channels > 0 ? channels : 0));
        camera_detail::check(cba_undistort_map_apply(h_map_, static_cast<int32_t>(cams.size()), cams.data(), src_width, src_height, channels,
                                                     sizeof(T) == 1 ? CBA_DTYPE_U8 : CBA_DTYPE_F32, border, images.data(), out.data()));
        return out;
    }

  private:
    int n_, w_, h_;
    cba_undistort_map* h_map_ = nullptr;
};

}  // namespace calibba_adapter
