// calibba_distortion.hpp — header-only C++ adapter of the distortion fits and the linear intrinsic estimators: the reference's
// fit_distortion_full, fit_distortion, fit_distortion_dual, estimate_intrinsics_linear and estimate_intrinsics_linear_iterative
// with their signatures, on top of the C ABI of include/calibba.h (cba_fit_distortion_batch,
// cba_estimate_intrinsics_linear_batch, cba_estimate_intrinsics_linear_iterative_batch).  Like calibba_adapter.hpp it is compiled
// in the reference's tree (it needs Eigen and the reference's headers) and only flattens containers and maps status codes back
// to the reference's results.  It is a separate header: neither calibba_adapter.hpp nor calibba_linear.hpp pulls in the
// distortion model headers.
//
//   replaces                                         (reference file:line)
//   calib::fit_distortion_full                       include/calib/models/distortion.h:229-363
//   calib::fit_distortion                            include/calib/models/distortion.h:365-371
//   calib::fit_distortion_dual                       include/calib/models/distortion.h:373-406
//   calib::estimate_intrinsics_linear                include/calib/estimation/linear/intrinsics.h:60-63 (intrinsicsdlt.cpp:289-312)
//   calib::estimate_intrinsics_linear_iterative      include/calib/estimation/linear/intrinsics.h:66-70 (intrinsicsdlt.cpp:319-368)
//
// The functions live in namespace calibba_adapter.  The fits run in double precision whatever T is.  Departures (normal
// equations from moments, num_radial in [0, 3], the iteration cap, the first duplicate fixed index winning) are listed in
// calibba.h; the fallback warning the reference prints is not reproduced.
#pragma once
#include <cstdint>
#include <optional>
#include <span>
#include <stdexcept>
#include <vector>

#include "calib/estimation/linear/intrinsics.h"
#include "calib/models/camera_matrix.h"
#include "calib/models/distortion.h"
#include "calib/models/pinhole.h"
#include "calibba.h"

namespace calibba_adapter {
namespace distortion_detail {

inline void check(cba_status st) {
    if (st == CBA_OK) return;
    if (st == CBA_ERR_INVALID_ARGUMENT) throw std::invalid_argument(cba_last_error());
    throw std::runtime_error(cba_last_error());
}

struct Flat {
    int64_t off[2] = {0, 0};
    std::vector<double> x, y, u, v;
    template <typename T>
    explicit Flat(const std::vector<calib::Observation<T>>& obs) {
        for (const auto& o : obs) {
            x.push_back(static_cast<double>(o.x)); y.push_back(static_cast<double>(o.y));
            u.push_back(static_cast<double>(o.u)); v.push_back(static_cast<double>(o.v));
        }
        off[1] = static_cast<int64_t>(obs.size());
    }
};

template <typename T>
inline void kmtx5(const calib::CameraMatrixT<T>& k, double* out) {
    out[0] = static_cast<double>(k.fx); out[1] = static_cast<double>(k.fy); out[2] = static_cast<double>(k.cx);
    out[3] = static_cast<double>(k.cy); out[4] = static_cast<double>(k.skew);
}

inline calib::CameraMatrix camera(const double* k) { return calib::CameraMatrix{k[0], k[1], k[2], k[3], k[4]}; }

// one fit (dual: also the inverse); false where the reference returns nullopt
template <typename T>
inline bool fit(const std::vector<calib::Observation<T>>& obs, const calib::CameraMatrixT<T>& intr, int num_radial,
                std::span<const int> fixed_indices, std::span<const T> fixed_values, bool dual, std::vector<double>& coeffs,
                std::vector<double>& inverse, std::vector<double>& residuals) {
    if (obs.size() < 8) return false;  // before the fixed indices are checked, as in the reference (distortion.h:235-238)
    const Flat f(obs);
    double K[5];
    kmtx5(intr, K);
    std::vector<int32_t> idx(fixed_indices.begin(), fixed_indices.end());
    std::vector<double> val(idx.size(), 0.0);  // missing values count as 0
    for (size_t i = 0; i < idx.size() && i < fixed_values.size(); ++i) val[i] = static_cast<double>(fixed_values[i]);
    const size_t m = num_radial >= 0 ? static_cast<size_t>(num_radial) + 2 : 0;
    coeffs.assign(m, 0.0);
    inverse.assign(dual ? m : 0, 0.0);
    residuals.assign(2 * obs.size(), 0.0);
    int32_t ok = 0;
    check(cba_fit_distortion_batch(1, f.off, f.x.data(), f.y.data(), f.u.data(), f.v.data(), K, num_radial, static_cast<int32_t>(idx.size()),
                                   idx.empty() ? nullptr : idx.data(), val.empty() ? nullptr : val.data(), dual ? 1 : 0, coeffs.data(),
                                   dual ? inverse.data() : nullptr, &ok, residuals.data()));
    return ok != 0;
}

template <typename T>
inline Eigen::Matrix<T, Eigen::Dynamic, 1> vec(const std::vector<double>& a) {
    Eigen::Matrix<T, Eigen::Dynamic, 1> out(static_cast<Eigen::Index>(a.size()));
    for (size_t i = 0; i < a.size(); ++i) out[static_cast<Eigen::Index>(i)] = static_cast<T>(a[i]);
    return out;
}

}  // namespace distortion_detail

template <typename T>
[[nodiscard]] auto fit_distortion_full(const std::vector<calib::Observation<T>>& observations, const calib::CameraMatrixT<T>& intrinsics,
                                       int num_radial = 2, std::span<const int> fixed_indices = {}, std::span<const T> fixed_values = {})
    -> std::optional<calib::DistortionWithResiduals<T>> {
    std::vector<double> c, inv, r;
    if (!distortion_detail::fit(observations, intrinsics, num_radial, fixed_indices, fixed_values, false, c, inv, r)) return std::nullopt;
    return calib::DistortionWithResiduals<T>{distortion_detail::vec<T>(c), distortion_detail::vec<T>(r)};
}

template <typename T>
auto fit_distortion(const std::vector<calib::Observation<T>>& observations, const calib::CameraMatrixT<T>& intrinsics, int num_radial = 2,
                    std::span<const int> fixed_indices = {}, std::span<const T> fixed_values = {})
    -> std::optional<calib::DistortionWithResiduals<T>> {
    return fit_distortion_full(observations, intrinsics, num_radial, fixed_indices, fixed_values);
}

inline auto fit_distortion_dual(const std::vector<calib::Observation<double>>& observations, const calib::CameraMatrix& intrinsics,
                                int num_radial = 2, std::span<const int> fixed_indices = {}, std::span<const double> fixed_values = {})
    -> std::optional<calib::DualDistortionWithResiduals> {
    std::vector<double> c, inv, r;
    if (!distortion_detail::fit(observations, intrinsics, num_radial, fixed_indices, fixed_values, true, c, inv, r)) return std::nullopt;
    calib::DualDistortionWithResiduals out;
    out.distortion.forward = distortion_detail::vec<double>(c);
    out.distortion.inverse = distortion_detail::vec<double>(inv);
    out.residuals = distortion_detail::vec<double>(r);
    return out;
}

inline auto estimate_intrinsics_linear(const std::vector<calib::Observation<double>>& observations,
                                       std::optional<calib::CalibrationBounds> bounds = std::nullopt, bool use_skew = false)
    -> std::optional<calib::CameraMatrix> {
    const distortion_detail::Flat f(observations);
    double lo[5], hi[5], K[5];
    if (bounds) {
        const calib::CalibrationBounds& b = *bounds;
        const double l[5] = {b.fx_min, b.fy_min, b.cx_min, b.cy_min, b.skew_min}, h[5] = {b.fx_max, b.fy_max, b.cx_max, b.cy_max, b.skew_max};
        for (int i = 0; i < 5; ++i) { lo[i] = l[i]; hi[i] = h[i]; }
    }
    int32_t status = 0, fallback = 0;
    distortion_detail::check(cba_estimate_intrinsics_linear_batch(1, f.off, f.x.data(), f.y.data(), f.u.data(), f.v.data(), bounds ? lo : nullptr,
                                                                  bounds ? hi : nullptr, use_skew ? 1 : 0, K, &status, &fallback));
    if (status != CBA_LINEAR_OK) return std::nullopt;
    return distortion_detail::camera(K);
}

inline auto estimate_intrinsics_linear_iterative(const std::vector<calib::Observation<double>>& observations, int num_radial,
                                                 int max_iterations = 5, bool use_skew = false)
    -> std::optional<calib::PinholeCamera<calib::BrownConradyd>> {
    const distortion_detail::Flat f(observations);
    double K[5];
    std::vector<double> c(num_radial >= 0 ? static_cast<size_t>(num_radial) + 2 : 0, 0.0);
    int32_t status = 0, iterations = 0, fallback = 0;
    distortion_detail::check(cba_estimate_intrinsics_linear_iterative_batch(1, f.off, f.x.data(), f.y.data(), f.u.data(), f.v.data(), num_radial,
                                                                            max_iterations, use_skew ? 1 : 0, K, c.data(), &status, &iterations,
                                                                            &fallback));
    if (status != CBA_LINEAR_OK) return std::nullopt;
    calib::PinholeCamera<calib::BrownConradyd> cam;
    cam.kmtx = distortion_detail::camera(K);
    cam.distortion.coeffs = distortion_detail::vec<double>(c);
    return cam;
}

}  // namespace calibba_adapter
