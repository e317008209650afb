// TEST-ONLY STAND-IN.  Not Eigen and not the reference: the smallest set of declarations with the names, members and defaults of
// the Eigen / calib:: types include/calibba_linear.hpp touches (the reference's include/calib/estimation/linear/{homography,
// intrinsics,posefromhomography,zhang,planarpose}.h, estimation/common/ransac.h and models/camera_matrix.h), so that the header
// can be type-checked and driven in an image without Eigen.  It pins nothing; in the reference's tree the header is compiled
// against the real headers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

namespace Eigen {
using Index = std::ptrdiff_t;
constexpr int Dynamic = -1;
template <class T, int R, int C>
class Matrix {  // column-major; fixed sizes zero-initialised (the real ones are not), Dynamic vectors only
  public:
    using Scalar = T;
    Matrix() : a_(R == Dynamic ? 0 : static_cast<size_t>(R * C), T(0)) {}
    explicit Matrix(Index n) : a_(static_cast<size_t>(n), T(0)) {}
    template <int RR = R, class = std::enable_if_t<RR == 2>>
    Matrix(T x, T y) : a_{x, y} {}
    template <int RR = R, class = std::enable_if_t<RR == 3>>
    Matrix(T x, T y, T z) : a_{x, y, z} {}
    static Matrix Zero() { return Matrix(); }
    static Matrix Zero(Index n) { return Matrix(n); }
    Index rows() const { return R == Dynamic ? static_cast<Index>(a_.size()) : R; }
    Index cols() const { return R == Dynamic ? 1 : C; }
    Index size() const { return static_cast<Index>(a_.size()); }
    T* data() { return a_.data(); }
    const T* data() const { return a_.data(); }
    T& operator()(Index r, Index c) { return a_[static_cast<size_t>(r + c * rows())]; }
    const T& operator()(Index r, Index c) const { return a_[static_cast<size_t>(r + c * rows())]; }
    T& operator[](Index i) { return a_[static_cast<size_t>(i)]; }
    const T& operator[](Index i) const { return a_[static_cast<size_t>(i)]; }
    T& x() { return a_[0]; }
    const T& x() const { return a_[0]; }
    T& y() { return a_[1]; }
    const T& y() const { return a_[1]; }
    T& z() { return a_[2]; }
    const T& z() const { return a_[2]; }
    void setZero() { for (T& v : a_) v = T(0); }

  private:
    std::vector<T> a_;
};
using VectorXd = Matrix<double, Dynamic, 1>;
using Vector2d = Matrix<double, 2, 1>;
using Vector3d = Matrix<double, 3, 1>;
using Vector4d = Matrix<double, 4, 1>;
using Matrix3d = Matrix<double, 3, 3>;
using Matrix4d = Matrix<double, 4, 4>;
class Isometry3d {  // linear() and translation() only
  public:
    static Isometry3d Identity() {
        Isometry3d T;
        for (int i = 0; i < 3; ++i) T.R_(i, i) = 1.0;
        return T;
    }
    Matrix3d& linear() { return R_; }
    const Matrix3d& linear() const { return R_; }
    Vector3d& translation() { return t_; }
    const Vector3d& translation() const { return t_; }

  private:
    Matrix3d R_;
    Vector3d t_;
};
}  // namespace Eigen

namespace calib {
struct CameraMatrix final {
    double fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0, skew = 0.0;
};

struct CalibrationBounds final {
    double fx_min = 0.0, fx_max = 2000.0, fy_min = 0.0, fy_max = 2000.0, cx_min = 0.0, cx_max = 1280.0, cy_min = 0.0, cy_max = 720.0;
    double skew_min = -0.01, skew_max = 0.01;
};

struct PlanarObservation {
    Eigen::Vector2d object_xy;
    Eigen::Vector2d image_uv;
};
using PlanarView = std::vector<PlanarObservation>;

struct RansacOptions final {
    int max_iters = 1000;
    double thresh = 2.0;
    int min_inliers = 12;
    double confidence = 0.99;
    uint64_t seed = 1234567;
    bool refit_on_inliers = true;
};

struct HomographyResult final {
    bool success{false};
    Eigen::Matrix3d hmtx = Eigen::Matrix3d::Zero();  // the reference's default is the identity
    std::vector<int> inliers;
    double symmetric_rms_px{0.0};
};

struct IntrinsicsEstimOptions final {
    std::optional<CalibrationBounds> bounds = std::nullopt;
    std::optional<RansacOptions> homography_ransac = std::nullopt;
    bool use_skew = false;
};

struct ViewEstimateData final {
    size_t view_index = 0;
    Eigen::Isometry3d c_se3_t = Eigen::Isometry3d::Identity();
    HomographyResult homography;
    double forward_rms_px = 0.0;
};

struct IntrinsicsEstimateResult final {
    bool success{false};
    CameraMatrix kmtx;
    std::vector<double> dist = {0, 0, 0, 0};
    std::vector<ViewEstimateData> views;
    std::string log;
};

struct PoseFromHResult final {
    bool success{false};
    Eigen::Isometry3d c_se3_t = Eigen::Isometry3d::Identity();
    double scale{1.0};
    double cond_check{1.0};
    std::string message;
};
}  // namespace calib
