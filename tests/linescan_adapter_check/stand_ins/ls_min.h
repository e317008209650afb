// TEST-ONLY STAND-IN.  Not Eigen and not the reference: the smallest set of declarations with the names, members and defaults of
// the Eigen / calib:: types include/calibba_linescan.hpp touches (the reference's include/calib/estimation/linear/{linescan,
// planefit,planarpose}.h, estimation/common/ransac.h, models/{camera_matrix,pinhole,distortion,scheimpflug}.h and
// pipeline/facades/linescan.h), so that the header can be type-checked and driven in an image without Eigen.  It pins nothing;
// in the reference's tree the header is compiled against the real headers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
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
}  // namespace Eigen

namespace calib {
template <typename Scalar>
struct CameraMatrixT final {
    Scalar fx = Scalar(0), fy = Scalar(0), cx = Scalar(0), cy = Scalar(0), skew = Scalar(0);
};
using CameraMatrix = CameraMatrixT<double>;

template <typename Cam>
concept camera_model = requires { typename Cam::Scalar; };

template <typename T>
struct BrownConrady final {
    using Scalar = T;
    Eigen::Matrix<T, Eigen::Dynamic, 1> coeffs;
};
using BrownConradyd = BrownConrady<double>;

template <typename T>
struct DualBrownConrady final {
    using Scalar = T;
    Eigen::Matrix<T, Eigen::Dynamic, 1> forward;
    Eigen::Matrix<T, Eigen::Dynamic, 1> inverse;
};
using DualDistortion = DualBrownConrady<double>;

template <typename DistortionT>
class PinholeCamera final {
  public:
    using Scalar = typename DistortionT::Scalar;
    CameraMatrixT<Scalar> kmtx;
    DistortionT distortion;
    PinholeCamera() = default;
    PinholeCamera(const CameraMatrixT<Scalar>& matrix, const DistortionT& d) : kmtx(matrix), distortion(d) {}
};

template <camera_model CameraT>
struct ScheimpflugCamera final {
    using Scalar = typename CameraT::Scalar;
    CameraT camera;
    Scalar tau_x{0}, tau_y{0};
    ScheimpflugCamera() = default;
    ScheimpflugCamera(const CameraT& cam, Scalar tx, Scalar ty) : camera(cam), tau_x(tx), tau_y(ty) {}
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

struct PlaneRansacResult final {
    bool success{false};
    Eigen::Vector4d plane{Eigen::Vector4d::Zero()};
    std::vector<int> inliers;
    double inlier_rms{std::numeric_limits<double>::infinity()};
};

struct LineScanView final {
    PlanarView target_view;
    std::vector<Eigen::Vector2d> laser_uv;
};

struct LineScanCalibrationResult final {
    Eigen::Vector4d plane;
    Eigen::Matrix4d covariance;
    Eigen::Matrix3d homography;
    double rms_error = 0.0;
    std::string summary;
    std::size_t inlier_count = 0;
};

struct LineScanPlaneFitOptions final {
    bool use_ransac = false;
    RansacOptions ransac_options{};
};

namespace pipeline {
struct LinescanCalibrationRunResult final {
    bool success = false;
    std::size_t used_views = 0;
    LineScanCalibrationResult result;
};
struct LinescanCalibrationOptions final {
    LineScanPlaneFitOptions plane_fit;
};
}  // namespace pipeline
}  // namespace calib
