// TEST-ONLY STAND-IN.  Not Eigen and not the reference: the smallest set of declarations with the names, members and defaults of
// the Eigen / calib:: types include/calibba_distortion.hpp touches (the reference's include/calib/models/{distortion,camera_matrix,
// pinhole}.h and estimation/linear/intrinsics.h), so that the header can be type-checked and driven in an image without Eigen.
// It pins nothing; in the reference's tree the header is compiled against the real headers.
#pragma once
#include <cstddef>
#include <optional>
#include <vector>

namespace Eigen {
using Index = std::ptrdiff_t;
constexpr int Dynamic = -1;
template <class T, int R, int C>
class Matrix {  // Dynamic column vectors only
  public:
    using Scalar = T;
    Matrix() = default;
    explicit Matrix(Index n) : a_(static_cast<size_t>(n), T(0)) {}
    Index size() const { return static_cast<Index>(a_.size()); }
    T* data() { return a_.data(); }
    const T* data() const { return a_.data(); }
    T& operator[](Index i) { return a_[static_cast<size_t>(i)]; }
    const T& operator[](Index i) const { return a_[static_cast<size_t>(i)]; }

  private:
    std::vector<T> a_;
};
using VectorXd = Matrix<double, Dynamic, 1>;
}  // namespace Eigen

namespace calib {
template <typename Scalar>
struct CameraMatrixT final {
    Scalar fx = Scalar(0), fy = Scalar(0), cx = Scalar(0), cy = Scalar(0), skew = Scalar(0);
};
using CameraMatrix = CameraMatrixT<double>;

struct CalibrationBounds final {
    double fx_min = 0.0, fx_max = 2000.0, fy_min = 0.0, fy_max = 2000.0, cx_min = 0.0, cx_max = 1280.0, cy_min = 0.0, cy_max = 720.0;
    double skew_min = -0.01, skew_max = 0.01;
};

template <typename T>
struct Observation final {
    T x, y;
    T u, v;
};

template <typename T>
struct DistortionWithResiduals final {
    Eigen::Matrix<T, Eigen::Dynamic, 1> distortion;
    Eigen::Matrix<T, Eigen::Dynamic, 1> residuals;
};

template <typename Scalar_>
struct BrownConrady final {
    using Scalar = Scalar_;
    Eigen::Matrix<Scalar, Eigen::Dynamic, 1> coeffs;
};
using BrownConradyd = BrownConrady<double>;

template <typename Scalar_>
struct DualBrownConrady final {
    using Scalar = Scalar_;
    Eigen::Matrix<Scalar, Eigen::Dynamic, 1> forward;
    Eigen::Matrix<Scalar, Eigen::Dynamic, 1> inverse;
};
using DualDistortion = DualBrownConrady<double>;

struct DualDistortionWithResiduals final {
    DualDistortion distortion;
    Eigen::VectorXd residuals;
};

template <typename DistortionT>
class PinholeCamera final {
  public:
    using Scalar = typename DistortionT::Scalar;
    CameraMatrixT<Scalar> kmtx;
    DistortionT distortion;
};
}  // namespace calib
