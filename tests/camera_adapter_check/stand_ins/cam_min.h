// TEST-ONLY STAND-IN.  Not Eigen and not the reference: the smallest set of declarations with the names, members and defaults of
// the Eigen / calib:: types include/calibba_camera.hpp touches (the reference's include/calib/models/{distortion,camera_matrix,
// pinhole,scheimpflug}.h), so that the header can be type-checked and driven in an image without Eigen.  It pins nothing; in the
// reference's tree the header is compiled against the real headers.
#pragma once
#include <cstddef>
#include <vector>

namespace Eigen {
using Index = std::ptrdiff_t;
constexpr int Dynamic = -1;
template <class T, int R, int C>
class Matrix {  // fixed 2- and 3-vectors, and Dynamic column vectors
  public:
    using Scalar = T;
    Matrix() : a_(R > 0 ? static_cast<size_t>(R) : 0, T(0)) {}
    explicit Matrix(Index n) : a_(static_cast<size_t>(n), T(0)) {}
    Matrix(T x, T y) : a_{x, y} {}
    Matrix(T x, T y, T z) : a_{x, y, z} {}
    Index size() const { return static_cast<Index>(a_.size()); }
    T* data() { return a_.data(); }
    const T* data() const { return a_.data(); }
    T& operator[](Index i) { return a_[static_cast<size_t>(i)]; }
    const T& operator[](Index i) const { return a_[static_cast<size_t>(i)]; }
    T x() const { return a_[0]; }
    T y() const { return a_[1]; }
    T z() const { return a_[2]; }

  private:
    std::vector<T> a_;
};
using VectorXd = Matrix<double, Dynamic, 1>;
using Vector2d = Matrix<double, 2, 1>;
using Vector3d = Matrix<double, 3, 1>;
}  // namespace Eigen

namespace calib {
template <typename Scalar>
struct CameraMatrixT final {
    Scalar fx = Scalar(0), fy = Scalar(0), cx = Scalar(0), cy = Scalar(0), skew = Scalar(0);
};
using CameraMatrix = CameraMatrixT<double>;

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

template <typename DistortionT>
class PinholeCamera final {
  public:
    using Scalar = typename DistortionT::Scalar;
    CameraMatrixT<Scalar> kmtx;
    DistortionT distortion;
};

template <typename CameraT>
class ScheimpflugCamera final {
  public:
    using Scalar = typename CameraT::Scalar;
    CameraT camera;
    Scalar tau_x{0};
    Scalar tau_y{0};
};
}  // namespace calib
