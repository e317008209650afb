// TEST-ONLY STAND-IN.  Not Eigen and not the reference: the smallest set of declarations with the names and members of the Eigen /
// calib:: types include/calibba_extrinsics.hpp and its driver touch (the reference's include/calib/estimation/linear/extrinsics.h
// and planarpose.h, models/camera_matrix.h, pinhole.h, scheimpflug.h), so that the header can be type-checked and driven in an
// image without Eigen.  It pins nothing; in the reference's tree the header is compiled against the real headers.
#pragma once
#include <cstddef>
#include <cstdint>
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

struct PlanarObservation {
    Eigen::Vector2d object_xy;
    Eigen::Vector2d image_uv;
};
using PlanarView = std::vector<PlanarObservation>;
using MulticamPlanarView = std::vector<PlanarView>;

struct ExtrinsicPoses final {
    std::vector<Eigen::Isometry3d> c_se3_r;
    std::vector<Eigen::Isometry3d> r_se3_t;
};

struct DualDistortion {
    Eigen::VectorXd forward, inverse;
};

template <class DistortionT>
class PinholeCamera final {
  public:
    PinholeCamera() = default;
    PinholeCamera(const CameraMatrix& k, const DistortionT& d) : kmtx(k), distortion(d) {}
    CameraMatrix kmtx;
    DistortionT distortion;
};

template <class CameraT>
class ScheimpflugCamera final {
  public:
    ScheimpflugCamera(CameraT cam, double tx, double ty) : camera(cam), tau_x(tx), tau_y(ty) {}
    CameraT camera;
    double tau_x = 0.0, tau_y = 0.0;
};
}  // namespace calib
