// linescan_math.hpp — calibrate_laser_plane (include/calib/estimation/linear/linescan.h:39-144, planefit.cpp) as
// __host__ __device__ code: camera unprojection, the per-view homography + pose (points_from_view, :63-91), the
// back-projection of one laser pixel, the plane from centred moments and the sign convention of every returned plane.
// The GPU kernels (linescan.hip) call it per wavefront / per lane; tests/linescan_cpu compiles the same header with g++.
//
// Unprojection:
//   pinhole + Brown-Conrady   normalize (camera_matrix.h:33-39), then either the 5-step fixed point of undistort
//                             (distortion.h:119-134) or, with inverse coefficients (DualDistortion), ONE evaluation of
//                             apply_distortion with them (distortion.h:213-217).
//   Scheimpflug               the exact inverse of the projection reproj_math.hpp implements (scheimpflug.h:139-181):
//                             normalize, subtract the sensor offset m0, undistort, add m0, map the sensor ray
//                             mx a + my b + n (the tilted basis = columns of Rs) back to (x/z, y/z).  The reference's own
//                             ScheimpflugCamera::unproject cannot be instantiated (see calibba.h).
// Plane sign: the reference's is whatever its SVD returns.  Every plane returned here has d > 0, or, when
// |d| <= 1e-12 max|p|, its largest-magnitude normal component positive.
#pragma once
#include <cstdint>
#include "seed_math.hpp"

namespace cba {

// Brown-Conrady with any number of radial terms: coeffs = [k1 .. k_nr, p1, p2], n = nr + 2 (distortion.h:91-116)
CBA_HD void ls_apply_distortion(double x, double y, const double* coeffs, int n, double* xd, double* yd) {
    const int nr = n - 2;
    const double r2 = x * x + y * y;
    double radial = 1.0, rpow = r2;
    for (int i = 0; i < nr; ++i) {
        radial += coeffs[i] * rpow;
        rpow *= r2;
    }
    const double p1 = coeffs[nr], p2 = coeffs[nr + 1];
    *xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
    *yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
}

// undistort: inverse coefficients (n_inv >= 2) -> one polynomial evaluation; otherwise 5 fixed-point steps on intr[5..9]
CBA_HD void ls_undistort(const double* intr, int n_inv, const double* inv, double xd, double yd, double* x, double* y) {
    if (n_inv >= 2) {
        ls_apply_distortion(xd, yd, inv, n_inv, x, y);
        return;
    }
    double ux = xd, uy = yd;
    for (int it = 0; it < 5; ++it) {
        double dx, dy;
        ls_apply_distortion(ux, uy, intr + 5, 5, &dx, &dy);
        ux += xd - dx;
        uy += yd - dy;
    }
    *x = ux;
    *y = uy;
}

// normalize (camera_matrix.h:33-39): intr = [fx fy cx cy skew ...]
CBA_HD void ls_normalize(const double* intr, double u, double v, double* x, double* y) {
    *y = (v - intr[3]) / intr[1];
    *x = (u - intr[2] - intr[4] * *y) / intr[0];
}

CBA_HD void unproject_pinhole_bc(const double* intr10, int n_inv, const double* inv, double u, double v, double* x, double* y) {
    double xd, yd;
    ls_normalize(intr10, u, v, &xd, &yd);
    ls_undistort(intr10, n_inv, inv, xd, yd, x, y);
}

// sd: scheimpflug_consts(intr12) (reproj_math.hpp)
CBA_HD void unproject_scheimpflug(const double* intr12, const double* sd, int n_inv, const double* inv, double u, double v, double* x,
                                  double* y) {
    double mx, my;
    ls_normalize(intr12, u, v, &mx, &my);  // = distorted delta + m0 (reproj_residual: su, sv)
    double dx, dy;
    ls_undistort(intr12, n_inv, inv, mx - sd[SD_M0], my - sd[SD_M0 + 1], &dx, &dy);
    mx = dx + sd[SD_M0];
    my = dy + sd[SD_M0 + 1];
    const double* Rs = sd + SD_RS;  // P = Rs (mx, my, 1)
    const double P0 = Rs[0] * mx + Rs[1] * my + Rs[2];
    const double P1 = Rs[3] * mx + Rs[4] * my + Rs[5];
    const double P2 = Rs[6] * mx + Rs[7] * my + Rs[8];
    *x = P0 / P2;
    *y = P1 / P2;
}

// One camera as the kernels see it: model, intrinsics, optional inverse coefficients, Scheimpflug constants.
constexpr int LS_MAX_INV = 16;  // most inverse (DualDistortion) coefficients
struct LsCamera {
    int model;      // CAM_PINHOLE_BC | CAM_SCHEIMPFLUG
    int n_inv;      // 0: iterative undistort
    double intr[12];
    double inv[LS_MAX_INV];
    double sd[SD_SIZE];
};
static_assert(sizeof(LsCamera) == 520, "LsCamera is a kernel argument: its layout is fixed");

constexpr int cam_intr_size(int model) { return model == CAM_SCHEIMPFLUG ? 12 : 10; }

// The intrinsics of one camera as the kernels take them: padded with zeros to 12, and the Scheimpflug constants (zero for the pinhole)
CBA_HD void ls_fill_intr(int model, const double* intr, double* out12, double* sd) {
    for (int k = 0; k < 12; ++k) out12[k] = k < cam_intr_size(model) ? intr[k] : 0.0;
    for (int k = 0; k < SD_SIZE; ++k) sd[k] = 0.0;
    if (model == CAM_SCHEIMPFLUG) scheimpflug_consts(out12, sd);
}

// inv: n_inv inverse coefficients or NULL (then n_inv is 0); every entry past the ones given is zero
CBA_HD void ls_fill_camera(int model, const double* intr, int n_inv, const double* inv, LsCamera* c) {
    c->model = model;
    c->n_inv = inv ? n_inv : 0;
    ls_fill_intr(model, intr, c->intr, c->sd);
    for (int k = 0; k < LS_MAX_INV; ++k) c->inv[k] = k < c->n_inv ? inv[k] : 0.0;
}

CBA_HD void ls_unproject(const LsCamera& cam, double u, double v, double* x, double* y) {
    if (cam.model == CAM_SCHEIMPFLUG)
        unproject_scheimpflug(cam.intr, cam.sd, cam.n_inv, cam.inv, u, v, x, y);
    else
        unproject_pinhole_bc(cam.intr, cam.n_inv, cam.inv, u, v, x, y);
}

// Per-view geometry of points_from_view (linescan.h:63-91).  The view's target pixels are unprojected into nu/nv (scratch of
// n entries; each lane writes and later reads only its own strided entries), the DLT homography target -> normalised runs on
// them (dlt_homography_view with K = identity), pose = pose_from_homography_normalized(H), Hinv = H^-1 / Hinv(2,2).
// geo = [Hinv (9, row-major) | R (9, row-major) | t (3)].  Returns false when the homography fails (the view gives no points).
constexpr int LS_GEO = 21;
template <class Coop>
CBA_HD bool ls_view_geometry(const LsCamera& cam, int n, const double* X, const double* Y, const double* u, const double* v,
                             double* nu, double* nv, Coop& co, double* geo) {
    for (int i = co.lane(); i < n; i += co.width()) ls_unproject(cam, u[i], v[i], nu + i, nv + i);
    const double K[5] = {1.0, 1.0, 0.0, 0.0, 0.0};
    double H[9];
    if (!dlt_homography_view(n, X, Y, nu, nv, K, co, H)) return false;
    double R[9], t[3];
    seed_pose_from_h(H, R, t);
    // H^-1 by cofactors (Eigen's 3x3 inverse)
    const double c00 = H[4] * H[8] - H[5] * H[7], c01 = H[5] * H[6] - H[3] * H[8], c02 = H[3] * H[7] - H[4] * H[6];
    const double det = H[0] * c00 + H[1] * c01 + H[2] * c02;
    const double id = 1.0 / det;
    double Hi[9] = {c00 * id, (H[2] * H[7] - H[1] * H[8]) * id, (H[1] * H[5] - H[2] * H[4]) * id,
                    c01 * id, (H[0] * H[8] - H[2] * H[6]) * id, (H[2] * H[3] - H[0] * H[5]) * id,
                    c02 * id, (H[1] * H[6] - H[0] * H[7]) * id, (H[0] * H[4] - H[1] * H[3]) * id};
    if (fabs(Hi[8]) > 1e-15) {  // linescan.h:77-79
        const double s = 1.0 / Hi[8];
        for (int k = 0; k < 9; ++k) Hi[k] *= s;
    }
    for (int k = 0; k < 9; ++k) { geo[k] = Hi[k]; geo[9 + k] = R[k]; }
    for (int k = 0; k < 3; ++k) geo[18 + k] = t[k];
    return true;
}

// One laser pixel -> camera-frame point (linescan.h:83-89)
CBA_HD void ls_backproject(const LsCamera& cam, const double* geo, double u, double v, double* p) {
    double x, y;
    ls_unproject(cam, u, v, &x, &y);
    const double* Hi = geo;
    const double h0 = Hi[0] * x + Hi[1] * y + Hi[2], h1 = Hi[3] * x + Hi[4] * y + Hi[5], h2 = Hi[6] * x + Hi[7] * y + Hi[8];
    const double X = h0 / h2, Y = h1 / h2;
    const double* R = geo + 9;
    const double* t = geo + 18;
    p[0] = R[0] * X + R[1] * Y + t[0];
    p[1] = R[3] * X + R[4] * Y + t[1];
    p[2] = R[6] * X + R[7] * Y + t[2];
}

// The sign convention (see the top of the file).  scale = max |p| over the fitted points.
CBA_HD void ls_plane_sign(double* plane, double scale) {
    bool flip;
    if (fabs(plane[3]) > 1e-12 * scale) {
        flip = plane[3] < 0.0;
    } else {
        int k = 0;
        for (int j = 1; j < 3; ++j) if (fabs(plane[j]) > fabs(plane[k])) k = j;
        flip = plane[k] < 0.0;
    }
    if (flip)
        for (int j = 0; j < 4; ++j) plane[j] = -plane[j];
}

// fit_plane_svd (planefit.cpp:68-85) from the centroid c and the centred scatter S6 = [xx xy xz yy yz zz]: the eigenvector of
// the smallest eigenvalue of S is the smallest right singular vector of the centred N x 3 matrix; d = -n.c; unit normal.
// No sign convention here (ls_plane_sign).
CBA_HD void ls_plane_from_scatter(const double* c, const double* S6, double* plane) {
    const double S[9] = {S6[0], S6[1], S6[2], S6[1], S6[3], S6[4], S6[2], S6[4], S6[5]};
    double d[3], V[9];
    seed_eig3(S, d, V);
    int k = 0;
    for (int j = 1; j < 3; ++j) if (d[j] < d[k]) k = j;
    double n0 = V[0 * 3 + k], n1 = V[1 * 3 + k], n2 = V[2 * 3 + k];
    const double nn = 1.0 / sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    n0 *= nn; n1 *= nn; n2 *= nn;
    plane[0] = n0; plane[1] = n1; plane[2] = n2;
    plane[3] = -(n0 * c[0] + n1 * c[1] + n2 * c[2]);
}

// PlaneRansacEstimator::fit (planefit.cpp:14-32): plane through three points; false when |v1 x v2| < 1e-12 (degenerate)
CBA_HD bool ls_plane_from_3(const double* p0, const double* p1, const double* p2, double* plane) {
    const double v1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, v2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    double n[3];
    cross3(v1, v2, n);
    const double nrm = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (nrm < 1e-12) return false;
    for (int j = 0; j < 3; ++j) plane[j] = n[j] / nrm;
    plane[3] = -(plane[0] * p0[0] + plane[1] * p0[1] + plane[2] * p0[2]);
    return true;
}

// build_plane_homography (linescan.h:49-61), row-major
CBA_HD void ls_plane_homography(const double* plane, double* Hout) {
    const double n[3] = {plane[0], plane[1], plane[2]};
    const double p0[3] = {-plane[3] * n[0], -plane[3] * n[1], -plane[3] * n[2]};
    const double tmp[3] = {fabs(n[2]) < 0.9 ? 0.0 : 1.0, 0.0, fabs(n[2]) < 0.9 ? 1.0 : 0.0};
    double e1[3], e2[3];
    cross3(n, tmp, e1);
    double s = 1.0 / sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    for (int j = 0; j < 3; ++j) e1[j] *= s;
    cross3(n, e1, e2);
    s = 1.0 / sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    for (int j = 0; j < 3; ++j) e2[j] *= s;
    const double M[9] = {e1[0], e2[0], p0[0], e1[1], e2[1], p0[1], e1[2], e2[2], p0[2]};
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const double id = 1.0 / (M[0] * c00 + M[1] * c01 + M[2] * c02);
    const double Hi[9] = {c00 * id, (M[2] * M[7] - M[1] * M[8]) * id, (M[1] * M[5] - M[2] * M[4]) * id,
                          c01 * id, (M[0] * M[8] - M[2] * M[6]) * id, (M[2] * M[3] - M[0] * M[5]) * id,
                          c02 * id, (M[1] * M[6] - M[0] * M[7]) * id, (M[0] * M[4] - M[1] * M[3]) * id};
    for (int k = 0; k < 9; ++k) Hout[k] = Hi[k];
}

// ---- RANSAC hypotheses ---------------------------------------------------------------------------------------------------
// Hypothesis k draws its three DISTINCT point indices from splitmix64 of (seed, 3k + j), j = 0, 1, 2 (counter-based, so every
// hypothesis is independent of every other and of the launch shape).  Range reduction: the high 64 bits of x * m.
CBA_HD uint64_t ls_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
CBA_HD uint64_t ls_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}
// n >= 3 points
CBA_HD void ls_hypothesis(uint64_t seed, int64_t k, int64_t n, int64_t* idx) {
    const uint64_t base = seed ^ 0x5851F42D4C957F2Dull;
    const uint64_t r0 = ls_splitmix64(base + 3 * static_cast<uint64_t>(k));
    const uint64_t r1 = ls_splitmix64(base + 3 * static_cast<uint64_t>(k) + 1);
    const uint64_t r2 = ls_splitmix64(base + 3 * static_cast<uint64_t>(k) + 2);
    const int64_t a = static_cast<int64_t>(ls_mulhi64(r0, static_cast<uint64_t>(n)));
    int64_t b = static_cast<int64_t>(ls_mulhi64(r1, static_cast<uint64_t>(n - 1)));
    if (b >= a) ++b;
    int64_t c = static_cast<int64_t>(ls_mulhi64(r2, static_cast<uint64_t>(n - 2)));
    const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
    if (c >= lo) ++c;
    if (c >= hi) ++c;
    idx[0] = a; idx[1] = b; idx[2] = c;
}

}  // namespace cba
