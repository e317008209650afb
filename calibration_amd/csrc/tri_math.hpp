// tri_math.hpp — multi-camera triangulation of one point (calibba.h: cba_triangulate) as __host__ __device__ code: the ray seed,
// the Levenberg-Marquardt refinement through the full forward model, the outlier-camera restarts, the final statistics and the
// covariance.  k_triangulate (triangulate.hip) calls tri_point per lane; tests/triangulate_cpu compiles the same header with g++.
// The reference has no triangulation: the procedure is this project's own and is stated in full in calibba.h.
//
//   projection     cam_project / cam_denominator (camera_math.hpp) as they are for the final statistics, so rms_px agrees with a
//                  cba_camera_project round trip; tri_project_jac restates reproj_core's u, v, du/dP and dv/dP (reproj_math.hpp: the
//                  LM's hot path keeps its own copy) for the linearisations.
//   unprojection   ls_unproject (linescan_math.hpp), called where it is.
//   3x3 solves     chol_n<3> / chol_solve_n<3> (small_lm.hpp), unpivoted; symmetric results in sym3's order 00 01 02 11 12 22.
//
// The camera set of a point is a bit mask, the cameras are walked in index order and every loop over them indexes the table with the
// loop counter alone: on the device the table reads are wave-uniform (scalar loads) and no private array is indexed dynamically.
#pragma once
#include <cmath>
#include <cstdint>

#include "camera_math.hpp"
#include "small_lm.hpp"

namespace cba {

constexpr int TRI_MAX_CAMS = CBA_TRI_MAX_CAMS;
constexpr double TRI_LAMBDA0 = 1e-4;      // first damping factor of every (re)start
constexpr double TRI_LAMBDA_MIN = 1e-10;  // floor of lambda / 10 after an accepted step
constexpr double TRI_PIVOT_MIN = 1e-12;   // seed: a Cholesky pivot of sum (I - d d^T) at or below this times n_used is degenerate
// The cost's rounding floor: 2 sqrt(2) eps_px with eps_px = 1e-12 px (a pixel coordinate of a few thousand px carries ~2^-52 * 4096 of
// rounding, and a few operations of it), times sqrt(n_used * cost).  A trial is accepted when its cost is not higher than the current
// one by more than this, and an accepted step that lowers the cost by no more than this ends the iteration: below the floor the sign
// of a cost difference is noise, and with two cameras the step itself stays above 1e-12 |X| (measured: ~3e-12 at 0.3 px noise).
constexpr double TRI_COST_SLACK_PX = 4e-12;

// One camera of the table: LsCamera (model, intrinsics, inverse coefficients, Scheimpflug constants), the rotation of c_T_r
// (row-major), its translation, and the camera centre o = -R^T t in the reference frame.
struct TriCamera {
    LsCamera cam;
    double R[9];
    double t[3];
    double o[3];
};
static_assert(sizeof(TriCamera) == 640, "TriCamera is read by k_triangulate: its layout is fixed");

struct TriResult {
    double X[3];
    double rms;
    double cov[6];
    uint32_t mask;
    int32_t status;
    int32_t linearisations;  // every pass of tri_linearize, restarts included (tools/bench_triangulate.py)
};

CBA_HD void tri_fill_camera(int model, const double* intr, int n_inv, const double* inv, const double* pose7, TriCamera* k) {
    ls_fill_camera(model, intr, n_inv, inv, &k->cam);
    quat_to_rotmat(pose7, k->R);
    for (int j = 0; j < 3; ++j) k->t[j] = pose7[4 + j];
    double c[3];
    mat3_tvec(k->R, k->t, c);
    for (int j = 0; j < 3; ++j) k->o[j] = -c[j];
}

// the pixel of one camera: one 16-byte load per lane on the device (camera-major pixels: consecutive lanes, consecutive pixels)
CBA_HD void tri_load_px(const double* p, double* u, double* v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double2 q = *reinterpret_cast<const double2*>(p);
    *u = q.x;
    *v = q.y;
#else
    *u = p[0];
    *v = p[1];
#endif
}

CBA_HD bool tri_finite(double a) { return fabs(a) <= 1.7976931348623157e308; }  // false for NaN and +-inf

// P = R X + t, not contracted: the caller of cba_camera_project who forms the same sum gets the same camera-frame point
CBA_HD void tri_to_camera(const TriCamera& k, const double* X, double* P) {
    CBA_NO_CONTRACT
    P[0] = k.R[0] * X[0] + k.R[1] * X[1] + k.R[2] * X[2] + k.t[0];
    P[1] = k.R[3] * X[0] + k.R[4] * X[1] + k.R[5] * X[2] + k.t[1];
    P[2] = k.R[6] * X[0] + k.R[7] * X[1] + k.R[8] * X[2] + k.t[2];
}

// u, v, the denominator and du = d u / d P, dv = d v / d P of a camera-frame point, in reproj_core's expression order
template <int MODEL>
CBA_HD void tri_project_jac(const double* intr, const double* sd, const double* P, double* u, double* v, double* den, double* du,
                            double* dv) {
    const double fx = intr[0], fy = intr[1], skew = intr[4];
    const double k1 = intr[5], k2 = intr[6], k3 = intr[7], p1 = intr[8], p2 = intr[9];
    double x, y, gx[3], gy[3], m0x = 0.0, m0y = 0.0;
    if (MODEL == CAM_PINHOLE_BC) {
        *den = P[2];
        const double iz = 1.0 / P[2];
        x = P[0] * iz; y = P[1] * iz;
        gx[0] = iz; gx[1] = 0.0; gx[2] = -x * iz;
        gy[0] = 0.0; gy[1] = iz; gy[2] = -y * iz;
    } else {
        const double* Rs = sd + SD_RS;
        *den = Rs[2] * P[0] + Rs[5] * P[1] + Rs[8] * P[2];
        const double is = 1.0 / *den;
        const double mx = (Rs[0] * P[0] + Rs[3] * P[1] + Rs[6] * P[2]) * is;
        const double my = (Rs[1] * P[0] + Rs[4] * P[1] + Rs[7] * P[2]) * is;
        m0x = sd[SD_M0]; m0y = sd[SD_M0 + 1];
        x = mx - m0x; y = my - m0y;
        for (int i = 0; i < 3; ++i) {
            gx[i] = (Rs[3 * i] - mx * Rs[3 * i + 2]) * is;
            gy[i] = (Rs[3 * i + 1] - my * Rs[3 * i + 2]) * is;
        }
    }
    const double r2 = x * x + y * y, xx = x * x, yy = y * y, xy = x * y;
    const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    const double drad = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2);
    const double xd = x * rad + 2.0 * p1 * xy + p2 * (r2 + 2.0 * xx);
    const double yd = y * rad + p1 * (r2 + 2.0 * yy) + 2.0 * p2 * xy;
    *u = fx * xd + skew * yd + intr[2] + (fx * m0x + skew * m0y);
    *v = fy * yd + intr[3] + fy * m0y;
    // d(xd, yd)/d(x, y), d(u, v)/d(x, y), d(u, v)/dP
    const double dxdx = rad + 2.0 * xx * drad + 2.0 * p1 * y + 6.0 * p2 * x;
    const double dxdy = 2.0 * xy * drad + 2.0 * p1 * x + 2.0 * p2 * y;
    const double dydy = rad + 2.0 * yy * drad + 6.0 * p1 * y + 2.0 * p2 * x;
    const double ux = fx * dxdx + skew * dxdy, uy = fx * dxdy + skew * dydy;
    const double vx = fy * dxdy, vy = fy * dydy;
    for (int i = 0; i < 3; ++i) {
        du[i] = ux * gx[i] + uy * gy[i];
        dv[i] = vx * gx[i] + vy * gy[i];
    }
}

// The ray seed over the cameras of mask: A = sum (I - d d^T), b = sum (I - d d^T) o, A X = b.  false: degenerate (parallel rays).
CBA_HD bool tri_seed(const TriCamera* cams, int n_cams, uint32_t mask, int n_used, const double* uv, int64_t stride, double* X) {
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < n_cams; ++c) {
        if (!((mask >> c) & 1u)) continue;
        const TriCamera& k = cams[c];
        double u, v, x, y;
        tri_load_px(uv + c * stride, &u, &v);
        ls_unproject(k.cam, u, v, &x, &y);
        double d0 = k.R[0] * x + k.R[3] * y + k.R[6], d1 = k.R[1] * x + k.R[4] * y + k.R[7], d2 = k.R[2] * x + k.R[5] * y + k.R[8];
        const double in = 1.0 / sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        d0 *= in; d1 *= in; d2 *= in;
        const double od = d0 * k.o[0] + d1 * k.o[1] + d2 * k.o[2];
        A[0] += 1.0 - d0 * d0; A[1] -= d0 * d1; A[2] -= d0 * d2;
        A[3] += 1.0 - d1 * d1; A[4] -= d1 * d2; A[5] += 1.0 - d2 * d2;
        b[0] += k.o[0] - d0 * od; b[1] += k.o[1] - d1 * od; b[2] += k.o[2] - d2 * od;
    }
    double L[9] = {A[0], A[1], A[2], A[1], A[3], A[4], A[2], A[4], A[5]};
    if (!chol_n<3>(L)) return false;
    const double lim = TRI_PIVOT_MIN * n_used;
    if (!(L[0] * L[0] > lim && L[4] * L[4] > lim && L[8] * L[8] > lim)) return false;
    for (int j = 0; j < 3; ++j) X[j] = b[j];
    chol_solve_n<3>(L, X);
    return true;
}

// One linearisation at X over the cameras of mask: cost = sum |r|^2, H = J^T J (sym3 order), g = J^T r; rows of J are (du/dP) R and
// (dv/dP) R.  Returns whether every used camera has a positive denominator.
template <int MODEL>
CBA_HD bool tri_linearize(const TriCamera* cams, int n_cams, uint32_t mask, const double* uv, int64_t stride, const double* X,
                          double* cost, double* H, double* g) {
    double s = 0.0;
    for (int j = 0; j < 6; ++j) H[j] = 0.0;
    for (int j = 0; j < 3; ++j) g[j] = 0.0;
    bool front = true;
    for (int c = 0; c < n_cams; ++c) {
        if (!((mask >> c) & 1u)) continue;
        const TriCamera& k = cams[c];
        double uo, vo, P[3], u, v, den, du[3], dv[3];
        tri_load_px(uv + c * stride, &uo, &vo);
        tri_to_camera(k, X, P);
        tri_project_jac<MODEL>(k.cam.intr, k.cam.sd, P, &u, &v, &den, du, dv);
        const double ru = u - uo, rv = v - vo;
        double Ju[3], Jv[3];
        for (int j = 0; j < 3; ++j) {
            Ju[j] = du[0] * k.R[j] + du[1] * k.R[3 + j] + du[2] * k.R[6 + j];
            Jv[j] = dv[0] * k.R[j] + dv[1] * k.R[3 + j] + dv[2] * k.R[6 + j];
        }
        s += ru * ru + rv * rv;
        H[0] += Ju[0] * Ju[0] + Jv[0] * Jv[0]; H[1] += Ju[0] * Ju[1] + Jv[0] * Jv[1]; H[2] += Ju[0] * Ju[2] + Jv[0] * Jv[2];
        H[3] += Ju[1] * Ju[1] + Jv[1] * Jv[1]; H[4] += Ju[1] * Ju[2] + Jv[1] * Jv[2]; H[5] += Ju[2] * Ju[2] + Jv[2] * Jv[2];
        for (int j = 0; j < 3; ++j) g[j] += Ju[j] * ru + Jv[j] * rv;
        front = front && den > 0.0;
    }
    *cost = s;
    return front;
}

// Levenberg-Marquardt from the seed X.  H: the linearisation at the returned X (the last accepted one, or the seed's).  Returns
// CBA_TRI_OK (step tolerance met, or the cost's rounding floor reached) or CBA_TRI_NOT_CONVERGED (max_iterations steps tried); *lin counts the linearisations.
template <int MODEL>
CBA_HD int tri_refine(const TriCamera* cams, int n_cams, uint32_t mask, int n_used, const double* uv, int64_t stride,
                      int max_iterations, double step_tolerance, double* X, double* H, int* lin) {
    double g[3], cost;
    tri_linearize<MODEL>(cams, n_cams, mask, uv, stride, X, &cost, H, g);
    ++*lin;
    double lambda = TRI_LAMBDA0;
    for (int it = 0; it < max_iterations; ++it) {
        double L[9] = {H[0] + lambda * H[0], H[1], H[2], H[1], H[3] + lambda * H[3], H[4], H[2], H[4], H[5] + lambda * H[5]};
        if (!chol_n<3>(L)) {  // counts as a rejected step
            lambda *= 10.0;
            continue;
        }
        double d[3] = {-g[0], -g[1], -g[2]};
        chol_solve_n<3>(L, d);
        const double Xt[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
        const bool small = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) <= step_tolerance * sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
        double Ht[6], gt[3], ct;
        const bool front = tri_linearize<MODEL>(cams, n_cams, mask, uv, stride, Xt, &ct, Ht, gt);
        ++*lin;
        // the cost is known to the rounding of the projected pixels only: |sum 2 r e| <= 2 |r| |e|, |e| <= eps_px sqrt(2 n_used)
        const double slack = TRI_COST_SLACK_PX * sqrt(n_used * cost);
        const double decrease = cost - ct;
        bool floor_reached = false;
        if (front && decrease >= -slack) {
            for (int j = 0; j < 3; ++j) { X[j] = Xt[j]; g[j] = gt[j]; }
            for (int j = 0; j < 6; ++j) H[j] = Ht[j];
            cost = ct;
            lambda = fmax(lambda / 10.0, TRI_LAMBDA_MIN);
            floor_reached = decrease <= slack;
        } else {
            lambda *= 10.0;
        }
        if (small || floor_reached) return CBA_TRI_OK;
    }
    return CBA_TRI_NOT_CONVERGED;
}

// The final statistics at X with cam_project itself: sum of e_u^2 + e_v^2 in camera order, the worst camera (the lowest index among
// equals) and its squared error, and whether every used camera has a positive denominator.
template <int MODEL>
CBA_HD bool tri_errors(const TriCamera* cams, int n_cams, uint32_t mask, const double* uv, int64_t stride, const double* X, double* sum,
                       double* worst, int* worst_cam) {
    CBA_NO_CONTRACT
    double s = 0.0, w = -1.0;
    int wc = -1;
    bool front = true;
    for (int c = 0; c < n_cams; ++c) {
        if (!((mask >> c) & 1u)) continue;
        const TriCamera& k = cams[c];
        double uo, vo, P[3], u, v;
        tri_load_px(uv + c * stride, &uo, &vo);
        tri_to_camera(k, X, P);
        cam_project<MODEL>(k.cam.intr, k.cam.sd, P[0], P[1], P[2], &u, &v);
        const double eu = u - uo, ev = v - vo;
        const double e2 = eu * eu + ev * ev;
        s += e2;
        if (e2 > w) { w = e2; wc = c; }
        front = front && cam_denominator<MODEL>(k.cam.sd, P[0], P[1], P[2]) > 0.0;
    }
    *sum = s;
    *worst = w;
    *worst_cam = wc;
    return front;
}

// (H)^-1 in sym3 order by Cholesky; NaN where H is not positive definite
CBA_HD void tri_covariance(const double* H, double* cov) {
    double L[9] = {H[0], H[1], H[2], H[1], H[3], H[4], H[2], H[4], H[5]};
    if (!chol_n<3>(L)) {
        for (int j = 0; j < 6; ++j) cov[j] = NAN;
        return;
    }
    double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
    chol_solve_n<3>(L, e0);
    chol_solve_n<3>(L, e1);
    chol_solve_n<3>(L, e2);
    cov[0] = e0[0]; cov[1] = e0[1]; cov[2] = e0[2];
    cov[3] = e1[1]; cov[4] = e1[2]; cov[5] = e2[2];
}

// The whole procedure of one point.  uv: the point's pixel in camera 0; camera c's is at uv + c * stride (stride = 2 n doubles).
template <int MODEL, bool COV>
CBA_HD void tri_point(const TriCamera* cams, int n_cams, const double* uv, int64_t stride, const cba_triangulate_options& o, TriResult* r) {
    uint32_t mask = 0;
    for (int c = 0; c < n_cams; ++c) {
        double u, v;
        tri_load_px(uv + c * stride, &u, &v);
        const bool seen = tri_finite(u) & tri_finite(v);  // no short circuit: the pixel stays one 16-byte load
        if (seen) mask |= 1u << c;
    }
    const int min_cams = o.min_cams < 2 ? 2 : o.min_cams;
    const double lim2 = o.max_reproj_px * o.max_reproj_px;
    for (int j = 0; j < 3; ++j) r->X[j] = NAN;
    for (int j = 0; j < 6; ++j) r->cov[j] = NAN;
    r->rms = NAN;
    r->linearisations = 0;
    for (;;) {
        const int n_used = __builtin_popcount(mask);
        if (n_used < min_cams) {  // only before the first seed: a restart keeps more than max(min_cams, 2) - 1 cameras
            r->mask = 0;
            r->status = CBA_TRI_TOO_FEW;
            return;
        }
        r->mask = mask;
        double X[3], H[6];
        if (!tri_seed(cams, n_cams, mask, n_used, uv, stride, X)) {
            r->status = CBA_TRI_DEGENERATE;
            return;
        }
        int status = tri_refine<MODEL>(cams, n_cams, mask, n_used, uv, stride, o.max_iterations, o.step_tolerance, X, H, &r->linearisations);
        double sum, worst;
        int worst_cam;
        const bool front = tri_errors<MODEL>(cams, n_cams, mask, uv, stride, X, &sum, &worst, &worst_cam);
        if (worst > lim2 && n_used > min_cams) {  // drop the worst camera and start again from the seed
            mask &= ~(1u << worst_cam);
            continue;
        }
        if (!front) status = CBA_TRI_BEHIND;
        for (int j = 0; j < 3; ++j) r->X[j] = X[j];
        r->rms = sqrt(sum / n_used);
        r->status = status;
        if (COV) tri_covariance(H, r->cov);
        return;
    }
}

}  // namespace cba
