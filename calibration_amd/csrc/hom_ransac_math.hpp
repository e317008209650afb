// hom_ransac_math.hpp — the linear seed of planar intrinsic calibration (estimate_intrinsics,
// src/estimation/linear/intrinsicsdlt.cpp:101-145) as __host__ __device__ code: the RANSAC homography of one view
// (HomographyEstimator, src/estimation/linear/homographyestimator.cpp, driven by ransac<>, common/ransac.h:121-194), Zhang's
// closed form (src/estimation/linear/zhang.cpp:9-208), pose_from_homography (posefromhomography.cpp:11-62) and
// sanitize_intrinsics (common/intrinsics_utils.h).  The GPU kernels (hom_ransac.hip) call it per lane; tests/hom_ransac_cpu
// compiles the same header with g++.
//
// Departures of form, each agreeing with the reference to rounding:
//   minimal fit   the exact 8 x 8 solve (h22 = 1, partial pivoting) of the Hartley-normalised 4-point DLT instead of the SVD null
//                 vector; both give the same homography on a non-degenerate sample.
//   inlier test   r <= thresh is evaluated division-free: with q = H (x, y, 1) and s = H^-1 (u, v, 1),
//                 r^2 = (A / q2^2 + B / s2^2) / 2, so r^2 <= t^2  <=>  A s2^2 + B q2^2 <= 2 t^2 q2^2 s2^2 (q2 s2 != 0).
//   refit         the Hartley-normalised DLT over an inlier set from 24 moments: once the centroids and scales are known, the
//                 9 x 9 Gram of the normalised design matrix is built from the 6 monomials of m m^T, m = (x, y, 1), weighted
//                 by 1, u, v and u^2 + v^2; its smallest eigenvector by inverse iteration, as dlt_homography_view does.
//   Zhang         the null vector of the 2m x 6 design matrix as the smallest eigenvector (cyclic Jacobi) of its 6 x 6 Gram.
//   polar factor  project_to_so3's U V^T through the eigen-decomposition of R^T R (seed_math.hpp), with its det < 0 rule.
// The Cholesky failure of the refit's inverse iteration (the reference's SVD cannot fail) keeps the raw model, as a refit that
// returns nullopt does.
#pragma once
#include <cstdint>
#include "seed_math.hpp"

namespace cba {

// ---- sampling ---------------------------------------------------------------------------------------------------------------
// Hypothesis k draws its four DISTINCT indices in [0, n) from splitmix64 of (seed, 4k + j), j = 0..3: draw j is uniform over the
// n - j indices not yet taken (the high 64 bits of r * (n - j), stepped over the earlier draws in increasing order).  The stream
// depends only on (seed, k, n): a view gets the same samples wherever it sits in a batch.  n >= 4.
CBA_HD uint64_t hr_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
CBA_HD uint64_t hr_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}
CBA_HD void hr_sample(uint64_t seed, int64_t k, int64_t n, int* idx) {
    const uint64_t base = (seed ^ 0x5851F42D4C957F2Dull) + 4 * static_cast<uint64_t>(k);
    int sorted[4];
    for (int j = 0; j < 4; ++j) {
        int64_t r = static_cast<int64_t>(hr_mulhi64(hr_splitmix64(base + j), static_cast<uint64_t>(n - j)));
        for (int a = 0; a < j; ++a)  // sorted[0..j) ascending
            if (r >= sorted[a]) ++r;
        idx[j] = static_cast<int>(r);
        int a = j;  // insert
        while (a > 0 && sorted[a - 1] > idx[j]) { sorted[a] = sorted[a - 1]; --a; }
        sorted[a] = idx[j];
    }
}

// ---- HomographyEstimator --------------------------------------------------------------------------------------------------
// has_near_collinear_triplet (homographyestimator.cpp:100-119): twice the area of any triplet of OBJECT points below 1e-6
CBA_HD bool hr_degenerate(const double* X, const double* Y) {
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            for (int k = j + 1; k < 4; ++k) {
                const double a = fabs((X[j] - X[i]) * (Y[k] - Y[i]) - (Y[j] - Y[i]) * (X[k] - X[i]));
                if (a < 1e-6) return true;
            }
    return false;
}

// Eigen's 3 x 3 inverse (cofactors / det), row-major
CBA_HD void hr_inv3(const double* H, double* Hi) {
    const double c00 = H[4] * H[8] - H[5] * H[7], c01 = H[5] * H[6] - H[3] * H[8], c02 = H[3] * H[7] - H[4] * H[6];
    const double id = 1.0 / (H[0] * c00 + H[1] * c01 + H[2] * c02);
    Hi[0] = c00 * id; Hi[1] = (H[2] * H[7] - H[1] * H[8]) * id; Hi[2] = (H[1] * H[5] - H[2] * H[4]) * id;
    Hi[3] = c01 * id; Hi[4] = (H[0] * H[8] - H[2] * H[6]) * id; Hi[5] = (H[2] * H[3] - H[0] * H[5]) * id;
    Hi[6] = c02 * id; Hi[7] = (H[1] * H[6] - H[0] * H[7]) * id; Hi[8] = (H[0] * H[4] - H[1] * H[3]) * id;
}

CBA_HD bool hr_finite9(const double* H) {
    for (int a = 0; a < 9; ++a)
        if (!(H[a] == H[a]) || fabs(H[a]) > 1.7976931348623157e308) return false;
    return true;
}

// the reference's failure test of fit / refit (homographyestimator.cpp:139, 160): std::isfinite(hmtx(0,0)) only.  A model
// with another non-finite entry passes, as there; it then scores no inliers (every comparison with NaN / inf is false).
CBA_HD bool hr_fit_ok(const double* H) { return fabs(H[0]) <= 1.7976931348623157e308; }

// H = T_dst^-1 Hn T_src (homographyestimator.cpp:79-87), T = [s 0 -s c; 0 s -s c; 0 0 1]
CBA_HD void hr_denormalise(const double* Hn, double ss, double csx, double csy, double sd, double cdx, double cdy, double* H) {
    const double Ts[9] = {ss, 0.0, -ss * csx, 0.0, ss, -ss * csy, 0.0, 0.0, 1.0};
    const double Tdi[9] = {1.0 / sd, 0.0, cdx, 0.0, 1.0 / sd, cdy, 0.0, 0.0, 1.0};
    double T1[9];
    mat3_mul(Hn, Ts, T1);
    mat3_mul(Tdi, T1, H);
}

// HomographyEstimator::fit on a 4-point sample (homographyestimator.cpp:17-87, 123-146): Hartley normalisation of the 4 source
// and 4 destination points (normalize_points_2d), the exact solve with h22 = 1, denormalisation.  False: singular system or a
// non-finite H(0,0) (fit returns nullopt).
CBA_HD bool hr_fit4(const double* X, const double* Y, const double* u, const double* v, double* H) {
    double csx = 0.0, csy = 0.0, cdx = 0.0, cdy = 0.0;
    for (int i = 0; i < 4; ++i) { csx += X[i]; csy += Y[i]; cdx += u[i]; cdy += v[i]; }
    csx /= 4.0; csy /= 4.0; cdx /= 4.0; cdy /= 4.0;
    double ms = 0.0, md = 0.0;
    for (int i = 0; i < 4; ++i) {
        ms += sqrt((X[i] - csx) * (X[i] - csx) + (Y[i] - csy) * (Y[i] - csy));
        md += sqrt((u[i] - cdx) * (u[i] - cdx) + (v[i] - cdy) * (v[i] - cdy));
    }
    ms /= 4.0; md /= 4.0;
    const double ss = ms > 0.0 ? 1.4142135623730951 / ms : 1.0, sd = md > 0.0 ? 1.4142135623730951 / md : 1.0;
    // rows [-x -y -1 0 0 0 ux uy] h = -u, [0 0 0 -x -y -1 vx vy] h = -v
    double A[8][9];
    for (int i = 0; i < 4; ++i) {
        const double x = ss * X[i] - ss * csx, y = ss * Y[i] - ss * csy, uu = sd * u[i] - sd * cdx, vv = sd * v[i] - sd * cdy;
        double* r0 = A[2 * i];
        double* r1 = A[2 * i + 1];
        r0[0] = -x; r0[1] = -y; r0[2] = -1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = uu * x; r0[7] = uu * y; r0[8] = -uu;
        r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = -x; r1[4] = -y; r1[5] = -1.0; r1[6] = vv * x; r1[7] = vv * y; r1[8] = -vv;
    }
    for (int c = 0; c < 8; ++c) {  // Gaussian elimination with partial pivoting on the augmented 8 x 9 system
        int p = c;
        for (int r = c + 1; r < 8; ++r)
            if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
        if (!(fabs(A[p][c]) > 0.0)) return false;
        if (p != c)
            for (int j = c; j < 9; ++j) { const double t = A[c][j]; A[c][j] = A[p][j]; A[p][j] = t; }
        const double inv = 1.0 / A[c][c];
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] * inv;
            for (int j = c + 1; j < 9; ++j) A[r][j] -= f * A[c][j];
        }
    }
    double Hn[9];
    Hn[8] = 1.0;
    for (int c = 7; c >= 0; --c) {
        double s = A[c][8];
        for (int j = c + 1; j < 8; ++j) s -= A[c][j] * Hn[j];
        Hn[c] = s / A[c][c];
    }
    hr_denormalise(Hn, ss, csx, csy, sd, cdx, cdy, H);
    return hr_fit_ok(H);
}

// symmetric_transfer_error (homographyestimator.cpp:80-94) in the parts the kernels use: A = |uv q2 - q01|^2, B = |xy s2 - s01|^2,
// q = H (x, y, 1), s = Hi (u, v, 1); r^2 = (A / q2^2 + B / s2^2) / 2.
struct HrResid {
    double A, B, q2s, s2s;  // q2^2, s2^2
};
CBA_HD HrResid hr_resid_parts(const double* H, const double* Hi, double x, double y, double u, double v) {
    const double q0 = fma(H[0], x, fma(H[1], y, H[2])), q1 = fma(H[3], x, fma(H[4], y, H[5])), q2 = fma(H[6], x, fma(H[7], y, H[8]));
    const double s0 = fma(Hi[0], u, fma(Hi[1], v, Hi[2])), s1 = fma(Hi[3], u, fma(Hi[4], v, Hi[5])), s2 = fma(Hi[6], u, fma(Hi[7], v, Hi[8]));
    const double e0 = fma(u, q2, -q0), e1 = fma(v, q2, -q1), f0 = fma(x, s2, -s0), f1 = fma(y, s2, -s1);
    HrResid r;
    r.A = fma(e0, e0, e1 * e1);
    r.B = fma(f0, f0, f1 * f1);
    r.q2s = q2 * q2;
    r.s2s = s2 * s2;
    return r;
}
// r <= thresh (t2 = thresh^2), division-free; false for a point mapped to infinity either way (the reference's r is inf / NaN)
CBA_HD bool hr_is_inlier(const HrResid& r, double t2) {
    const double den = r.q2s * r.s2s;
    return den > 0.0 && fma(r.A, r.s2s, r.B * r.q2s) <= 2.0 * t2 * den;
}
CBA_HD double hr_r2(const HrResid& r) { return fma(r.A, r.s2s, r.B * r.q2s) / (2.0 * r.q2s * r.s2s); }

// ---- refit from moments -------------------------------------------------------------------------------------------------
// Moments of one inlier set after centring and scaling (x, y: object, s* (X - c*); u, v: image, s_d (u - c_d)):
// M[6 w + m], m over (xx, xy, x, yy, y, 1), w over (1, u, v, u^2 + v^2).
constexpr int HR_NMOM = 24;
CBA_HD void hr_accumulate(double x, double y, double uu, double vv, double* M) {
    const double mm[6] = {x * x, x * y, x, y * y, y, 1.0};
    const double w3 = fma(uu, uu, vv * vv);
    for (int m = 0; m < 6; ++m) {
        M[m] += mm[m];
        M[6 + m] = fma(uu, mm[m], M[6 + m]);
        M[12 + m] = fma(vv, mm[m], M[12 + m]);
        M[18 + m] = fma(w3, mm[m], M[18 + m]);
    }
}

// the normalised DLT's smallest right singular vector from its 9 x 9 Gram (dlt_homography_view: shift 1e-14 trace, 8 inverse
// iteration steps), Hn / Hn(2,2) (homographyestimator.cpp:70), denormalised.  False: Cholesky failure or a non-finite H(0,0).
CBA_HD bool hr_refit(const double* M, double ss, double csx, double csy, double sd, double cdx, double cdy, double* H) {
    // (a, b) of m m^T -> monomial index
    const int mi[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    double A[81];
    for (int e = 0; e < 81; ++e) A[e] = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const int m = mi[a][b];
            A[a * 9 + b] = M[m];
            A[(3 + a) * 9 + 3 + b] = M[m];
            A[a * 9 + 6 + b] = -M[6 + m];
            A[(6 + b) * 9 + a] = -M[6 + m];
            A[(3 + a) * 9 + 6 + b] = -M[12 + m];
            A[(6 + b) * 9 + 3 + a] = -M[12 + m];
            A[(6 + a) * 9 + 6 + b] = M[18 + m];
        }
    double tr = 0.0;
    for (int a = 0; a < 9; ++a) tr += A[a * 9 + a];
    const double shift = 1e-14 * tr + 1e-300;
    for (int a = 0; a < 9; ++a) A[a * 9 + a] += shift;
    if (!chol_n<9>(A)) return false;
    double h[9] = {0.37, -0.61, 0.83, 0.29, 0.71, -0.43, 0.53, -0.19, 0.97};
    for (int it = 0; it < 8; ++it) {
        chol_solve_n<9>(A, h);
        double nn = 0.0;
        for (int a = 0; a < 9; ++a) nn += h[a] * h[a];
        nn = 1.0 / sqrt(nn);
        for (int a = 0; a < 9; ++a) h[a] *= nn;
    }
    double Hn[9];
    for (int a = 0; a < 9; ++a) Hn[a] = h[a] / h[8];
    hr_denormalise(Hn, ss, csx, csy, sd, cdx, cdy, H);
    return hr_fit_ok(H);
}

// ---- Zhang --------------------------------------------------------------------------------------------------------------
// normalize_hmtx (zhang.cpp:112-138): h33 >= 0, then / h33, or (|h33| <= 1e-12) / ||H||_F.  Non-finite H is returned as is.
CBA_HD void hr_normalize_hmtx(const double* H, double* o) {
    for (int a = 0; a < 9; ++a) o[a] = H[a];
    if (!hr_finite9(o)) return;
    if (o[8] < 0.0)
        for (int a = 0; a < 9; ++a) o[a] = -o[a];
    const double h33 = o[8];
    if (fabs(h33) > 1e-12) {
        for (int a = 0; a < 9; ++a) o[a] /= h33;
        return;
    }
    double nf = 0.0;
    for (int a = 0; a < 9; ++a) nf += o[a] * o[a];
    nf = sqrt(nf);
    if (nf > 1e-12)
        for (int a = 0; a < 9; ++a) o[a] /= nf;
}

// v_ij (zhang.cpp:93-107), H row-major
CBA_HD void hr_vij(const double* H, int i, int j, double* v) {
    const double h0i = H[i], h1i = H[3 + i], h2i = H[6 + i], h0j = H[j], h1j = H[3 + j], h2j = H[6 + j];
    v[0] = h0i * h0j; v[1] = h0i * h1j + h1i * h0j; v[2] = h1i * h1j;
    v[3] = h0i * h2j + h2i * h0j; v[4] = h1i * h2j + h2i * h1j; v[5] = h2i * h2j;
}

// The two rows of one view (make_zhang_design_matrix, zhang.cpp:140-172), each normalised to unit length, added to the
// 6 x 6 Gram G (row-major, full).
CBA_HD void hr_zhang_accumulate(const double* H, double* G) {
    double Hn[9], r0[6], v11[6], v22[6], r1[6];
    hr_normalize_hmtx(H, Hn);
    hr_vij(Hn, 0, 1, r0);
    hr_vij(Hn, 0, 0, v11);
    hr_vij(Hn, 1, 1, v22);
    for (int k = 0; k < 6; ++k) r1[k] = v11[k] - v22[k];
    double* rows[2] = {r0, r1};
    for (double* r : rows) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += r[k] * r[k];
        s = sqrt(s);
        if (s > 0.0)
            for (int k = 0; k < 6; ++k) r[k] /= s;
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) G[a * 6 + b] += r[a] * r[b];
    }
}

// cyclic Jacobi on a symmetric N x N: eigenvalues in d, eigenvectors in the columns of V
template <int N>
CBA_HD void hr_eig_sym(const double* S, double* d, double* V) {
    double A[N * N];
    for (int i = 0; i < N * N; ++i) { A[i] = S[i]; V[i] = (i % (N + 1) == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 50; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < N; ++p) {
            diag += A[p * N + p] * A[p * N + p];
            for (int q = p + 1; q < N; ++q) off += A[p * N + q] * A[p * N + q];
        }
        if (off <= 1e-36 * diag || off <= 1e-300) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; ++k) {
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = c * akp - s * akq;
                    A[k * N + q] = s * akp + c * akq;
                }
                for (int k = 0; k < N; ++k) {
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = c * apk - s * aqk;
                    A[q * N + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < N; ++k) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int p = 0; p < N; ++p) d[p] = A[p * N + p];
}

// try_factor of kmtx_from_dual_conic (zhang.cpp:40-80) on B: LLT (B = U^T U), K = U^-1 / K22, flipped when fx <= 0 or fy <= 0.
// K row-major upper triangular.
CBA_HD bool hr_try_factor(const double* B, double* K) {
    for (int a = 0; a < 9; ++a)
        if (!(B[a] == B[a]) || fabs(B[a]) > 1.7976931348623157e308) return false;
    // Eigen::LLT: lower L column by column, fails on a non-positive pivot
    double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 3; ++j) {
        double s = B[j * 3 + j];
        for (int k = 0; k < j; ++k) s -= L[j * 3 + k] * L[j * 3 + k];
        if (!(s > 0.0)) return false;
        const double ljj = sqrt(s);
        L[j * 3 + j] = ljj;
        for (int i = j + 1; i < 3; ++i) {
            double t = B[i * 3 + j];
            for (int k = 0; k < j; ++k) t -= L[i * 3 + k] * L[j * 3 + k];
            L[i * 3 + j] = t / ljj;
        }
    }
    // U = L^T; K = U^-1 (upper triangular inverse)
    const double u00 = L[0], u01 = L[3], u02 = L[6], u11 = L[4], u12 = L[7], u22 = L[8];
    double Km[9] = {1.0 / u00, -u01 / (u00 * u11), (u01 * u12 - u02 * u11) / (u00 * u11 * u22),
                    0.0, 1.0 / u11, -u12 / (u11 * u22),
                    0.0, 0.0, 1.0 / u22};
    if (!hr_finite9(Km)) return false;
    const double k22 = Km[8];
    if (fabs(k22) < 1e-15) return false;
    for (int a = 0; a < 9; ++a) Km[a] /= k22;
    if (Km[0] <= 0.0 || Km[4] <= 0.0)
        for (int a = 0; a < 9; ++a) Km[a] = -Km[a];
    for (int a = 0; a < 9; ++a) K[a] = Km[a];
    return true;
}

// kmtx_from_dual_conic (zhang.cpp:33-91): B = sym(b), then -B
CBA_HD bool hr_k_from_b(const double* b, double* K) {
    const double B[9] = {b[0], b[1], b[3], b[1], b[2], b[4], b[3], b[4], b[5]};
    if (hr_try_factor(B, K)) return true;
    double Bm[9];
    for (int a = 0; a < 9; ++a) Bm[a] = -B[a];
    return hr_try_factor(Bm, K);
}

// zhang_intrinsics_from_hs (zhang.cpp:174-206) from the accumulated Gram of m views: kmtx5 = [fx, fy, cx, cy, skew].
CBA_HD bool hr_zhang_solve(int m, const double* G, double* kmtx5) {
    if (m < 4) return false;
    double d[6], V[36];
    hr_eig_sym<6>(G, d, V);
    int kmin = 0;
    for (int k = 1; k < 6; ++k) if (d[k] < d[kmin]) kmin = k;
    double b[6];
    for (int k = 0; k < 6; ++k) b[k] = V[k * 6 + kmin];
    double K[9];
    bool ok = hr_k_from_b(b, K);
    if (!ok) {  // zhang.cpp:193-201 (the second sign is already tried inside; kept as the reference has it)
        for (int k = 0; k < 6; ++k) b[k] = -b[k];
        ok = hr_k_from_b(b, K);
    }
    if (!ok) return false;
    kmtx5[0] = K[0]; kmtx5[1] = K[4]; kmtx5[2] = K[2]; kmtx5[3] = K[5]; kmtx5[4] = K[1];
    return true;
}

// ---- pose_from_homography -----------------------------------------------------------------------------------------------
// project_to_so3 (se3_utils.h:10-19): U diag(1, 1, det(U V^T) < 0 ? -1 : 1) V^T of the SVD of M
CBA_HD void hr_project_to_so3(const double* Ri, double* R) {
    double S[9], d[3], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[i * 3 + j] = Ri[0 * 3 + i] * Ri[0 * 3 + j] + Ri[1 * 3 + i] * Ri[1 * 3 + j] + Ri[2 * 3 + i] * Ri[2 * 3 + j];
    seed_eig3(S, d, V);
    const double det = Ri[0] * (Ri[4] * Ri[8] - Ri[5] * Ri[7]) - Ri[1] * (Ri[3] * Ri[8] - Ri[5] * Ri[6]) + Ri[2] * (Ri[3] * Ri[7] - Ri[4] * Ri[6]);
    int kmin = 0;
    for (int k = 1; k < 3; ++k) if (d[k] < d[kmin]) kmin = k;
    double w[3];
    for (int k = 0; k < 3; ++k) w[k] = 1.0 / sqrt(d[k] > 1e-300 ? d[k] : 1e-300);
    if (det < 0.0) w[kmin] = -w[kmin];
    double Q[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Q[i * 3 + j] = V[i * 3 + 0] * w[0] * V[j * 3 + 0] + V[i * 3 + 1] * w[1] * V[j * 3 + 1] + V[i * 3 + 2] * w[2] * V[j * 3 + 2];
    mat3_mul(Ri, Q, R);
}

// pose_from_homography (posefromhomography.cpp:11-62) with K = [fx, fy, cx, cy, skew].  Out: R row-major, t, scale, cond_check.
CBA_HD bool hr_pose_from_homography(const double* k5, const double* H, double* R, double* t, double* scale, double* cond) {
    const double fx = k5[0], fy = k5[1], cx = k5[2], cy = k5[3], sk = k5[4];
    const double big = 1.7976931348623157e308;
    if (!(fabs(fx) <= big) || !(fabs(fy) <= big) || cx <= 0.0 || cy <= 0.0) return false;
    if (!(fabs(H[8]) <= big)) return false;
    const double K[9] = {fx, sk, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
    double Ki[9], Hn[9];
    hr_inv3(K, Ki);
    mat3_mul(Ki, H, Hn);
    const double n1 = sqrt(Hn[0] * Hn[0] + Hn[3] * Hn[3] + Hn[6] * Hn[6]);
    const double n2 = sqrt(Hn[1] * Hn[1] + Hn[4] * Hn[4] + Hn[7] * Hn[7]);
    if (!(n1 > 1e-15) || !(n2 > 1e-15)) return false;
    const double s = 1.0 / ((n1 + n2) * 0.5);
    *scale = s;
    *cond = n1 > n2 ? n1 / n2 : n2 / n1;
    const double r1[3] = {s * Hn[0], s * Hn[3], s * Hn[6]}, r2[3] = {s * Hn[1], s * Hn[4], s * Hn[7]};
    double r3[3];
    cross3(r1, r2, r3);
    const double Ri[9] = {r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2]};
    hr_project_to_so3(Ri, R);
    for (int k = 0; k < 3; ++k) t[k] = s * Hn[3 * k + 2];
    if (t[2] <= 0.0) {
        for (int k = 0; k < 9; ++k) R[k] = -R[k];
        for (int k = 0; k < 3; ++k) t[k] = -t[k];
    }
    return true;
}

// ---- sanitize_intrinsics (common/intrinsics_utils.h) ----------------------------------------------------------------------
// lo5 / hi5 = [fx, fy, cx, cy, skew] bounds (no bounds: the caller passes nothing and K is kept).  Returns `modified`.
CBA_HD bool hr_sanitize(const double* k5, const double* lo5, const double* hi5, double* out5) {
    const double big = 1.7976931348623157e308;
    bool mod = false;
    for (int k = 0; k < 5; ++k) out5[k] = k5[k];
    for (int k = 0; k < 2; ++k)  // enforce_min_focal
        if (!(fabs(out5[k]) <= big) || out5[k] < lo5[k]) { mod = true; out5[k] = lo5[k]; }
    for (int k = 2; k < 4; ++k)  // adjust_principal_point
        if (!(fabs(out5[k]) <= big) || out5[k] < lo5[k] || out5[k] > hi5[k]) { mod = true; out5[k] = 0.5 * (lo5[k] + hi5[k]); }
    const double smin = lo5[4] < hi5[4] ? lo5[4] : hi5[4], smax = lo5[4] < hi5[4] ? hi5[4] : lo5[4];
    if (!(fabs(out5[4]) <= big) || out5[4] < smin || out5[4] > smax) {
        mod = true;
        out5[4] = 0.0 < smin ? smin : (smax < 0.0 ? smax : 0.0);  // std::clamp(0.0, smin, smax)
    }
    return mod;
}

}  // namespace cba
