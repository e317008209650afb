// distortion_fit_math.hpp — fit_distortion_full / fit_distortion_dual (include/calib/models/distortion.h:229-406) and
// estimate_intrinsics_linear / estimate_intrinsics_linear_iterative (src/estimation/linear/intrinsicsdlt.cpp:147-368) as
// __host__ __device__ code.  distortion_fit.hip runs the moment update per observation and the tails per lane;
// tests/distortion_cpu compiles the same header with g++.
//
// Moment form.  With m = nr + 2 coefficients [k1 .. k_nr, p1, p2], each observation (x, y, u, v) defines two K-independent
// m-vectors
//   a = [x r^2, .., x r^(2 nr), 2xy, r^2 + 2x^2]        b = [y r^2, .., y r^(2 nr), r^2 + 2y^2, 2xy]
// The reference's design row for u is fx a + skew b, the one for v is fy b, and apply_distortion(p) - p = (alpha.a, alpha.b).
// So every Gram matrix and right-hand side of the distortion fit for a given K, and every sum of the linear K fit on the
// distortion-corrected observations, is a closed-form combination of the fixed moments (DfitLayout)
//   Σ a aᵀ, Σ b bᵀ (upper triangles), Σ a bᵀ, Σ a·{x, y, u, 1}, Σ b·{x, y, u, v, 1}, Σ{xx, xy, yy, x, y, xu, yu, u, yv, v, 1}
// (111 at nr = 3).  One pass over the data gives them; the alternation of the iterative estimator then runs on them alone.
//
// Solves (departure (a) of calibba.h).  The reference solves the 2N x m design with JacobiSVD::solve (minimum-norm least
// squares) and the K fit's 2N x {2, 3} designs with a σ_min < 1e-12 rejection.  Here both become the normal equations from the
// moments: the Gram matrix is column-equilibrated (unit diagonal; an all-zero column keeps scale 1) and eigen-decomposed by
// cyclic Jacobi.  The distortion fit drops eigenvalues <= DFIT_EIG_RTOL * λ_max and returns the minimum-norm member of the
// remaining solution set (the dropped directions are mapped back to coefficient space and projected out, so the minimum is
// taken in the reference's coordinates, not the equilibrated ones).  The K fit is DEGENERATE when λ_min <= DFIT_EIG_RTOL * λ_max.
#pragma once
#include <cstdint>
#include "reproj_math.hpp"

namespace cba {

constexpr int DFIT_MAX_M = 5;                // num_radial <= 3
constexpr double DFIT_EIG_RTOL = 1e-13;      // relative eigenvalue cutoff of the equilibrated Grams (σ ratio ~3.2e-7)
constexpr double DFIT_CONVERGENCE = 1e-6;    // intrinsicsdlt.cpp:331
constexpr int DFIT_MIN_FIT_OBS = 8;          // distortion.h:235
constexpr int DFIT_MIN_K_OBS = 2;            // intrinsicsdlt.cpp:293
enum { DFIT_OK = 0, DFIT_TOO_FEW = 1, DFIT_DEGENERATE = 2 };  // = CBA_LINEAR_* of calibba.h

// A compiler-only barrier: the iterative tail re-reads its moments from memory every iteration instead of holding all of them
// in registers across the loop (no spill to scratch on the device).
#define CBA_DFIT_RELOAD() __asm__ volatile("" ::: "memory")

template <int M>
struct DfitLayout {
    static constexpr int NS = M * (M + 1) / 2;
    static constexpr int AA = 0;           // Σ a_i a_j, i <= j, row by row
    static constexpr int BB = AA + NS;     // Σ b_i b_j, i <= j
    static constexpr int AB = BB + NS;     // Σ a_i b_j, [i][j]
    static constexpr int AX = AB + M * M;  // Σ a_i x, Σ a_i y, Σ a_i u, Σ a_i: [4][M]
    static constexpr int BX = AX + 4 * M;  // Σ b_i x, Σ b_i y, Σ b_i u, Σ b_i v, Σ b_i: [5][M]
    static constexpr int SC = BX + 5 * M;  // Σ xx, xy, yy, x, y, xu, yu, u, yv, v, 1
    static constexpr int NM = SC + 11;
    static constexpr int tri(int i, int j) { return i * M - i * (i - 1) / 2 + (j - i); }  // i <= j
};

// fixed coefficients of one call: bit i of mask = coefficient i is held at val[i]
struct DfitFixed {
    int mask;
    double val[DFIT_MAX_M];
};

// CalibrationBounds as [fx, fy, cx, cy, skew] (camera_matrix.h:50-60)
struct DfitBounds {
    double lo[5];
    double hi[5];
};
CBA_HD DfitBounds dfit_default_bounds() {
    return DfitBounds{{0.0, 0.0, 0.0, 0.0, -0.01}, {2000.0, 2000.0, 1280.0, 720.0, 0.01}};
}

template <int M>
CBA_HD void dfit_basis(double x, double y, double* a, double* b) {
    const double r2 = x * x + y * y;
    double rp = r2;
#pragma unroll
    for (int j = 0; j < M - 2; ++j) {
        a[j] = x * rp;
        b[j] = y * rp;
        rp *= r2;
    }
    const double xy2 = 2.0 * x * y;
    a[M - 2] = xy2;
    a[M - 1] = r2 + 2.0 * x * x;
    b[M - 2] = r2 + 2.0 * y * y;
    b[M - 1] = xy2;
}

// the NM moments of one observation, in DfitLayout order
template <int M>
CBA_HD void dfit_obs_moments(double x, double y, double u, double v, double* mo) {
    using L = DfitLayout<M>;
    double a[M], b[M];
    dfit_basis<M>(x, y, a, b);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j) {
            mo[L::AA + L::tri(i, j)] = a[i] * a[j];
            mo[L::BB + L::tri(i, j)] = b[i] * b[j];
        }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) mo[L::AB + i * M + j] = a[i] * b[j];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        mo[L::AX + i] = a[i] * x;
        mo[L::AX + M + i] = a[i] * y;
        mo[L::AX + 2 * M + i] = a[i] * u;
        mo[L::AX + 3 * M + i] = a[i];
        mo[L::BX + i] = b[i] * x;
        mo[L::BX + M + i] = b[i] * y;
        mo[L::BX + 2 * M + i] = b[i] * u;
        mo[L::BX + 3 * M + i] = b[i] * v;
        mo[L::BX + 4 * M + i] = b[i];
    }
    mo[L::SC + 0] = x * x;
    mo[L::SC + 1] = x * y;
    mo[L::SC + 2] = y * y;
    mo[L::SC + 3] = x;
    mo[L::SC + 4] = y;
    mo[L::SC + 5] = x * u;
    mo[L::SC + 6] = y * u;
    mo[L::SC + 7] = u;
    mo[L::SC + 8] = y * v;
    mo[L::SC + 9] = v;
    mo[L::SC + 10] = 1.0;
}

// fit_distortion_dual's inverse observation (distortion.h:384-390): the K-normalised pixel and the undistorted pixel; K5 =
// [fx, fy, cx, cy, skew]
CBA_HD void dfit_dual_obs(const double* K, double x, double y, double u, double v, double* xo, double* yo, double* uo, double* vo) {
    const double y_dist = (v - K[3]) / K[1];
    const double x_dist = (u - K[2] - K[4] * y_dist) / K[0];
    *uo = K[0] * x + K[4] * y + K[2];
    *vo = K[1] * y + K[3];
    *xo = x_dist;
    *yo = y_dist;
}

// cyclic Jacobi on a symmetric N x N (row-major; A is diagonalised in place, eigenvectors in the columns of V).  Fixed sweep
// order, so bitwise reproducible; a pair whose off-diagonal entry is exactly 0 is not rotated (decoupled blocks stay decoupled).
template <int N>
CBA_HD void dfit_jacobi(double* A, double* V) {
#pragma unroll
    for (int i = 0; i < N * N; ++i) V[i] = (i % (N + 1) == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int p = 0; p < N; ++p) {
            dia += A[p * N + p] * A[p * N + p];
#pragma unroll
            for (int q = p + 1; q < N; ++q) off += A[p * N + q] * A[p * N + q];
        }
        if (!(off > 1e-36 * dia)) break;
#pragma unroll
        for (int p = 0; p < N; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
                const double at = fabs(theta);
                const double t = at > 1e150 ? 0.5 / theta : (theta >= 0.0 ? 1.0 : -1.0) / (at + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < N; ++k) {  // A J
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = c * akp - s * akq;
                    A[k * N + q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {  // J^T (A J)
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = c * apk - s * aqk;
                    A[q * N + k] = s * apk + c * aqk;
                }
                A[p * N + q] = 0.0;
                A[q * N + p] = 0.0;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
}

// Equilibrate G (N x N symmetric) and decompose it: d = column scales, A = diagonal of eigenvalues, V = eigenvectors.
template <int N>
CBA_HD void dfit_eq_eig(const double* G, double* d, double* A, double* V) {
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = G[i * N + i] > 0.0 ? 1.0 / sqrt(G[i * N + i]) : 1.0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) A[i * N + j] = d[i] * G[i * N + j] * d[j];
    dfit_jacobi<N>(A, V);
}

// x = G⁺ h restricted to the eigenvalues above the cutoff, minimum-norm in x's own coordinates.  Returns the number of dropped
// directions.  keep_all: solve with every eigenvalue (the K fit, whose degeneracy is tested before).
template <int N>
CBA_HD int dfit_solve_sym(const double* G, const double* h, double* x, bool keep_all) {
    double d[N], A[N * N], V[N * N];
    dfit_eq_eig<N>(G, d, A, V);
    double lmax = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) lmax = fmax(lmax, A[k * N + k]);
    double beta[N];
#pragma unroll
    for (int i = 0; i < N; ++i) beta[i] = 0.0;
    bool drop[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double lam = A[k * N + k];
        drop[k] = !keep_all && !(lam > DFIT_EIG_RTOL * lmax);
        if (drop[k]) continue;
        double c = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) c += V[i * N + k] * (d[i] * h[i]);
        c /= lam;
#pragma unroll
        for (int i = 0; i < N; ++i) beta[i] += c * V[i * N + k];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = d[i] * beta[i];
    // project out the dropped directions d ∘ v_k (modified Gram-Schmidt in x's coordinates; row k of Q is the k-th direction)
    int ndrop = 0;
    double Q[N * N];
    bool qv[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        qv[k] = false;
        if (!drop[k]) continue;
        double w[N];
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = d[i] * V[i * N + k];
#pragma unroll
        for (int q = 0; q < k; ++q) {
            if (!qv[q]) continue;
            double dot = 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) dot += Q[q * N + i] * w[i];
#pragma unroll
            for (int i = 0; i < N; ++i) w[i] -= dot * Q[q * N + i];
        }
        double nrm = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) nrm += w[i] * w[i];
        nrm = sqrt(nrm);
        if (!(nrm > 0.0)) continue;
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            w[i] /= nrm;
            dot += w[i] * x[i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            x[i] -= dot * w[i];
            Q[k * N + i] = w[i];
        }
        qv[k] = true;
        ++ndrop;
    }
    return ndrop;
}

// true when the equilibrated Gram's λ_min <= DFIT_EIG_RTOL λ_max (the K fit's counterpart of σ_min < 1e-12)
template <int N>
CBA_HD bool dfit_degenerate(const double* G) {
    double d[N], A[N * N], V[N * N];
    dfit_eq_eig<N>(G, d, A, V);
    double lmin = A[0], lmax = A[0];
#pragma unroll
    for (int k = 1; k < N; ++k) {
        lmin = fmin(lmin, A[k * N + k]);
        lmax = fmax(lmax, A[k * N + k]);
    }
    return lmin <= DFIT_EIG_RTOL * lmax;
}

// The distortion fit's normal equations for K: G = Dᵀ D, h = Dᵀ rhs with D's rows fx a + skew b and fy b, and rhs = (u, v)
// minus the undistorted pixel (distortion.h:256-290).
template <int M>
CBA_HD void dfit_gram(const double* mo, const double* K, double* G, double* h) {
    using L = DfitLayout<M>;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], s = K[4];
    const double caa = fx * fx, cab = fx * s, cbb = s * s + fy * fy;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j) {
            const double g = caa * mo[L::AA + L::tri(i, j)] + cab * (mo[L::AB + i * M + j] + mo[L::AB + j * M + i]) +
                             cbb * mo[L::BB + L::tri(i, j)];
            G[i * M + j] = g;
            G[j * M + i] = g;
        }
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const double hu_a = mo[L::AX + 2 * M + i] - fx * mo[L::AX + i] - s * mo[L::AX + M + i] - cx * mo[L::AX + 3 * M + i];
        const double hu_b = mo[L::BX + 2 * M + i] - fx * mo[L::BX + i] - s * mo[L::BX + M + i] - cx * mo[L::BX + 4 * M + i];
        const double hv_b = mo[L::BX + 3 * M + i] - fy * mo[L::BX + M + i] - cy * mo[L::BX + 4 * M + i];
        h[i] = fx * hu_a + s * hu_b + fy * hv_b;
    }
}

// fit_distortion_full's coefficients for K from the moments (the caller has checked N >= 8).  Fixed entries are copied, so they
// come back bit-exact; the free ones solve the normal equations of the reduced design with rhs - D_F alpha_F (distortion.h:340-356).
template <int M>
CBA_HD void dfit_solve(const double* mo, const double* K, const DfitFixed& fx, double* alpha) {
    if (fx.mask == (1 << M) - 1) {  // every coefficient fixed (distortion.h:334-337)
#pragma unroll
        for (int i = 0; i < M; ++i) alpha[i] = fx.val[i];
        return;
    }
    double G[M * M], h[M];
    dfit_gram<M>(mo, K, G, h);
    if (fx.mask) {
#pragma unroll
        for (int i = 0; i < M; ++i) {
            if (fx.mask >> i & 1) continue;
#pragma unroll
            for (int j = 0; j < M; ++j)
                if (fx.mask >> j & 1) h[i] -= G[i * M + j] * fx.val[j];
        }
#pragma unroll
        for (int i = 0; i < M; ++i) {
            if (!(fx.mask >> i & 1)) continue;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                G[i * M + j] = i == j ? 1.0 : 0.0;
                G[j * M + i] = i == j ? 1.0 : 0.0;
            }
            h[i] = 0.0;
        }
    }
    dfit_solve_sym<M>(G, h, alpha, false);
#pragma unroll
    for (int i = 0; i < M; ++i)
        if (fx.mask >> i & 1) alpha[i] = fx.val[i];
}

// std::clamp
CBA_HD double dfit_clamp(double v, double lo, double hi) { return v < lo ? lo : (hi < v ? hi : v); }

// estimate_intrinsics_linear (intrinsicsdlt.cpp:289-312) on the observations corrected by alpha at Kprev
// (correct_observations_for_distortion, :249-267; alpha == nullptr: the raw observations).  n >= 2 is the caller's check.
// Returns DFIT_OK or DFIT_DEGENERATE; K out = [fx, fy, cx, cy, skew]; *fell_back = 1 when apply_bounds_and_fallback took its
// fallback (the reference's stderr warning).
template <int M>
CBA_HD int dfit_linear_k(const double* mo, const double* Kprev, const double* alpha, bool use_skew, const DfitBounds& B,
                         double* K, int* fell_back) {
    using L = DfitLayout<M>;
    const double sxx = mo[L::SC + 0], sxy = mo[L::SC + 1], syy = mo[L::SC + 2], sx = mo[L::SC + 3], sy = mo[L::SC + 4];
    const double n = mo[L::SC + 10];
    double sxu = mo[L::SC + 5], syu = mo[L::SC + 6], su = mo[L::SC + 7], syv = mo[L::SC + 8], sv = mo[L::SC + 9];
    if (alpha) {  // u_c = u - fx alpha.a - skew alpha.b, v_c = v - fy alpha.b
        const double fx = Kprev[0], fy = Kprev[1], s = Kprev[4];
#pragma unroll
        for (int i = 0; i < M; ++i) {
            sxu -= alpha[i] * (fx * mo[L::AX + i] + s * mo[L::BX + i]);
            syu -= alpha[i] * (fx * mo[L::AX + M + i] + s * mo[L::BX + M + i]);
            su -= alpha[i] * (fx * mo[L::AX + 3 * M + i] + s * mo[L::BX + 4 * M + i]);
            syv -= alpha[i] * fy * mo[L::BX + M + i];
            sv -= alpha[i] * fy * mo[L::BX + 4 * M + i];
        }
    }
    double fx, cx, skew = 0.0;
    if (use_skew) {  // u = fx x + skew y + cx
        const double G[9] = {sxx, sxy, sx, sxy, syy, sy, sx, sy, n};
        const double h[3] = {sxu, syu, su};
        if (dfit_degenerate<3>(G)) return DFIT_DEGENERATE;
        double xu[3];
        dfit_solve_sym<3>(G, h, xu, true);
        fx = xu[0];
        skew = xu[1];
        cx = xu[2];
    } else {  // u = fx x + cx
        const double G[4] = {sxx, sx, sx, n};
        const double h[2] = {sxu, su};
        if (dfit_degenerate<2>(G)) return DFIT_DEGENERATE;
        double xu[2];
        dfit_solve_sym<2>(G, h, xu, true);
        fx = xu[0];
        cx = xu[1];
    }
    const double Gv[4] = {syy, sy, sy, n};
    const double hv[2] = {syv, sv};
    if (dfit_degenerate<2>(Gv)) return DFIT_DEGENERATE;
    double xv[2];
    dfit_solve_sym<2>(Gv, hv, xv, true);
    const double fy = xv[0], cy = xv[1];
    const bool out = fx < B.lo[0] || fx > B.hi[0] || fy < B.lo[1] || fy > B.hi[1] || cx < B.lo[2] || cx > B.hi[2] || cy < B.lo[3] ||
                     cy > B.hi[3] || (use_skew && (skew < B.lo[4] || skew > B.hi[4]));
    if (out) {  // apply_bounds_and_fallback (:213-247)
        K[0] = dfit_clamp(fmax(500.0, fx), B.lo[0], B.hi[0]);
        K[1] = dfit_clamp(fmax(500.0, fy), B.lo[1], B.hi[1]);
        K[2] = dfit_clamp(su / n / 2.0, B.lo[2], B.hi[2]);
        K[3] = dfit_clamp(sv / n / 2.0, B.lo[3], B.hi[3]);
        K[4] = use_skew ? dfit_clamp(skew, B.lo[4], B.hi[4]) : 0.0;
        *fell_back = 1;
    } else {
        K[0] = fx;
        K[1] = fy;
        K[2] = cx;
        K[3] = cy;
        K[4] = skew;
        *fell_back = 0;
    }
    return DFIT_OK;
}

// estimate_intrinsics_linear_iterative (intrinsicsdlt.cpp:319-368) of one problem of n observations from its moments.  K and
// alpha are written on DFIT_OK only (zero otherwise); iterations = K refits adopted; fallbacks = fits of K that took the
// fallback (the initial one included), i.e. the warnings the reference prints.  max_iterations is the caller's clamped value.
template <int M>
CBA_HD int dfit_iterative(const double* mo, int64_t n, int max_iterations, bool use_skew, double* K, double* alpha, int* iterations,
                          int* fallbacks) {
    *iterations = 0;
    *fallbacks = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) K[i] = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) alpha[i] = 0.0;
    if (n < DFIT_MIN_K_OBS) return DFIT_TOO_FEW;
    const DfitBounds B = dfit_default_bounds();  // the estimator passes nullopt (:323, :343)
    const DfitFixed none{0, {0.0, 0.0, 0.0, 0.0, 0.0}};
    double Kc[5];
    int fb = 0;
    if (dfit_linear_k<M>(mo, nullptr, nullptr, use_skew, B, Kc, &fb) != DFIT_OK) return DFIT_DEGENERATE;
    int nfb = fb, it = 0;
    for (int iter = 0; iter < max_iterations; ++iter) {
        CBA_DFIT_RELOAD();
        if (n < DFIT_MIN_FIT_OBS) break;  // fit_distortion fails
        double a[M], Kn[5];
        dfit_solve<M>(mo, Kc, none, a);
        if (dfit_linear_k<M>(mo, Kc, a, use_skew, B, Kn, &fb) != DFIT_OK) break;
        nfb += fb;
        const double change = fabs(Kc[0] - Kn[0]) + fabs(Kc[1] - Kn[1]) + fabs(Kc[2] - Kn[2]) + fabs(Kc[3] - Kn[3]) + fabs(Kc[4] - Kn[4]);
#pragma unroll
        for (int i = 0; i < 5; ++i) Kc[i] = Kn[i];
        ++it;
        if (change < DFIT_CONVERGENCE) break;
    }
    *iterations = it;
    *fallbacks = nfb;
    if (n < DFIT_MIN_FIT_OBS) return DFIT_TOO_FEW;  // the final fit_distortion_full fails
    CBA_DFIT_RELOAD();
    dfit_solve<M>(mo, Kc, none, alpha);
#pragma unroll
    for (int i = 0; i < 5; ++i) K[i] = Kc[i];
    return DFIT_OK;
}

// one observation's residual pair (design * alpha - rhs, distortion.h:295, rows 2i and 2i + 1)
template <int M>
CBA_HD void dfit_residual(double x, double y, double u, double v, const double* K, const double* alpha, double* ru, double* rv) {
    double a[M], b[M];
    dfit_basis<M>(x, y, a, b);
    double da = 0.0, db = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        da += alpha[i] * a[i];
        db += alpha[i] * b[i];
    }
    *ru = K[0] * da + K[4] * db - (u - (K[0] * x + K[4] * y + K[2]));
    *rv = K[1] * db - (v - (K[1] * y + K[3]));
}

}  // namespace cba
