// df_driver.cpp — TEST-ONLY: extern "C" wrappers of distortion_fit_math.hpp for ctypes (tests/test_distortion_cpu.py).  Moments are
// summed in observation order on the host; the device sums them by chunks, so the two agree to rounding, not bitwise.
#include <vector>

#include "../../calibration_amd/csrc/distortion_fit_math.hpp"

using namespace cba;

namespace {

template <int M>
std::vector<double> moments(int64_t n, const double* x, const double* y, const double* u, const double* v, const double* Kdual) {
    std::vector<double> mo(DfitLayout<M>::NM, 0.0), one(DfitLayout<M>::NM);
    for (int64_t i = 0; i < n; ++i) {
        double xi = x[i], yi = y[i], ui = u[i], vi = v[i];
        if (Kdual) dfit_dual_obs(Kdual, x[i], y[i], u[i], v[i], &xi, &yi, &ui, &vi);
        dfit_obs_moments<M>(xi, yi, ui, vi, one.data());
        for (int k = 0; k < DfitLayout<M>::NM; ++k) mo[k] += one[k];
    }
    return mo;
}

template <int M>
int fit(int64_t n, const double* x, const double* y, const double* u, const double* v, const double* K, int mask, const double* val,
        int dual, double* coeffs, double* inverse, double* residuals) {
    if (n < DFIT_MIN_FIT_OBS) return 0;
    DfitFixed fx{mask, {0, 0, 0, 0, 0}};
    for (int i = 0; i < M; ++i) fx.val[i] = val[i];
    const std::vector<double> mo = moments<M>(n, x, y, u, v, nullptr);
    dfit_solve<M>(mo.data(), K, fx, coeffs);
    if (dual) {
        const std::vector<double> mi = moments<M>(n, x, y, u, v, K);
        dfit_solve<M>(mi.data(), K, fx, inverse);
    }
    if (residuals)
        for (int64_t i = 0; i < n; ++i) dfit_residual<M>(x[i], y[i], u[i], v[i], K, coeffs, residuals + 2 * i, residuals + 2 * i + 1);
    return 1;
}

template <int M>
int iterative(int64_t n, const double* x, const double* y, const double* u, const double* v, int max_it, int use_skew, double* K,
              double* coeffs, int* iters, int* fallbacks) {
    const std::vector<double> mo = moments<M>(n, x, y, u, v, nullptr);
    return dfit_iterative<M>(mo.data(), n, max_it, use_skew != 0, K, coeffs, iters, fallbacks);
}

}  // namespace

extern "C" {

int df_moment_count(int nr) {
    switch (nr) {
        case 0: return DfitLayout<2>::NM;
        case 1: return DfitLayout<3>::NM;
        case 2: return DfitLayout<4>::NM;
        default: return DfitLayout<5>::NM;
    }
}

// fit_distortion_full (and the inverse of fit_distortion_dual when dual != 0): returns ok
int df_fit(int64_t n, const double* x, const double* y, const double* u, const double* v, const double* K, int nr, int mask,
           const double* val5, int dual, double* coeffs, double* inverse, double* residuals) {
    switch (nr) {
        case 0: return fit<2>(n, x, y, u, v, K, mask, val5, dual, coeffs, inverse, residuals);
        case 1: return fit<3>(n, x, y, u, v, K, mask, val5, dual, coeffs, inverse, residuals);
        case 2: return fit<4>(n, x, y, u, v, K, mask, val5, dual, coeffs, inverse, residuals);
        default: return fit<5>(n, x, y, u, v, K, mask, val5, dual, coeffs, inverse, residuals);
    }
}

// estimate_intrinsics_linear: returns the status; bounds lo5 / hi5
int df_linear(int64_t n, const double* x, const double* y, const double* u, const double* v, const double* lo5, const double* hi5,
              int use_skew, double* K, int* fallback) {
    *fallback = 0;
    if (n < DFIT_MIN_K_OBS) return DFIT_TOO_FEW;
    const std::vector<double> mo = moments<2>(n, x, y, u, v, nullptr);
    DfitBounds B;
    for (int i = 0; i < 5; ++i) {
        B.lo[i] = lo5[i];
        B.hi[i] = hi5[i];
    }
    return dfit_linear_k<2>(mo.data(), nullptr, nullptr, use_skew != 0, B, K, fallback);
}

// estimate_intrinsics_linear_iterative: returns the status
int df_iterative(int64_t n, const double* x, const double* y, const double* u, const double* v, int nr, int max_it, int use_skew,
                 double* K, double* coeffs, int* iters, int* fallbacks) {
    switch (nr) {
        case 0: return iterative<2>(n, x, y, u, v, max_it, use_skew, K, coeffs, iters, fallbacks);
        case 1: return iterative<3>(n, x, y, u, v, max_it, use_skew, K, coeffs, iters, fallbacks);
        case 2: return iterative<4>(n, x, y, u, v, max_it, use_skew, K, coeffs, iters, fallbacks);
        default: return iterative<5>(n, x, y, u, v, max_it, use_skew, K, coeffs, iters, fallbacks);
    }
}

}  // extern "C"
