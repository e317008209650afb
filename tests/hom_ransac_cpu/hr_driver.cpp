// hr_driver.cpp — TEST-ONLY: extern "C" wrappers of hom_ransac_math.hpp for ctypes (tests/test_hom_ransac_cpu.py).
#include <cmath>

#include "../../calibration_amd/csrc/hom_ransac_math.hpp"

using namespace cba;

extern "C" {

void hr_sample_c(uint64_t seed, int64_t k, int64_t n, int* idx) { hr_sample(seed, k, n, idx); }
int hr_degenerate_c(const double* X, const double* Y) { return hr_degenerate(X, Y) ? 1 : 0; }
int hr_fit4_c(const double* X, const double* Y, const double* u, const double* v, double* H) { return hr_fit4(X, Y, u, v, H) ? 1 : 0; }

// r of every correspondence (sqrt of the kernels' r^2) and the division-free inlier test at thresh
void hr_residuals_c(const double* H, int n, const double* X, const double* Y, const double* u, const double* v, double thresh, double* r,
                    int* inlier) {
    double Hi[9];
    hr_inv3(H, Hi);
    for (int i = 0; i < n; ++i) {
        const HrResid p = hr_resid_parts(H, Hi, X[i], Y[i], u[i], v[i]);
        r[i] = std::sqrt(hr_r2(p));
        inlier[i] = hr_is_inlier(p, thresh * thresh) ? 1 : 0;
    }
}

// the refit over the points with sel[i] != 0, in the kernel's three passes (centroids, mean distances, moments)
int hr_refit_c(int n, const double* X, const double* Y, const double* u, const double* v, const int* sel, double* H) {
    double c = 0, aX = 0, aY = 0, au = 0, av = 0;
    for (int i = 0; i < n; ++i)
        if (sel[i]) { c += 1; aX += X[i]; aY += Y[i]; au += u[i]; av += v[i]; }
    const double csx = aX / c, csy = aY / c, cdx = au / c, cdy = av / c;
    double ms = 0, md = 0;
    for (int i = 0; i < n; ++i)
        if (sel[i]) {
            ms += std::sqrt((X[i] - csx) * (X[i] - csx) + (Y[i] - csy) * (Y[i] - csy));
            md += std::sqrt((u[i] - cdx) * (u[i] - cdx) + (v[i] - cdy) * (v[i] - cdy));
        }
    ms /= c; md /= c;
    const double ss = ms > 0 ? 1.4142135623730951 / ms : 1.0, sd = md > 0 ? 1.4142135623730951 / md : 1.0;
    double M[HR_NMOM] = {};
    for (int i = 0; i < n; ++i)
        if (sel[i]) hr_accumulate(ss * X[i] - ss * csx, ss * Y[i] - ss * csy, sd * u[i] - sd * cdx, sd * v[i] - sd * cdy, M);
    return hr_refit(M, ss, csx, csy, sd, cdx, cdy, H) ? 1 : 0;
}

int hr_zhang_c(int m, const double* h9, double* k5) {
    double G[36] = {};
    for (int i = 0; i < m; ++i) hr_zhang_accumulate(h9 + 9 * i, G);
    return hr_zhang_solve(m, G, k5) ? 1 : 0;
}

int hr_pose_c(const double* k5, const double* H, double* R, double* t, double* sc) {
    return hr_pose_from_homography(k5, H, R, t, sc, sc + 1) ? 1 : 0;
}

}  // extern "C"
