// ls_driver.cpp — TEST-ONLY: extern "C" wrappers of linescan_math.hpp for ctypes (tests/test_linescan_cpu.py).
#include <cmath>
#include <vector>

#include "../../calibration_amd/csrc/linescan_math.hpp"

using namespace cba;

static LsCamera camera(int model, const double* intr, int n_inv, const double* inv) {
    LsCamera c;
    ls_fill_camera(model, intr, n_inv, inv, &c);
    return c;
}

extern "C" {

void ls_unproject(int model, const double* intr, int n_inv, const double* inv, int n, const double* u, const double* v, double* x,
                  double* y) {
    const LsCamera c = camera(model, intr, n_inv, inv);
    for (int i = 0; i < n; ++i) ls_unproject(c, u[i], v[i], x + i, y + i);
}

// points_from_view of one view: returns 1 and pts [m][3] when the homography succeeds, else 0
int ls_points_from_view(int model, const double* intr, int n_inv, const double* inv, int n, const double* X, const double* Y,
                        const double* u, const double* v, int m, const double* lu, const double* lv, double* pts) {
    const LsCamera c = camera(model, intr, n_inv, inv);
    std::vector<double> nu(n), nv(n);
    double geo[LS_GEO];
    SerialCoop co;
    if (!ls_view_geometry(c, n, X, Y, u, v, nu.data(), nv.data(), co, geo)) return 0;
    for (int i = 0; i < m; ++i) ls_backproject(c, geo, lu[i], lv[i], pts + 3 * i);
    return 1;
}

// fit_plane_svd as the device runs it: two-pass centred scatter, seed_eig3, sign convention
void ls_fit_plane(int n, const double* p, double* plane) {
    double c[3] = {0, 0, 0}, scale = 0.0;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) { c[k] += p[3 * i + k]; scale = std::fmax(scale, std::fabs(p[3 * i + k])); }
    for (double& ck : c) ck /= n;
    double S[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        const double dx = p[3 * i] - c[0], dy = p[3 * i + 1] - c[1], dz = p[3 * i + 2] - c[2];
        S[0] += dx * dx; S[1] += dx * dy; S[2] += dx * dz; S[3] += dy * dy; S[4] += dy * dz; S[5] += dz * dz;
    }
    ls_plane_from_scatter(c, S, plane);
    ls_plane_sign(plane, scale);
}

void ls_sign(double* plane, double scale) { ls_plane_sign(plane, scale); }
void ls_homography(const double* plane, double* H) { ls_plane_homography(plane, H); }
void ls_hyp(uint64_t seed, int64_t k, int64_t n, int64_t* idx) { ls_hypothesis(seed, k, n, idx); }

}  // extern "C"
