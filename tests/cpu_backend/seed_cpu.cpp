// tests/cpu_backend/seed_cpu.cpp — TEST-ONLY host run of seed_math.hpp (the per-view pose seed the GPU computes one wavefront
// per view) with the single-thread cooperative group.  Never linked into the product.
#include "../../calibration_amd/csrc/seed_math.hpp"

using namespace cba;

extern "C" void hm_planar_seed(int n, const double* X, const double* Y, const double* u, const double* v, const double* kmtx5, double* pose7) {
    SerialCoop co;
    planar_seed_view(n, X, Y, u, v, kmtx5, co, pose7);
}

// estimate_homography's DLT path on raw pixels, as k_dlt_homography calls it: H9 row-major (left as given when the fit fails); -> ok flag
extern "C" int hm_dlt_homography(int n, const double* X, const double* Y, const double* u, const double* v, double* H9) {
    SerialCoop co;
    const double K[5] = {1.0, 1.0, 0.0, 0.0, 0.0};
    return dlt_homography_view(n, X, Y, u, v, K, co, H9) ? 1 : 0;
}
