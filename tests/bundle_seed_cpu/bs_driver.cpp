// bs_driver.cpp — TEST-ONLY: extern "C" wrappers of bundle_seed_math.hpp for ctypes (tests/test_bundle_seed_cpu.py).
#include "../../calibration_amd/csrc/bundle_seed_math.hpp"

using namespace cba;

extern "C" {

// one pose-table row [Rb tb Rc tc] of a block
void bs_pose_row_c(const double* bTg12, const double* c_T_t7, double* row24) { bs_pose_row(bTg12, c_T_t7, row24); }

// the initial target over n candidates b_T_g[k] * g_T_c[cam[k]] * c_T_t[k], averaged in the given order (the device order is
// camera-major, then list order)
void bs_target_c(int n, const double* bTg12, const int* cam, const double* g7, const double* c7, double* out7) {
    ExtAvg acc;
    ext_avg_init(acc);
    for (int k = 0; k < n; ++k) {
        double q[4], t[3];
        bs_candidate(bTg12 + 12 * k, g7 + 7 * cam[k], c7 + 7 * k, q, t);
        ext_avg_add(acc, q, t);
    }
    ext_avg_finish(acc, out7);
}

}  // extern "C"
