// ext_driver.cpp — TEST-ONLY: extern "C" wrappers of extrinsic_dlt_math.hpp for ctypes (tests/test_extrinsic_dlt_cpu.py).
#include "../../calibration_amd/csrc/extrinsic_dlt_math.hpp"

using namespace cba;

extern "C" {

// average_isometries of n poses pose7 [n][7], in the given order
void ext_average_c(int n, const double* pose7, double* out7) {
    ExtAvg acc;
    ext_avg_init(acc);
    for (int i = 0; i < n; ++i) {
        double R[9];
        quat_to_rotmat(pose7 + 7 * i, R);
        double q[4];
        seed_rotmat_to_quat(R, q);
        ext_avg_add(acc, q, pose7 + 7 * i + 4);
    }
    ext_avg_finish(acc, out7);
}

// steps 2-3 over a dense [n_views][n_cams] set of block poses pose7 and point counts npts, in the order the device kernels use
void ext_steps_c(int n_views, int n_cams, const double* pose7, const int* npts, double* c_T_r, double* r_T_t) {
    auto has = [&](int v, int c) { return npts[v * n_cams + c] >= 4; };
    auto blk = [&](int v, int c) { return pose7 + 7 * (v * n_cams + c); };
    for (int k = 0; k < 7; ++k) c_T_r[k] = k == 0 ? 1.0 : 0.0;
    for (int c = 1; c < n_cams; ++c) {
        ExtAvg acc;
        ext_avg_init(acc);
        for (int v = 0; v < n_views; ++v) {
            if (!has(v, 0) || !has(v, c)) continue;
            double q[4], t[3];
            ext_rel_pose(blk(v, c), blk(v, 0), q, t);
            ext_avg_add(acc, q, t);
        }
        ext_avg_finish(acc, c_T_r + 7 * c);
    }
    for (int v = 0; v < n_views; ++v) {
        ExtAvg acc;
        ext_avg_init(acc);
        for (int c = 0; c < n_cams; ++c) {
            if (!has(v, c)) continue;
            double Rc[9], q[4], t[3];
            quat_to_rotmat(c_T_r + 7 * c, Rc);
            ext_inv_mul(Rc, c_T_r + 7 * c + 4, blk(v, c), q, t);
            ext_avg_add(acc, q, t);
        }
        ext_avg_finish(acc, r_T_t + 7 * v);
    }
}

}  // extern "C"
