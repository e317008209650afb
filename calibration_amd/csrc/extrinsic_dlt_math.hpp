// extrinsic_dlt_math.hpp — the per-lane algebra of estimate_extrinsic_dlt (include/calib/estimation/linear/extrinsics.h:27-78)
// as __host__ __device__ code: the relative poses of steps 2 and 3 and average_isometries (estimation/common/se3_utils.h:75-95).
// Step 1 (one planar pose per (view, camera) block) is seed_math.hpp::planar_seed_view.
//
// Poses are pose7 = [qw qx qy qz tx ty tz]; a block pose's rotation is quat_to_rotmat(q) (the quaternion planar_seed_view
// returns is unit to rounding).  average_isometries keeps the reference's running quaternion sum: each new q is negated when its
// dot product with the sum SO FAR is negative, so the result depends on the order of the poses (the callers add them in
// increasing view / camera index).  The sum is normalised at the end (Eigen's Quaternion::normalize: q / |q|) and returned as the
// averaged pose's quaternion; the translation is the arithmetic mean.
#pragma once
#include "seed_math.hpp"

namespace cba {

// a * b^-1 (extrinsics.h:59): R = Ra Rb^T, t = ta - R tb; out: q (4, Eigen's matrix -> quaternion), t (3)
CBA_HD void ext_rel_pose(const double* a7, const double* b7, double* q, double* t) {
    double Ra[9], Rb[9], R[9];
    quat_to_rotmat(a7, Ra);
    quat_to_rotmat(b7, Rb);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Ra[3 * i] * Rb[3 * j] + Ra[3 * i + 1] * Rb[3 * j + 1] + Ra[3 * i + 2] * Rb[3 * j + 2];
    for (int i = 0; i < 3; ++i) t[i] = a7[4 + i] - (R[3 * i] * b7[4] + R[3 * i + 1] * b7[5] + R[3 * i + 2] * b7[6]);
    seed_rotmat_to_quat(R, q);
}

// c^-1 * b (extrinsics.h:70): R = Rc^T Rb, t = Rc^T (tb - tc); Rc row-major (the caller converts c's quaternion once)
CBA_HD void ext_inv_mul(const double* Rc, const double* tc, const double* b7, double* q, double* t) {
    double Rb[9], R[9];
    quat_to_rotmat(b7, Rb);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Rc[i] * Rb[j] + Rc[3 + i] * Rb[3 + j] + Rc[6 + i] * Rb[6 + j];
    const double d[3] = {b7[4] - tc[0], b7[5] - tc[1], b7[6] - tc[2]};
    mat3_tvec(Rc, d, t);
    seed_rotmat_to_quat(R, q);
}

// average_isometries (se3_utils.h:75-95), fed one pose at a time in the caller's order
struct ExtAvg {
    double q[4], t[3];
    int n;
};

CBA_HD void ext_avg_init(ExtAvg& a) {
    for (int k = 0; k < 4; ++k) a.q[k] = 0.0;
    for (int k = 0; k < 3; ++k) a.t[k] = 0.0;
    a.n = 0;
}

CBA_HD void ext_avg_add(ExtAvg& a, const double* q, const double* t) {
    for (int k = 0; k < 3; ++k) a.t[k] += t[k];
    const double dot = a.q[0] * q[0] + a.q[1] * q[1] + a.q[2] * q[2] + a.q[3] * q[3];
    const double s = dot < 0.0 ? -1.0 : 1.0;  // against the running sum, not the first quaternion (:84-86)
    for (int k = 0; k < 4; ++k) a.q[k] += s * q[k];
    ++a.n;
}

// pose7 out: the identity when nothing was added (:76-78)
CBA_HD void ext_avg_finish(const ExtAvg& a, double* pose7) {
    if (a.n == 0) {
        pose7[0] = 1.0;
        for (int k = 1; k < 7; ++k) pose7[k] = 0.0;
        return;
    }
    const double nrm = sqrt(a.q[0] * a.q[0] + a.q[1] * a.q[1] + a.q[2] * a.q[2] + a.q[3] * a.q[3]);
    for (int k = 0; k < 4; ++k) pose7[k] = nrm > 0.0 ? a.q[k] / nrm : a.q[k];
    const double cnt = static_cast<double>(a.n);
    for (int k = 0; k < 3; ++k) pose7[4 + k] = a.t[k] / cnt;
}

}  // namespace cba
