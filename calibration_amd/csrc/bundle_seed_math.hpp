// bundle_seed_math.hpp — the per-lane algebra of the hand-eye / bundle seed (bundle_seed.hip) as __host__ __device__ code:
//   bs_pose_row       one row [Rb(9) tb(3) Rc(9) tc(3)] of a camera's Tsai-Lenz pose table (the layout k_axxb reads): Rb, tb from
//                     the row-major b_T_g of cba_optimize_bundle's layout, Rc from the block pose's quaternion normalised and then
//                     quat_to_rotmat'd, as the single-camera path (handeye.hip, HipAxxb) forms it on the host
//   bs_handeye_pose7  g_T_c from the Tsai-Lenz R_X and t (seed_rotmat_to_quat, as handeye_dlt writes it)
//   bs_candidate      one initial-target candidate b_T_g * g_T_c * c_T_t (choose_initial_target, bundle_utils.cpp:217-227), as
//                     Eigen's Isometry3d products associate it: ((b_T_g * g_T_c) * c_T_t); out: its quaternion (4) and translation (3)
// The candidates are averaged with extrinsic_dlt_math.hpp's ExtAvg (average_isometries with the running-sum sign rule).
#pragma once
#include "extrinsic_dlt_math.hpp"

namespace cba {

CBA_HD void bs_pose_row(const double* bTg12, const double* c_T_t7, double* row) {
    for (int k = 0; k < 12; ++k) row[k] = bTg12[k];
    double nc = 0.0, qc[4];
    for (int a = 0; a < 4; ++a) nc += c_T_t7[a] * c_T_t7[a];
    for (int a = 0; a < 4; ++a) qc[a] = c_T_t7[a] / sqrt(nc);
    quat_to_rotmat(qc, row + 12);
    for (int a = 0; a < 3; ++a) row[21 + a] = c_T_t7[4 + a];
}

CBA_HD void bs_handeye_pose7(const double* RX, const double* t, double* pose7) {
    seed_rotmat_to_quat(RX, pose7);
    for (int k = 0; k < 3; ++k) pose7[4 + k] = t[k];
}

// bTg12: row-major R (9) then t (3); g7, c7: pose7 whose quaternions are read as they are (quat_to_rotmat, no renormalisation)
CBA_HD void bs_candidate(const double* bTg12, const double* g7, const double* c7, double* q, double* t) {
    double Rg[9], Rc[9], M[9], R[9], tg[3];
    quat_to_rotmat(g7, Rg);
    quat_to_rotmat(c7, Rc);
    mat3_mul(bTg12, Rg, M);  // b_T_g * g_T_c = (Rb Rg, Rb tg + tb)
    mat3_vec(bTg12, g7 + 4, tg);
    for (int k = 0; k < 3; ++k) tg[k] += bTg12[9 + k];
    mat3_mul(M, Rc, R);  // ... * c_T_t = (M Rc, M tc + (Rb tg + tb))
    mat3_vec(M, c7 + 4, t);
    for (int k = 0; k < 3; ++k) t[k] += tg[k];
    seed_rotmat_to_quat(R, q);
}

}  // namespace cba
