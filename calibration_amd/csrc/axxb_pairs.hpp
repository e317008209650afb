// axxb_pairs.hpp — the workgroup bodies of the all-pairs AX = XB kernels (device only), shared by handeye.hip (one pose list) and
// bundle_seed.hip (one pose list per camera, all cameras in one launch), so both reduce a pose list's pairs in the same order.
//   axxb_pair_tile    256 lanes = the pairs (i, j) for one first pose i and 256 consecutive j; pairs with j <= i or j >= n are
//                     zero.  The 29 sums of the tile (wave_sum63 per wave, then (w0 + w1) + (w2 + w3)) go to one partial row.
//   axxb_rows_sum     the sum of rows [t0, t1) of a [rows][AXXB_NACC] table: thread (column e, group r) adds rows t0 + r, + 8, ...,
//                     the 8 group sums are combined in group order through LDS.
#pragma once
#include "wave_reduce.hpp"  // first: brings in the HIP runtime the CBA_HD headers need
#include "axxb_math.hpp"

namespace cba {

// MODE 0: the AX = XB residual blocks of optimize_handeye; MODE 1 / 2: the rotation / translation sums of the Tsai-Lenz
// all-pairs seed estimate_handeye_dlt (handeyedlt.cpp:84-137) — same pair enumeration, same filter, same reduction.
template <int MODE>
__device__ __forceinline__ void axxb_pair_tile(int n, const double* __restrict__ poses /*[n][24]: Rb tb Rc tc*/,
                                               const double* __restrict__ X /*RX(9) tX(3)*/, double min_angle, double axis_eps,
                                               double huber_delta, int i, int j, double (*sh)[AXXB_NACC], double* __restrict__ row) {
    double acc[AXXB_NACC];
#pragma unroll
    for (int e = 0; e < AXXB_NACC; ++e) acc[e] = 0.0;
    if (j > i && j < n) {
        const double* pi = poses + 24 * static_cast<int64_t>(i);
        const double* pj = poses + 24 * static_cast<int64_t>(j);
        double RA[9], RB[9], tA[3], tB[3];
        if (motion_pair(pi, pi + 9, pj, pj + 9, pi + 12, pi + 21, pj + 12, pj + 21, min_angle, axis_eps, RA, RB, tA, tB)) {
            if (MODE == 0) {
                double r[6], J[36];
                axxb_point(X, X + 9, RA, RB, tA, tB, r, J);
                axxb_accumulate(r, J, huber_delta, acc);
            } else {
                tsai_lenz_accumulate(MODE - 1, RA, RB, tA, tB, X, acc);
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < AXXB_NACC; ++e) {
        const double v = wave_sum63(acc[e]);
        if (lane == 63) sh[wave][e] = v;
    }
    __syncthreads();
    if (threadIdx.x < AXXB_NACC) row[threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

__device__ __forceinline__ void axxb_rows_sum(int64_t t0, int64_t t1, const double* __restrict__ rows, double (*sh)[32],
                                              double* __restrict__ out) {
    const int e = threadIdx.x & 31, r = threadIdx.x >> 5;
    double s = 0.0;
    if (e < AXXB_NACC)
        for (int64_t t = t0 + r; t < t1; t += 8) s += rows[t * AXXB_NACC + e];
    sh[r][e] = s;
    __syncthreads();
    if (r == 0 && e < AXXB_NACC) {
        double tot = 0.0;
        for (int k = 0; k < 8; ++k) tot += sh[k][e];
        out[e] = tot;
    }
}

}  // namespace cba
