// block_reduce.hpp — fixed-order reductions of a 256-thread workgroup through LDS (device only).
#pragma once
#include <hip/hip_runtime.h>

#include "reproj_math.hpp"

namespace cba {

// out = {sum of c, sum of ss} over the workgroup's 256 threads: one binary tree for both columns (fixed order: bitwise
// reproducible), stored by thread 0.  `out` may be page-locked host memory.
__device__ __forceinline__ void block_sum2(double (*sh)[256], double c, double ss, double* __restrict__ out) {
    sh[0][threadIdx.x] = c;
    sh[1][threadIdx.x] = ss;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (static_cast<int>(threadIdx.x) < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = sh[0][0]; out[1] = sh[1][0]; }
}

// out2 = {1/2 sum rho(s_b), sum s_b} over b = b0 + t, b0 + t + 256, ... < b1; lds: 2 * 256 doubles.  Every cost of the LM step is
// this body: over all blocks (k_cost, k_sys_stage2), or over 2048 of them per workgroup with the pairs added in order afterwards.
__device__ __forceinline__ void cost_range_body(double* lds, int b0, int b1, const double* __restrict__ blk_s, double huber_delta, double* __restrict__ out2) {
    double c = 0.0, ss = 0.0;
    for (int b = b0 + static_cast<int>(threadIdx.x); b < b1; b += 256) {
        double rho, w;
        huber(blk_s[b], huber_delta, &rho, &w);
        c += 0.5 * rho;
        ss += blk_s[b];
    }
    block_sum2(reinterpret_cast<double (*)[256]>(lds), c, ss, out2);
}

}  // namespace cba
