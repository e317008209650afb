// block_pose.hpp — the block-pose kernel shared by extrinsic_dlt.hip and bundle_seed.hip: one wavefront per block of a blocked
// layout (blk_offset, blk_cam) runs seed_math.hpp::planar_seed_view with the block camera's K, the code k_planar_seed (seed.hip)
// runs, so a block's pose is bitwise what cba_estimate_planar_pose_batch gives.  A template, so both translation units may
// instantiate it.
#pragma once
#include "hip_glue.hpp"
#include "seed_math.hpp"

namespace cba {

constexpr int EXT_WAVES = 4;  // block-pose kernel: wavefronts (blocks) per workgroup

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_ext_block_pose(int n_blocks, const int64_t* __restrict__ off,
                                                               const int32_t* __restrict__ blk_cam, const double* __restrict__ X,
                                                               const double* __restrict__ Y, const double* __restrict__ u,
                                                               const double* __restrict__ v, const double* __restrict__ kmtx5,
                                                               double* __restrict__ pose7, int32_t* __restrict__ ok) {
    const int i = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (i >= n_blocks) return;  // whole wave leaves together
    double K[5], p[7];
    const double* K5 = kmtx5 + 5 * static_cast<int64_t>(blk_cam[i]);
    for (int k = 0; k < 5; ++k) K[k] = K5[k];
    WaveCoop co;
    const bool good = planar_seed_view(static_cast<int>(off[i + 1] - off[i]), X + off[i], Y + off[i], u + off[i], v + off[i], K, co, p);
    if (co.lane() == 0) {
        for (int k = 0; k < 7; ++k) pose7[7 * static_cast<int64_t>(i) + k] = p[k];
        ok[i] = good ? 1 : 0;
    }
}

inline void launch_block_pose(int n_blocks, const int64_t* off, const int32_t* blk_cam, const double* X, const double* Y, const double* u,
                              const double* v, const double* kmtx5, double* pose7, int32_t* ok, hipStream_t stream) {
    hipLaunchKernelGGL(k_ext_block_pose<EXT_WAVES>, dim3((n_blocks + EXT_WAVES - 1) / EXT_WAVES), dim3(64 * EXT_WAVES), 0, stream, n_blocks,
                       off, blk_cam, X, Y, u, v, kmtx5, pose7, ok);
    CBA_HIP(hipGetLastError());
}

}  // namespace cba
