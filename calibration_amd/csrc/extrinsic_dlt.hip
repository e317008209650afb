// extrinsic_dlt.hip — estimate_extrinsic_dlt (include/calib/estimation/linear/extrinsics.h:27-78) for an N-camera rig on the GPU:
// the linear seed of optimize_extrinsics (cba_optimize_extrinsics), on the same blocked layout.  Three kernels on one stream:
//   k_ext_block_pose   one wavefront per (view, camera) block: seed_math.hpp::planar_seed_view with the block's camera K, the
//                      code k_planar_seed (seed.hip) runs, so a block's pose is bitwise what cba_estimate_planar_pose_batch gives
//                      (block_pose.hpp, shared with bundle_seed.hip)
//   k_ext_cam_avg      one workgroup per camera c >= 1: lanes form T[v][c] T[v][0]^-1 and its quaternion for a chunk of views,
//                      lane 0 then adds the chunk to the running sign-aligned sum in increasing view order (LDS hand-off)
//   k_ext_target_avg   one lane per view: c_T_r[c]^-1 T[v][c] averaged over cameras in increasing c
// Blocks are found through a dense [n_views][n_cams] table (block index or -1) built and checked on the host, so the averaging
// order comes from (view, camera) and never from the order the blocks are listed in.
#include <vector>

#include "block_pose.hpp"
#include "pipelines.hpp"
#include "extrinsic_dlt_math.hpp"

namespace cba {

constexpr int EXT_CHUNK = 256;  // camera-average kernel: views per chunk = lanes per workgroup; target kernel: views per workgroup

// block b of (view, cam), or -1 when it is absent or has fewer than 4 points (the reference's skip rule, extrinsics.h:57, 68)
__device__ __forceinline__ int ext_block(const int32_t* __restrict__ table, const int64_t* __restrict__ off, int n_cams, int view, int cam) {
    const int b = table[static_cast<int64_t>(view) * n_cams + cam];
    return (b >= 0 && off[b + 1] - off[b] >= 4) ? b : -1;
}

__global__ __launch_bounds__(EXT_CHUNK) void k_ext_cam_avg(int n_views, int n_cams, const int32_t* __restrict__ table,
                                                          const int64_t* __restrict__ off, const double* __restrict__ pose7,
                                                          double* __restrict__ c_T_r) {
    const int c = blockIdx.x;
    const int lane = threadIdx.x;
    if (c == 0) {  // c_se3_r[0] = I (:55)
        if (lane < 7) c_T_r[lane] = lane == 0 ? 1.0 : 0.0;
        return;  // uniform over the workgroup
    }
    __shared__ double sq[EXT_CHUNK * 4], st[EXT_CHUNK * 3];
    __shared__ int sok[EXT_CHUNK];
    ExtAvg acc;
    ext_avg_init(acc);
    for (int v0 = 0; v0 < n_views; v0 += EXT_CHUNK) {
        const int vi = v0 + lane;
        int good = 0;
        if (vi < n_views) {
            const int b0 = ext_block(table, off, n_cams, vi, 0), bc = ext_block(table, off, n_cams, vi, c);
            if (b0 >= 0 && bc >= 0) {
                ext_rel_pose(pose7 + 7 * static_cast<int64_t>(bc), pose7 + 7 * static_cast<int64_t>(b0), sq + 4 * lane, st + 3 * lane);
                good = 1;
            }
        }
        sok[lane] = good;
        __syncthreads();
        if (lane == 0) {
            const int m = min(EXT_CHUNK, n_views - v0);
            for (int k = 0; k < m; ++k)
                if (sok[k]) ext_avg_add(acc, sq + 4 * k, st + 3 * k);
        }
        __syncthreads();  // the chunk is consumed before the next one overwrites it
    }
    if (lane == 0) ext_avg_finish(acc, c_T_r + 7 * static_cast<int64_t>(c));
}

__global__ __launch_bounds__(EXT_CHUNK) void k_ext_target_avg(int n_views, int n_cams, const int32_t* __restrict__ table,
                                                             const int64_t* __restrict__ off, const double* __restrict__ pose7,
                                                             const double* __restrict__ c_T_r, double* __restrict__ r_T_t) {
    const int vi = blockIdx.x * EXT_CHUNK + threadIdx.x;
    if (vi >= n_views) return;
    ExtAvg acc;
    ext_avg_init(acc);
    for (int c = 0; c < n_cams; ++c) {
        const int b = ext_block(table, off, n_cams, vi, c);
        if (b < 0) continue;
        double Rc[9], q[4], t[3];
        const double* cr = c_T_r + 7 * static_cast<int64_t>(c);
        quat_to_rotmat(cr, Rc);
        ext_inv_mul(Rc, cr + 4, pose7 + 7 * static_cast<int64_t>(b), q, t);
        ext_avg_add(acc, q, t);
    }
    ext_avg_finish(acc, r_T_t + 7 * static_cast<int64_t>(vi));
}

// ---- host glue -----------------------------------------------------------------------------------------------------------
void extrinsic_dlt_gpu(int n_cams, int n_views, int n_blocks, const int64_t* blk_offset, const int32_t* blk_cam, const int32_t* table,
                       const double* X, const double* Y, const double* u, const double* v, const double* kmtx5, double* c_T_r,
                       double* r_T_t, double* blk_pose, int32_t* blk_ok, double* stage_ms, int device) {
    StreamLease lease(device);
    const hipStream_t stream = lease;
    {
        StageTimer<4> tm(stream, stage_ms != nullptr);  // device events between the stages
        ObsSoA d;
        DevBuf<double> dK, dP, dC, dR;
        DevBuf<int32_t> dcam, dtab, dok;
        d.upload(stream, n_blocks, blk_offset, X, Y, u, v);
        dP.alloc(7 * static_cast<size_t>(n_blocks)); dok.alloc(n_blocks);
        dC.alloc(7 * static_cast<size_t>(n_cams)); dR.alloc(7 * static_cast<size_t>(n_views));
        dK.assign(kmtx5, 5 * static_cast<size_t>(n_cams), stream);
        dcam.assign(blk_cam, n_blocks, stream);
        dtab.assign(table, static_cast<size_t>(n_views) * static_cast<size_t>(n_cams), stream);
        tm.mark(0);
        launch_block_pose(n_blocks, d.off.p, dcam.p, d.X.p, d.Y.p, d.u.p, d.v.p, dK.p, dP.p, dok.p, stream);
        tm.mark(1);
        hipLaunchKernelGGL(k_ext_cam_avg, dim3(n_cams), dim3(EXT_CHUNK), 0, stream, n_views, n_cams, dtab.p, d.off.p, dP.p, dC.p);
        CBA_HIP(hipGetLastError());
        tm.mark(2);
        hipLaunchKernelGGL(k_ext_target_avg, dim3((n_views + EXT_CHUNK - 1) / EXT_CHUNK), dim3(EXT_CHUNK), 0, stream, n_views, n_cams,
                           dtab.p, d.off.p, dP.p, dC.p, dR.p);
        CBA_HIP(hipGetLastError());
        tm.mark(3);
        dC.download(c_T_r, 7 * static_cast<size_t>(n_cams), stream);
        dR.download(r_T_t, 7 * static_cast<size_t>(n_views), stream);
        if (blk_pose) dP.download(blk_pose, 7 * static_cast<size_t>(n_blocks), stream);
        if (blk_ok) dok.download(blk_ok, n_blocks, stream);
        CBA_HIP(hipStreamSynchronize(stream));
        tm.report(stage_ms);  // stage_ms [4]: block poses, camera averages, target averages ...
        if (stage_ms) stage_ms[3] = tm.ms(0, 3);  // ... and the total
    }
}

}  // namespace cba
