// bundle_seed.hip — the seed of the hand-eye and bundle stages on the GPU: every camera's all-pairs Tsai-Lenz g_T_c
// (compute_handeye_initialization, src/pipeline/detail/bundle_utils.cpp:154-200, with estimate_handeye_dlt, handeyedlt.cpp:126-137)
// and the initial target b_T_t (choose_initial_target, bundle_utils.cpp:202-237), on the blocked layout of cba_optimize_bundle.
// One stream, one synchronise:
//   k_ext_block_pose    one wavefront per block: planar_seed_view with the block camera's K (block_pose.hpp, shared with
//                       extrinsic_dlt.hip), so a block's pose is bitwise what cba_estimate_planar_pose_batch gives
//   k_bs_pose_table     one lane per listed block: the [Rb tb Rc tc] row of its camera's pose table (bundle_seed_math.hpp)
//   k_bs_pairs<1>       one workgroup per (camera, first pose i, 256 second poses) of every DLT camera at once: axxb_pair_tile
//                       (axxb_pairs.hpp), the tile k_axxb runs, with the tiling of the single-camera path inside each camera
//   k_bs_chunk_sum/_total   the two fixed-order levels of k_axxb_chunk_sum, per camera: cameras never share a partial row
//   k_bs_rot_solve      one lane per DLT camera: NO_PAIRS / ridge solve / exp_so3
//   k_bs_pairs<2> + sums    the translation sums at each camera's R_X, then k_bs_trans_solve writes g_T_c
//   k_bs_candidates     one lane per listed block: b_T_g * g_T_c[cam] * c_T_t (camera-major, then list order)
//   k_bs_scan           one wavefront: the sequential sign-rule quaternion sum over 64-candidate chunks staged in LDS, the next
//                       chunk's loads in flight meanwhile; the translations summed in parallel in a fixed order
// A camera's list (cam_start / cam_blk, built by the caller) is its blocks of >= 4 points in increasing block index: the order the
// reference's SensorAccumulator receives them in.
#include <algorithm>
#include <vector>

#include "axxb_pairs.hpp"
#include "block_pose.hpp"
#include "bundle_seed_math.hpp"
#include "pipelines.hpp"

namespace cba {

namespace {
struct BsCam {       // one camera that gets the DLT
    int32_t cam;     // camera index
    int32_t first;   // its first row in the pose table (= cam_start[cam])
    int32_t n;       // its listed blocks (>= 2)
    int32_t gx;      // (n + 255) / 256: workgroups per first pose, as HipAxxb tiles one pose list
};
}  // namespace

// the d with bound[d] <= w < bound[d + 1] (bound strictly increasing, bound[0] = 0)
__device__ __forceinline__ int bs_find(const int64_t* __restrict__ bound, int n, int64_t w) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bound[mid] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_bs_pose_table(int n_list, const int32_t* __restrict__ cam_blk, const double* __restrict__ bTg,
                                                       const double* __restrict__ pose7, double* __restrict__ table) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_list) return;
    const int64_t b = cam_blk[k];
    bs_pose_row(bTg + 12 * b, pose7 + 7 * b, table + 24 * static_cast<int64_t>(k));
}

// workgroup w = row w of the partial table; camera d owns rows [row_bound[d], row_bound[d + 1]) = (i, jx) in i-major order
template <int MODE>
__global__ __launch_bounds__(256) void k_bs_pairs(int n_dlt, const BsCam* __restrict__ cams, const int64_t* __restrict__ row_bound,
                                                  const double* __restrict__ table, const double* __restrict__ Xs, double min_angle,
                                                  double* __restrict__ partial) {
    __shared__ double sh[4][AXXB_NACC];
    const int64_t w = blockIdx.x;
    const int d = bs_find(row_bound, n_dlt, w);
    const BsCam c = cams[d];
    const int64_t r = w - row_bound[d];
    const int i = static_cast<int>(r / c.gx), jx = static_cast<int>(r % c.gx);
    axxb_pair_tile<MODE>(c.n, table + 24 * static_cast<int64_t>(c.first), Xs + 12 * static_cast<int64_t>(c.cam), min_angle, 1e-3, 0.0, i,
                         jx * 256 + static_cast<int>(threadIdx.x), sh, partial + w * AXXB_NACC);
}

// level 1: chunk w of camera d sums its rows [row_bound[d] + 64 k, ...) clipped to the camera's rows
__global__ __launch_bounds__(256) void k_bs_chunk_sum(int n_dlt, const int64_t* __restrict__ row_bound, const int64_t* __restrict__ chunk_bound,
                                                      const double* __restrict__ partial, double* __restrict__ partial2) {
    __shared__ double sh[8][32];
    const int64_t w = blockIdx.x;
    const int d = bs_find(chunk_bound, n_dlt, w);
    const int64_t t0 = row_bound[d] + 64 * (w - chunk_bound[d]), t1 = min(t0 + 64, row_bound[d + 1]);
    axxb_rows_sum(t0, t1, partial, sh, partial2 + w * AXXB_NACC);
}

// level 2: workgroup d sums camera d's chunk sums as one chunk
__global__ __launch_bounds__(256) void k_bs_chunk_total(const int64_t* __restrict__ chunk_bound, const double* __restrict__ partial2,
                                                        double* __restrict__ sums) {
    __shared__ double sh[8][32];
    const int d = blockIdx.x;
    axxb_rows_sum(chunk_bound[d], chunk_bound[d + 1], partial2, sh, sums + static_cast<int64_t>(d) * AXXB_NACC);
}

__global__ void k_bs_rot_solve(int n_dlt, const BsCam* __restrict__ cams, const double* __restrict__ sums, double* __restrict__ Xs,
                               int32_t* __restrict__ status, int32_t* __restrict__ pairs) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_dlt) return;
    const int c = cams[d].cam;
    const double* acc = sums + static_cast<int64_t>(d) * AXXB_NACC;
    pairs[c] = static_cast<int32_t>(acc[9] + 0.5);
    double w[3];
    if (acc[9] < 0.5) {  // handeyedlt.cpp:76-79
        status[c] = CBA_HANDEYE_NO_PAIRS;
    } else if (!tsai_lenz_solve(acc, 1e-12, w)) {
        status[c] = CBA_HANDEYE_SINGULAR;
    } else {
        exp_so3(w, Xs + 12 * static_cast<int64_t>(c));
        status[c] = CBA_HANDEYE_DLT;
    }
}

__global__ void k_bs_trans_solve(int n_dlt, const BsCam* __restrict__ cams, const double* __restrict__ sums, const double* __restrict__ Xs,
                                 int32_t* __restrict__ status, double* __restrict__ g7) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_dlt) return;
    const int c = cams[d].cam;
    double t[3];
    double* out = g7 + 7 * static_cast<int64_t>(c);
    if (status[c] == CBA_HANDEYE_DLT && !tsai_lenz_solve(sums + static_cast<int64_t>(d) * AXXB_NACC, 1e-12, t)) status[c] = CBA_HANDEYE_SINGULAR;
    if (status[c] == CBA_HANDEYE_DLT) {
        bs_handeye_pose7(Xs + 12 * static_cast<int64_t>(c), t, out);
    } else {  // a failed seed keeps the identity (compute_handeye_initialization, bundle_utils.cpp:163)
        out[0] = 1.0;
        for (int k = 1; k < 7; ++k) out[k] = 0.0;
    }
}

__global__ __launch_bounds__(256) void k_bs_candidates(int n_list, const int32_t* __restrict__ cam_blk, const int32_t* __restrict__ blk_cam,
                                                       const double* __restrict__ bTg, const double* __restrict__ pose7,
                                                       const double* __restrict__ g7, double* __restrict__ cq, double* __restrict__ ct) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_list) return;
    const int64_t b = cam_blk[k];
    bs_candidate(bTg + 12 * b, g7 + 7 * static_cast<int64_t>(blk_cam[b]), pose7 + 7 * b, cq + 4 * static_cast<int64_t>(k),
                 ct + 3 * static_cast<int64_t>(k));
}

// average_isometries over the n candidates in order (one wavefront of 64 lanes).  Only the quaternion sum is sequential (each
// candidate's sign against the running sum, se3_utils.h:84-86).  The candidates go through LDS in chunks of 64: lane l loads
// candidate base + 64 + l while the chain walks the chunk at base, so the memory round trip overlaps 64 steps of the chain and
// the chain's own reads are LDS broadcasts that do not depend on it.  The translations are summed off the chain, lane l over
// candidates l, l + 64, ... and then the 64 lane sums in a fixed DPP order (wave_sum63).
__global__ __launch_bounds__(64) void k_bs_scan(int n, const double* __restrict__ cq, const double* __restrict__ ct, double* __restrict__ out7) {
    __shared__ double sq[64 * 4];
    const int lane = threadIdx.x;
    ExtAvg acc;
    ext_avg_init(acc);
    double r[4] = {0.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
    if (lane < n)
        for (int e = 0; e < 4; ++e) r[e] = cq[4 * lane + e];
    for (int base = 0; base < n; base += 64) {
        for (int e = 0; e < 4; ++e) sq[4 * lane + e] = r[e];
        __syncthreads();
        const int64_t nxt = static_cast<int64_t>(base) + 64 + lane;  // the next chunk's loads, in flight during this chunk
        if (nxt < n)
            for (int e = 0; e < 4; ++e) r[e] = cq[4 * nxt + e];
        if (base + lane < n)
            for (int e = 0; e < 3; ++e) t[e] += ct[3 * (static_cast<int64_t>(base) + lane) + e];
        const int m = min(64, n - base);
#pragma unroll 8
        for (int s = 0; s < m; ++s) {
            const double* q = sq + 4 * s;
            const double dot = acc.q[0] * q[0] + acc.q[1] * q[1] + acc.q[2] * q[2] + acc.q[3] * q[3];
            const double sg = dot < 0.0 ? -1.0 : 1.0;
            for (int e = 0; e < 4; ++e) acc.q[e] += sg * q[e];
        }
        __syncthreads();  // the chunk is consumed before the next one overwrites it
    }
    for (int e = 0; e < 3; ++e) acc.t[e] = wave_sum63(t[e]);  // the total lands in lane 63
    acc.n = n;
    if (lane == 63) ext_avg_finish(acc, out7);
}

// ---- host glue -----------------------------------------------------------------------------------------------------------
void bundle_seed_gpu(int n_cams, int n_blocks, const int64_t* blk_offset, const int32_t* blk_cam, const double* blk_b_T_g, const double* X,
                     const double* Y, const double* u, const double* v, const double* kmtx5, double min_angle_deg, const int32_t* cam_start,
                     const int32_t* cam_blk, double* g_T_c, int32_t* cam_status, int32_t* cam_pairs, const double* b_T_t_given,
                     double* b_T_t, double* blk_pose, int32_t* blk_ok, double* stage_ms, int device) {
    // the cameras that get the DLT, and their row / chunk ranges in the partial tables
    std::vector<BsCam> cams;
    std::vector<int64_t> row_bound{0}, chunk_bound{0};
    for (int c = 0; c < n_cams; ++c) {
        if (cam_status[c] != CBA_HANDEYE_DLT) continue;
        const int n = cam_start[c + 1] - cam_start[c];
        const int gx = (n + 255) / 256;
        const int64_t rows = static_cast<int64_t>(gx) * (n - 1);
        cams.push_back(BsCam{c, cam_start[c], n, gx});
        row_bound.push_back(row_bound.back() + rows);
        chunk_bound.push_back(chunk_bound.back() + (rows + 63) / 64);
        cam_pairs[c] = 0;
    }
    const int n_dlt = static_cast<int>(cams.size());
    const int n_list = cam_start[n_cams];
    const int64_t n_rows = row_bound.back(), n_chunks = chunk_bound.back();
    if (n_rows > 0x7fffffffLL) throw std::invalid_argument("too many pose pairs for one launch");

    StreamLease lease(device);
    const hipStream_t stream = lease;
    {
        StageTimer<6> tm(stream, stage_ms != nullptr);  // device events between the stages
        const size_t nb = static_cast<size_t>(n_blocks), nc = static_cast<size_t>(n_cams), nl = static_cast<size_t>(std::max(n_list, 1));
        ObsSoA d;
        DevBuf<double> dK, dB, dP, dT, dXs, dG, dPart, dPart2, dSum, dCq, dCt, dOut;
        DevBuf<int64_t> drow, dchunk;
        DevBuf<int32_t> dcam, dok, dlist, dstat, dpairs;
        DevBuf<BsCam> dcams;
        d.upload(stream, n_blocks, blk_offset, X, Y, u, v);
        dP.alloc(7 * nb); dok.alloc(nb); dT.alloc(24 * nl); dCq.alloc(4 * nl); dCt.alloc(3 * nl); dOut.alloc(7);
        dPart.alloc(static_cast<size_t>(std::max<int64_t>(n_rows, 1)) * AXXB_NACC);
        dPart2.alloc(static_cast<size_t>(std::max<int64_t>(n_chunks, 1)) * AXXB_NACC);
        dSum.alloc(static_cast<size_t>(std::max(n_dlt, 1)) * AXXB_NACC);
        dK.assign(kmtx5, 5 * nc, stream);
        dB.assign(blk_b_T_g, 12 * nb, stream);
        dcam.assign(blk_cam, nb, stream);
        dlist.assign(cam_blk, static_cast<size_t>(n_list), stream);
        std::vector<double> xs(12 * nc, 0.0);  // R_X = I until the rotation solve
        for (size_t c = 0; c < nc; ++c) xs[12 * c] = xs[12 * c + 4] = xs[12 * c + 8] = 1.0;
        dXs.assign(xs.data(), xs.size(), stream);
        dG.assign(g_T_c, 7 * nc, stream);  // given / identity rows; the DLT cameras' rows are overwritten
        dstat.assign(cam_status, nc, stream);
        dpairs.assign(cam_pairs, nc, stream);
        dcams.assign(cams.data(), cams.size(), stream);
        drow.assign(row_bound.data(), row_bound.size(), stream);
        dchunk.assign(chunk_bound.data(), chunk_bound.size(), stream);
        const double min_angle = min_angle_deg * 3.14159265358979323846 / 180.0;  // as handeye_dlt converts it
        const unsigned list_grid = static_cast<unsigned>((n_list + 255) / 256), dlt_grid = static_cast<unsigned>((n_dlt + 63) / 64);
        auto sums = [&]() {
            hipLaunchKernelGGL(k_bs_chunk_sum, dim3(static_cast<unsigned>(n_chunks)), dim3(256), 0, stream, n_dlt, drow.p, dchunk.p, dPart.p, dPart2.p);
            hipLaunchKernelGGL(k_bs_chunk_total, dim3(static_cast<unsigned>(n_dlt)), dim3(256), 0, stream, dchunk.p, dPart2.p, dSum.p);
        };

        tm.mark(0);
        launch_block_pose(n_blocks, d.off.p, dcam.p, d.X.p, d.Y.p, d.u.p, d.v.p, dK.p, dP.p, dok.p, stream);
        tm.mark(1);
        if (n_list > 0) hipLaunchKernelGGL(k_bs_pose_table, dim3(list_grid), dim3(256), 0, stream, n_list, dlist.p, dB.p, dP.p, dT.p);
        if (n_dlt > 0) {
            hipLaunchKernelGGL(k_bs_pairs<1>, dim3(static_cast<unsigned>(n_rows)), dim3(256), 0, stream, n_dlt, dcams.p, drow.p, dT.p, dXs.p,
                               min_angle, dPart.p);
            sums();
            hipLaunchKernelGGL(k_bs_rot_solve, dim3(dlt_grid), dim3(64), 0, stream, n_dlt, dcams.p, dSum.p, dXs.p, dstat.p, dpairs.p);
        }
        CBA_HIP(hipGetLastError());
        tm.mark(2);
        if (n_dlt > 0) {
            hipLaunchKernelGGL(k_bs_pairs<2>, dim3(static_cast<unsigned>(n_rows)), dim3(256), 0, stream, n_dlt, dcams.p, drow.p, dT.p, dXs.p,
                               min_angle, dPart.p);
            sums();
            hipLaunchKernelGGL(k_bs_trans_solve, dim3(dlt_grid), dim3(64), 0, stream, n_dlt, dcams.p, dSum.p, dXs.p, dstat.p, dG.p);
        }
        CBA_HIP(hipGetLastError());
        tm.mark(3);
        const bool scan = !b_T_t_given && n_list > 0;
        if (scan)
            hipLaunchKernelGGL(k_bs_candidates, dim3(list_grid), dim3(256), 0, stream, n_list, dlist.p, dcam.p, dB.p, dP.p, dG.p, dCq.p, dCt.p);
        tm.mark(4);
        if (scan) hipLaunchKernelGGL(k_bs_scan, dim3(1), dim3(64), 0, stream, n_list, dCq.p, dCt.p, dOut.p);
        CBA_HIP(hipGetLastError());
        tm.mark(5);
        dG.download(g_T_c, 7 * nc, stream);
        dstat.download(cam_status, nc, stream);
        dpairs.download(cam_pairs, nc, stream);
        if (scan) dOut.download(b_T_t, 7, stream);
        if (blk_pose) dP.download(blk_pose, 7 * nb, stream);
        if (blk_ok) dok.download(blk_ok, nb, stream);
        CBA_HIP(hipStreamSynchronize(stream));
        if (stage_ms) {  // stage_ms [6]: block poses, pass 1 + solve, pass 2 + solve, candidates + scan, total, scan alone
            stage_ms[0] = tm.ms(0, 1);
            stage_ms[1] = tm.ms(1, 2);
            stage_ms[2] = tm.ms(2, 3);
            stage_ms[3] = tm.ms(3, 5);
            stage_ms[4] = tm.ms(0, 5);
            stage_ms[5] = tm.ms(4, 5);
        }
    }
}

}  // namespace cba
