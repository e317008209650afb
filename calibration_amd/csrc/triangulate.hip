// triangulate.hip — multi-camera triangulation on the GPU (tri_math.hpp, calibba.h: cba_triangulate).  One stream, one
// synchronise per call:
//   k_triangulate<MODEL, COV>  one lane per point, 256-thread blocks.  The whole per-point procedure (ray seed, LM refinement,
//                              outlier restarts, final statistics, covariance) is tri_point in the lane's registers: X, H (6), g (3),
//                              lambda, cost and the camera set as a bit mask.  Pixels are camera-major, so each camera's pixel is
//                              one coalesced 16-byte load per lane; they are read again by every linearisation instead of being held
//                              in up to 32 registers.  The camera table is indexed by the loop counter alone,
//                              which is wave-uniform: its reads are scalar loads, as in k_cam_map.  Lanes that finish early idle
//                              until the last lane of their wavefront is done; no lane reads or writes another's data and there
//                              are no atomics, so a point's result does not depend on its neighbours.
#include <vector>

#include "pipelines.hpp"
#include "tri_math.hpp"

namespace cba {

constexpr int TRI_BLOCK = 256;

template <int MODEL, bool COV>
__global__ __launch_bounds__(TRI_BLOCK) void k_triangulate(int64_t n, int n_cams, const TriCamera* __restrict__ cams,
                                                           const double* __restrict__ uv, cba_triangulate_options o,
                                                           double* __restrict__ xyz, double* __restrict__ rms,
                                                           uint32_t* __restrict__ used_mask, int32_t* __restrict__ status,
                                                           double* __restrict__ cov6, int32_t* __restrict__ linearisations) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(TRI_BLOCK) + threadIdx.x;
    if (i >= n) return;
    TriResult r;
    tri_point<MODEL, COV>(cams, n_cams, uv + 2 * i, 2 * n, o, &r);
    xyz[3 * i] = r.X[0];
    xyz[3 * i + 1] = r.X[1];
    xyz[3 * i + 2] = r.X[2];
    rms[i] = r.rms;
    used_mask[i] = r.mask;
    status[i] = r.status;
    if (COV) {
#pragma unroll
        for (int j = 0; j < 6; ++j) cov6[6 * i + j] = r.cov[j];
    }
    if (linearisations) linearisations[i] = r.linearisations;
}

// stage_ms [3] (experiment builds): upload, kernel, download.  linearisations [n] optional (the bench tool's per-point counts).
void triangulate_gpu(int model, int n_cams, const double* intr, int n_inv, const double* inv, const double* c_T_r, int64_t n,
                     const double* uv, const cba_triangulate_options& o, double* xyz, double* rms_px, uint32_t* used_mask, int32_t* status,
                     double* cov6, int32_t* linearisations, double* stage_ms, int device) {
    const int ni = cam_intr_size(model);
    std::vector<TriCamera> hc(n_cams);
    for (int c = 0; c < n_cams; ++c)
        tri_fill_camera(model, intr + static_cast<size_t>(c) * ni, n_inv, inv ? inv + static_cast<size_t>(c) * n_inv : nullptr,
                        c_T_r + 7 * static_cast<size_t>(c), &hc[c]);
    StreamLease lease(device);
    const hipStream_t s = lease;
    StageTimer<4> tm(s, stage_ms != nullptr);
    const size_t np = static_cast<size_t>(n);
    DevBuf<TriCamera> dcams;
    DevBuf<double> duv, dxyz, drms, dcov;
    DevBuf<uint32_t> dmask;
    DevBuf<int32_t> dstatus, dlin;
    dcams.alloc(n_cams);
    duv.alloc(2 * np * n_cams);
    dxyz.alloc(3 * np);
    drms.alloc(np);
    dmask.alloc(np);
    dstatus.alloc(np);
    if (cov6) dcov.alloc(6 * np);
    if (linearisations) dlin.alloc(np);
    tm.mark(0);
    dcams.upload(hc.data(), n_cams, s);
    duv.upload(uv, 2 * np * n_cams, s);
    tm.mark(1);
    const dim3 grid(static_cast<unsigned>((n + TRI_BLOCK - 1) / TRI_BLOCK));
#define TRI_LAUNCH(MODEL, COV)                                                                                                  \
    hipLaunchKernelGGL((k_triangulate<MODEL, COV>), grid, dim3(TRI_BLOCK), 0, s, n, n_cams, dcams.p, duv.p, o, dxyz.p, drms.p, dmask.p, \
                       dstatus.p, dcov.p, dlin.p)
    if (model == CAM_SCHEIMPFLUG) {
        if (cov6) TRI_LAUNCH(CAM_SCHEIMPFLUG, true); else TRI_LAUNCH(CAM_SCHEIMPFLUG, false);
    } else {
        if (cov6) TRI_LAUNCH(CAM_PINHOLE_BC, true); else TRI_LAUNCH(CAM_PINHOLE_BC, false);
    }
#undef TRI_LAUNCH
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    dxyz.download(xyz, 3 * np, s);
    dstatus.download(status, np, s);
    if (rms_px) drms.download(rms_px, np, s);
    if (used_mask) dmask.download(used_mask, np, s);
    if (cov6) dcov.download(cov6, 6 * np, s);
    if (linearisations) dlin.download(linearisations, np, s);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));  // hc and the device buffers go out of scope
    tm.report(stage_ms);
}

}  // namespace cba
