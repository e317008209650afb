// hom_ransac.hip — the linear seed of planar intrinsic calibration on the GPU: estimate_homography with RansacOptions
// (src/estimation/optim/homography.cpp:45-60 -> ransac<HomographyEstimator>, common/ransac.h:121-194) for a batch of views, and
// estimate_intrinsics (src/estimation/linear/intrinsicsdlt.cpp:101-145) as one device pipeline.  Device math: hom_ransac_math.hpp.
//
//   k_hr_score    grid (view, block of 256 hypotheses): one lane per hypothesis.  The lane draws its 4-point sample, rejects a
//                 near-collinear one, fits the minimal homography, then walks the view's points (staged tile by tile in LDS,
//                 every lane reading the same address) in up to four passes:
//                   1. raw inliers: count and the sums of their object / image points (the refit's centroids);
//                   2. mean distances to those centroids (Hartley scales);            } refit_on_inliers and >= 4 inliers
//                   3. the 24 moments of the normalised DLT Gram;                      }
//                   4. inliers of the final model (the refit, or the raw model when the refit fails or is off): count, sum r^2.
//                 Hypotheses below min_inliers drop out.  The block keeps its best lane by (count desc, rms asc, k asc) and
//                 writes one candidate record [HR_CAND].
//   k_hr_dlt      (no RANSAC) one wavefront per view: dlt_homography_view over all points -> one candidate record.
//   k_hr_finish   one workgroup per view: the best candidate in block order (the reference's strict "first best wins" loop),
//                 the optional h22 rescale, the inlier mask and symmetric_rms_px (a sum of r, not r^2: intrinsicsdlt.cpp:21-30).
//   k_hr_zhang    one lane: Zhang's 6 x 6 Gram over the successful views in view order, K, sanitize_intrinsics.
//   k_hr_pose     one lane per view: pose_from_homography with the sanitised K.
//
// Every reduction runs in a fixed order and every grid depends only on the input sizes: two identical calls are bitwise
// identical, and a view's result does not depend on the other views of the batch.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pipelines.hpp"
#include "hom_ransac_math.hpp"

namespace cba {

constexpr int HR_BLOCK = 256;
constexpr int HR_TILE = 1024;  // points per LDS tile of the scoring kernel (4 x 8 KiB)
constexpr int HR_VIEW_WAVES = 4;
// candidate record: valid, inlier count, inlier rms, hypothesis index, H (9, row-major)
enum { HC_VALID = 0, HC_CNT = 1, HC_RMS = 2, HC_K = 3, HC_H = 4, HR_CAND = 13 };
// kst: the Zhang stage's result
enum { KS_OK = 0, KS_MOD = 1, KS_K = 2, KS_SIZE = 7 };
enum { HM_0, HM_SCORE, HM_HOM, HM_ZHANG, HM_POSE, HR_NMARKS };

// f(x, y, u, v) for every point of the view, in point order, from LDS tiles.  Called by every thread of the block.
template <class F>
__device__ __forceinline__ void hr_tiles(int n, const double* __restrict__ X, const double* __restrict__ Y, const double* __restrict__ u,
                                         const double* __restrict__ v, double* sX, double* sY, double* su, double* sv, F&& f) {
    for (int t0 = 0; t0 < n; t0 += HR_TILE) {
        const int cnt = min(HR_TILE, n - t0);
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += HR_BLOCK) {
            sX[j] = X[t0 + j]; sY[j] = Y[t0 + j]; su[j] = u[t0 + j]; sv[j] = v[t0 + j];
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) f(sX[j], sY[j], su[j], sv[j]);
    }
}

// is_better_model (ransac.h:113-119) over (valid, count, rms) with the lower hypothesis index winning ties: a total order
__device__ __forceinline__ bool hr_better(bool va, double ca, double ra, int ka, bool vb, double cb, double rb, int kb) {
    if (va != vb) return va;
    if (ca != cb) return ca > cb;
    if (ra != rb) return ra < rb;
    return ka < kb;
}

__global__ __launch_bounds__(HR_BLOCK) void k_hr_score(int H, double thresh, int min_inliers, int refit, uint64_t seed,
                                                      const int64_t* __restrict__ off, const double* __restrict__ X,
                                                      const double* __restrict__ Y, const double* __restrict__ u,
                                                      const double* __restrict__ v, double* __restrict__ cand) {
    __shared__ double sX[HR_TILE], sY[HR_TILE], su[HR_TILE], sv[HR_TILE];
    __shared__ double rc[HR_BLOCK], rr[HR_BLOCK];
    __shared__ int rk[HR_BLOCK], rv[HR_BLOCK];
    const int view = blockIdx.x;
    const int k = blockIdx.y * HR_BLOCK + threadIdx.x;
    const int64_t o = off[view];
    const int n = static_cast<int>(off[view + 1] - o);
    double* out = cand + (static_cast<int64_t>(view) * gridDim.y + blockIdx.y) * HR_CAND;
    if (n < 4) {  // ransac returns no model (ransac.h:126-128); block-uniform
        if (threadIdx.x == 0) {
            for (int e = 0; e < HR_CAND; ++e) out[e] = 0.0;
        }
        return;
    }
    X += o; Y += o; u += o; v += o;
    const double t2 = thresh * thresh;
    double Hm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Hi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool valid = k < H;
    if (valid) {
        int idx[4];
        hr_sample(seed, k, n, idx);
        double sx[4], sy[4], suu[4], svv[4];
        for (int j = 0; j < 4; ++j) { sx[j] = X[idx[j]]; sy[j] = Y[idx[j]]; suu[j] = u[idx[j]]; svv[j] = v[idx[j]]; }
        valid = !hr_degenerate(sx, sy) && hr_fit4(sx, sy, suu, svv, Hm);
        if (valid) hr_inv3(Hm, Hi);
        else for (int a = 0; a < 9; ++a) Hm[a] = 0.0;  // scores no inliers (q2 = s2 = 0)
    }
    // pass 1: the raw model's inliers
    double c1 = 0.0, aX = 0.0, aY = 0.0, au = 0.0, av = 0.0;
    if (__syncthreads_or(valid)) {
        hr_tiles(n, X, Y, u, v, sX, sY, su, sv, [&](double x, double y, double uu, double vv) {
            const double w = hr_is_inlier(hr_resid_parts(Hm, Hi, x, y, uu, vv), t2) ? 1.0 : 0.0;
            c1 += w;
            aX = fma(w, x, aX); aY = fma(w, y, aY); au = fma(w, uu, au); av = fma(w, vv, av);
        });
    }
    valid = valid && c1 >= static_cast<double>(min_inliers);
    double Hf[9], Hfi[9];
    for (int a = 0; a < 9; ++a) { Hf[a] = Hm[a]; Hfi[a] = Hi[a]; }
    // passes 2, 3: refit_model (ransac.h:98-111) — HomographyEstimator::refit needs >= 4 inliers
    const bool do_refit = valid && refit && c1 >= 4.0;
    if (__syncthreads_or(do_refit)) {
        const double ic = c1 > 0.0 ? 1.0 / c1 : 0.0;
        const double csx = aX * ic, csy = aY * ic, cdx = au * ic, cdy = av * ic;
        double ms = 0.0, md = 0.0;
        hr_tiles(n, X, Y, u, v, sX, sY, su, sv, [&](double x, double y, double uu, double vv) {
            if (hr_is_inlier(hr_resid_parts(Hm, Hi, x, y, uu, vv), t2)) {
                ms += sqrt((x - csx) * (x - csx) + (y - csy) * (y - csy));
                md += sqrt((uu - cdx) * (uu - cdx) + (vv - cdy) * (vv - cdy));
            }
        });
        ms *= ic; md *= ic;
        const double ss = ms > 0.0 ? 1.4142135623730951 / ms : 1.0, sd = md > 0.0 ? 1.4142135623730951 / md : 1.0;
        double M[HR_NMOM];
        for (int e = 0; e < HR_NMOM; ++e) M[e] = 0.0;
        hr_tiles(n, X, Y, u, v, sX, sY, su, sv, [&](double x, double y, double uu, double vv) {
            if (hr_is_inlier(hr_resid_parts(Hm, Hi, x, y, uu, vv), t2))
                hr_accumulate(ss * x - ss * csx, ss * y - ss * csy, sd * uu - sd * cdx, sd * vv - sd * cdy, M);
        });
        double H2[9];
        if (do_refit && hr_refit(M, ss, csx, csy, sd, cdx, cdy, H2)) {
            for (int a = 0; a < 9; ++a) Hf[a] = H2[a];
            hr_inv3(Hf, Hfi);
        }
    }
    // pass 4: the final model's inliers (find_inliers) and their rms (detail::rms)
    double c5 = 0.0, s5 = 0.0;
    if (__syncthreads_or(valid)) {
        hr_tiles(n, X, Y, u, v, sX, sY, su, sv, [&](double x, double y, double uu, double vv) {
            const HrResid r = hr_resid_parts(Hf, Hfi, x, y, uu, vv);
            if (hr_is_inlier(r, t2)) {
                c5 += 1.0;
                s5 += hr_r2(r);
            }
        });
    }
    const double rms = c5 > 0.0 ? sqrt(s5 / c5) : __builtin_inf();
    // the block's best lane (fixed tree; the order is total, so the winner does not depend on the tree)
    rc[threadIdx.x] = c5; rr[threadIdx.x] = rms; rk[threadIdx.x] = k; rv[threadIdx.x] = valid ? 1 : 0;
    __syncthreads();
    for (int s = HR_BLOCK / 2; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) {
            const int a = threadIdx.x, b = threadIdx.x + s;
            if (hr_better(rv[b] != 0, rc[b], rr[b], rk[b], rv[a] != 0, rc[a], rr[a], rk[a])) {
                rc[a] = rc[b]; rr[a] = rr[b]; rk[a] = rk[b]; rv[a] = rv[b];
            }
        }
        __syncthreads();
    }
    if (k == rk[0]) {
        out[HC_VALID] = valid ? 1.0 : 0.0;
        out[HC_CNT] = c5;
        out[HC_RMS] = rms;
        out[HC_K] = k;
        for (int a = 0; a < 9; ++a) out[HC_H + a] = Hf[a];
    }
}

// estimate_homography's DLT path (homography.cpp:31-43): one candidate record per view
__global__ __launch_bounds__(64 * HR_VIEW_WAVES) void k_hr_dlt(int n_views, const int64_t* __restrict__ off, const double* __restrict__ X,
                                                              const double* __restrict__ Y, const double* __restrict__ u,
                                                              const double* __restrict__ v, double* __restrict__ cand) {
    const int i = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * HR_VIEW_WAVES + (threadIdx.x >> 6)));
    if (i >= n_views) return;
    const double K[5] = {1.0, 1.0, 0.0, 0.0, 0.0};
    double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    WaveCoop co;
    const int n = static_cast<int>(off[i + 1] - off[i]);
    const bool good = dlt_homography_view(n, X + off[i], Y + off[i], u + off[i], v + off[i], K, co, H);
    if (co.lane() == 0) {
        double* out = cand + static_cast<int64_t>(i) * HR_CAND;
        out[HC_VALID] = good ? 1.0 : 0.0;
        out[HC_CNT] = n;
        out[HC_RMS] = 0.0;
        out[HC_K] = 0.0;
        for (int a = 0; a < 9; ++a) out[HC_H + a] = H[a];
    }
}

// One workgroup per view.  ransac: the best of nb candidate records and inliers by the threshold test; otherwise record 0 and
// every point an inlier.  rescale: H / H22 when |H22| > 1e-15 (intrinsicsdlt.cpp:56-58, 69-71) before symmetric_rms_px.
__global__ __launch_bounds__(HR_BLOCK) void k_hr_finish(int nb, int ransac, int rescale, double thresh, const int64_t* __restrict__ off,
                                                       const double* __restrict__ X, const double* __restrict__ Y,
                                                       const double* __restrict__ u, const double* __restrict__ v,
                                                       const double* __restrict__ cand, double* __restrict__ h9, int32_t* __restrict__ ok,
                                                       int32_t* __restrict__ count, double* __restrict__ srms, uint8_t* __restrict__ mask) {
    __shared__ double sH[9];
    __shared__ int sok;
    __shared__ double red[2][HR_BLOCK];
    const int view = blockIdx.x;
    const int64_t o = off[view];
    const int n = static_cast<int>(off[view + 1] - o);
    if (threadIdx.x == 0) {
        const double* c = cand + static_cast<int64_t>(view) * nb * HR_CAND;
        int best = -1;
        for (int b = 0; b < nb; ++b) {  // strictly better only: the lowest hypothesis index wins ties
            const double* r = c + static_cast<int64_t>(b) * HR_CAND;
            if (r[HC_VALID] == 0.0) continue;
            if (best < 0) { best = b; continue; }
            const double* q = c + static_cast<int64_t>(best) * HR_CAND;
            if (r[HC_CNT] > q[HC_CNT] || (r[HC_CNT] == q[HC_CNT] && r[HC_RMS] < q[HC_RMS])) best = b;
        }
        sok = best >= 0 ? 1 : 0;
        for (int a = 0; a < 9; ++a) sH[a] = best >= 0 ? c[static_cast<int64_t>(best) * HR_CAND + HC_H + a] : (a % 4 == 0 ? 1.0 : 0.0);
    }
    __syncthreads();
    const bool good = sok != 0;
    double Hm[9], Hi[9], Hr[9], Hri[9];
    for (int a = 0; a < 9; ++a) Hm[a] = sH[a];
    hr_inv3(Hm, Hi);
    for (int a = 0; a < 9; ++a) Hr[a] = Hm[a];
    if (rescale && fabs(Hm[8]) > 1e-15) {
        const double s = Hm[8];
        for (int a = 0; a < 9; ++a) Hr[a] = Hm[a] / s;
    }
    hr_inv3(Hr, Hri);
    const double t2 = thresh * thresh;
    double cnt = 0.0, sr = 0.0;
    for (int i = threadIdx.x; i < n; i += HR_BLOCK) {
        bool in = false;
        if (good) {
            in = !ransac || hr_is_inlier(hr_resid_parts(Hm, Hi, X[o + i], Y[o + i], u[o + i], v[o + i]), t2);
            if (in) {
                cnt += 1.0;
                sr += sqrt(hr_r2(hr_resid_parts(Hr, Hri, X[o + i], Y[o + i], u[o + i], v[o + i])));
            }
        }
        if (mask) mask[o + i] = in ? 1 : 0;
    }
    red[0][threadIdx.x] = cnt;
    red[1][threadIdx.x] = sr;
    __syncthreads();
    for (int s = HR_BLOCK / 2; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int a = 0; a < 9; ++a) h9[9 * static_cast<int64_t>(view) + a] = good ? Hr[a] : (a % 4 == 0 ? 1.0 : 0.0);
        ok[view] = good ? 1 : 0;
        count[view] = good ? static_cast<int32_t>(red[0][0]) : 0;
        // symmetric_rms_px: sqrt(sum r / 2n), inf over an empty set; 0 (the HomographyResult default) for a failed view
        srms[view] = good ? (red[0][0] > 0.0 ? sqrt(red[1][0] / (2.0 * red[0][0])) : __builtin_inf()) : 0.0;
    }
}

// zhang_intrinsics_from_hs over the successful views in view order, then sanitize_intrinsics (bounds optional)
__global__ void k_hr_zhang(int n_views, const int32_t* __restrict__ ok, const double* __restrict__ h9, int has_bounds,
                           const double* __restrict__ b10, double* __restrict__ kst) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double G[36];
    for (int e = 0; e < 36; ++e) G[e] = 0.0;
    int m = 0;
    for (int i = 0; i < n_views; ++i) {
        if (!ok[i]) continue;
        double H[9];
        for (int a = 0; a < 9; ++a) H[a] = h9[9 * static_cast<int64_t>(i) + a];
        hr_zhang_accumulate(H, G);
        ++m;
    }
    double k5[5] = {0, 0, 0, 0, 0}, ks[5];
    const bool good = hr_zhang_solve(m, G, k5);
    bool mod = false;
    for (int k = 0; k < 5; ++k) ks[k] = k5[k];
    if (good && has_bounds) {
        double lo[5], hi[5];
        for (int k = 0; k < 5; ++k) { lo[k] = b10[k]; hi[k] = b10[5 + k]; }
        mod = hr_sanitize(k5, lo, hi, ks);
    }
    kst[KS_OK] = good ? 1.0 : 0.0;
    kst[KS_MOD] = mod ? 1.0 : 0.0;
    for (int k = 0; k < 5; ++k) kst[KS_K + k] = ks[k];
}

// rt12 = [R (9, row-major) | t (3)]; the identity where the pose fails
__global__ void k_hr_pose(int n_views, const int32_t* __restrict__ ok, const double* __restrict__ h9, const double* __restrict__ kst,
                          double* __restrict__ rt12, int32_t* __restrict__ pose_ok) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_views) return;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    bool good = false;
    if (kst[KS_OK] != 0.0 && ok[i]) {
        double k5[5], H[9], Rp[9], tp[3], s, c;
        for (int k = 0; k < 5; ++k) k5[k] = kst[KS_K + k];
        for (int a = 0; a < 9; ++a) H[a] = h9[9 * static_cast<int64_t>(i) + a];
        good = hr_pose_from_homography(k5, H, Rp, tp, &s, &c);
        if (good) {
            for (int a = 0; a < 9; ++a) R[a] = Rp[a];
            for (int k = 0; k < 3; ++k) t[k] = tp[k];
        }
    }
    for (int a = 0; a < 9; ++a) rt12[12 * static_cast<int64_t>(i) + a] = R[a];
    for (int k = 0; k < 3; ++k) rt12[12 * static_cast<int64_t>(i) + 9 + k] = t[k];
    pose_ok[i] = good ? 1 : 0;
}

// ---- host glue -----------------------------------------------------------------------------------------------------------
namespace {

using HrTimer = StageTimer<HR_NMARKS>;

// Device inputs and per-view homography outputs of one call
struct HrViews {
    ObsSoA obs;
    DevBuf<double> cand, h9, srms;
    DevBuf<int32_t> ok, cnt;
    DevBuf<uint8_t> mask;

    void upload(hipStream_t s, int n_views, const int64_t* off_h, const double* Xh, const double* Yh, const double* uh, const double* vh,
                bool want_mask) {
        obs.upload(s, n_views, off_h, Xh, Yh, uh, vh);
        h9.alloc(9 * static_cast<size_t>(n_views)); srms.alloc(n_views); ok.alloc(n_views); cnt.alloc(n_views);
        if (want_mask) mask.alloc(static_cast<size_t>(off_h[n_views]));
    }

    // every view's homography (RANSAC when o is given, else the all-points DLT), queued on s
    void homographies(hipStream_t s, int n_views, const cba_ransac_options* o, int rescale, HrTimer& tm) {
        int nb = 1;
        if (o) {
            // max_iters <= CBA_RANSAC_MAX_ITERS (checked at the C ABI): at most 256 candidate records per view
            nb = std::max(1, (o->max_iters + HR_BLOCK - 1) / HR_BLOCK);
            cand.alloc(static_cast<size_t>(n_views) * nb * HR_CAND);
            hipLaunchKernelGGL(k_hr_score, dim3(n_views, nb), dim3(HR_BLOCK), 0, s, o->max_iters, o->thresh, o->min_inliers,
                               o->refit_on_inliers, o->seed, obs.off.p, obs.X.p, obs.Y.p, obs.u.p, obs.v.p, cand.p);
        } else {
            cand.alloc(static_cast<size_t>(n_views) * HR_CAND);
            hipLaunchKernelGGL(k_hr_dlt, dim3((n_views + HR_VIEW_WAVES - 1) / HR_VIEW_WAVES), dim3(64 * HR_VIEW_WAVES), 0, s, n_views,
                               obs.off.p, obs.X.p, obs.Y.p, obs.u.p, obs.v.p, cand.p);
        }
        CBA_HIP(hipGetLastError());
        tm.mark(HM_SCORE);
        hipLaunchKernelGGL(k_hr_finish, dim3(n_views), dim3(HR_BLOCK), 0, s, nb, o ? 1 : 0, rescale, o ? o->thresh : 0.0, obs.off.p, obs.X.p,
                           obs.Y.p, obs.u.p, obs.v.p, cand.p, h9.p, ok.p, cnt.p, srms.p, mask.p);
        CBA_HIP(hipGetLastError());
        tm.mark(HM_HOM);
    }
};

}  // namespace

void homography_ransac_batch(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                             const cba_ransac_options* o, double* h9, int32_t* success, int32_t* inlier_count, double* symmetric_rms,
                             uint8_t* inlier_mask, int device) {
    StreamLease lease(device);
    const hipStream_t stream = lease;
    {
        HrTimer tm(stream, false);
        HrViews d;
        d.upload(stream, n_views, view_offset, X, Y, u, v, inlier_mask != nullptr);
        d.homographies(stream, n_views, o, 0, tm);
        d.h9.download(h9, 9 * static_cast<size_t>(n_views), stream);
        d.ok.download(success, n_views, stream);
        d.cnt.download(inlier_count, n_views, stream);
        d.srms.download(symmetric_rms, n_views, stream);
        if (inlier_mask) d.mask.download(inlier_mask, view_offset[n_views], stream);
        CBA_HIP(hipStreamSynchronize(stream));
    }
}

void estimate_intrinsics_gpu(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                             const cba_ransac_options* o, const double* bounds_lo5, const double* bounds_hi5, int32_t* success,
                             double* kmtx5, int32_t* sanitized, int32_t* view_ok, double* h9, double* forward_rms_px, double* rt12,
                             int32_t* pose_ok, uint8_t* inlier_mask, double* stage_ms, int device) {
    StreamLease lease(device);
    const hipStream_t stream = lease;
    double kst[KS_SIZE];
    {
        HrTimer tm(stream, stage_ms != nullptr);
        HrViews d;
        DevBuf<double> b10, dkst, dpose;
        DevBuf<int32_t> dpok;
        d.upload(stream, n_views, view_offset, X, Y, u, v, inlier_mask != nullptr);
        const int has_bounds = bounds_lo5 && bounds_hi5;
        b10.alloc(10); dkst.alloc(KS_SIZE); dpose.alloc(12 * static_cast<size_t>(n_views)); dpok.alloc(n_views);
        if (has_bounds) {
            b10.upload(bounds_lo5, 5, stream);
            b10.upload(bounds_hi5, 5, stream, 5);
        }
        tm.mark(HM_0);
        d.homographies(stream, n_views, o, 1, tm);
        hipLaunchKernelGGL(k_hr_zhang, dim3(1), dim3(64), 0, stream, n_views, d.ok.p, d.h9.p, has_bounds, b10.p, dkst.p);
        CBA_HIP(hipGetLastError());
        tm.mark(HM_ZHANG);
        hipLaunchKernelGGL(k_hr_pose, dim3((n_views + HR_BLOCK - 1) / HR_BLOCK), dim3(HR_BLOCK), 0, stream, n_views, d.ok.p, d.h9.p, dkst.p,
                           dpose.p, dpok.p);
        CBA_HIP(hipGetLastError());
        tm.mark(HM_POSE);
        dkst.download(kst, KS_SIZE, stream);
        d.h9.download(h9, 9 * static_cast<size_t>(n_views), stream);
        d.ok.download(view_ok, n_views, stream);
        d.srms.download(forward_rms_px, n_views, stream);
        dpose.download(rt12, 12 * static_cast<size_t>(n_views), stream);
        dpok.download(pose_ok, n_views, stream);
        if (inlier_mask) d.mask.download(inlier_mask, view_offset[n_views], stream);
        CBA_HIP(hipStreamSynchronize(stream));
        if (stage_ms) {  // stage_ms [5]: homographies (scoring), homographies (select + rms), Zhang + sanitize, poses, total
            stage_ms[0] = tm.ms(HM_0, HM_SCORE);
            stage_ms[1] = tm.ms(HM_SCORE, HM_HOM);
            stage_ms[2] = tm.ms(HM_HOM, HM_ZHANG);
            stage_ms[3] = tm.ms(HM_ZHANG, HM_POSE);
            stage_ms[4] = tm.ms(HM_0, HM_POSE);
        }
    }
    *success = kst[KS_OK] != 0.0 ? 1 : 0;
    *sanitized = kst[KS_MOD] != 0.0 ? 1 : 0;
    for (int k = 0; k < 5; ++k) kmtx5[k] = *success ? kst[KS_K + k] : 0.0;
}

}  // namespace cba
