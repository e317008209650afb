// linescan.hip — calibrate_laser_plane (include/calib/estimation/linear/linescan.h:101-144) and fit_plane_svd /
// fit_plane_ransac (planefit.cpp) on the GPU.  Device math: linescan_math.hpp.
//
//   k_ls_views    one wavefront per view: unproject the target pixels, DLT homography, pose, H^-1 (geo [n_views][21], ok)
//   k_ls_prefix   one lane: where each used view's points start in the compact point arrays, and their total
//   k_ls_points   grid-stride over the laser pixels (view by binary search on laser_offset): camera-frame point, written
//                 compact as SoA (px, py, pz) and, on request, as [n_laser][3] rows with NaN for failed views
//   k_ls_mom      grid-stride moments over the compact points with a fixed grid (LS_GRID blocks at most): count / sum /
//                 max|p|, the centred scatter, or count / sum r^2 against a plane; one partial row per block
//   k_ls_fin      one lane: the block partials in block order -> centroid, plane (seed_eig3 + sign convention), rms
//   RANSAC        k_ls_hyp (one lane per hypothesis) -> k_ls_score<MOMENTS> -> k_ls_refit -> k_ls_score<RESIDUALS> ->
//                 k_ls_hyp_sum -> k_ls_pick, then the winner's exact refit through k_ls_mom / k_ls_fin.
//
// The scoring kernel is the compute-bound part: a workgroup owns 256 hypotheses (one per lane, the plane in VGPRs) and one
// chunk of the points; it stages the chunk tile by tile in LDS (shifted by the global centroid, so the moments stay small),
// and every lane reads the same LDS address (a broadcast) and accumulates in registers.  Partials per (hypothesis, chunk)
// are reduced over the chunks in chunk order, so every result is bitwise reproducible.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pipelines.hpp"
#include "linescan_math.hpp"

namespace cba {

constexpr int LS_VIEW_WAVES = 4;
constexpr int LS_BLOCK = 256;
constexpr int LS_GRID = 1024;  // most blocks of a grid-stride moment pass (the partial layout depends on the input size only)
constexpr int LS_TILE = 1024;  // points per LDS tile of the scoring kernel (24 KiB)
constexpr int LS_NMOM = 10;    // scoring pass 1: count, sum q (3), sum q q^T (6)

// st: the device-side state of one fit
enum {
    ST_NIN = 0,     // count of the last k_ls_mom SUM pass
    ST_C = 1,       // centroid of that pass (3)
    ST_SCALE = 4,   // max |p| over all points (set by the unfiltered SUM pass)
    ST_PLANE = 5,   // current plane (4)
    ST_RMS = 9,
    ST_CNT = 10,    // count of the last RES pass
    ST_FILT = 11,   // filter plane of the moment passes (4): the RANSAC winner's raw model
    ST_OK = 15,     // RANSAC found a model
    ST_WIN = 16,    // winning hypothesis
    ST_SHIFT = 17,  // centroid of all points: the shift of the scoring passes (3)
    ST_SIZE = 20
};
enum { MK_V0, MK_V1, MK_FIT0, MK_S1A, MK_S1B, MK_S2A, MK_S2B, MK_FIT1, LS_NSTAGE_MARKS };
enum { MOM_SUM = 0, MOM_SCATTER = 1, MOM_RES = 2 };
enum { FIN_CENTROID = 0, FIN_PLANE = 1, FIN_RMS = 2, FIN_RAW = 3 };

__global__ __launch_bounds__(64 * LS_VIEW_WAVES) void k_ls_views(int n_views, const int64_t* __restrict__ toff, const double* __restrict__ X,
                                                                const double* __restrict__ Y, const double* __restrict__ u,
                                                                const double* __restrict__ v, LsCamera cam, double* __restrict__ nu,
                                                                double* __restrict__ nv, double* __restrict__ geo, int32_t* __restrict__ ok) {
    const int i = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * LS_VIEW_WAVES + (threadIdx.x >> 6)));
    if (i >= n_views) return;  // whole wave leaves together
    const int64_t o = toff[i];
    double g[LS_GEO];
    WaveCoop co;
    const bool good = ls_view_geometry(cam, static_cast<int>(toff[i + 1] - o), X + o, Y + o, u + o, v + o, nu + o, nv + o, co, g);
    if (co.lane() == 0) {
        for (int k = 0; k < LS_GEO; ++k) geo[LS_GEO * static_cast<int64_t>(i) + k] = good ? g[k] : 0.0;
        ok[i] = good ? 1 : 0;
    }
}

__global__ void k_ls_prefix(int n_views, const int64_t* __restrict__ loff, const int32_t* __restrict__ ok, int64_t* __restrict__ coff,
                            int64_t* __restrict__ n_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t s = 0;
    for (int i = 0; i < n_views; ++i) {
        coff[i] = s;
        if (ok[i]) s += loff[i + 1] - loff[i];
    }
    *n_out = s;
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_points(int n_views, int64_t n_laser, const int64_t* __restrict__ loff,
                                                       const double* __restrict__ lu, const double* __restrict__ lv, LsCamera cam,
                                                       const double* __restrict__ geo, const int32_t* __restrict__ ok,
                                                       const int64_t* __restrict__ coff, double* __restrict__ px, double* __restrict__ py,
                                                       double* __restrict__ pz, double* __restrict__ xyz) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n_laser;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        int lo = 0, hi = n_views;  // the largest view with loff[view] <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (loff[mid] <= i) lo = mid; else hi = mid;
        }
        double p[3];
        if (ok[lo]) {
            double g[LS_GEO];
            for (int k = 0; k < LS_GEO; ++k) g[k] = geo[LS_GEO * static_cast<int64_t>(lo) + k];
            ls_backproject(cam, g, lu[i], lv[i], p);
            const int64_t c = coff[lo] + (i - loff[lo]);
            px[c] = p[0]; py[c] = p[1]; pz[c] = p[2];
        } else {
            p[0] = p[1] = p[2] = __builtin_nan("");
        }
        if (xyz) { xyz[3 * i] = p[0]; xyz[3 * i + 1] = p[1]; xyz[3 * i + 2] = p[2]; }
    }
}

__global__ __launch_bounds__(LS_BLOCK) void k_ls_aos_to_soa(int64_t n, const double* __restrict__ xyz, double* __restrict__ px,
                                                           double* __restrict__ py, double* __restrict__ pz) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        px[i] = xyz[3 * i]; py[i] = xyz[3 * i + 1]; pz[i] = xyz[3 * i + 2];
    }
}

// Moment pass over the n compact points (grid-stride; block b writes part[b][6]).  filter: only points with
// |filt . p| <= thresh (filt = st[ST_FILT]) count.  SUM: [count, sum p (3), max|p|, 0]; SCATTER: sum (p-c)(p-c)^T with
// c = st[ST_C]; RES: [count, sum r^2] of r = st[ST_PLANE] . p (mask[i] = inlier when mask is given).
__global__ __launch_bounds__(LS_BLOCK) void k_ls_mom(int mode, int filter, double thresh, const int64_t* __restrict__ n_ptr,
                                                    const double* __restrict__ px, const double* __restrict__ py,
                                                    const double* __restrict__ pz, const double* __restrict__ st, double* __restrict__ part,
                                                    uint8_t* __restrict__ mask) {
    __shared__ double red[6][LS_BLOCK];
    const int64_t n = *n_ptr;
    const double f0 = st[ST_FILT], f1 = st[ST_FILT + 1], f2 = st[ST_FILT + 2], f3 = st[ST_FILT + 3];
    const double c0 = st[ST_C], c1 = st[ST_C + 1], c2 = st[ST_C + 2];
    const double q0 = st[ST_PLANE], q1 = st[ST_PLANE + 1], q2 = st[ST_PLANE + 2], q3 = st[ST_PLANE + 3];
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const double x = px[i], y = py[i], z = pz[i];
        if (filter && !(fabs(f0 * x + f1 * y + f2 * z + f3) <= thresh)) {
            if (mode == MOM_RES && mask) mask[i] = 0;
            continue;
        }
        if (mode == MOM_SUM) {
            a[0] += 1.0; a[1] += x; a[2] += y; a[3] += z;
            a[4] = fmax(a[4], fmax(fabs(x), fmax(fabs(y), fabs(z))));
        } else if (mode == MOM_SCATTER) {
            const double dx = x - c0, dy = y - c1, dz = z - c2;
            a[0] += dx * dx; a[1] += dx * dy; a[2] += dx * dz; a[3] += dy * dy; a[4] += dy * dz; a[5] += dz * dz;
        } else {
            const double r = q0 * x + q1 * y + q2 * z + q3;
            a[0] += 1.0; a[1] += r * r;
            if (mask) mask[i] = 1;
        }
    }
    for (int e = 0; e < 6; ++e) red[e][threadIdx.x] = a[e];
    __syncthreads();
    for (int s = LS_BLOCK / 2; s > 0; s >>= 1) {  // fixed tree: bitwise reproducible
        if (static_cast<int>(threadIdx.x) < s)
            for (int e = 0; e < 6; ++e)
                red[e][threadIdx.x] = (mode == MOM_SUM && e == 4) ? fmax(red[e][threadIdx.x], red[e][threadIdx.x + s])
                                                                   : red[e][threadIdx.x] + red[e][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 6) part[6 * static_cast<int64_t>(blockIdx.x) + threadIdx.x] = red[threadIdx.x][0];
}

// One lane: block partials in block order -> the state.  set_scale: the SUM pass ran over all points (ST_SCALE, ST_SHIFT).
__global__ void k_ls_fin(int stage, int nblk, int set_scale, const double* __restrict__ part, double* __restrict__ st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nblk; ++b)
        for (int e = 0; e < 6; ++e) s[e] = (stage == FIN_CENTROID && e == 4) ? fmax(s[e], part[6 * b + e]) : s[e] + part[6 * b + e];
    if (stage == FIN_CENTROID) {
        st[ST_NIN] = s[0];
        for (int k = 0; k < 3; ++k) st[ST_C + k] = s[1 + k] / s[0];
        if (set_scale) {
            st[ST_SCALE] = s[4];
            for (int k = 0; k < 3; ++k) st[ST_SHIFT + k] = st[ST_C + k];
        }
    } else if (stage == FIN_PLANE) {
        double pl[4];
        if (st[ST_NIN] >= 3.0) {
            const double c[3] = {st[ST_C], st[ST_C + 1], st[ST_C + 2]};
            ls_plane_from_scatter(c, s, pl);
        } else {  // refit_model keeps the raw model when refit has < 3 points
            for (int k = 0; k < 4; ++k) pl[k] = st[ST_FILT + k];
        }
        ls_plane_sign(pl, st[ST_SCALE]);
        for (int k = 0; k < 4; ++k) st[ST_PLANE + k] = pl[k];
    } else if (stage == FIN_RAW) {
        double pl[4];
        for (int k = 0; k < 4; ++k) pl[k] = st[ST_FILT + k];
        ls_plane_sign(pl, st[ST_SCALE]);
        for (int k = 0; k < 4; ++k) st[ST_PLANE + k] = pl[k];
    } else {
        st[ST_CNT] = s[0];
        st[ST_RMS] = sqrt(s[1] / s[0]);
    }
}

__global__ void k_ls_copy_plane(double* __restrict__ st) {
    if (threadIdx.x < 4 && blockIdx.x == 0) st[ST_FILT + threadIdx.x] = st[ST_PLANE + threadIdx.x];
}

// ---- RANSAC --------------------------------------------------------------------------------------------------------------
// hyp [Hp][4]: hypothesis k's plane in the SHIFTED frame (q = p - shift): (n, d + n.shift); degenerate / padding: (0, 0, 0, inf)
__global__ void k_ls_hyp(int H, int Hp, uint64_t seed, const int64_t* __restrict__ n_ptr, const double* __restrict__ px,
                         const double* __restrict__ py, const double* __restrict__ pz, const double* __restrict__ st,
                         double* __restrict__ hyp, int32_t* __restrict__ hstate) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Hp) return;
    const int64_t n = *n_ptr;
    double pl[4] = {0.0, 0.0, 0.0, __builtin_inf()};
    bool good = false;
    if (k < H && n >= 3) {
        int64_t idx[3];
        ls_hypothesis(seed, k, n, idx);
        double p[3][3];
        for (int j = 0; j < 3; ++j) { p[j][0] = px[idx[j]]; p[j][1] = py[idx[j]]; p[j][2] = pz[idx[j]]; }
        good = ls_plane_from_3(p[0], p[1], p[2], pl);
        if (good) pl[3] += pl[0] * st[ST_SHIFT] + pl[1] * st[ST_SHIFT + 1] + pl[2] * st[ST_SHIFT + 2];
        else { pl[0] = pl[1] = pl[2] = 0.0; pl[3] = __builtin_inf(); }
    }
    for (int j = 0; j < 4; ++j) hyp[4 * k + j] = pl[j];
    hstate[k] = good ? 1 : 0;
}

// Grid (Hp / 256, C).  MOMENTS: part[e][chunk][Hp], e < 10 = count, sum q, sum q q^T of the inliers;
// RESIDUALS: e < 2 = count, sum r^2.
template <bool MOMENTS>
__global__ __launch_bounds__(LS_BLOCK) void k_ls_score(int Hp, int C, double thresh, const int64_t* __restrict__ n_ptr,
                                                      const double* __restrict__ px, const double* __restrict__ py,
                                                      const double* __restrict__ pz, const double* __restrict__ st,
                                                      const double* __restrict__ hyp, double* __restrict__ part) {
    __shared__ double sx[LS_TILE], sy[LS_TILE], sz[LS_TILE];
    const int h = blockIdx.x * LS_BLOCK + threadIdx.x;
    const int chunk = blockIdx.y;
    const int64_t n = *n_ptr;
    const int64_t per = (n + C - 1) / C;
    const int64_t beg = chunk * per, end = std::min<int64_t>(n, beg + per);
    const double s0 = st[ST_SHIFT], s1 = st[ST_SHIFT + 1], s2 = st[ST_SHIFT + 2];
    const double a = hyp[4 * h], b = hyp[4 * h + 1], c = hyp[4 * h + 2], d = hyp[4 * h + 3];
    double cnt = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0;
    for (int64_t t0 = beg; t0 < end; t0 += LS_TILE) {
        const int cntt = static_cast<int>(std::min<int64_t>(LS_TILE, end - t0));
        __syncthreads();
        for (int j = threadIdx.x; j < cntt; j += LS_BLOCK) {
            sx[j] = px[t0 + j] - s0; sy[j] = py[t0 + j] - s1; sz[j] = pz[t0 + j] - s2;
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cntt; ++j) {
            const double x = sx[j], y = sy[j], z = sz[j];
            const double r = fma(a, x, fma(b, y, fma(c, z, d)));
            const bool in = fabs(r) <= thresh;
            if (MOMENTS) {
                const double wx = in ? x : 0.0, wy = in ? y : 0.0, wz = in ? z : 0.0;
                cnt += in ? 1.0 : 0.0;
                m0 += wx; m1 += wy; m2 += wz;
                m00 = fma(wx, x, m00); m01 = fma(wx, y, m01); m02 = fma(wx, z, m02);
                m11 = fma(wy, y, m11); m12 = fma(wy, z, m12); m22 = fma(wz, z, m22);
            } else {
                const double wr = in ? r : 0.0;
                cnt += in ? 1.0 : 0.0;
                m0 = fma(wr, wr, m0);
            }
        }
    }
    const int64_t stride = static_cast<int64_t>(C) * Hp, o = static_cast<int64_t>(chunk) * Hp + h;
    part[o] = cnt;
    part[o + stride] = m0;
    if (MOMENTS) {
        part[o + 2 * stride] = m1; part[o + 3 * stride] = m2;
        part[o + 4 * stride] = m00; part[o + 5 * stride] = m01; part[o + 6 * stride] = m02;
        part[o + 7 * stride] = m11; part[o + 8 * stride] = m12; part[o + 9 * stride] = m22;
    }
}

// One lane per hypothesis: its pass-1 moments over the chunks in chunk order; hypotheses with fewer than min_inliers inliers
// are dropped (hstate 0); with refit, the plane is refit from the inliers' centred moments (refit_model; < 3 inliers keeps the
// raw model).  hyp2 [Hp][4] = the model pass 2 scores (shifted frame).
__global__ void k_ls_refit(int H, int Hp, int C, int min_inliers, int refit, const double* __restrict__ part, const double* __restrict__ hyp,
                           int32_t* __restrict__ hstate, double* __restrict__ hyp2) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Hp) return;
    double pl[4] = {hyp[4 * k], hyp[4 * k + 1], hyp[4 * k + 2], hyp[4 * k + 3]};
    if (k < H && hstate[k]) {
        double m[LS_NMOM];
        for (int e = 0; e < LS_NMOM; ++e) {
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += part[(static_cast<int64_t>(e) * C + c) * Hp + k];
            m[e] = s;
        }
        if (m[0] < static_cast<double>(min_inliers)) {
            hstate[k] = 0;
        } else if (refit && m[0] >= 3.0) {
            const double inv = 1.0 / m[0];
            const double cq[3] = {m[1] * inv, m[2] * inv, m[3] * inv};
            const double S[6] = {m[4] - m[1] * cq[0], m[5] - m[1] * cq[1], m[6] - m[1] * cq[2],
                                 m[7] - m[2] * cq[1], m[8] - m[2] * cq[2], m[9] - m[3] * cq[2]};
            ls_plane_from_scatter(cq, S, pl);
        }
    }
    for (int j = 0; j < 4; ++j) hyp2[4 * k + j] = pl[j];
}

// One lane per hypothesis: pass-2 count and inlier rms (chunk order)
__global__ void k_ls_hyp_sum(int H, int Hp, int C, const double* __restrict__ part, double* __restrict__ hcnt, double* __restrict__ hrms) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= H) return;
    double c0 = 0.0, c1 = 0.0;
    for (int c = 0; c < C; ++c) {
        c0 += part[static_cast<int64_t>(c) * Hp + k];
        c1 += part[(static_cast<int64_t>(C) + c) * Hp + k];
    }
    hcnt[k] = c0;
    hrms[k] = c0 > 0.0 ? sqrt(c1 / c0) : __builtin_inf();
}

// One lane: the best hypothesis by (count desc, rms asc, k asc) (is_better_model, ransac.h:115-119); its raw model (the refit's
// inlier set) goes to ST_FILT and its scored model to ST_PLANE, both unshifted.
__global__ void k_ls_pick(int H, const int32_t* __restrict__ hstate, const double* __restrict__ hcnt, const double* __restrict__ hrms,
                          const double* __restrict__ hyp, const double* __restrict__ hyp2, double* __restrict__ st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int best = -1;
    for (int k = 0; k < H; ++k) {
        if (!hstate[k]) continue;
        if (best < 0 || hcnt[k] > hcnt[best] || (hcnt[k] == hcnt[best] && hrms[k] < hrms[best])) best = k;
    }
    st[ST_OK] = best >= 0 ? 1.0 : 0.0;
    st[ST_WIN] = best;
    const double s[3] = {st[ST_SHIFT], st[ST_SHIFT + 1], st[ST_SHIFT + 2]};
    for (int j = 0; j < 4; ++j) {
        st[ST_FILT + j] = best >= 0 ? hyp[4 * best + j] : __builtin_nan("");
        st[ST_PLANE + j] = best >= 0 ? hyp2[4 * best + j] : __builtin_nan("");
    }
    st[ST_FILT + 3] -= st[ST_FILT] * s[0] + st[ST_FILT + 1] * s[1] + st[ST_FILT + 2] * s[2];
    st[ST_PLANE + 3] -= st[ST_PLANE] * s[0] + st[ST_PLANE + 1] * s[1] + st[ST_PLANE + 2] * s[2];
}

// ---- host glue -----------------------------------------------------------------------------------------------------------
namespace {

// Optional stage timing (cba_calibrate_laser_plane_timed): events recorded between the stages of one call.
using LsTimer = StageTimer<LS_NSTAGE_MARKS>;

// The plane fit over the n (on the device: *dn, at most n_cap) compact points px/py/pz; cmask [n_cap] optional.  Queued on
// `stream`; the caller synchronises and reads st (ST_SIZE doubles) back.
struct PlaneFitter {
    DevBuf<double> part, st, hyp, hyp2, hpart, hcnt, hrms;
    DevBuf<int32_t> hstate;

    void run(hipStream_t stream, int64_t n_cap, const int64_t* dn, const double* px, const double* py, const double* pz,
             const cba_plane_fit_options& o, uint8_t* cmask, LsTimer& tm) {
        const int G = launch_grid(n_cap, LS_BLOCK, LS_GRID);
        part.alloc(6 * static_cast<size_t>(G));
        st.alloc(ST_SIZE);
        st.zero(stream);
        auto mom = [&](int mode, int filter, uint8_t* mask) {
            hipLaunchKernelGGL(k_ls_mom, dim3(G), dim3(LS_BLOCK), 0, stream, mode, filter, o.thresh, dn, px, py, pz, st.p, part.p, mask);
            CBA_HIP(hipGetLastError());
        };
        auto fin = [&](int stage, int set_scale) {
            hipLaunchKernelGGL(k_ls_fin, dim3(1), dim3(64), 0, stream, stage, G, set_scale, part.p, st.p);
            CBA_HIP(hipGetLastError());
        };
        tm.mark(MK_FIT0);
        mom(MOM_SUM, 0, nullptr);
        fin(FIN_CENTROID, 1);
        if (!o.use_ransac) {
            mom(MOM_SCATTER, 0, nullptr);
            fin(FIN_PLANE, 0);
            mom(MOM_RES, 0, cmask);
            fin(FIN_RMS, 0);
            tm.mark(MK_FIT1);
            return;
        }
        // max_iters <= CBA_PLANE_FIT_MAX_ITERS (checked at the C ABI), so Hp and the partial sizes below fit their types
        const int H = o.max_iters;
        const int hb = static_cast<int>((static_cast<int64_t>(H) + LS_BLOCK - 1) / LS_BLOCK), Hp = hb * LS_BLOCK;
        // chunks: ~2048 workgroups for the 256 CUs, each chunk at least one LDS tile
        const int C = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n_cap + LS_TILE - 1) / LS_TILE, (2048 + hb - 1) / hb)));
        hyp.alloc(4 * static_cast<size_t>(Hp)); hyp2.alloc(4 * static_cast<size_t>(Hp));
        hstate.alloc(Hp); hcnt.alloc(H); hrms.alloc(H);
        hpart.alloc(static_cast<size_t>(LS_NMOM) * static_cast<size_t>(C) * static_cast<size_t>(Hp));
        hipLaunchKernelGGL(k_ls_hyp, dim3(hb), dim3(LS_BLOCK), 0, stream, H, Hp, o.seed, dn, px, py, pz, st.p, hyp.p, hstate.p);
        CBA_HIP(hipGetLastError());
        tm.mark(MK_S1A);
        hipLaunchKernelGGL(k_ls_score<true>, dim3(hb, C), dim3(LS_BLOCK), 0, stream, Hp, C, o.thresh, dn, px, py, pz, st.p, hyp.p, hpart.p);
        CBA_HIP(hipGetLastError());
        tm.mark(MK_S1B);
        hipLaunchKernelGGL(k_ls_refit, dim3(hb), dim3(LS_BLOCK), 0, stream, H, Hp, C, o.min_inliers, o.refit_on_inliers, hpart.p, hyp.p,
                           hstate.p, hyp2.p);
        CBA_HIP(hipGetLastError());
        tm.mark(MK_S2A);
        hipLaunchKernelGGL(k_ls_score<false>, dim3(hb, C), dim3(LS_BLOCK), 0, stream, Hp, C, o.thresh, dn, px, py, pz, st.p, hyp2.p,
                           hpart.p);
        CBA_HIP(hipGetLastError());
        tm.mark(MK_S2B);
        hipLaunchKernelGGL(k_ls_hyp_sum, dim3(hb), dim3(LS_BLOCK), 0, stream, H, Hp, C, hpart.p, hcnt.p, hrms.p);
        CBA_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ls_pick, dim3(1), dim3(64), 0, stream, H, hstate.p, hcnt.p, hrms.p, hyp.p, hyp2.p, st.p);
        CBA_HIP(hipGetLastError());
        // the winner: refit exactly (two-pass centred) on its raw model's inliers, as refit_model does
        if (o.refit_on_inliers) {
            mom(MOM_SUM, 1, nullptr);
            fin(FIN_CENTROID, 0);
            mom(MOM_SCATTER, 1, nullptr);
            fin(FIN_PLANE, 0);
        } else {
            fin(FIN_RAW, 0);
        }
        // ... and its inliers recounted against the returned plane
        hipLaunchKernelGGL(k_ls_copy_plane, dim3(1), dim3(64), 0, stream, st.p);
        CBA_HIP(hipGetLastError());
        mom(MOM_RES, 1, cmask);
        fin(FIN_RMS, 0);
        tm.mark(MK_FIT1);
    }
};

void set_result_plane(const double* st, bool ransac, int iters, cba_laser_plane_result* r) {
    for (int k = 0; k < 4; ++k) r->plane[k] = st[ST_PLANE + k];
    ls_plane_homography(r->plane, r->homography);
    r->rms_error = st[ST_RMS];
    r->inlier_count = static_cast<int64_t>(st[ST_CNT]);
    r->iters = ransac ? iters : 0;
    std::memset(r->summary, 0, sizeof(r->summary));
    std::strcpy(r->summary, ransac ? "ransac" : "linear_svd");
}

void timings(const LsTimer& t, double* ms) {
    if (!ms) return;
    ms[0] = t.ms(MK_V0, MK_V1);
    ms[1] = t.ms(MK_V1, MK_FIT0);
    ms[2] = t.ms(MK_FIT0, MK_FIT1);
    ms[3] = t.ms(MK_S1A, MK_S1B);
    ms[4] = t.ms(MK_S2A, MK_S2B);
}

}  // namespace

void laser_plane_calibrate(int model, const double* intr, int n_inv, const double* inv, int n_views, const int64_t* toff, const double* X, const double* Y, const double* u,
                           const double* v, const int64_t* loff, const double* lu, const double* lv, const cba_plane_fit_options& o,
                           cba_laser_plane_result* res, double* points_xyz, uint8_t* inlier_mask, double* stage_ms, int device) {
    LsCamera cam;
    ls_fill_camera(model, intr, n_inv, inv, &cam);
    StreamLease lease(device);
    const hipStream_t stream = lease;
    const int64_t n_t = toff[n_views], n_l = loff[n_views];
    std::vector<int32_t> ok(n_views);
    std::vector<uint8_t> cmask;
    double st[ST_SIZE];
    int64_t n_valid = 0;
    {
        LsTimer tm(stream, stage_ms != nullptr);
        ObsSoA tgt;  // the target points
        DevBuf<double> dnu, dnv, dlu, dlv, dgeo, px, py, pz, dxyz;
        DevBuf<int64_t> dloff, dcoff, dn;
        DevBuf<int32_t> dok;
        DevBuf<uint8_t> dmask;
        const size_t nt = static_cast<size_t>(n_t), nl = static_cast<size_t>(n_l);
        tgt.upload(stream, n_views, toff, X, Y, u, v);
        dnu.alloc(nt); dnv.alloc(nt); px.alloc(nl); py.alloc(nl); pz.alloc(nl);
        dgeo.alloc(LS_GEO * static_cast<size_t>(n_views)); dok.alloc(n_views); dcoff.alloc(n_views); dn.alloc(1);
        if (points_xyz) dxyz.alloc(3 * nl);
        if (inlier_mask) dmask.alloc(nl);
        dlu.assign(lu, nl, stream); dlv.assign(lv, nl, stream);
        dloff.assign(loff, static_cast<size_t>(n_views) + 1, stream);
        tm.mark(MK_V0);
        hipLaunchKernelGGL(k_ls_views, dim3((n_views + LS_VIEW_WAVES - 1) / LS_VIEW_WAVES), dim3(64 * LS_VIEW_WAVES), 0, stream, n_views,
                           tgt.off.p, tgt.X.p, tgt.Y.p, tgt.u.p, tgt.v.p, cam, dnu.p, dnv.p, dgeo.p, dok.p);
        CBA_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ls_prefix, dim3(1), dim3(64), 0, stream, n_views, dloff.p, dok.p, dcoff.p, dn.p);
        CBA_HIP(hipGetLastError());
        tm.mark(MK_V1);
        if (n_l > 0) {
            hipLaunchKernelGGL(k_ls_points, dim3(launch_grid(n_l, LS_BLOCK, LS_GRID) * 2), dim3(LS_BLOCK), 0, stream, n_views, n_l, dloff.p, dlu.p, dlv.p, cam,
                               dgeo.p, dok.p, dcoff.p, px.p, py.p, pz.p, points_xyz ? dxyz.p : nullptr);
            CBA_HIP(hipGetLastError());
        }
        PlaneFitter fit;
        fit.run(stream, std::max<int64_t>(n_l, 1), dn.p, px.p, py.p, pz.p, o, inlier_mask ? dmask.p : nullptr, tm);
        fit.st.download(st, ST_SIZE, stream);
        dn.download(&n_valid, 1, stream);
        dok.download(ok.data(), n_views, stream);
        if (points_xyz) dxyz.download(points_xyz, 3 * nl, stream);
        if (inlier_mask) {
            cmask.resize(nl);
            dmask.download(cmask.data(), nl, stream);
        }
        CBA_HIP(hipStreamSynchronize(stream));
        timings(tm, stage_ms);
    }
    if (n_valid < 3) throw std::invalid_argument("Not enough laser points to fit a plane");
    if (o.use_ransac && st[ST_OK] == 0.0) throw std::runtime_error("RANSAC plane fitting failed");
    set_result_plane(st, o.use_ransac != 0, o.max_iters, res);
    res->n_points = n_valid;
    int used = 0;
    for (int i = 0; i < n_views; ++i) used += ok[i] ? 1 : 0;
    res->n_views_used = used;
    if (inlier_mask) {  // compact -> per laser pixel
        int64_t c = 0;
        for (int i = 0; i < n_views; ++i) {
            const int64_t m = loff[i + 1] - loff[i];
            if (ok[i]) {
                for (int64_t j = 0; j < m; ++j) inlier_mask[loff[i] + j] = o.use_ransac ? cmask[c + j] : 1;
                c += m;
            } else {
                std::memset(inlier_mask + loff[i], 0, static_cast<size_t>(m));
            }
        }
    }
}

void plane_fit(int64_t n, const double* xyz, const cba_plane_fit_options& o, double* plane, double* rms, int64_t* count, uint8_t* mask,
               int device) {
    StreamLease lease(device);
    const hipStream_t stream = lease;
    double st[ST_SIZE];
    {
        DevBuf<double> dxyz, px, py, pz;
        DevBuf<int64_t> dn;
        DevBuf<uint8_t> dmask;
        px.alloc(n); py.alloc(n); pz.alloc(n);
        if (mask) dmask.alloc(n);
        dxyz.assign(xyz, 3 * static_cast<size_t>(n), stream);
        dn.assign(&n, 1, stream);
        hipLaunchKernelGGL(k_ls_aos_to_soa, dim3(launch_grid(n, LS_BLOCK, LS_GRID)), dim3(LS_BLOCK), 0, stream, n, dxyz.p, px.p, py.p, pz.p);
        CBA_HIP(hipGetLastError());
        LsTimer tm(stream, false);
        PlaneFitter fit;
        fit.run(stream, n, dn.p, px.p, py.p, pz.p, o, mask ? dmask.p : nullptr, tm);
        fit.st.download(st, ST_SIZE, stream);
        if (mask) dmask.download(mask, n, stream);
        CBA_HIP(hipStreamSynchronize(stream));
    }
    if (o.use_ransac && st[ST_OK] == 0.0) throw std::runtime_error("RANSAC plane fitting failed");
    for (int k = 0; k < 4; ++k) plane[k] = st[ST_PLANE + k];
    *rms = st[ST_RMS];
    *count = static_cast<int64_t>(st[ST_CNT]);
}

}  // namespace cba
