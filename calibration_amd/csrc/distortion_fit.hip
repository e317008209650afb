// distortion_fit.hip — fit_distortion_full / fit_distortion_dual and estimate_intrinsics_linear(_iterative) on the GPU, for a
// batch of independent problems (problem p owns observations [offset[p], offset[p+1])).  The arithmetic is
// distortion_fit_math.hpp; one stream, one synchronise per call:
//   k_df_moments<M, DUAL>   one workgroup of 4 wavefronts per chunk of <= DF_CHUNK observations of one problem (chunk boundaries
//                           are problem-local).  Wavefront w accumulates its own slice of the NM moments over every observation
//                           of the chunk (no lane holds more than 32 accumulators), reduces them with wave_transpose_sum and
//                           writes the chunk's partials [chunk][NM].  DUAL: the moments of fit_distortion_dual's inverse
//                           observations, formed from the chunk's problem K.
//   k_df_chunk_sum<M>       one workgroup per problem: lane k of each wavefront sums moment k (and k + 64) over a fixed share of
//                           the problem's chunks with several loads in flight; the shares are combined in a fixed order
//   k_df_*_tail<M>          one lane per problem: the solve / the K fit / the alternation on the moments alone
//   k_df_residuals<M>       optional: one workgroup per chunk writes the reference's residual vector (rows 2i, 2i + 1)
// Every sum runs in a fixed order that depends only on the problem's own observations, so a problem's results do not depend on
// its position in the batch or on the other problems, and two calls are bitwise identical.
#include <algorithm>
#include <vector>

#include "pipelines.hpp"
#include "distortion_fit_math.hpp"
#include "wave_reduce.hpp"

namespace cba {

constexpr int DF_CHUNK = 4096;  // observations per moment workgroup
constexpr int DF_WAVES = 4;
constexpr int DF_BLOCK = 64 * DF_WAVES;
constexpr int DF_MOM_U = 4;  // observations per lane per trip of the moment walk

template <int M>
struct DfSplit {
    static constexpr int NM = DfitLayout<M>::NM;
    static constexpr int Q = (NM + DF_WAVES - 1) / DF_WAVES;  // moments per wavefront
    static constexpr int QP = TransposeSum<16>::pad(Q);       // padded for the transposed reduction
};

template <int M, bool DUAL, int W>
__device__ __forceinline__ void df_wave_moments(int64_t b, int64_t e, int lane, const double* __restrict__ x, const double* __restrict__ y,
                                                const double* __restrict__ u, const double* __restrict__ v, const double* K,
                                                double* __restrict__ part) {
    using S = DfSplit<M>;
    constexpr int K0 = W * S::Q;
    constexpr int K1 = (K0 + S::Q < S::NM) ? K0 + S::Q : S::NM;
    double acc[S::QP];
#pragma unroll
    for (int j = 0; j < S::QP; ++j) acc[j] = 0.0;
    // DF_MOM_U observations per lane per trip: their loads are all issued (from clamped, valid indices) before any arithmetic, and
    // the moments are added in increasing observation index, so the per-lane order of the sums is that of a plain walk
    for (int64_t i0 = b + lane; i0 < e; i0 += 64 * DF_MOM_U) {
        double ox[DF_MOM_U], oy[DF_MOM_U], ou[DF_MOM_U], ov[DF_MOM_U];
#pragma unroll
        for (int t = 0; t < DF_MOM_U; ++t) {
            const int64_t i = i0 + 64 * t < e ? i0 + 64 * t : e - 1;
            ox[t] = x[i]; oy[t] = y[i]; ou[t] = u[i]; ov[t] = v[i];
        }
#pragma unroll
        for (int t = 0; t < DF_MOM_U; ++t) {
            double xi = ox[t], yi = oy[t], ui = ou[t], vi = ov[t];
            if constexpr (DUAL) dfit_dual_obs(K, ox[t], oy[t], ou[t], ov[t], &xi, &yi, &ui, &vi);
            double mo[S::NM];
            dfit_obs_moments<M>(xi, yi, ui, vi, mo);
            if (i0 + 64 * t < e) {
#pragma unroll
                for (int j = 0; j < K1 - K0; ++j) acc[j] += mo[K0 + j];
            }
        }
    }
    bool owner = false;
    const int base = wave_transpose_sum<S::QP>(acc, lane, &owner);
    if (owner) {
#pragma unroll
        for (int j = 0; j < TransposeSum<S::QP>::CNT; ++j)
            if (base + j < K1 - K0) part[K0 + base + j] = acc[j];
    }
}

template <int M, bool DUAL>
__global__ __launch_bounds__(DF_BLOCK) void k_df_moments(const int64_t* __restrict__ cbeg, const int32_t* __restrict__ cprob,
                                                        const double* __restrict__ x, const double* __restrict__ y,
                                                        const double* __restrict__ u, const double* __restrict__ v,
                                                        const double* __restrict__ K5, double* __restrict__ part) {
    const int c = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = cbeg[c], e = cbeg[c + 1];
    double K[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (DUAL) {
        const double* kp = K5 + 5 * static_cast<int64_t>(cprob[c]);
#pragma unroll
        for (int k = 0; k < 5; ++k) K[k] = kp[k];
    }
    double* out = part + static_cast<int64_t>(c) * DfSplit<M>::NM;
    // wave-uniform branches: each wavefront's moment slice is a compile-time range
    if (wave == 0) df_wave_moments<M, DUAL, 0>(b, e, lane, x, y, u, v, K, out);
    else if (wave == 1) df_wave_moments<M, DUAL, 1>(b, e, lane, x, y, u, v, K, out);
    else if (wave == 2) df_wave_moments<M, DUAL, 2>(b, e, lane, x, y, u, v, K, out);
    else df_wave_moments<M, DUAL, 3>(b, e, lane, x, y, u, v, K, out);
}

// One workgroup of DF_SUM_WAVES wavefronts per problem sums the problem's chunk partials.  Lane k of every wavefront owns moments
// k and k + 64; wavefront w takes the groups of DF_SUM_U consecutive chunks starting at c0 + (w + t DF_SUM_WAVES) DF_SUM_U, one
// running sum per position in the group, so each lane keeps DF_SUM_U x 2 independent loads in flight (the loads of one chunk are
// contiguous over the lanes).  The partial sums are combined in a fixed order: the DF_SUM_U sums of a lane pairwise, then the
// wavefronts in increasing w through LDS.  The order depends only on the problem's chunk count.
constexpr int DF_SUM_WAVES = 16;
constexpr int DF_SUM_U = 4;

template <int M>
__global__ __launch_bounds__(64 * DF_SUM_WAVES) void k_df_chunk_sum(const int32_t* __restrict__ pchunk, const double* __restrict__ part,
                                                                   double* __restrict__ mom) {
    constexpr int NM = DfitLayout<M>::NM;
    constexpr int NK = (NM + 63) / 64;
    static_assert(DF_SUM_U == 4, "the pairwise combination below is written for 4 running sums");
    __shared__ double red[DF_SUM_WAVES][NK * 64];
    const int p = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c0 = pchunk[p], c1 = pchunk[p + 1];
    double acc[NK][DF_SUM_U];
#pragma unroll
    for (int q = 0; q < NK; ++q)
#pragma unroll
        for (int j = 0; j < DF_SUM_U; ++j) acc[q][j] = 0.0;
    for (int g = c0 + wave * DF_SUM_U; g < c1; g += DF_SUM_WAVES * DF_SUM_U) {
        // every load is issued unconditionally from a clamped, valid address before any sum waits on one; out-of-range
        // positions are then left out by a select
        double val[NK][DF_SUM_U];
#pragma unroll
        for (int j = 0; j < DF_SUM_U; ++j)
#pragma unroll
            for (int q = 0; q < NK; ++q) {
                const int c = min(g + j, c1 - 1), k = min(lane + 64 * q, NM - 1);
                val[q][j] = part[static_cast<int64_t>(c) * NM + k];
            }
#pragma unroll
        for (int j = 0; j < DF_SUM_U; ++j)
#pragma unroll
            for (int q = 0; q < NK; ++q)
                if (g + j < c1) acc[q][j] += val[q][j];
    }
#pragma unroll
    for (int q = 0; q < NK; ++q) red[wave][q * 64 + lane] = (acc[q][0] + acc[q][1]) + (acc[q][2] + acc[q][3]);
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < NK; ++q) {
            const int k = lane + 64 * q;
            double sum = 0.0;
#pragma unroll
            for (int w = 0; w < DF_SUM_WAVES; ++w) sum += red[w][q * 64 + lane];
            if (k < NM) mom[static_cast<int64_t>(p) * NM + k] = sum;
        }
    }
}

template <int M>
__global__ __launch_bounds__(64) void k_df_fit_tail(int n_problems, const int64_t* __restrict__ off, const double* __restrict__ mom_f,
                                                   const double* __restrict__ mom_i, const double* __restrict__ K5, DfitFixed fixed,
                                                   double* __restrict__ coeffs, double* __restrict__ inverse, int32_t* __restrict__ ok) {
    constexpr int NM = DfitLayout<M>::NM;
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_problems) return;
    const bool good = off[p + 1] - off[p] >= DFIT_MIN_FIT_OBS;
    ok[p] = good ? 1 : 0;
    double K[5], a[M];
#pragma unroll
    for (int k = 0; k < 5; ++k) K[k] = K5[5 * static_cast<int64_t>(p) + k];
#pragma unroll
    for (int i = 0; i < M; ++i) a[i] = 0.0;
    if (good) dfit_solve<M>(mom_f + static_cast<int64_t>(p) * NM, K, fixed, a);
#pragma unroll
    for (int i = 0; i < M; ++i) coeffs[static_cast<int64_t>(p) * M + i] = a[i];
    if (mom_i) {
#pragma unroll
        for (int i = 0; i < M; ++i) a[i] = 0.0;
        if (good) dfit_solve<M>(mom_i + static_cast<int64_t>(p) * NM, K, fixed, a);
#pragma unroll
        for (int i = 0; i < M; ++i) inverse[static_cast<int64_t>(p) * M + i] = a[i];
    }
}

__global__ __launch_bounds__(64) void k_df_linear_tail(int n_problems, const int64_t* __restrict__ off, const double* __restrict__ mom,
                                                      int use_skew, DfitBounds B, double* __restrict__ K5, int32_t* __restrict__ status,
                                                      int32_t* __restrict__ fallback) {
    constexpr int NM = DfitLayout<2>::NM;
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_problems) return;
    double K[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int fb = 0, st = DFIT_TOO_FEW;
    if (off[p + 1] - off[p] >= DFIT_MIN_K_OBS) {
        st = dfit_linear_k<2>(mom + static_cast<int64_t>(p) * NM, nullptr, nullptr, use_skew != 0, B, K, &fb);
        if (st != DFIT_OK) {
#pragma unroll
            for (int k = 0; k < 5; ++k) K[k] = 0.0;
            fb = 0;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) K5[5 * static_cast<int64_t>(p) + k] = K[k];
    status[p] = st;
    fallback[p] = fb;
}

template <int M>
__global__ __launch_bounds__(64) void k_df_iter_tail(int n_problems, const int64_t* __restrict__ off, const double* __restrict__ mom,
                                                    int max_iterations, int use_skew, double* __restrict__ K5, double* __restrict__ coeffs,
                                                    int32_t* __restrict__ status, int32_t* __restrict__ iterations,
                                                    int32_t* __restrict__ fallback) {
    constexpr int NM = DfitLayout<M>::NM;
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_problems) return;
    double K[5], a[M];
    int it = 0, fb = 0;
    const int st = dfit_iterative<M>(mom + static_cast<int64_t>(p) * NM, off[p + 1] - off[p], max_iterations, use_skew != 0, K, a, &it, &fb);
#pragma unroll
    for (int k = 0; k < 5; ++k) K5[5 * static_cast<int64_t>(p) + k] = K[k];
#pragma unroll
    for (int i = 0; i < M; ++i) coeffs[static_cast<int64_t>(p) * M + i] = a[i];
    status[p] = st;
    iterations[p] = it;
    fallback[p] = fb;
}

template <int M>
__global__ __launch_bounds__(DF_BLOCK) void k_df_residuals(const int64_t* __restrict__ cbeg, const int32_t* __restrict__ cprob,
                                                          const double* __restrict__ x, const double* __restrict__ y,
                                                          const double* __restrict__ u, const double* __restrict__ v,
                                                          const double* __restrict__ K5, const double* __restrict__ coeffs,
                                                          const int32_t* __restrict__ ok, double* __restrict__ res) {
    const int c = blockIdx.x;
    const int p = cprob[c];
    const int64_t b = cbeg[c], e = cbeg[c + 1];
    double K[5], a[M];
#pragma unroll
    for (int k = 0; k < 5; ++k) K[k] = K5[5 * static_cast<int64_t>(p) + k];
#pragma unroll
    for (int i = 0; i < M; ++i) a[i] = coeffs[static_cast<int64_t>(p) * M + i];
    const bool good = ok[p] != 0;
    for (int64_t i = b + threadIdx.x; i < e; i += DF_BLOCK) {
        double ru = 0.0, rv = 0.0;
        if (good) dfit_residual<M>(x[i], y[i], u[i], v[i], K, a, &ru, &rv);
        res[2 * i] = ru;
        res[2 * i + 1] = rv;
    }
}

// ---- host glue -----------------------------------------------------------------------------------------------------------
namespace {

// device events between the stages (experiment builds' stage timing): 5 start, 0 uploaded, 1 moment passes, 2 chunk sums, 3 tail,
// 4 residuals
using DfTimer = StageTimer<6>;

// the observations, the problem offsets and the chunk table, on the device (the host tables live as long as the call)
struct DfInput {
    int n_problems = 0, n_chunks = 0;
    std::vector<int64_t> hb;
    std::vector<int32_t> hp, hc;
    ObsSoA obs;
    DevBuf<int64_t> cbeg;
    DevBuf<int32_t> cprob, pchunk;

    DfInput(int P, const int64_t* offset, const double* hx, const double* hy, const double* hu, const double* hv, hipStream_t s) {
        n_problems = P;
        hc.assign(static_cast<size_t>(P) + 1, 0);
        for (int p = 0; p < P; ++p) {
            hc[p] = static_cast<int32_t>(hp.size());
            for (int64_t i = offset[p]; i < offset[p + 1]; i += DF_CHUNK) {
                hb.push_back(i);
                hp.push_back(p);
            }
        }
        hc[P] = static_cast<int32_t>(hp.size());
        hb.push_back(offset[P]);
        n_chunks = static_cast<int>(hp.size());
        obs.upload(s, P, offset, hx, hy, hu, hv);
        cbeg.assign(hb.data(), hb.size(), s);
        cprob.assign(hp.data(), hp.size(), s);
        pchunk.assign(hc.data(), hc.size(), s);
    }
};

// the chunk partials [n_chunks][NM] of the observations (dual: of the inverse observations, formed with dK)
template <int M>
void df_moment_pass(const DfInput& in, bool dual, const double* dK, DevBuf<double>& part, hipStream_t s) {
    constexpr int NM = DfitLayout<M>::NM;
    part.alloc(static_cast<size_t>(std::max(in.n_chunks, 1)) * NM);
    if (in.n_chunks == 0) return;
    if (dual)
        hipLaunchKernelGGL((k_df_moments<M, true>), dim3(in.n_chunks), dim3(DF_BLOCK), 0, s, in.cbeg.p, in.cprob.p, in.obs.X.p, in.obs.Y.p,
                           in.obs.u.p, in.obs.v.p, dK, part.p);
    else
        hipLaunchKernelGGL((k_df_moments<M, false>), dim3(in.n_chunks), dim3(DF_BLOCK), 0, s, in.cbeg.p, in.cprob.p, in.obs.X.p, in.obs.Y.p,
                           in.obs.u.p, in.obs.v.p, dK, part.p);
    CBA_HIP(hipGetLastError());
}

// the problems' moments [P][NM] from the chunk partials
template <int M>
void df_chunk_sum(const DfInput& in, const DevBuf<double>& part, DevBuf<double>& mom, hipStream_t s) {
    mom.alloc(static_cast<size_t>(in.n_problems) * DfitLayout<M>::NM);
    hipLaunchKernelGGL((k_df_chunk_sum<M>), dim3(in.n_problems), dim3(64 * DF_SUM_WAVES), 0, s, in.pchunk.p, part.p, mom.p);
    CBA_HIP(hipGetLastError());
}

inline unsigned df_lane_blocks(int n) { return static_cast<unsigned>((n + 63) / 64); }

template <int M>
void df_fit_m(int P, const int64_t* offset, const double* x, const double* y, const double* u, const double* v, const double* kmtx5,
              const DfitFixed& fixed, bool dual, double* coeffs, double* inverse, int32_t* ok, double* residuals, double* stage_ms) {
    StreamLease lease;
    const hipStream_t s = lease;
    DfTimer tm(s, stage_ms != nullptr);
    tm.mark(5);
    DfInput in(P, offset, x, y, u, v, s);
    DevBuf<double> dK, partf, momf, parti, momi, dC, dI, dR;
    DevBuf<int32_t> dok;
    dK.assign(kmtx5, 5 * static_cast<size_t>(P), s);
    dC.alloc(static_cast<size_t>(P) * M);
    dok.alloc(static_cast<size_t>(P));
    if (dual) dI.alloc(static_cast<size_t>(P) * M);
    tm.mark(0);
    df_moment_pass<M>(in, false, dK.p, partf, s);
    if (dual) df_moment_pass<M>(in, true, dK.p, parti, s);
    tm.mark(1);
    df_chunk_sum<M>(in, partf, momf, s);
    if (dual) df_chunk_sum<M>(in, parti, momi, s);
    tm.mark(2);
    hipLaunchKernelGGL((k_df_fit_tail<M>), dim3(df_lane_blocks(P)), dim3(64), 0, s, P, in.obs.off.p, momf.p, dual ? momi.p : nullptr, dK.p,
                       fixed, dC.p, dual ? dI.p : nullptr, dok.p);
    CBA_HIP(hipGetLastError());
    tm.mark(3);
    const int64_t n = offset[P];
    if (residuals && in.n_chunks > 0) {
        dR.alloc(2 * static_cast<size_t>(n));
        hipLaunchKernelGGL((k_df_residuals<M>), dim3(in.n_chunks), dim3(DF_BLOCK), 0, s, in.cbeg.p, in.cprob.p, in.obs.X.p, in.obs.Y.p,
                           in.obs.u.p, in.obs.v.p, dK.p, dC.p, dok.p, dR.p);
        CBA_HIP(hipGetLastError());
    }
    tm.mark(4);
    dC.download(coeffs, static_cast<size_t>(P) * M, s);
    if (dual) dI.download(inverse, static_cast<size_t>(P) * M, s);
    dok.download(ok, static_cast<size_t>(P), s);
    if (residuals && in.n_chunks > 0) dR.download(residuals, 2 * static_cast<size_t>(n), s);
    CBA_HIP(hipStreamSynchronize(s));
    if (stage_ms) {  // moment passes, chunk sums, uploads, tail, residuals, total without uploads
        stage_ms[0] = tm.ms(0, 1);
        stage_ms[1] = tm.ms(1, 2);
        stage_ms[2] = tm.ms(5, 0);
        stage_ms[3] = tm.ms(2, 3);
        stage_ms[4] = tm.ms(3, 4);
        stage_ms[5] = tm.ms(0, 4);
    }
}

template <int M>
void df_iter_m(int P, const int64_t* offset, const double* x, const double* y, const double* u, const double* v, int max_iterations,
               int use_skew, double* kmtx5, double* coeffs, int32_t* status, int32_t* iterations, int32_t* fallback, double* stage_ms) {
    StreamLease lease;
    const hipStream_t s = lease;
    DfTimer tm(s, stage_ms != nullptr);
    tm.mark(5);
    DfInput in(P, offset, x, y, u, v, s);
    DevBuf<double> part, mom, dK, dC;
    DevBuf<int32_t> dst, dit, dfb;
    dK.alloc(5 * static_cast<size_t>(P)); dC.alloc(static_cast<size_t>(P) * M);
    dst.alloc(static_cast<size_t>(P)); dit.alloc(static_cast<size_t>(P)); dfb.alloc(static_cast<size_t>(P));
    tm.mark(0);
    df_moment_pass<M>(in, false, nullptr, part, s);
    tm.mark(1);
    df_chunk_sum<M>(in, part, mom, s);
    tm.mark(2);
    hipLaunchKernelGGL((k_df_iter_tail<M>), dim3(df_lane_blocks(P)), dim3(64), 0, s, P, in.obs.off.p, mom.p, max_iterations, use_skew, dK.p,
                       dC.p, dst.p, dit.p, dfb.p);
    CBA_HIP(hipGetLastError());
    tm.mark(3);
    tm.mark(4);
    dK.download(kmtx5, 5 * static_cast<size_t>(P), s);
    dC.download(coeffs, static_cast<size_t>(P) * M, s);
    dst.download(status, static_cast<size_t>(P), s);
    dit.download(iterations, static_cast<size_t>(P), s);
    dfb.download(fallback, static_cast<size_t>(P), s);
    CBA_HIP(hipStreamSynchronize(s));
    if (stage_ms) {
        stage_ms[0] = tm.ms(0, 1);
        stage_ms[1] = tm.ms(1, 2);
        stage_ms[2] = tm.ms(5, 0);
        stage_ms[3] = tm.ms(2, 3);
        stage_ms[4] = 0.0;
        stage_ms[5] = tm.ms(0, 4);
    }
}

}  // namespace

void distortion_fit_gpu(int n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v,
                        const double* kmtx5, int num_radial, int fixed_mask, const double* fixed_val5, bool dual, double* coeffs,
                        double* inverse, int32_t* ok, double* residuals, double* stage_ms, int device) {
    CBA_HIP(hipSetDevice(device));
    DfitFixed fixed{fixed_mask, {0.0, 0.0, 0.0, 0.0, 0.0}};
    for (int i = 0; i < DFIT_MAX_M; ++i) fixed.val[i] = fixed_val5[i];
    switch (num_radial) {
        case 0: df_fit_m<2>(n_problems, offset, x, y, u, v, kmtx5, fixed, dual, coeffs, inverse, ok, residuals, stage_ms); break;
        case 1: df_fit_m<3>(n_problems, offset, x, y, u, v, kmtx5, fixed, dual, coeffs, inverse, ok, residuals, stage_ms); break;
        case 2: df_fit_m<4>(n_problems, offset, x, y, u, v, kmtx5, fixed, dual, coeffs, inverse, ok, residuals, stage_ms); break;
        default: df_fit_m<5>(n_problems, offset, x, y, u, v, kmtx5, fixed, dual, coeffs, inverse, ok, residuals, stage_ms); break;
    }
}

void intrinsics_linear_gpu(int n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v,
                           const double* bounds_lo5, const double* bounds_hi5, int use_skew, double* kmtx5, int32_t* status,
                           int32_t* fallback, int device) {
    CBA_HIP(hipSetDevice(device));
    DfitBounds bounds;
    for (int k = 0; k < 5; ++k) {
        bounds.lo[k] = bounds_lo5[k];
        bounds.hi[k] = bounds_hi5[k];
    }
    StreamLease lease;
    const hipStream_t s = lease;
    DfInput in(n_problems, offset, x, y, u, v, s);
    DevBuf<double> part, mom, dK;
    DevBuf<int32_t> dst, dfb;
    dK.alloc(5 * static_cast<size_t>(n_problems));
    dst.alloc(static_cast<size_t>(n_problems)); dfb.alloc(static_cast<size_t>(n_problems));
    // the K fit without distortion reads only the 11 scalar sums of the nr = 0 layout; the 28 others cost one extra wavefront's
    // accumulation per chunk in a call that is bound by its upload, and the shared moment kernel keeps one reduction order
    df_moment_pass<2>(in, false, nullptr, part, s);
    df_chunk_sum<2>(in, part, mom, s);
    hipLaunchKernelGGL(k_df_linear_tail, dim3(df_lane_blocks(n_problems)), dim3(64), 0, s, n_problems, in.obs.off.p, mom.p, use_skew, bounds,
                       dK.p, dst.p, dfb.p);
    CBA_HIP(hipGetLastError());
    dK.download(kmtx5, 5 * static_cast<size_t>(n_problems), s);
    dst.download(status, static_cast<size_t>(n_problems), s);
    dfb.download(fallback, static_cast<size_t>(n_problems), s);
    CBA_HIP(hipStreamSynchronize(s));
}

void intrinsics_linear_iterative_gpu(int n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v,
                                     int num_radial, int max_iterations, int use_skew, double* kmtx5, double* coeffs, int32_t* status,
                                     int32_t* iterations, int32_t* fallback, double* stage_ms, int device) {
    CBA_HIP(hipSetDevice(device));
    switch (num_radial) {
        case 0: df_iter_m<2>(n_problems, offset, x, y, u, v, max_iterations, use_skew, kmtx5, coeffs, status, iterations, fallback, stage_ms); break;
        case 1: df_iter_m<3>(n_problems, offset, x, y, u, v, max_iterations, use_skew, kmtx5, coeffs, status, iterations, fallback, stage_ms); break;
        case 2: df_iter_m<4>(n_problems, offset, x, y, u, v, max_iterations, use_skew, kmtx5, coeffs, status, iterations, fallback, stage_ms); break;
        default: df_iter_m<5>(n_problems, offset, x, y, u, v, max_iterations, use_skew, kmtx5, coeffs, status, iterations, fallback, stage_ms); break;
    }
}

}  // namespace cba
