// residual_stats.hip — reprojection diagnostics: raw residual statistics over the Mode R tiles.
//
//   k_resid_stats<MODEL, T, FETCH>  one WAVEFRONT per Mode R tile (Engine::tilesB): per observation r = projection - observation
//                                   (reproj_residual, resid_tile's expression order) and e2 = r_u^2 + r_v^2 in fp64 with no FMA
//                                   contraction; one partial row {sum e2, max e2, #not kept, #obs} per tile.  FETCH: also r_u, r_v
//                                   (SoA) and a keep byte per observation, at the padded index relative to the range's first block
//   k_stats_blocks                  fixed-order combine of a block's tile rows (sums in tile order, max for the max)
//   k_stats_total                   fixed-order tree over the blocks (one workgroup)
//
// No atomics: two calls give the same bits.  The pass refreshes the block constants like cba_reproj_cost and otherwise writes only
// its own buffers (Engine::diag_*): never partial / blk_s / blk_w / scalar_out, the LM state or the gate, and its launches do not
// read the gate.
#include <cmath>

#include "engine.hpp"
#include "reproj_math.hpp"
#include "wave_reduce.hpp"

namespace cba {

namespace {

__device__ __forceinline__ int64_t stats_wave_index() {
    return static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

// e2 of one observation, never contracted into an FMA: numpy reproduces it bit for bit from the fetched residuals
__device__ __forceinline__ double sq_norm_nc(double a, double b) {
#pragma clang fp contract(off)
    return a * a + b * b;
}

constexpr int STATS_W = 4;   // partial row: {sum e2, max e2, #not kept, #obs}
constexpr int STATS_U = 8;   // 64-observation passes whose loads are issued together (32 loads in flight per lane)

// t2: the largest e2 whose sqrt is <= the threshold (capi.cpp keep_bound), so "kept" is exactly sqrt(e2) <= threshold_px; NaN is
// never kept.  Lanes past the tile's end load the tile's first observation (in bounds) and are masked out of every result.
template <int MODEL, typename T, bool FETCH>
__global__ __launch_bounds__(256) void k_resid_stats(const Tile* __restrict__ tiles, int64_t n_tiles, const T* __restrict__ bc,
                                                     const T* __restrict__ intr, const T* __restrict__ sd,
                                                     const int32_t* __restrict__ blk_cam, const T* __restrict__ X,
                                                     const T* __restrict__ Y, const T* __restrict__ u, const T* __restrict__ v,
                                                     double t2, double* __restrict__ part, double* __restrict__ ru,
                                                     double* __restrict__ rv, uint8_t* __restrict__ keep, int64_t out_base) {
    constexpr int PI = IntrSize<MODEL>::value;
    const int64_t w = stats_wave_index();
    if (w >= n_tiles) return;
    const Tile t = tiles[w];
    const int lane = threadIdx.x & 63;
    const T* bcp = bc + static_cast<int64_t>(t.blk) * BC_SIZE;
    const int cam = blk_cam[t.blk];
    const T* ip = intr + static_cast<int64_t>(cam) * PI;
    const T* sp = sd + static_cast<int64_t>(cam) * SD_SIZE;
    double s = 0.0, m = 0.0;
    uint64_t over = 0;  // wave-uniform
#pragma unroll 1
    for (int k0 = 0; 64 * k0 < t.count; k0 += STATS_U) {
        T xs[STATS_U], ys[STATS_U], us[STATS_U], vs[STATS_U];
#pragma unroll
        for (int q = 0; q < STATS_U; ++q) {
            const int j = lane + 64 * (k0 + q);
            const int jj = j < t.count ? j : 0;
            xs[q] = X[t.xy_start + jj]; ys[q] = Y[t.xy_start + jj];
            us[q] = u[t.start + jj]; vs[q] = v[t.start + jj];
        }
#pragma unroll
        for (int q = 0; q < STATS_U; ++q) {
            const int j = lane + 64 * (k0 + q);
            const bool valid = j < t.count;
            T rr[2];
            reproj_residual<MODEL, T>(bcp, ip, sp, xs[q], ys[q], us[q], vs[q], rr);
            const double e2 = sq_norm_nc(static_cast<double>(rr[0]), static_cast<double>(rr[1]));
            const bool in = e2 <= t2;  // false for NaN
            if (valid) {
                s += e2;
                m = fmax(m, e2);
            }
            over += static_cast<uint64_t>(__popcll(__ballot(valid && !in)));
            if (FETCH && valid) {
                const int64_t o = t.start + j - out_base;
                ru[o] = static_cast<double>(rr[0]);
                rv[o] = static_cast<double>(rr[1]);
                keep[o] = in ? 1 : 0;
            }
        }
    }
    s = wave_sum63(s);
    m = wave_max63(m);
    if (lane == 63) {
        double* p = part + w * STATS_W;
        p[0] = s;
        p[1] = m;
        p[2] = static_cast<double>(over);
        p[3] = static_cast<double>(t.count);
    }
}

__global__ void k_stats_blocks(int n_blocks, const int64_t* __restrict__ blk_tile_off, const double* __restrict__ part,
                               double* __restrict__ out) {
    const int b = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n_blocks) return;
    double s = 0.0, m = 0.0, c = 0.0, n = 0.0;
    for (int64_t t = blk_tile_off[b]; t < blk_tile_off[b + 1]; ++t) {
        s += part[t * STATS_W];
        m = fmax(m, part[t * STATS_W + 1]);
        c += part[t * STATS_W + 2];
        n += part[t * STATS_W + 3];
    }
    double* o = out + static_cast<int64_t>(b) * STATS_W;
    o[0] = s; o[1] = m; o[2] = c; o[3] = n;
}

__global__ __launch_bounds__(256) void k_stats_total(int n_blocks, const double* __restrict__ blk, double* __restrict__ out) {
    __shared__ double sh[STATS_W][256];
    double a[STATS_W] = {0.0, 0.0, 0.0, 0.0};
    for (int b = static_cast<int>(threadIdx.x); b < n_blocks; b += 256) {
        const double* r = blk + static_cast<int64_t>(b) * STATS_W;
        a[0] += r[0];
        a[1] = fmax(a[1], r[1]);
        a[2] += r[2];
        a[3] += r[3];
    }
    for (int k = 0; k < STATS_W; ++k) sh[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (static_cast<int>(threadIdx.x) < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] = fmax(sh[1][threadIdx.x], sh[1][threadIdx.x + o]);
            sh[2][threadIdx.x] += sh[2][threadIdx.x + o];
            sh[3][threadIdx.x] += sh[3][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < STATS_W) out[threadIdx.x] = sh[threadIdx.x][0];
}

template <bool FETCH>
void launch_stats_tiles(Engine& e, int64_t tile0, int64_t n_tiles, double t2, double* part, double* ru, double* rv, uint8_t* keep,
                        int64_t out_base) {
    if (n_tiles <= 0) return;
    const dim3 g(static_cast<unsigned>((n_tiles + 3) / 4)), blk(256);
    const Tile* tl = e.tilesB.p + tile0;
#define STATS_F64(M) hipLaunchKernelGGL((k_resid_stats<M, double, FETCH>), g, blk, 0, e.stream, tl, n_tiles, e.bc.p, e.intr[e.active].p, \
                                        e.sd.p, e.d_blk_cam.p, e.X.p, e.Y.p, e.u.p, e.v.p, t2, part, ru, rv, keep, out_base)
#define STATS_F32(M) hipLaunchKernelGGL((k_resid_stats<M, float, FETCH>), g, blk, 0, e.stream, tl, n_tiles, e.bcf.p, e.intrf.p, e.sdf.p, \
                                        e.d_blk_cam.p, e.Xf.p, e.Yf.p, e.uf.p, e.vf.p, t2, part, ru, rv, keep, out_base)
    if (e.model == CAM_PINHOLE_BC) { if (e.scalar) STATS_F32(CAM_PINHOLE_BC); else STATS_F64(CAM_PINHOLE_BC); }
    else { if (e.scalar) STATS_F32(CAM_SCHEIMPFLUG); else STATS_F64(CAM_SCHEIMPFLUG); }
#undef STATS_F64
#undef STATS_F32
}

// block constants of the current parameters, launched unconditionally (the gate belongs to the LM driver)
void refresh_consts(Engine& e) {
    const double* g = e.gate;
    e.gate = nullptr;
    launch_block_consts(e, 0);
    e.gate = g;
}

}  // namespace

void residual_stats_launch(Engine& e, double t2) {
    refresh_consts(e);
    const size_t nt = static_cast<size_t>(std::max<int64_t>(1, e.n_tilesB)) * STATS_W;
    const size_t nb = static_cast<size_t>(std::max(1, e.n_blocks)) * STATS_W;
    e.diag_part.ensure(nt);
    e.diag_blk.ensure(nb);
    e.diag_tot.ensure(STATS_W);
    launch_stats_tiles<false>(e, 0, e.n_tilesB, t2, e.diag_part.p, nullptr, nullptr, nullptr, 0);
    if (e.n_blocks > 0)
        hipLaunchKernelGGL(k_stats_blocks, dim3(static_cast<unsigned>((e.n_blocks + 255) / 256)), dim3(256), 0, e.stream, e.n_blocks,
                           e.d_blk_tile_off.p, e.diag_part.p, e.diag_blk.p);
    hipLaunchKernelGGL(k_stats_total, dim3(1), dim3(256), 0, e.stream, e.n_blocks, e.diag_blk.p, e.diag_tot.p);
    CBA_HIP(hipGetLastError());
}

void residual_stats(Engine& e, double t2, double* blk_stats, double* total) {
    residual_stats_launch(e, t2);
    if (blk_stats && e.n_blocks > 0) e.diag_blk.download(blk_stats, static_cast<size_t>(e.n_blocks) * STATS_W, e.stream);
    if (total) e.diag_tot.download(total, STATS_W, e.stream);
    CBA_HIP(hipStreamSynchronize(e.stream));
    // max e2 -> max sqrt(e2) (px): sqrt is monotone and correctly rounded on the host, so this IS the largest per-observation error
    if (blk_stats)
        for (int b = 0; b < e.n_blocks; ++b) blk_stats[static_cast<int64_t>(b) * STATS_W + 1] = std::sqrt(blk_stats[static_cast<int64_t>(b) * STATS_W + 1]);
    if (total) total[1] = std::sqrt(total[1]);
}

void residuals_fetch_range(Engine& e, int b0, int b1, double t2, double* r, uint8_t* keep) {
    if (b1 <= b0) return;
    refresh_consts(e);
    const int64_t tb0 = e.blk_tile_off[b0], tb1 = e.blk_tile_off[b1];
    const int64_t p0 = e.pad_offset[b0], np = e.pad_offset[b1] - p0;
    // sized to the requested range (grown, never to the whole problem unless the whole problem is asked for)
    const size_t nt = static_cast<size_t>(std::max<int64_t>(1, tb1 - tb0)) * STATS_W;
    const size_t no = static_cast<size_t>(std::max<int64_t>(2, np));
    e.diag_fpart.ensure(nt);
    if (e.diag_ru.n < no) { e.diag_ru.alloc(no); e.diag_rv.alloc(no); e.diag_keep.alloc(no); }
    launch_stats_tiles<true>(e, tb0, tb1 - tb0, t2, e.diag_fpart.p, e.diag_ru.p, e.diag_rv.p, e.diag_keep.p, p0);
    CBA_HIP(hipGetLastError());
    std::vector<double> hu(static_cast<size_t>(r ? np : 0)), hv(static_cast<size_t>(r ? np : 0));
    std::vector<uint8_t> hk(static_cast<size_t>(keep ? np : 0));
    if (r) {
        e.diag_ru.download(hu.data(), static_cast<size_t>(np), e.stream);
        e.diag_rv.download(hv.data(), static_cast<size_t>(np), e.stream);
    }
    if (keep) e.diag_keep.download(hk.data(), static_cast<size_t>(np), e.stream);
    CBA_HIP(hipStreamSynchronize(e.stream));
    // padded SoA -> the Ceres layout of cba_reproj_eval_fetch_blocks (indexed from block b0's first observation)
    const int64_t base = e.blk_offset[b0];
    for (int b = b0; b < b1; ++b) {
        const int64_t n = e.blk_offset[b + 1] - e.blk_offset[b], pb = e.pad_offset[b] - p0, ob = e.blk_offset[b] - base;
        for (int64_t j = 0; j < n; ++j) {
            if (r) { r[2 * (ob + j)] = hu[static_cast<size_t>(pb + j)]; r[2 * (ob + j) + 1] = hv[static_cast<size_t>(pb + j)]; }
            if (keep) keep[ob + j] = hk[static_cast<size_t>(pb + j)];
        }
    }
}

}  // namespace cba
