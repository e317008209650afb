// lm_kernels.hpp — the O(#views) / O(#blocks) device code of one LM step.  Included by backend_hip.hip ALONE: the kernels stay
// in HipBackend's translation unit (one code object, loaded once by init_lm_state), as mode_b.hpp's do in kernels_modeb.hip.
//
// The bodies:
//   weights          rho'(s_b) per residual block (ceres HuberLoss + corrector)
//   cam_partial      weighted per-camera sums of the block normal equations (chunked, fixed order), seg_sum their totals
//   schur_view_wave  per private view, one wavefront: damped H_pp = L L^T, y = L^-1 g_p, Z_b = L^-1 E_b
//   schur_syrk       S_schur = sum_v Z_v^T Z_v (+ g_schur = sum_v Z_v^T y_v), 64x64 output tiles, VALU or fp64 MFMA
//   backsub          delta_p, trial poses, step norms and the views' share of the model-cost terms
// In the LM loop the bodies that do not depend on each other share launches (k_step_head, k_sys_stage2, k_sys_stage3, k_sys_pack:
// "the fused stages" below); the one-kernel-per-body launches remain for the paths off the loop.
// All reductions are two-stage with a fixed summation order (no atomics on fp64), so runs are
// bitwise reproducible and 1/2/4/8-rank runs differ only by the all-reduce's own rounding.
#pragma once
#include "block_reduce.hpp"
#include "lm_ctl.hpp"
#include "schur_math.hpp"
#include "wave_reduce.hpp"

namespace cba {

constexpr int VCHUNK = 8;    // views per syrk / gvec workgroup
constexpr size_t CTL_REC_FETCH = 2 * CS_COUNT + 8;  // HipLMState::ctl_rec = [control record | staged scalars + lmp | fetched parameters]
constexpr int CCHUNK = 16;   // blocks per camera-sum chunk

__global__ void k_weights(int n_blocks, int NACC, int s_idx, const double* __restrict__ blk_acc, double huber_delta,
                          double* __restrict__ blk_w, double* __restrict__ blk_s) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const double s = blk_acc[static_cast<int64_t>(b) * NACC + s_idx];
    double rho, w;
    huber(s, huber_delta, &rho, &w);
    blk_w[b] = w;
    blk_s[b] = s;
}

// k_weights and k_cost (kernels_reproj.hip) in one launch for up to 4096 blocks: the same per-thread strides and the same LDS
// tree as k_cost, so the cost is bit-identical to the two-kernel form.  out = {1/2 sum rho(s_b), sum s_b} (may be pinned host memory)
__global__ __launch_bounds__(256) void k_weights_cost(int n_blocks, int NACC, int s_idx, const double* __restrict__ blk_acc,
                                                      double huber_delta, double* __restrict__ blk_w, double* __restrict__ blk_s,
                                                      double* __restrict__ out) {
    __shared__ double sh[2][256];
    double c = 0.0, ss = 0.0;
    // up to 16 independent loads in flight per thread (each is a cache line of its own: one block's |r|^2), summed in the same order
    constexpr int NQ = 16;
    for (int b0 = static_cast<int>(threadIdx.x); b0 < n_blocks; b0 += NQ * 256) {
        double sv[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int b = b0 + q * 256;
            sv[q] = b < n_blocks ? blk_acc[static_cast<int64_t>(b) * NACC + s_idx] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int b = b0 + q * 256;
            if (b < n_blocks) {
                double rho, w;
                huber(sv[q], huber_delta, &rho, &w);
                blk_w[b] = w;
                blk_s[b] = sv[q];
                c += 0.5 * rho;
                ss += sv[q];
            }
        }
    }
    block_sum2(sh, c, ss, out);
}

// partial[k][e] = sum over chunk k's blocks (in list order) of w_b * acc[b][e]
__device__ __forceinline__ void cam_partial_body(int k, int NACC, const int64_t* __restrict__ chunk_off, const int32_t* __restrict__ cam_blk,
                                                 const double* __restrict__ blk_w, const double* __restrict__ blk_acc,
                                                 double* __restrict__ partial) {
    const int64_t p0 = chunk_off[k], p1 = chunk_off[k + 1];
    for (int e = threadIdx.x; e < NACC; e += blockDim.x) {
        double s = 0.0;
        for (int64_t p = p0; p < p1; p += CCHUNK) {  // the chunk's block rows in flight together, added in list order
            double a[CCHUNK], w[CCHUNK];
#pragma unroll
            for (int q = 0; q < CCHUNK; ++q) {
                const bool in = p + q < p1;
                const int b = in ? cam_blk[p + q] : 0;
                w[q] = in ? blk_w[b] : 0.0;
                a[q] = in ? blk_acc[static_cast<int64_t>(b) * NACC + e] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < CCHUNK; ++q)
                if (p + q < p1) s += w[q] * a[q];
        }
        partial[static_cast<int64_t>(k) * NACC + e] = s;
    }
}
__global__ void k_cam_partial(int NACC, const int64_t* __restrict__ chunk_off, const int32_t* __restrict__ cam_blk,
                              const double* __restrict__ blk_w, const double* __restrict__ blk_acc,
                              double* __restrict__ partial) {
    cam_partial_body(blockIdx.x, NACC, chunk_off, cam_blk, blk_w, blk_acc, partial);
}

// Column sums of a row-major partial table in a FIXED order, 8 row groups per column: thread (column c, group r)
// adds rows r, r+8, r+16, ... and the 8 group sums are combined in group order through LDS — 8x the parallelism
// and 1/8 the dependent chain of one thread per column (125 chunk rows at 1000 views, 500 at 4000).
constexpr int RS_COLS = 32, RS_GROUPS = 8;

__device__ __forceinline__ double grouped_column_sum(const double* __restrict__ rows, int64_t t0, int64_t t1, int64_t width,
                                                     int64_t e, bool valid, double (*sh)[RS_COLS]) {
    const int c = threadIdx.x % RS_COLS, r = threadIdx.x / RS_COLS;
    double s = 0.0;
    if (valid)
        for (int64_t t = t0 + r; t < t1; t += RS_GROUPS) s += rows[t * width + e];
    sh[r][c] = s;
    __syncthreads();
    double tot = 0.0;
    if (r == 0)
        for (int k = 0; k < RS_GROUPS; ++k) tot += sh[k][c];
    __syncthreads();
    return tot;
}

// out[o][e] = sum_{t in [seg[o], seg[o+1])} rows[t][e]; grid (ceil(width / 32), n_out), 256 threads
__device__ __forceinline__ void seg_sum_body(double* lds, int bx, int o, int width, const int64_t* __restrict__ seg, const double* __restrict__ rows,
                                             double* __restrict__ out) {
    double (*sh)[RS_COLS] = reinterpret_cast<double (*)[RS_COLS]>(lds);
    const int64_t e = static_cast<int64_t>(bx) * RS_COLS + threadIdx.x % RS_COLS;
    const double tot = grouped_column_sum(rows, seg[o], seg[o + 1], width, e, e < width, sh);
    if (threadIdx.x < RS_COLS && e < width) out[static_cast<int64_t>(o) * width + e] = tot;
}
__global__ __launch_bounds__(RS_COLS * RS_GROUPS) void k_seg_sum(int n_out, int width, const int64_t* __restrict__ seg,
                                                                  const double* __restrict__ rows, double* __restrict__ out) {
    __shared__ double lds[RS_GROUPS * RS_COLS];
    (void)n_out;
    seg_sum_body(lds, blockIdx.x, blockIdx.y, width, seg, rows, out);
}

// out[e] = sum_{t < n_rows} rows[t][e]; grid ceil(width / 32), 256 threads
__global__ __launch_bounds__(RS_COLS * RS_GROUPS) void k_row_sum(int64_t n_rows, int64_t width, const double* __restrict__ rows,
                                                                  double* __restrict__ out) {
    __shared__ double sh[RS_GROUPS][RS_COLS];
    const int64_t e = static_cast<int64_t>(blockIdx.x) * RS_COLS + threadIdx.x % RS_COLS;
    const double tot = grouped_column_sum(rows, 0, n_rows, width, e, e < width, sh);
    if (threadIdx.x < RS_COLS && e < width) out[e] = tot;
}

// single workgroup: out[c] = sum_i in[i*w + c] (c < w <= 4); if aux: out[w] = max_i aux[i] and out[w + 1] = #{i : aux[i] < 0}
// (k_schur_view marks a view whose damped H_pp is not positive definite with -1).  `out` may be page-locked host memory.
constexpr int COL_REDUCE_LDS = 6 * 256;  // doubles of LDS scratch (the fused stages hand every body a piece of ONE buffer: the
                                         // compiler does not overlay the static LDS of branches that exclude each other)
__device__ __forceinline__ void col_reduce_body(double* lds, int n, int w, const double* __restrict__ in, const double* __restrict__ aux,
                                                double* __restrict__ out) {
    double (*sh)[256] = reinterpret_cast<double (*)[256]>(lds);
    double acc[4] = {0, 0, 0, 0}, mx = 0.0, bad = 0.0;
    for (int i = static_cast<int>(threadIdx.x); i < n; i += 256) {
        for (int c = 0; c < w; ++c) acc[c] += in[static_cast<int64_t>(i) * w + c];
        if (aux) { mx = fmax(mx, aux[i]); bad += aux[i] < 0.0 ? 1.0 : 0.0; }
    }
    for (int c = 0; c < 4; ++c) sh[c][threadIdx.x] = acc[c];
    sh[4][threadIdx.x] = mx;
    sh[5][threadIdx.x] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (static_cast<int>(threadIdx.x) < o) {
            for (int c = 0; c < 4; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + o];
            sh[4][threadIdx.x] = fmax(sh[4][threadIdx.x], sh[4][threadIdx.x + o]);
            sh[5][threadIdx.x] += sh[5][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int c = 0; c < w; ++c) out[c] = sh[c][0];
        if (aux) { out[w] = sh[4][0]; out[w + 1] = sh[5][0]; }
    }
}
__global__ __launch_bounds__(256) void k_col_reduce(int n, int w, const double* __restrict__ in, const double* __restrict__ aux,
                                                    double* __restrict__ out, const double* __restrict__ gate = nullptr) {
    __shared__ double lds[COL_REDUCE_LDS];
    if (gate && *gate == 0.0) return;  // (kernels_reproj.hip k_block_consts: a launch queued ahead of the decision it depends on)
    col_reduce_body(lds, n, w, in, aux, out);
}

__global__ void k_schur_view(SchurDims d, int n_views, const int64_t* __restrict__ link_off, const int32_t* __restrict__ link_blk,
                             const double* __restrict__ blk_acc, const double* __restrict__ blk_w,
                             const int32_t* __restrict__ fixed, const double* __restrict__ lmp /*[radius, init_scale]*/, int constrained,
                             const double* __restrict__ view, double* __restrict__ scale2, double* __restrict__ L,
                             double* __restrict__ y, double* __restrict__ D, double* __restrict__ gp, double* __restrict__ blk_Z,
                             double* __restrict__ gmax /* -1 marks a failed elimination */) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_views) return;
    const int nb = static_cast<int>(link_off[v + 1] - link_off[v]);
    double gm = 0.0;
    const double radius = lmp[0];
    const bool init_scale = lmp[1] != 0.0;
    const bool ok = schur_view_body(d, nb, link_blk + link_off[v], blk_acc, blk_w, fixed[v] != 0, radius, init_scale,
                                    constrained != 0, view + 7 * static_cast<int64_t>(v), scale2 + 6 * static_cast<int64_t>(v),
                                    L + 36 * static_cast<int64_t>(v), y + 6 * static_cast<int64_t>(v), D + 6 * static_cast<int64_t>(v),
                                    gp + 6 * static_cast<int64_t>(v), blk_Z, &gm);
    gmax[v] = ok ? gm : -1.0;
}

// The same elimination with ONE WAVEFRONT per view (4 views per workgroup).  One thread per view is a ~100 us latency chain however
// few views there are (8-camera rig: 8 blocks x 16 shared columns of forward substitutions per view, 107 us for 500 views and 84 us
// for 4000): here every lane runs the short factor part redundantly and the lanes split the (block, column) pairs of Z.  Same
// operations per value as the serial body: bit-identical results.
__device__ __forceinline__ void schur_view_wave_body(int bx, const SchurDims& d, int n_views, const int64_t* __restrict__ link_off,
                                                     const int32_t* __restrict__ link_blk, const double* __restrict__ blk_acc,
                                                     const double* __restrict__ blk_w, const int32_t* __restrict__ fixed,
                                                     const double* __restrict__ lmp, int constrained, const double* __restrict__ view,
                                                     double* __restrict__ scale2, double* __restrict__ L, double* __restrict__ y,
                                                     double* __restrict__ D, double* __restrict__ gp, double* __restrict__ blk_Z,
                                                     double* __restrict__ gmax) {
    const int v = bx * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= n_views) return;
    const int nb = static_cast<int>(link_off[v + 1] - link_off[v]);
    const int32_t* blks = link_blk + link_off[v];
    const int n_pairs = nb * d.PSH;
    if (fixed[v] != 0) {
        if (lane == 0) {
            double* Lv = L + 36 * static_cast<int64_t>(v);
            for (int i = 0; i < 36; ++i) Lv[i] = (i % 7 == 0) ? 1.0 : 0.0;
            for (int i = 0; i < 6; ++i) {
                y[6 * static_cast<int64_t>(v) + i] = 0.0; D[6 * static_cast<int64_t>(v) + i] = 0.0; gp[6 * static_cast<int64_t>(v) + i] = 0.0;
                if (lmp[1] != 0.0) scale2[6 * static_cast<int64_t>(v) + i] = 1.0;
            }
            gmax[v] = 0.0;
        }
        for (int p = lane; p < n_pairs; p += 64) {
            const int k = p / d.PSH, c = p - k * d.PSH;
            double* Z = blk_Z + static_cast<int64_t>(blks[k]) * 6 * d.PSH;
            for (int i = 0; i < 6; ++i) Z[i * d.PSH + c] = 0.0;
        }
        return;
    }
    double F[36], rd[6], gm = 0.0;
    const bool ok = schur_view_factor(d, nb, blks, blk_acc, blk_w, lmp[0], lmp[1] != 0.0, constrained != 0, view + 7 * static_cast<int64_t>(v),
                                      scale2 + 6 * static_cast<int64_t>(v), L + 36 * static_cast<int64_t>(v), y + 6 * static_cast<int64_t>(v),
                                      D + 6 * static_cast<int64_t>(v), gp + 6 * static_cast<int64_t>(v), &gm, lane == 0, F, rd);
    if (lane == 0) gmax[v] = ok ? gm : -1.0;
    if (!ok) return;
    for (int p = lane; p < n_pairs; p += 64) {
        const int k = p / d.PSH, c = p - k * d.PSH;
        const int b = blks[k];
        schur_view_zcol(d, F, rd, blk_w[b], blk_acc + static_cast<int64_t>(b) * d.NACC, c, blk_Z + static_cast<int64_t>(b) * 6 * d.PSH);
    }
}
__global__ __launch_bounds__(256) void k_schur_view_wave(SchurDims d, int n_views, const int64_t* __restrict__ link_off,
                                                         const int32_t* __restrict__ link_blk, const double* __restrict__ blk_acc,
                                                         const double* __restrict__ blk_w, const int32_t* __restrict__ fixed,
                                                         const double* __restrict__ lmp, int constrained, const double* __restrict__ view,
                                                         double* __restrict__ scale2, double* __restrict__ L, double* __restrict__ y,
                                                         double* __restrict__ D, double* __restrict__ gp, double* __restrict__ blk_Z,
                                                         double* __restrict__ gmax) {
    schur_view_wave_body(blockIdx.x, d, n_views, link_off, link_blk, blk_acc, blk_w, fixed, lmp, constrained, view, scale2, L, y, D, gp, blk_Z, gmax);
}

// ... and the back-substitution: the lanes split a = Z d_c over the (block, column) pairs (fixed assignment, fixed-order DPP
// wave sums: deterministic; rounding differs from the serial body's summation order), lane 63 finishes
__device__ __forceinline__ void backsub_wave_sums(const SchurDims& d, int nb, const int32_t* __restrict__ blks, const int32_t* __restrict__ blk_cam,
                                                  const double* __restrict__ blk_Z, const double* __restrict__ delta_sh, bool fx, int lane,
                                                  double a[6]) {
    for (int i = 0; i < 6; ++i) a[i] = 0.0;
    if (fx) return;
    const int n_pairs = nb * d.PSH;
    for (int p = lane; p < n_pairs; p += 64) {
        const int k = p / d.PSH, c = p - k * d.PSH;
        const int b = blks[k];
        const double dc = delta_sh[blk_cam[b] * d.PC + c];
        const double* Z = blk_Z + static_cast<int64_t>(b) * 6 * d.PSH + c;
        for (int i = 0; i < 6; ++i) a[i] += Z[i * d.PSH] * dc;
    }
    for (int i = 0; i < 6; ++i) a[i] = wave_sum63(a[i]);  // total in lane 63
}
__global__ __launch_bounds__(256) void k_backsub_wave(SchurDims d, int n_views, const int64_t* __restrict__ link_off,
                                                      const int32_t* __restrict__ link_blk, const int32_t* __restrict__ blk_cam,
                                                      const double* __restrict__ blk_Z, const double* __restrict__ delta_sh,
                                                      const int32_t* __restrict__ fixed, const double* __restrict__ L, const double* __restrict__ y,
                                                      const double* __restrict__ D, const double* __restrict__ gp, const double* __restrict__ x,
                                                      double* __restrict__ delta_p, double* __restrict__ xt, double* __restrict__ stats,
                                                      const double* __restrict__ gate = nullptr) {
    if (gate && *gate == 0.0) return;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= n_views) return;
    const int nb = static_cast<int>(link_off[v + 1] - link_off[v]);
    const int32_t* blks = link_blk + link_off[v];
    const bool fx = fixed[v] != 0;
    double a[6];
    backsub_wave_sums(d, nb, blks, blk_cam, blk_Z, delta_sh, fx, lane, a);
    if (lane == 63) {
        double o4[4];
        backsub_view_finish(fx, a, L + 36 * static_cast<int64_t>(v), y + 6 * static_cast<int64_t>(v), D + 6 * static_cast<int64_t>(v),
                            gp + 6 * static_cast<int64_t>(v), x + 7 * static_cast<int64_t>(v), delta_p + 6 * static_cast<int64_t>(v),
                            xt + 7 * static_cast<int64_t>(v), o4);
        for (int k = 0; k < 4; ++k) stats[4 * static_cast<int64_t>(v) + k] = o4[k];
    }
}

// Stage the 6 * VCHUNK rows of Z of one view chunk for the 64 columns from c0 (Zs[6 * (v - v0) + k][c]; zero past the shared block,
// past the last view and where the view does not see the column's camera).  Two phases so that no load depends on another one:
// the chunk's (view, camera) -> block table goes to LDS first, then every thread's Z entries are independent, unconditional
// loads (the chain view -> block -> Z row, 24 times in sequence per thread, was most of the syrk kernels' time).
constexpr int SYRK_MAX_CAMS = 64;
__device__ __forceinline__ void stage_block_table(const SchurDims& d, int n_views, int v0, const int32_t* __restrict__ view_cam_blk, int* bsh) {
    if (d.n_cams > SYRK_MAX_CAMS) return;  // (a rig of more than 64 cameras: stage_Z reads the table from global memory)
    for (int t = threadIdx.x; t < VCHUNK * d.n_cams; t += blockDim.x) {
        const int v = v0 + t / d.n_cams;
        bsh[t] = v < n_views ? view_cam_blk[static_cast<int64_t>(v) * d.n_cams + t % d.n_cams] : -1;
    }
}
__device__ __forceinline__ void stage_Z(const SchurDims& d, const int* bsh, int n_views, int v0, const int32_t* __restrict__ view_cam_blk,
                                        const double* __restrict__ blk_Z, int c0, int nsh, double (*Zs)[64]) {
    const bool table = d.n_cams <= SYRK_MAX_CAMS;
#pragma unroll 4
    for (int idx = threadIdx.x; idx < 6 * VCHUNK * 64; idx += 256) {
        const int row = idx >> 6, c = idx & 63, g = c0 + c;
        const int gg = g < nsh ? g : 0;
        const int cam = gg / d.PC, lc = gg - cam * d.PC;
        const int v = v0 + row / 6;
        const int b = table ? bsh[(row / 6) * d.n_cams + cam] : (v < n_views ? view_cam_blk[static_cast<int64_t>(v) * d.n_cams + cam] : -1);
        const double z = blk_Z[(static_cast<int64_t>(b < 0 ? 0 : b) * 6 + row % 6) * d.PSH + lc];
        Zs[row][c] = (g < nsh && b >= 0) ? z : 0.0;
    }
}

// g_schur partial of one view chunk: out[g] = sum_{v in chunk} sum_k Z_v[k][g] y_v[k] (fixed (v, k) order), from the rows of Z the
// syrk kernels have staged in LDS (Zs[6 * views + k][column - c0]) — read from global memory the chain view -> block index -> Z row
// is two dependent loads per view and was most of the kernels' time.  Run by the DIAGONAL tile pair of a chunk for its 64
// columns, so that the whole elimination result is one partial row per chunk and ONE k_row_sum.
__device__ __forceinline__ void schur_gvec_chunk(const double (*Zs)[64], const double* ysh, int nrow, int c0, int nsh, double* __restrict__ out) {
    const int c = threadIdx.x;
    if (c >= 64 || c0 + c >= nsh) return;
    double s = 0.0;
    for (int r = 0; r < nrow; ++r) s += Zs[r][c] * ysh[r];
    out[c0 + c] = s;
}

// grid (view chunks, upper tile pairs); one workgroup = one 64x64 output tile over a chunk of VCHUNK views.
// partial[chunk] = [pair][64*64] then g_schur[nsh]  (row stride n_pairs * 4096 + nsh)
constexpr int SYRK_ROWS = 6 * VCHUNK;  // 48, a multiple of 4
constexpr int SYRK_LDS = 2 * SYRK_ROWS * 64 + SYRK_ROWS + VCHUNK * SYRK_MAX_CAMS / 2;  // doubles: Zi | Zj | y | block table (ints)

// the upper-triangular tile pairs in (ti, tj >= ti) order
__device__ __forceinline__ void tile_pair(int pair, int n_tiles, int* ti, int* tj) {
    int i = 0;
    while (pair >= n_tiles - i) { pair -= n_tiles - i; ++i; }
    *ti = i;
    *tj = i + pair;
}

// The tile's inner product on the vector ALU: 256 threads = 16x16, each a 4x4 micro-tile; the products are added in (view, k) order
__device__ __forceinline__ void syrk_tile_valu(const double (*Zi)[64], const double (*Zc)[64], int nrow, double* __restrict__ out) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int r = 0; r < nrow; ++r) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = Zi[r][ty * 4 + q]; b[q] = Zc[r][tx * 4 + q]; }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[p][q] += a[p] * b[q];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(ty * 4 + p) * 64 + tx * 4 + q] = acc[p][q];
}

// The same on the matrix cores, used when the shared block is a real contraction (nsh >= 64: the 8-camera rig of BASELINE
// config 3 has nsh = 128, K = 6 x #views).  Every wavefront owns a 16 x 64 strip = four 16x16 accumulators and issues
// v_mfma_f64_16x16x4_f64 over the 12 four-row steps of the staged rows (A[i][k]: lane i = l & 15, k = l >> 4; B[k][j] likewise;
// D: col = l & 15, row = (l >> 4) + 4 reg; rows past the last view are staged as zeros).  fp64 MFMA runs at the vector-FMA rate
// on MI355X (78.6 TFLOP/s both), so this is about USING the matrix pipe where the north-star asks for it, not about speed: the
// kernel is ~40 us of a 6 ms LM step.
typedef double v4f64 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void syrk_tile_mfma(const double (*Zi)[64], const double (*Zc)[64], double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    v4f64 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int step = 0; step < SYRK_ROWS / 4; ++step) {
        const int r = 4 * step + lk;
        const double a = Zi[r][wave * 16 + li];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Zc[r][c * 16 + li], acc[c], 0, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(wave * 16 + lk + 4 * reg) * 64 + c * 16 + li] = acc[c][reg];
}

template <bool MFMA>
__device__ __forceinline__ void schur_syrk_body(double* lds, int bx, int by, int gy, const SchurDims& d, int n_views, int nsh, int n_tiles,
        const int32_t* __restrict__ view_cam_blk, const double* __restrict__ blk_Z, const double* __restrict__ y, double* __restrict__ partial) {
    // the chunk's 6 * VCHUNK rows of Z are staged in one go (one barrier per workgroup, not two per view: the staging of a
    // 10-wide shared block is all latency)
    double (*Zi)[64] = reinterpret_cast<double (*)[64]>(lds), (*Zj)[64] = Zi + SYRK_ROWS;
    double* ysh = lds + 2 * SYRK_ROWS * 64;
    int* bsh = reinterpret_cast<int*>(ysh + SYRK_ROWS);
    int ti, tj;
    tile_pair(by, n_tiles, &ti, &tj);
    const int i0 = ti * 64, j0 = tj * 64;
    const int v0 = bx * VCHUNK;
    const int nrow = 6 * (min(n_views, v0 + VCHUNK) - v0);
    stage_block_table(d, n_views, v0, view_cam_blk, bsh);
    __syncthreads();
    stage_Z(d, bsh, n_views, v0, view_cam_blk, blk_Z, i0, nsh, Zi);
    if (tj != ti) stage_Z(d, bsh, n_views, v0, view_cam_blk, blk_Z, j0, nsh, Zj);
    if (static_cast<int>(threadIdx.x) < SYRK_ROWS) ysh[threadIdx.x] = static_cast<int>(threadIdx.x) < nrow ? y[6 * static_cast<int64_t>(v0) + threadIdx.x] : 0.0;
    __syncthreads();
    const double (*Zc)[64] = tj != ti ? Zj : Zi;  // a diagonal tile: both factors are the same 64 columns, staged once
    double* row = partial + static_cast<int64_t>(bx) * (static_cast<int64_t>(gy) * 4096 + nsh);
    double* out = row + static_cast<int64_t>(by) * 4096;
    if constexpr (MFMA) syrk_tile_mfma(Zi, Zc, out);
    else syrk_tile_valu(Zi, Zc, nrow, out);
    if (ti == tj) schur_gvec_chunk(Zi, ysh, nrow, i0, nsh, row + static_cast<int64_t>(gy) * 4096);
}
__global__ __launch_bounds__(256) void k_schur_syrk(SchurDims d, int n_views, int nsh, int n_tiles, const int32_t* __restrict__ view_cam_blk,
        const double* __restrict__ blk_Z, const double* __restrict__ y, double* __restrict__ partial) {
    __shared__ double lds[SYRK_LDS];
    schur_syrk_body<false>(lds, blockIdx.x, blockIdx.y, gridDim.y, d, n_views, nsh, n_tiles, view_cam_blk, blk_Z, y, partial);
}
__global__ __launch_bounds__(256) void k_schur_syrk_mfma(SchurDims d, int n_views, int nsh, int n_tiles, const int32_t* __restrict__ view_cam_blk,
        const double* __restrict__ blk_Z, const double* __restrict__ y, double* __restrict__ partial) {
    __shared__ double lds[SYRK_LDS];
    schur_syrk_body<true>(lds, blockIdx.x, blockIdx.y, gridDim.y, d, n_views, nsh, n_tiles, view_cam_blk, blk_Z, y, partial);
}

__global__ void k_backsub(SchurDims d, int n_views, const int64_t* __restrict__ link_off, const int32_t* __restrict__ link_blk,
                          const int32_t* __restrict__ blk_cam, const double* __restrict__ blk_Z,
                          const double* __restrict__ delta_sh, const int32_t* __restrict__ fixed, const double* __restrict__ L,
                          const double* __restrict__ y, const double* __restrict__ D, const double* __restrict__ gp,
                          const double* __restrict__ x, double* __restrict__ delta_p, double* __restrict__ xt,
                          double* __restrict__ stats /*[n_views][4]*/, const double* __restrict__ gate = nullptr) {
    if (gate && *gate == 0.0) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_views) return;
    const int nb = static_cast<int>(link_off[v + 1] - link_off[v]);
    double o4[4];
    backsub_view_body(d, nb, link_blk + link_off[v], blk_cam, blk_Z, delta_sh, fixed[v] != 0, L + 36 * static_cast<int64_t>(v),
                      y + 6 * static_cast<int64_t>(v), D + 6 * static_cast<int64_t>(v), gp + 6 * static_cast<int64_t>(v),
                      x + 7 * static_cast<int64_t>(v), delta_p + 6 * static_cast<int64_t>(v), xt + 7 * static_cast<int64_t>(v), o4);
    for (int k = 0; k < 4; ++k) stats[4 * static_cast<int64_t>(v) + k] = o4[k];
}

// an accepted step: trial copies -> current copies (the shared pack and the private poses), one launch
__global__ void k_accept(int64_t n_shared, const double* __restrict__ shared_trial, double* __restrict__ shared_cur, int64_t n_view,
                         const double* __restrict__ view_trial, double* __restrict__ view_cur) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n_shared) shared_cur[i] = shared_trial[i];
    if (i < n_view) view_cur[i] = view_trial[i];
}

// The packed exchange buffer of one linear solve (lm_core.hpp PackLayout), assembled ON THE DEVICE: the camera sums are written
// in place by k_seg_sum; this kernel adds the step statistics, the cost, the dense S_schur unpacked from the syrk tiles, g_schur,
// the failure count and this rank's gradient-max slot (the other ranks' slots are zeroed: the all-reduce is a sum).
struct PackArgs {
    int64_t off_stats, off_cam, off_cost, off_nfail, off_S, off_g, off_gmax;
    int n, n_tiles, n_ranks, rank, n_cam_doubles;
    int has_blocks /* camera sums are in the pack */, has_cost /* stat[4] holds the cost */, has_schur, has_stats;
};
// the pack's scalar slots: the failure count, the cost and the step statistics (PackLayout's stats block)
__device__ __forceinline__ void pack_scalars(const PackArgs& a, const double* __restrict__ stat, double nfail, double* __restrict__ pack) {
    pack[a.off_nfail] = nfail;
    pack[a.off_cost] = a.has_cost ? stat[4] : 0.0;
    // has_stats: 1 = a trial step (stat[2], stat[3] = the views' g^T d, d^T H d), 2 = a line-search sample (stat[2] = their slope)
    pack[a.off_stats + 0] = a.has_stats == 1 ? stat[2] : 0.0;  // PackLayout::GD
    pack[a.off_stats + 1] = a.has_stats == 1 ? stat[3] : 0.0;  // DHD
    pack[a.off_stats + 2] = a.has_stats ? stat[0] : 0.0;       // STEP2
    pack[a.off_stats + 3] = a.has_stats ? stat[1] : 0.0;       // XNORM2
    pack[a.off_stats + 4] = (a.has_stats && a.has_cost) ? stat[4] : 0.0;  // TRIAL_COST
    pack[a.off_stats + 5] = a.has_stats == 2 ? stat[2] : 0.0;  // SLOPE
}
__global__ __launch_bounds__(256) void k_pack(PackArgs a, const double* __restrict__ stat /*[0..4): step2, xnorm2, gd, dHd; [4]: cost*/,
                                              const double* __restrict__ tiles /*[pairs*4096 | g | gmax, nfail]*/, double* __restrict__ pack) {
    const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t nn = static_cast<int64_t>(a.n) * a.n;
    const int64_t sw = static_cast<int64_t>(a.n_tiles) * (a.n_tiles + 1) / 2 * 4096;
    if (tid < nn) {  // S travels as its upper triangle, packed row-major (PackLayout)
        const int i = static_cast<int>(tid / a.n), j = static_cast<int>(tid % a.n);
        if (i <= j) {
            double val = 0.0;
            if (a.has_schur) {
                const int ti = i >> 6, tj = j >> 6;
                const int pair = ti * a.n_tiles - ti * (ti - 1) / 2 + (tj - ti);  // upper-triangular tile pairs in (ti, tj >= ti) order
                val = tiles[static_cast<int64_t>(pair) * 4096 + (i & 63) * 64 + (j & 63)];
            }
            pack[a.off_S + ctl_sidx(a.n, i, j)] = val;
        }
    }
    if (tid < a.n) pack[a.off_g + tid] = a.has_schur ? tiles[sw + tid] : 0.0;
    if (tid < a.n_ranks) pack[a.off_gmax + tid] = (a.has_schur && tid == a.rank) ? tiles[sw + a.n] : 0.0;
    if (tid == 0) pack_scalars(a, stat, a.has_schur ? tiles[sw + a.n + 1] : 0.0, pack);
    if (!a.has_blocks && tid < a.n_cam_doubles) pack[a.off_cam + tid] = 0.0;
}

// ---- the fused stages of one linear solve -----------------------------------------------------------------------------------------
// Between Mode B and the packed exchange an LM step needs ten small dependent reductions (block weights and cost, per-camera sums,
// per-view elimination, the Schur contraction and its sums, the pack).  As launches of their own each costs 4 - 6 us of dispatch
// and drain whatever its work (87 us per step for the 8-camera rig, a sixth of a step when the problem is split over 8 GPUs).
// Here the stages that do not depend on each other share ONE launch (ranges of blockIdx.x run different bodies), and every
// reduction keeps its own fixed order: the results are bit-identical to the one-kernel-per-stage sequence, which the paths off
// the LM loop (covariance, cost queries, the one-thread-per-view form) still use.
//   k_step_head   back-substitution of the views + their blocks' constants at the trial poses      (was 3 launches)
//   k_sys_stage2  per-camera chunk sums | per-view elimination | cost (or its partial sums)         (was 3)
//   k_sys_stage3  camera segment sums | Schur contraction | gradient max | step statistics | cost   (was 4 - 5)
//   k_sys_pack    sums over the view chunks straight into the packed exchange buffer                (was 2)
struct SysArgs {
    SchurDims d;
    int n_views, n_blocks, nsh, n_tiles, n_pairs, n_vchunks, n_cams, NACC, constrained;
    int n_cc, n_vb, n_costp;         // stage 2 ranges: camera chunks | view workgroups (4 views each) | cost workgroups (0, 1 or ceil(n_blocks / 2048))
    int n_seg_x, n_seg, n_syrk;      // stage 3 ranges: segment sums (n_seg_x per camera) | (chunk, tile pair) | then 1 + has_vstats + (n_costp > 1)
    int has_vstats;                  // the views' step statistics (k_step_head) are reduced in stage 3
    double huber;
    const int64_t *link_off, *cchunk_off, *cam_seg;
    const int32_t *link_blk, *cam_blk, *view_fixed, *view_cam_blk;
    const double *blk_acc, *blk_w, *blk_s, *lmp, *view;
    double *view_scale2, *view_L, *view_y, *view_D, *view_gp, *blk_Z, *view_gmax, *cam_partial, *cam_out, *cost_part, *cost_out;
    double *syrk_partial, *tiles_tail /* [gmax, #failed] */, *view_stats, *stat_out;
};

__global__ __launch_bounds__(256) void k_sys_stage2(SysArgs a) {
    __shared__ double lds[2 * 256];
    int bx = blockIdx.x;
    if (bx < a.n_cc) {
        cam_partial_body(bx, a.NACC, a.cchunk_off, a.cam_blk, a.blk_w, a.blk_acc, a.cam_partial);
        return;
    }
    bx -= a.n_cc;
    if (bx < a.n_vb) {
        schur_view_wave_body(bx, a.d, a.n_views, a.link_off, a.link_blk, a.blk_acc, a.blk_w, a.view_fixed, a.lmp, a.constrained, a.view,
                             a.view_scale2, a.view_L, a.view_y, a.view_D, a.view_gp, a.blk_Z, a.view_gmax);
        return;
    }
    bx -= a.n_vb;
    if (a.n_costp == 1) cost_range_body(lds, 0, a.n_blocks, a.blk_s, a.huber, a.cost_out);
    else cost_range_body(lds, bx * 2048, min(bx * 2048 + 2048, a.n_blocks), a.blk_s, a.huber, a.cost_part + 2 * bx);
}

template <bool MFMA>
__global__ __launch_bounds__(256) void k_sys_stage3(SysArgs a) {
    __shared__ double lds[SYRK_LDS];
    static_assert(SYRK_LDS >= COL_REDUCE_LDS && SYRK_LDS >= RS_GROUPS * RS_COLS, "one LDS buffer for every body");
    int bx = blockIdx.x;
    if (bx < a.n_seg) {
        seg_sum_body(lds, bx % a.n_seg_x, bx / a.n_seg_x, a.NACC, a.cam_seg, a.cam_partial, a.cam_out);
        return;
    }
    bx -= a.n_seg;
    if (bx < a.n_syrk) {
        const int chunk = bx % a.n_vchunks, pair = bx / a.n_vchunks;
        schur_syrk_body<MFMA>(lds, chunk, pair, a.n_pairs, a.d, a.n_views, a.nsh, a.n_tiles, a.view_cam_blk, a.blk_Z, a.view_y, a.syrk_partial);
        return;
    }
    bx -= a.n_syrk;
    if (bx == 0) { col_reduce_body(lds, a.n_views, 0, a.view_gmax, a.view_gmax, a.tiles_tail); return; }
    if (bx == 1 && a.has_vstats) { col_reduce_body(lds, a.n_views, 4, a.view_stats, nullptr, a.stat_out); return; }
    if (threadIdx.x == 0) {  // k_cost_final: the partial pairs in order
        double c = 0.0, ss = 0.0;
        for (int k = 0; k < a.n_costp; ++k) { c += a.cost_part[2 * k]; ss += a.cost_part[2 * k + 1]; }
        a.cost_out[0] = c;
        a.cost_out[1] = ss;
    }
}

// k_row_sum and k_pack in one: workgroup x sums 32 columns of the chunk table [n_vchunks][pairs * 4096 + nsh] (8 row groups, fixed
// order) and writes each straight to its place in the pack (S as its packed upper triangle, g_schur); workgroup 0 adds the scalars
__global__ __launch_bounds__(RS_COLS * RS_GROUPS) void k_sys_pack(PackArgs a, int64_t n_rows, const double* __restrict__ rows,
                                                                   const double* __restrict__ tail /*[gmax, #failed]*/,
                                                                   const double* __restrict__ stat, double* __restrict__ pack) {
    __shared__ double sh[RS_GROUPS][RS_COLS];
    const int64_t sw = static_cast<int64_t>(a.n_tiles) * (a.n_tiles + 1) / 2 * 4096, width = sw + a.n;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * RS_COLS + threadIdx.x % RS_COLS;
    const double tot = grouped_column_sum(rows, 0, n_rows, width, e, e < width, sh);
    if (threadIdx.x < RS_COLS && e < width) {
        if (e < sw) {
            int ti, tj;
            tile_pair(static_cast<int>(e >> 12), a.n_tiles, &ti, &tj);
            const int i = ti * 64 + static_cast<int>((e >> 6) & 63), j = tj * 64 + static_cast<int>(e & 63);
            if (i <= j && j < a.n) pack[a.off_S + ctl_sidx(a.n, i, j)] = tot;
        } else {
            pack[a.off_g + (e - sw)] = tot;
        }
    }
    const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (tid < a.n_ranks) pack[a.off_gmax + tid] = tid == a.rank ? tail[0] : 0.0;
    if (tid == 0) pack_scalars(a, stat, tail[1], pack);
    if (!a.has_blocks)
        for (int64_t k = tid; k < a.n_cam_doubles; k += static_cast<int64_t>(gridDim.x) * blockDim.x) pack[a.off_cam + k] = 0.0;
}

// k_backsub_wave, then the constants of the view's residual blocks at its trial pose (k_block_consts' work: a block's constants
// depend on its own view's pose and on the shared blocks the controller has left in copy 1) - the wavefront that has just formed
// the pose hands it to its lanes through registers, lane k takes the view's k-th block.  INTRINSIC / EXTRINSIC chains (the
// bundle chain has no private poses).
template <int CHAIN>
__global__ __launch_bounds__(256) void k_step_head(const double* __restrict__ gate, SchurDims d, int n_views, const int64_t* __restrict__ link_off,
                                                   const int32_t* __restrict__ link_blk, const int32_t* __restrict__ blk_cam,
                                                   const double* __restrict__ blk_Z, const double* __restrict__ delta_sh,
                                                   const int32_t* __restrict__ fixed, const double* __restrict__ L, const double* __restrict__ y,
                                                   const double* __restrict__ D, const double* __restrict__ gp, const double* __restrict__ x,
                                                   double* __restrict__ delta_p, double* __restrict__ xt, double* __restrict__ stats,
                                                   const double* __restrict__ cam_trial, double* __restrict__ bc) {
    if (gate && *gate == 0.0) return;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= n_views) return;
    const int nb = static_cast<int>(link_off[v + 1] - link_off[v]);
    const int32_t* blks = link_blk + link_off[v];
    const bool fx = fixed[v] != 0;
    double a[6];
    backsub_wave_sums(d, nb, blks, blk_cam, blk_Z, delta_sh, fx, lane, a);
    double pose[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (lane == 63) {
        double o4[4], dp[6];
        backsub_view_finish(fx, a, L + 36 * static_cast<int64_t>(v), y + 6 * static_cast<int64_t>(v), D + 6 * static_cast<int64_t>(v),
                            gp + 6 * static_cast<int64_t>(v), x + 7 * static_cast<int64_t>(v), dp, pose, o4);
        for (int k = 0; k < 6; ++k) delta_p[6 * static_cast<int64_t>(v) + k] = dp[k];
        for (int k = 0; k < 7; ++k) xt[7 * static_cast<int64_t>(v) + k] = pose[k];
        for (int k = 0; k < 4; ++k) stats[4 * static_cast<int64_t>(v) + k] = o4[k];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) pose[k] = __shfl(pose[k], 63);
    for (int k = lane; k < nb; k += 64) {
        const int b = blks[k];
        double out[BC_SIZE];
        block_consts<CHAIN>(pose, CHAIN == CH_EXTRINSIC ? cam_trial + 7 * static_cast<int64_t>(blk_cam[b]) : nullptr, nullptr, out);
        for (int i = 0; i < BC_SIZE; ++i) bc[static_cast<int64_t>(b) * BC_SIZE + i] = out[i];
    }
}

// line search sample (line_search.hpp): trial poses at step size a along the last back-substituted step; stats [n_views][4] =
// { |xt - x|^2, |x|^2, slope share (k_view_slope, or 0), 0 }
__global__ void k_scale_step(int n_views, double a, const int32_t* __restrict__ fixed, const double* __restrict__ x,
                             const double* __restrict__ delta_p, double* __restrict__ xt, double* __restrict__ stats) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_views) return;
    double o2[2];
    scale_step_view_body(fixed[v] != 0, a, x + 7 * static_cast<int64_t>(v), delta_p + 6 * static_cast<int64_t>(v), xt + 7 * static_cast<int64_t>(v), o2);
    stats[4 * static_cast<int64_t>(v)] = o2[0];
    stats[4 * static_cast<int64_t>(v) + 1] = o2[1];
    stats[4 * static_cast<int64_t>(v) + 2] = 0.0;
    stats[4 * static_cast<int64_t>(v) + 3] = 0.0;
}
__global__ void k_view_slope(SchurDims d, int n_views, const int64_t* __restrict__ link_off, const int32_t* __restrict__ link_blk,
                             const double* __restrict__ blk_acc, const double* __restrict__ blk_w, const int32_t* __restrict__ fixed,
                             const double* __restrict__ delta_p, double* __restrict__ stats) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_views) return;
    stats[4 * static_cast<int64_t>(v) + 2] = view_slope_body(d, static_cast<int>(link_off[v + 1] - link_off[v]), link_blk + link_off[v], blk_acc,
                                                              blk_w, fixed[v] != 0, delta_p + 6 * static_cast<int64_t>(v));
}

// an accepted SPECULATIVE step: besides the parameter copies, the trial linearisation's block sums and weights become current
__global__ void k_accept_blocks(int64_t n_acc, const double* __restrict__ acc_trial, double* __restrict__ acc_cur, int64_t n_w,
                                const double* __restrict__ w_trial, double* __restrict__ w_cur) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n_acc) acc_cur[i] = acc_trial[i];
    if (i < n_w) w_cur[i] = w_trial[i];
}

}  // namespace cba
