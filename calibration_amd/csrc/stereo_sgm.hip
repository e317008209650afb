// stereo_sgm.hip — semi-global matching on the GPU (sgm_math.hpp, calibba.h: cba_sgm_matcher).  One stream, one synchronise per call;
// the volumes hold `group` pairs at a time and process loops over groups.  With Dp = 16 K the padded candidate count (K = the
// candidates a lane keeps: 2, 4, 8 or 16, the smallest with 16 K >= D):
//   k_sgm_census   one lane per pixel of both images, grid-stride: the 62-bit code (sgm_census_code) as one uint64.
//   k_sgm_cost     one lane per pixel and sixteen candidates, the right codes of a row segment staged in LDS: C = popcount(codeL ^ codeR) as a uint8 volume [y][x][Dp], written once
//                  (0 at the padded candidates).  Stored, not recomputed per path: recomputing would read 16 B of codes per pixel
//                  from memory instead of Dp, but every lane would then fetch K 8-byte codes and run 4 K more vector instructions per
//                  step of a loop that is bound by its issue and latency, not by its bytes; stored, a lane's K costs are one load.
//   k_sgm_path<KP> one DPP row (16 lanes) per line of the direction (dx, dy), four lines per wavefront, one launch per direction.
//                  A lane keeps K = 2 KP consecutive candidates as KP packed uint16 pairs.  The d -+ 1 neighbours inside a lane are
//                  one v_alignbit each, those across lanes come from row_shr:1 / row_shl:1 (lanes 0 / 15 keep SGM_PATH_INF); M is
//                  the row minimum by four row_ror steps.  Candidates past D are held at SGM_PATH_INF by one v_pk_max.  The
//                  first direction writes S (uint16 [y][x][Dp]), the others add by read-modify-write: launches on one stream, no
//                  atomics.  The costs and sums of the next four pixels are in flight while four are stepped: a line is a serial
//                  chain and a launch has about one wavefront per SIMD, so the loop is bound by memory latency, not by issue.
//   k_sgm_select<RIGHT, KC>  one wavefront per tile of 64 columns of a row, one lane per pixel: KC candidates of the tile at a time
//                  go through LDS (loaded along d, 16 B per lane, read back along the pixels), and a lane pushes its admissible ones
//                  in ascending d through stereo_sel_push.  RIGHT reads S(x' + d, y, d): the tile then spans 64 + KC - 1 columns.
//   then the finish kernel of stereo_match.hip (stereo_finish_launch): left-right check and the points.
// No atomics, no scratch, no dynamically indexed private array; every index into a volume is 64-bit and every load lies inside its
// buffer (the volumes are padded to Dp, so a lane's K entries always exist).
#include <memory>
#include <type_traits>

#include "pipelines.hpp"
#include "sgm_math.hpp"

namespace cba {

constexpr int SGM_BLOCK = 256;
constexpr int SGM_GRID = 8192;  // grid-stride cap of the per-pixel kernels
constexpr int SGM_LINES = SGM_BLOCK / 16;  // lines of a workgroup of the path kernel
constexpr int SGM_AHEAD = 4;               // pixels of a line whose costs and sums are in flight while the previous ones are stepped
constexpr int SGM_SEL_T = 64;              // pixels of a selection tile: one wavefront, one lane per pixel

typedef uint16_t sgm_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(sgm_u16x2, a), __builtin_bit_cast(sgm_u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(sgm_u16x2, a), __builtin_bit_cast(sgm_u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(sgm_u16x2, a) + __builtin_bit_cast(sgm_u16x2, b));
}
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(sgm_u16x2, a) - __builtin_bit_cast(sgm_u16x2, b));
}

__global__ __launch_bounds__(SGM_BLOCK) void k_sgm_census(int64_t n_px, int W, int H, const uint8_t* __restrict__ left,
                                                          const uint8_t* __restrict__ right, uint64_t* __restrict__ codeL,
                                                          uint64_t* __restrict__ codeR) {
    const int64_t frame = static_cast<int64_t>(W) * H;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(SGM_BLOCK) + threadIdx.x; i < n_px; i += static_cast<int64_t>(gridDim.x) * SGM_BLOCK) {
        const int64_t pair = i / frame, j = i - pair * frame;
        const int y = static_cast<int>(j / W), x = static_cast<int>(j - static_cast<int64_t>(y) * W);
        codeL[i] = sgm_census_code(left + pair * frame, W, H, x, y);
        codeR[i] = sgm_census_code(right + pair * frame, W, H, x, y);
    }
}

// grid = rows * chunks workgroups, rows = n_pairs * H.  A workgroup takes TPX = SGM_BLOCK / parts adjacent pixels of a row (parts =
// Dp / 16 = 1 << lp, chunks = ceil(W / TPX)), stages the TPX + Dp - 1 right codes they meet in LDS (0 outside the row: the rule's
// code of a column outside the image), and a lane turns sixteen candidates of one pixel into one 16-byte store.  Read straight from
// memory, the four lanes of a quad fetch from four cache lines (128 bytes apart), which the load unit takes one after the other.
constexpr int SGM_COST_CODES = 272;  // >= TPX + Dp - 1 for Dp = 32, 64, 128, 256
__global__ __launch_bounds__(SGM_BLOCK) void k_sgm_cost(int chunks, int lp, int W, int dmin, int D, const uint64_t* __restrict__ codeL,
                                                        const uint64_t* __restrict__ codeR, uint4* __restrict__ C) {
    __shared__ uint64_t codes[SGM_COST_CODES];
    const int tid = static_cast<int>(threadIdx.x), Dp = 16 << lp, TPX = SGM_BLOCK >> lp;
    const unsigned rowid = blockIdx.x / static_cast<unsigned>(chunks);
    const int x0 = static_cast<int>(blockIdx.x - rowid * static_cast<unsigned>(chunks)) * TPX;
    const int64_t row = static_cast<int64_t>(rowid) * W;
    const int col0 = x0 - (dmin + Dp - 1);  // the image column of codes[0]
    for (int i = tid; i < TPX + Dp - 1; i += SGM_BLOCK) {
        const int col = col0 + i;
        codes[i] = col >= 0 && col < W ? codeR[row + col] : 0;
    }
    __syncthreads();
    const int xl = tid >> lp, x = x0 + xl, k0 = (tid & ((1 << lp) - 1)) << 4;
    if (x >= W) return;
    const uint64_t cl = codeL[row + x];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = k0 + j;  // right column x - dmin - k = codes[xl + Dp - 1 - k]
        const uint32_t c = static_cast<uint32_t>(sgm_cost(cl, codes[xl + Dp - 1 - k])) & (k < D ? 0xffu : 0u);
        w[j >> 2] |= c << (8 * (j & 3));
    }
    C[((row + x) << lp) + (k0 >> 4)] = make_uint4(w[0], w[1], w[2], w[3]);
}

struct SgmPathArgs {
    const uint8_t* C;  // [n_pairs][H][W][Dp]
    uint16_t* S;       // [n_pairs][H][W][Dp]
    int W, H, D;
    int dx, dy, lines;  // lines of one pair in this direction
    int chunks;         // workgroups of one pair: ceil(lines / SGM_LINES)
    int p1, p2, first;  // first: S is written, not added to
};

template <int KP>
struct SgmLane {
    uint32_t c[(KP + 1) / 2];  // 2 KP cost bytes (KP == 1: the low half of c[0])
    uint32_t s[KP];            // 2 KP sums
};

// N consecutive words at a pointer aligned to 4 N bytes (N = 1, 2, 4, 8): one or two wide loads / stores
template <int N>
__device__ __forceinline__ void sgm_ld(const void* p, uint32_t* w) {
    if constexpr (N == 1) {
        w[0] = *static_cast<const uint32_t*>(p);
    } else if constexpr (N == 2) {
        const uint2 v = *static_cast<const uint2*>(p);
        w[0] = v.x; w[1] = v.y;
    } else {
#pragma unroll
        for (int k = 0; k < N / 4; ++k) {
            const uint4 v = static_cast<const uint4*>(p)[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    }
}
template <int N>
__device__ __forceinline__ void sgm_st(void* p, const uint32_t* w) {
    if constexpr (N == 1) {
        *static_cast<uint32_t*>(p) = w[0];
    } else if constexpr (N == 2) {
        *static_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
        for (int k = 0; k < N / 4; ++k) static_cast<uint4*>(p)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
}

template <int KP>
__device__ __forceinline__ void sgm_load(const SgmPathArgs& a, int64_t off, bool with_s, SgmLane<KP>& v) {
    if constexpr (KP == 1) v.c[0] = *reinterpret_cast<const uint16_t*>(a.C + off);
    else sgm_ld<KP / 2>(a.C + off, v.c);
    if (with_s) {
        sgm_ld<KP>(a.S + off, v.s);
    } else {
#pragma unroll
        for (int k = 0; k < KP; ++k) v.s[k] = 0u;
    }
}

// packed pair k of the lane's costs: candidates 2k (low half) and 2k + 1
template <int KP>
__device__ __forceinline__ uint32_t sgm_cost_pair(const SgmLane<KP>& v, int k) {
    const uint32_t w = v.c[k >> 1] >> ((k & 1) * 16);
    return (w & 0xffu) | ((w & 0xff00u) << 8);
}

// grid = n_pairs * chunks workgroups; workgroup b serves lines [SGM_LINES c, SGM_LINES (c + 1)) of pair b / chunks, c = b % chunks, one
// row of 16 lanes per line
template <int KP>
__global__ __launch_bounds__(SGM_BLOCK) void k_sgm_path(SgmPathArgs a) {
    constexpr int K = 2 * KP, Dp = 16 * K;
    const int tid = static_cast<int>(threadIdx.x), l16 = tid & 15;
    const unsigned pair_u = blockIdx.x / static_cast<unsigned>(a.chunks);
    const int line = static_cast<int>(blockIdx.x - pair_u * static_cast<unsigned>(a.chunks)) * SGM_LINES + (tid >> 4);
    if (line >= a.lines) return;  // a whole row of 16 lanes leaves: the DPP moves below never cross rows
    const int64_t pair = pair_u;
    const int W = a.W, H = a.H, dx = a.dx, dy = a.dy;
    // the first pixel of the line: its predecessor lies outside the image
    int x, y;
    if (dy == 0) {
        x = dx > 0 ? 0 : W - 1; y = line;
    } else if (dx == 0 || line < W) {
        x = line; y = dy > 0 ? 0 : H - 1;
    } else {
        const int t = line - W + 1;  // 1 .. H - 1
        x = dx > 0 ? 0 : W - 1; y = dy > 0 ? t : H - 1 - t;
    }
    const uint32_t INF2 = SGM_PATH_INF * 0x10001u;
    uint32_t pad[KP], keep[KP];  // pad: SGM_PATH_INF at the candidates past D, 0 elsewhere; keep: 0 there, 0xffff elsewhere
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int d0 = l16 * K + 2 * k;
        pad[k] = (d0 >= a.D ? static_cast<uint32_t>(SGM_PATH_INF) : 0u) | (d0 + 1 >= a.D ? static_cast<uint32_t>(SGM_PATH_INF) << 16 : 0u);
        keep[k] = (d0 >= a.D ? 0u : 0xffffu) | (d0 + 1 >= a.D ? 0u : 0xffff0000u);
    }
    const uint32_t P1 = static_cast<uint32_t>(a.p1) * 0x10001u;
    const int64_t step = (static_cast<int64_t>(dy) * W + dx) * Dp;
    int64_t off = ((pair * H + y) * W + x) * Dp + l16 * K;  // elements of C and of S
    const bool with_s = a.first == 0;
    // pixels of the line: until x or y leaves the image (uniform over the row of 16 lanes)
    const int nx = dx > 0 ? W - x : dx < 0 ? x + 1 : 0x7fffffff, ny = dy > 0 ? H - y : dy < 0 ? y + 1 : 0x7fffffff;
    const int len = nx < ny ? nx : ny;
    SgmLane<KP> cur[SGM_AHEAD], nxt[SGM_AHEAD] = {};
#pragma unroll
    for (int u = 0; u < SGM_AHEAD; ++u)
        if (u < len) sgm_load<KP>(a, off + u * step, with_s, cur[u]);
    uint32_t L[KP];
    for (int base = 0; base < len; base += SGM_AHEAD, off += SGM_AHEAD * step) {
#pragma unroll
        for (int u = 0; u < SGM_AHEAD; ++u)  // the next SGM_AHEAD pixels' costs and sums, under this group's steps
            if (base + SGM_AHEAD + u < len) sgm_load<KP>(a, off + (SGM_AHEAD + u) * step, with_s, nxt[u]);
#pragma unroll
        for (int u = 0; u < SGM_AHEAD; ++u) {
            if (base + u >= len) break;
            if (u == 0 && base == 0) {  // the first pixel of the line
#pragma unroll
                for (int k = 0; k < KP; ++k) L[k] = pk_max(sgm_cost_pair<KP>(cur[u], k), pad[k]);
            } else {
                uint32_t m = L[0];
#pragma unroll
                for (int k = 1; k < KP; ++k) m = pk_min(m, L[k]);
                m = pk_min(m, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(m), 0x121, 0xF, 0xF, false)));  // row_ror:1
                m = pk_min(m, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(m), 0x122, 0xF, 0xF, false)));  // row_ror:2
                m = pk_min(m, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(m), 0x124, 0xF, 0xF, false)));  // row_ror:4
                m = pk_min(m, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(m), 0x128, 0xF, 0xF, false)));  // row_ror:8
                const uint32_t mlo = m & 0xffffu, mhi = m >> 16, M = mlo < mhi ? mlo : mhi;  // <= 62 + p2
                const uint32_t M2 = M * 0x10001u, far = (M + static_cast<uint32_t>(a.p2)) * 0x10001u;
                // the last pair of lane - 1 and the first pair of lane + 1; lanes 0 / 15 of the row keep SGM_PATH_INF
                const uint32_t below = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(INF2), static_cast<int>(L[KP - 1]), 0x111, 0xF, 0xF, false));  // row_shr:1
                const uint32_t above = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(INF2), static_cast<int>(L[0]), 0x101, 0xF, 0xF, false));       // row_shl:1
                uint32_t N[KP];
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    const uint32_t lo = k > 0 ? L[k - 1] : below, hi = k + 1 < KP ? L[k + 1] : above;
                    const uint32_t dm1 = (L[k] << 16) | (lo >> 16);  // candidates d - 1 of the pair
                    const uint32_t dp1 = (hi << 16) | (L[k] >> 16);  // candidates d + 1
                    uint32_t t = pk_add(pk_min(dm1, dp1), P1);
                    t = pk_min(pk_min(t, L[k]), far);
                    N[k] = pk_max(pk_sub(pk_add(sgm_cost_pair<KP>(cur[u], k), t), M2), pad[k]);
                }
#pragma unroll
                for (int k = 0; k < KP; ++k) L[k] = N[k];
            }
            uint32_t out[KP];
#pragma unroll
            for (int k = 0; k < KP; ++k) out[k] = pk_add(cur[u].s[k], L[k] & keep[k]);  // the padded candidates of S stay 0
            sgm_st<KP>(a.S + off + u * step, out);
        }
#pragma unroll
        for (int u = 0; u < SGM_AHEAD; ++u) cur[u] = nxt[u];
    }
}

struct SgmSelectArgs {
    const uint16_t* S;  // [n_pairs][H][W][Dp]
    int W, dmin, D, Dp, uniqueness_percent, subpixel;
    int tiles_x;        // tiles of a row: ceil(W / SGM_SEL_T)
    float* disparity;   // RIGHT = false only
    int32_t* cost;
    int16_t* dmap;      // d* (RIGHT = false) or d_R (RIGHT = true); STEREO_NO_DISP: no candidate
};

// grid = n_pairs * H * tiles_x workgroups of one wavefront: a tile of SGM_SEL_T columns of one row, KC candidates at a time.  The
// chunk's sums are loaded with 16-byte loads along d (whole lines of the volume at KC = 64) into LDS rows of KC / 2 + 1 words (the odd
// pitch keeps the lanes on different banks), then every lane walks its own pixel's candidates (RIGHT: pixel x' + d, candidate d).
template <bool RIGHT, int KC>
__global__ __launch_bounds__(SGM_SEL_T) void k_sgm_select(SgmSelectArgs a) {
    constexpr int NPX = RIGHT ? SGM_SEL_T + KC - 1 : SGM_SEL_T, PITCH = KC / 2 + 1, PIECES = KC / 8;
    __shared__ uint32_t tile[NPX * PITCH];
    const int lane = static_cast<int>(threadIdx.x), W = a.W, dmin = a.dmin;
    const unsigned rowid = blockIdx.x / static_cast<unsigned>(a.tiles_x);  // pair * H + y
    const int x0 = static_cast<int>(blockIdx.x - rowid * static_cast<unsigned>(a.tiles_x)) * SGM_SEL_T;
    const int64_t row = static_cast<int64_t>(rowid) * W;  // the row's first pixel
    const int x = x0 + lane, xe = min(x0 + SGM_SEL_T - 1, W - 1);
    int lo = 1, hi = 0, l0, h0, l1, h1;
    if (x < W) sgm_interval(x, W, dmin, a.D, RIGHT ? 1 : 0, &lo, &hi);
    sgm_interval(x0, W, dmin, a.D, RIGHT ? 1 : 0, &l0, &h0);  // the candidates some pixel of the tile admits: between those of its ends
    sgm_interval(xe, W, dmin, a.D, RIGHT ? 1 : 0, &l1, &h1);
    const int tlo = min(l0, l1), thi = max(h0, h1);
    StereoSel s;
    stereo_sel_init(s);
    for (int k0 = (tlo - dmin) / KC * KC; k0 <= thi - dmin; k0 += KC) {  // k0 + KC <= Dp: both are multiples of KC
        __syncthreads();
        const int xs = x0 + (RIGHT ? dmin + k0 : 0);  // the image column of the tile's first LDS row
        for (int it = lane; it < NPX * PIECES; it += SGM_SEL_T) {
            const int pi = it / PIECES, q = it - pi * PIECES, xg = xs + pi;
            uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (xg >= 0 && xg < W) v = *reinterpret_cast<const uint4*>(a.S + (row + xg) * a.Dp + k0 + 8 * q);
            uint32_t* t = tile + pi * PITCH + 4 * q;
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
        __syncthreads();
        const uint16_t* t16 = reinterpret_cast<const uint16_t*>(tile);
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int d = dmin + k0 + j;
            const int c = t16[(lane + (RIGHT ? j : 0)) * (2 * PITCH) + j];
            if (d >= lo && d <= hi) stereo_sel_push(s, d, c);
        }
    }
    if (x < W) {
        const int64_t i = row + x;
        const bool any = s.best != STEREO_INF;
        a.dmap[i] = any ? static_cast<int16_t>(s.bestd) : static_cast<int16_t>(STEREO_NO_DISP);
        if constexpr (!RIGHT) {
            a.disparity[i] = any ? stereo_disparity(s, a.uniqueness_percent, a.subpixel) : NAN;
            a.cost[i] = any ? s.best : -1;
        }
    }
}

// ---- host glue ---------------------------------------------------------------------------------------------------------------------
// The matcher: options and geometry fixed at create, the images and outputs sized for max_pairs and the volumes for `group` pairs
// there.  Every call ends with its stream synchronised.
struct SgmMatcher : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    cba_sgm_options opts;
    StereoGeom geom;
    bool has_geom = false;
    int W = 0, H = 0, max_pairs = 0;
    int KP = 0, Dp = 0, group = 0;
    DevBuf<uint8_t> left, right;   // max_pairs frames
    DevBuf<uint64_t> codeL, codeR;  // group frames
    DevBuf<uint8_t> C;              // group volumes
    DevBuf<uint16_t> S;
    DevBuf<float> disparity, xyz;
    DevBuf<int32_t> cost;
    DevBuf<int16_t> dl, dr;
    std::unique_ptr<DispFilter> filter;  // set_filter; null: none
};
static_assert(!std::is_copy_constructible_v<SgmMatcher> && !std::is_copy_assignable_v<SgmMatcher>, "a handle owns its stream and buffers");

SgmMatcher* sgm_matcher_create(int W, int H, int max_pairs, const cba_sgm_options& o, const cba_stereo_geometry* geom, const double* pose7,
                               int device) {
    auto h = std::make_unique<SgmMatcher>(device);
    h->opts = o;
    h->W = W; h->H = H; h->max_pairs = max_pairs;
    h->has_geom = geom != nullptr;
    if (geom) stereo_fill_geom(geom->focal, geom->cx, geom->cy, geom->baseline, pose7, &h->geom);
    else stereo_fill_geom(0.0, 0.0, 0.0, 0.0, nullptr, &h->geom);
    const int D = o.num_disparities;
    h->KP = D <= 32 ? 1 : D <= 64 ? 2 : D <= 128 ? 4 : 8;
    h->Dp = 32 * h->KP;
    const size_t frame = static_cast<size_t>(W) * H;
    const size_t pair_bytes = frame * (static_cast<size_t>(h->Dp) * 3 + 16);  // C, S and the two codes
    const size_t budget = static_cast<size_t>(o.workspace_mb > 0 ? o.workspace_mb : 2048) << 20;
    h->group = static_cast<int>(std::max<size_t>(1, std::min<size_t>(static_cast<size_t>(max_pairs), budget / pair_bytes)));
    const size_t px = static_cast<size_t>(max_pairs) * frame, gpx = static_cast<size_t>(h->group) * frame;
    h->left.alloc(px);
    h->right.alloc(px);
    h->codeL.alloc(gpx);
    h->codeR.alloc(gpx);
    h->C.alloc(gpx * h->Dp);
    h->S.alloc(gpx * h->Dp);
    h->disparity.alloc(px);
    h->cost.alloc(px);
    h->dl.alloc(px);
    if (o.lr_max_diff >= 0) h->dr.alloc(px);
    if (geom) h->xyz.alloc(3 * px);
    return h.release();
}

int sgm_matcher_max_pairs(const SgmMatcher* h) { return h->max_pairs; }
bool sgm_matcher_has_geometry(const SgmMatcher* h) { return h->has_geom; }

static void sgm_launch_path(int KP, const dim3& grid, hipStream_t s, const SgmPathArgs& a) {
    switch (KP) {
    case 1: hipLaunchKernelGGL(k_sgm_path<1>, grid, dim3(SGM_BLOCK), 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_sgm_path<2>, grid, dim3(SGM_BLOCK), 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_sgm_path<4>, grid, dim3(SGM_BLOCK), 0, s, a); break;
    default: hipLaunchKernelGGL(k_sgm_path<8>, grid, dim3(SGM_BLOCK), 0, s, a); break;
    }
    CBA_HIP(hipGetLastError());
}

// stage_ms (experiment builds), SGM_STAGES entries: upload, census, cost, the 8 path launches in the order of the rule (0 for the
// launches that 4 paths leave out), selection with the finish kernel, download.  The kernel stages are summed over the groups.
void sgm_matcher_process(SgmMatcher* h, int n_pairs, const uint8_t* left, const uint8_t* right, float* disparity, int32_t* cost, float* xyz,
                         double* stage_ms) {
    const hipStream_t s = h->begin();
    const int W = h->W, H = h->H, D = h->opts.num_disparities, Dp = h->Dp;
    const size_t frame = static_cast<size_t>(W) * H, px = static_cast<size_t>(n_pairs) * frame;
    const bool timed = stage_ms != nullptr;
    if (timed)
        for (int k = 0; k < SGM_STAGES; ++k) stage_ms[k] = 0.0;
    StageTimer<2> up(s, timed), down(s, timed);
    up.mark(0);
    h->left.upload(left, px, s);
    h->right.upload(right, px, s);
    up.mark(1);
    const bool lr = h->opts.lr_max_diff >= 0;
    for (int p0 = 0; p0 < n_pairs; p0 += h->group) {
        const int np = std::min(h->group, n_pairs - p0);
        const int64_t gpx = static_cast<int64_t>(np) * static_cast<int64_t>(frame);
        const size_t first = static_cast<size_t>(p0) * frame;
        StageTimer<12> tm(s, timed);
        tm.mark(0);
        hipLaunchKernelGGL(k_sgm_census, dim3(launch_grid(gpx, SGM_BLOCK, SGM_GRID)), dim3(SGM_BLOCK), 0, s, gpx, W, H, h->left.p + first,
                           h->right.p + first, h->codeL.p, h->codeR.p);
        CBA_HIP(hipGetLastError());
        tm.mark(1);
        const int lp = h->KP == 1 ? 1 : h->KP == 2 ? 2 : h->KP == 4 ? 3 : 4;  // Dp / 16 = 2 KP = 1 << lp
        const int tpx = SGM_BLOCK >> lp, chunks = (W + tpx - 1) / tpx;
        hipLaunchKernelGGL(k_sgm_cost, dim3(static_cast<unsigned>(np) * static_cast<unsigned>(H) * static_cast<unsigned>(chunks)), dim3(SGM_BLOCK), 0, s,
                           chunks, lp, W, h->opts.min_disparity, D, h->codeL.p, h->codeR.p, reinterpret_cast<uint4*>(h->C.p));
        CBA_HIP(hipGetLastError());
        tm.mark(2);
        for (int r = 0; r < 8; ++r) {
            if (r < h->opts.paths) {
                SgmPathArgs a;
                a.C = h->C.p; a.S = h->S.p;
                a.W = W; a.H = H; a.D = D;
                sgm_direction(r, &a.dx, &a.dy);
                a.lines = a.dy == 0 ? H : a.dx == 0 ? W : W + H - 1;
                a.chunks = (a.lines + SGM_LINES - 1) / SGM_LINES;
                a.p1 = h->opts.p1; a.p2 = h->opts.p2; a.first = r == 0 ? 1 : 0;
                sgm_launch_path(h->KP, dim3(static_cast<unsigned>(np) * static_cast<unsigned>(a.chunks)), s, a);
            }
            tm.mark(3 + r);
        }
        SgmSelectArgs a;
        a.S = h->S.p;
        a.W = W; a.dmin = h->opts.min_disparity; a.D = D; a.Dp = Dp;
        a.uniqueness_percent = h->opts.uniqueness_percent; a.subpixel = h->opts.subpixel;
        a.tiles_x = (W + SGM_SEL_T - 1) / SGM_SEL_T;
        a.disparity = h->disparity.p + first; a.cost = h->cost.p + first; a.dmap = h->dl.p + first;
        const dim3 grid(static_cast<unsigned>(np) * static_cast<unsigned>(H) * static_cast<unsigned>(a.tiles_x));
        if (Dp >= 64) hipLaunchKernelGGL((k_sgm_select<false, 64>), grid, dim3(SGM_SEL_T), 0, s, a);
        else hipLaunchKernelGGL((k_sgm_select<false, 32>), grid, dim3(SGM_SEL_T), 0, s, a);
        CBA_HIP(hipGetLastError());
        if (lr) {
            a.disparity = nullptr; a.cost = nullptr; a.dmap = h->dr.p + first;
            hipLaunchKernelGGL((k_sgm_select<true, 32>), grid, dim3(SGM_SEL_T), 0, s, a);
            CBA_HIP(hipGetLastError());
        }
        float* const gxyz = xyz && !h->filter ? h->xyz.p + 3 * first : nullptr;  // with a filter the points come from the filtered map
        if (lr || gxyz)  // a pixel's check stays inside its own row, so the finish step can run group by group
            stereo_finish_launch(s, gpx, W, H, h->opts.lr_max_diff, h->dl.p + first, lr ? h->dr.p + first : nullptr, h->disparity.p + first,
                                 gxyz, h->geom);
        tm.mark(11);
        if (timed) {
            CBA_HIP(hipStreamSynchronize(s));
            for (int k = 0; k < 11; ++k) stage_ms[1 + k] += tm.ms(k, k + 1);
        }
    }
    if (h->filter) matcher_filter_finish(*h->filter, s, n_pairs, h->disparity.p, xyz ? h->xyz.p : nullptr, h->geom);
    down.mark(0);
    if (disparity) h->disparity.download(disparity, px, s);
    if (cost) h->cost.download(cost, px, s);
    if (xyz) h->xyz.download(xyz, 3 * px, s);
    down.mark(1);
    CBA_HIP(hipStreamSynchronize(s));
    if (timed) {
        stage_ms[0] = up.ms(0, 1);
        stage_ms[SGM_STAGES - 1] = down.ms(0, 1);
    }
}

void sgm_matcher_set_filter(SgmMatcher* h, const cba_disparity_filter_options* o) { matcher_set_filter(h, o); }

void sgm_matcher_destroy(SgmMatcher* h) noexcept { destroy_handle(h); }

}  // namespace cba
