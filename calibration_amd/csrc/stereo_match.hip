// stereo_match.hip — stereo depth on the GPU (stereo_math.hpp, calibba.h: cba_stereo_matcher, cba_stereo_points).  One stream and one
// synchronise per call:
//   k_stereo_match<RIGHT>  block matching by sums of absolute differences.  A workgroup of four wavefronts owns a strip of SR rows x
//                          4 (64 - 2r) columns of one pair and stages the strip and its halo of both images as bytes in LDS (zeros
//                          outside the image).  A wavefront owns 64 adjacent columns, one per lane; its outer 2r lanes are halo.  For
//                          every row and candidate d a lane keeps the column sum V(x, d) of |ref - other| over 2r + 1 rows in LDS
//                          (uint16, [d][lane], touched by that lane alone: no barrier), updates it with the row that enters and the
//                          row that leaves (v_sad_u8), and the window sum is S(lane + r) - S(lane - r - 1) of the wave's inclusive
//                          prefix sum S of V (six DPP adds, two ds_bpermute): work per pixel and candidate does not grow with r.
//                          The candidates of a pixel arrive in ascending d and go through stereo_sel_push; the cost volume lives in
//                          registers only.  RIGHT = false writes disparity, cost and d*; RIGHT = true swaps the roles (other column
//                          x + d) and writes the left-right map d_R as int16.
//   k_stereo_finish        one lane per pixel, grid-stride: the left-right check and the pixel's 3D point (stereo_point).
//                          stereo_finish_launch queues it for the matchers of this file and of stereo_sgm.hip.
//   k_stereo_points        one lane per caller triple, grid-stride: stereo_point, after k_laser_points.
// No atomics, no scratch, no dynamically indexed private array; every sum is an exact integer, so results do not depend on the tiling.
// Image reads are single bytes inside [0, n_pairs W H); the image buffers are still allocated STM_IMG_PAD bytes longer.
#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

#include "pipelines.hpp"
#include "stereo_math.hpp"

namespace cba {

constexpr int STM_BLOCK = 256;
constexpr int STM_WAVES = STM_BLOCK / 64;
constexpr int STM_GRID = 8192;          // grid-stride cap of the per-pixel kernels
constexpr int STM_IMG_PAD = 16;
constexpr int STM_LDS_MAX = 160 * 1024;  // bytes of LDS a workgroup may take

struct StereoMatchArgs {
    const uint8_t* ref;  // the image whose pixels are matched, [n_pairs][H][W]
    const uint8_t* oth;  // the image searched
    int W, H;
    int dmin, D, r, uniqueness_percent, subpixel;
    int SR, tiles_x, strips;  // strip rows; column tiles and strips of a pair
    int refP, othP;           // LDS row pitches, bytes (multiples of 4)
    float* disparity;         // RIGHT = false only
    int32_t* cost;
    int16_t* dmap;            // d* (RIGHT = false) or d_R (RIGHT = true); STEREO_NO_DISP: no candidate
};

// the wave's inclusive prefix sum over its lanes
__device__ __forceinline__ int stm_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);  // row_shr:8 -> the prefix sum inside each 16-lane row
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);  // row_bcast15 into rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);  // row_bcast31 into rows 2, 3
    return v;
}

// grid = n_pairs * strips * tiles_x workgroups; dynamic LDS = rows (refP + othP) + STM_WAVES D 64 2 bytes, rows = SR + 2r
template <bool RIGHT>
__global__ __launch_bounds__(STM_BLOCK) void k_stereo_match(StereoMatchArgs a) {
    extern __shared__ __align__(16) uint8_t stm_lds[];
    const int r = a.r, W = a.W, H = a.H, D = a.D;
    const int nout = 64 - 2 * r, two = STM_WAVES * nout;  // output columns of a wavefront / of the workgroup
    const int rows = a.SR + 2 * r;
    uint8_t* sref = stm_lds;                  // [rows][refP]
    uint8_t* soth = sref + rows * a.refP;     // [rows][othP]
    uint16_t* sV = reinterpret_cast<uint16_t*>(soth + rows * a.othP);  // [STM_WAVES][D][64]
    int b = blockIdx.x;
    const int tx = b % a.tiles_x;
    b /= a.tiles_x;
    const int st = b % a.strips, pair = b / a.strips;
    const int X0 = tx * two, y0 = st * a.SR;
    const int dmax = a.dmin + D - 1;
    const int refWd = two + 2 * r, othWd = refWd + D - 1;             // staged columns (<= refP, othP)
    const int refX = X0 - r;                                           // image column of LDS column 0
    const int othX = RIGHT ? refX + a.dmin : refX - dmax;
    const int64_t fbase = static_cast<int64_t>(pair) * W * H;
    const int tid = static_cast<int>(threadIdx.x);
    for (int i = tid; i < rows * refWd; i += STM_BLOCK) {
        const int row = i / refWd, c = i - row * refWd;
        const int y = y0 - r + row, x = refX + c;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        sref[row * a.refP + c] = in ? a.ref[fbase + y * W + x] : uint8_t(0);
    }
    for (int i = tid; i < rows * othWd; i += STM_BLOCK) {
        const int row = i / othWd, c = i - row * othWd;
        const int y = y0 - r + row, x = othX + c;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        soth[row * a.othP + c] = in ? a.oth[fbase + y * W + x] : uint8_t(0);
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int cref = wave * nout + lane;  // this lane's LDS column of ref (< refWd)
    const int x = refX + cref;            // ... and its image column
    const bool emits = lane >= r && lane < 64 - r && x < W;  // x >= 0 for these lanes
    // the candidates any output pixel of the wavefront admits: nothing else is evaluated
    const int xa = max(refX + wave * nout + r, r), xb = min(refX + wave * nout + 63 - r, W - 1 - r);
    const int dlo = RIGHT ? max(a.dmin, r - xb) : max(a.dmin, xa + r - W + 1);
    const int dhi = RIGHT ? min(dmax, W - 1 - r - xa) : min(dmax, xb - r);
    const bool work = xa <= xb && dlo <= dhi;
    int lo = 1, hi = 0;
    if (emits) stereo_interval(x, W, r, a.dmin, D, RIGHT ? 1 : 0, &lo, &hi);
    uint16_t* V = sV + (wave * D) * 64 + lane;
    const int hi_addr = min(lane + r, 63) << 2, lo_lane = lane - r - 1, lo_addr = max(lo_lane, 0) << 2;
    bool haveV = false;
    for (int t = 0; t < a.SR; ++t) {
        const int y = y0 + t;
        if (y >= H) break;
        StereoSel s;
        stereo_sel_init(s);
        if (work && y >= r && y <= H - 1 - r) {  // wave-uniform
            const int lr = t + r;                // the LDS row of image row y
            const uint8_t* rnew = sref + (lr + r) * a.refP + cref;
            const uint8_t* onew = soth + (lr + r) * a.othP;
            const int step = (2 * r + 1) * a.othP;  // from the row that leaves (lr - r - 1) to the row that enters
            const unsigned Ln = *rnew, Lo = haveV ? *(rnew - (2 * r + 1) * a.refP) : 0u;
            for (int d = dlo; d <= dhi; ++d) {
                const int co = RIGHT ? cref + d - a.dmin : cref + dmax - d;  // the LDS column of other column x -+ d (< othWd)
                unsigned v;
                if (haveV) {
                    v = V[(d - a.dmin) * 64];
                    v = __builtin_amdgcn_sad_u8(Ln, onew[co], v) - __builtin_amdgcn_sad_u8(Lo, onew[co - step], 0u);
                } else {
                    v = 0u;
                    for (int j = -r; j <= r; ++j) v = __builtin_amdgcn_sad_u8(sref[(lr + j) * a.refP + cref], soth[(lr + j) * a.othP + co], v);
                }
                V[(d - a.dmin) * 64] = static_cast<uint16_t>(v);  // <= 21 * 255
                const int S = stm_scan(static_cast<int>(v));
                const int Shi = __builtin_amdgcn_ds_bpermute(hi_addr, S), Slo = __builtin_amdgcn_ds_bpermute(lo_addr, S);
                const int c = Shi - (lo_lane >= 0 ? Slo : 0);
                if (d >= lo && d <= hi) stereo_sel_push(s, d, c);
            }
            haveV = true;
        }
        if (emits) {
            const int64_t i = fbase + y * W + x;
            const bool any = s.best != STEREO_INF;
            a.dmap[i] = any ? static_cast<int16_t>(s.bestd) : static_cast<int16_t>(STEREO_NO_DISP);
            if constexpr (!RIGHT) {
                a.disparity[i] = any ? stereo_disparity(s, a.uniqueness_percent, a.subpixel) : NAN;
                a.cost[i] = any ? s.best : -1;
            }
        }
    }
}

__global__ __launch_bounds__(STM_BLOCK) void k_stereo_finish(int64_t n_px, int W, int H, int lr_max_diff, const int16_t* __restrict__ dl,
                                                             const int16_t* __restrict__ dr, float* __restrict__ disparity,
                                                             float* __restrict__ xyz, StereoGeom g) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(STM_BLOCK) + threadIdx.x; i < n_px; i += static_cast<int64_t>(gridDim.x) * STM_BLOCK) {
        float d = disparity[i];
        if (lr_max_diff >= 0) {
            const int ds = dl[i];
            if (ds != STEREO_NO_DISP && !stereo_lr_ok(ds, dr[i - ds], lr_max_diff)) {  // column x - d* of the same row: inside it
                d = NAN;
                disparity[i] = d;
            }
        }
        if (xyz) {
            const int64_t row = i / W;
            const int x = static_cast<int>(i - row * W), y = static_cast<int>(row % H);
            double P[3];
            stereo_point(g, static_cast<double>(x), static_cast<double>(y), static_cast<double>(d), P);
            xyz[3 * i] = static_cast<float>(P[0]);
            xyz[3 * i + 1] = static_cast<float>(P[1]);
            xyz[3 * i + 2] = static_cast<float>(P[2]);
        }
    }
}

__global__ __launch_bounds__(STM_BLOCK) void k_stereo_points(int64_t n, const double* __restrict__ uvd, double* __restrict__ xyz, StereoGeom g) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(STM_BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * STM_BLOCK) {
        double P[3];
        stereo_point(g, uvd[3 * i], uvd[3 * i + 1], uvd[3 * i + 2], P);
        xyz[3 * i] = P[0];
        xyz[3 * i + 1] = P[1];
        xyz[3 * i + 2] = P[2];
    }
}

// ---- host glue ---------------------------------------------------------------------------------------------------------------------
void stereo_finish_launch(hipStream_t s, int64_t n_px, int W, int H, int lr_max_diff, const int16_t* dl, const int16_t* dr, float* disparity,
                          float* xyz, const StereoGeom& g) {
    hipLaunchKernelGGL(k_stereo_finish, dim3(launch_grid(n_px, STM_BLOCK, STM_GRID)), dim3(STM_BLOCK), 0, s, n_px, W, H, lr_max_diff, dl, dr,
                       disparity, xyz, g);
    CBA_HIP(hipGetLastError());
}

void stereo_points_gpu(const cba_stereo_geometry& geom, const double* pose7, int64_t n, const double* uvd, double* xyz, int device) {
    StereoGeom g;
    stereo_fill_geom(geom.focal, geom.cx, geom.cy, geom.baseline, pose7, &g);
    StreamLease lease(device);
    const hipStream_t s = lease;
    const size_t np = static_cast<size_t>(n);
    DevBuf<double> duvd, dxyz;
    duvd.alloc(3 * np);
    dxyz.alloc(3 * np);
    duvd.upload(uvd, 3 * np, s);
    hipLaunchKernelGGL(k_stereo_points, dim3(launch_grid(n, STM_BLOCK, STM_GRID)), dim3(STM_BLOCK), 0, s, n, duvd.p, dxyz.p, g);
    CBA_HIP(hipGetLastError());
    dxyz.download(xyz, 3 * np, s);
    CBA_HIP(hipStreamSynchronize(s));
}

// The matcher: options and geometry fixed at create, every buffer sized for max_pairs there.  Every call ends with its stream
// synchronised.
struct StereoMatcher : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    cba_stereo_match_options opts;
    StereoGeom geom;
    bool has_geom = false;
    int W = 0, H = 0, max_pairs = 0;
    int SR = 0, refP = 0, othP = 0, tiles_x = 0, strips = 0;
    size_t lds = 0;
    DevBuf<uint8_t> left, right;  // max_pairs frames + STM_IMG_PAD
    DevBuf<float> disparity, xyz;
    DevBuf<int32_t> cost;
    DevBuf<int16_t> dl, dr;
    std::unique_ptr<DispFilter> filter;  // set_filter; null: none
};
static_assert(!std::is_copy_constructible_v<StereoMatcher> && !std::is_copy_assignable_v<StereoMatcher>, "a handle owns its stream and buffers");

StereoMatcher* stereo_matcher_create(int W, int H, int max_pairs, const cba_stereo_match_options& o, const cba_stereo_geometry* geom,
                                     const double* pose7, int device) {
    auto h = std::make_unique<StereoMatcher>(device);
    h->opts = o;
    h->W = W; h->H = H; h->max_pairs = max_pairs;
    h->has_geom = geom != nullptr;
    if (geom) stereo_fill_geom(geom->focal, geom->cx, geom->cy, geom->baseline, pose7, &h->geom);
    else stereo_fill_geom(0.0, 0.0, 0.0, 0.0, nullptr, &h->geom);
    const int r = o.half_window, D = o.num_disparities, two = STM_WAVES * (64 - 2 * r);
    h->refP = (two + 2 * r + 3) & ~3;
    h->othP = (two + 2 * r + D - 1 + 3) & ~3;
    for (int sr : {32, 16, 8}) {  // the tallest strip whose LDS fits: the first row of a strip costs 2r + 1 rows
        h->SR = sr;
        h->lds = static_cast<size_t>(sr + 2 * r) * (h->refP + h->othP) + static_cast<size_t>(STM_WAVES) * D * 64 * sizeof(uint16_t);
        if (h->lds <= STM_LDS_MAX) break;
    }
    h->tiles_x = (W + two - 1) / two;
    h->strips = (H + h->SR - 1) / h->SR;
    CBA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_stereo_match<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(h->lds)));
    CBA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_stereo_match<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                static_cast<int>(h->lds)));
    const size_t px = static_cast<size_t>(max_pairs) * W * H;
    h->left.alloc(px + STM_IMG_PAD);
    h->right.alloc(px + STM_IMG_PAD);
    h->disparity.alloc(px);
    h->cost.alloc(px);
    h->dl.alloc(px);
    if (o.lr_max_diff >= 0) h->dr.alloc(px);
    if (geom) h->xyz.alloc(3 * px);
    return h.release();
}

int stereo_matcher_max_pairs(const StereoMatcher* h) { return h->max_pairs; }
bool stereo_matcher_has_geometry(const StereoMatcher* h) { return h->has_geom; }

// stage_ms [3] (experiment builds): upload, kernels, download
void stereo_matcher_process(StereoMatcher* h, int n_pairs, const uint8_t* left, const uint8_t* right, float* disparity, int32_t* cost,
                            float* xyz, double* stage_ms) {
    const hipStream_t s = h->begin();
    const size_t px = static_cast<size_t>(n_pairs) * h->W * h->H;
    StageTimer<4> tm(s, stage_ms != nullptr);
    tm.mark(0);
    h->left.upload(left, px, s);
    h->right.upload(right, px, s);
    tm.mark(1);
    StereoMatchArgs a;
    a.ref = h->left.p; a.oth = h->right.p;
    a.W = h->W; a.H = h->H;
    a.dmin = h->opts.min_disparity; a.D = h->opts.num_disparities; a.r = h->opts.half_window;
    a.uniqueness_percent = h->opts.uniqueness_percent; a.subpixel = h->opts.subpixel;
    a.SR = h->SR; a.tiles_x = h->tiles_x; a.strips = h->strips;
    a.refP = h->refP; a.othP = h->othP;
    a.disparity = h->disparity.p; a.cost = h->cost.p; a.dmap = h->dl.p;
    const dim3 grid(static_cast<unsigned>(n_pairs * h->strips * h->tiles_x));
    hipLaunchKernelGGL(k_stereo_match<false>, grid, dim3(STM_BLOCK), h->lds, s, a);
    CBA_HIP(hipGetLastError());
    const bool lr = h->opts.lr_max_diff >= 0;
    if (lr) {
        a.ref = h->right.p; a.oth = h->left.p;
        a.disparity = nullptr; a.cost = nullptr; a.dmap = h->dr.p;
        hipLaunchKernelGGL(k_stereo_match<true>, grid, dim3(STM_BLOCK), h->lds, s, a);
        CBA_HIP(hipGetLastError());
    }
    if (h->filter) {
        if (lr) stereo_finish_launch(s, static_cast<int64_t>(px), h->W, h->H, h->opts.lr_max_diff, h->dl.p, h->dr.p, h->disparity.p, nullptr, h->geom);
        matcher_filter_finish(*h->filter, s, n_pairs, h->disparity.p, xyz ? h->xyz.p : nullptr, h->geom);
    } else if (lr || xyz) {
        stereo_finish_launch(s, static_cast<int64_t>(px), h->W, h->H, h->opts.lr_max_diff, h->dl.p, h->dr.p, h->disparity.p, xyz ? h->xyz.p : nullptr,
                             h->geom);
    }
    tm.mark(2);
    if (disparity) h->disparity.download(disparity, px, s);
    if (cost) h->cost.download(cost, px, s);
    if (xyz) h->xyz.download(xyz, 3 * px, s);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(stage_ms);
}

void stereo_matcher_set_filter(StereoMatcher* h, const cba_disparity_filter_options* o) { matcher_set_filter(h, o); }

void stereo_matcher_destroy(StereoMatcher* h) noexcept { destroy_handle(h); }

}  // namespace cba
