// corner_detect.hip — chessboard corner detection on the GPU (corner_math.hpp, calibba.h: cba_corner_detector).  One stream and one
// synchronise per call:
//   k_corner_response<WIDE>  a workgroup of four wavefronts owns a tile of CRN_TX x CRN_TY pixels of one image and stages the tile and
//                            its 5-pixel halo as bytes in LDS (zeros outside the image).  WIDE (the width is a multiple of 16, so every
//                            row starts on a 16-byte boundary): 16-byte loads of the aligned vectors that cover the tile; otherwise
//                            single bytes.  Both stay inside [0, n_images W H).  A lane owns 4 adjacent pixels of a row: it reads the
//                            dwords of the 9 ring rows that cover columns -8 .. +11 around its first pixel once and cuts every ring
//                            sample out of them with constant shifts.  The ring samples of a pixel are packed four to a dword: DR is two
//                            v_sad_u8, S16 four more against zero.  The response leaves as int16 (one 8-byte store per lane when the
//                            width is a multiple of 4), 0 in the border.
//   k_peak_walk, k_peak_prefix  the row-major peak list of peak_walk.hpp (shared with blob_detect.hip), instantiated for int16
//                            responses, strips of CRN_SH rows and the border CORNER_BORDER.
//   k_corner_refine          one lane per slot (image, corner), grid-stride: response, COG, GRADIENT, the angle sums
//                            (corner_refine_one); slots past the kept corners get NaN / 0.
// The host halves atan2 of the angle sums after the download.  No scratch, no dynamically indexed private array.
#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

#include "pipelines.hpp"
#include "corner_math.hpp"
#include "peak_walk.hpp"

namespace cba {

constexpr int CRN_BLOCK = 256;
constexpr int CRN_TX = 64, CRN_TY = 16;              // the tile: 16 lanes x 4 pixels wide, 16 rows
constexpr int CRN_ROWS = CRN_TY + 2 * CORNER_BORDER;  // staged rows
constexpr int CRN_LEFT = 16;                          // LDS column of the tile's first pixel
constexpr int CRN_PITCH = CRN_TX + 2 * CRN_LEFT;      // 96 bytes: six 16-byte vectors
constexpr int CRN_SH = 16;                            // strip height of the peak passes
constexpr int CRN_GRID = 4096;                        // grid-stride cap of k_corner_refine

struct CornerRespArgs {
    const uint8_t* img;  // [n_images][H][W]
    int16_t* resp;       // [n_images][H][W]
    int W, H, tiles_x, tiles_y;
};

// index of ring row dy in {-5, -3, -2, -1, 0, 1, 2, 3, 5} -> 0..8
__device__ __forceinline__ constexpr int crn_row(int dy) { return dy == -5 ? 0 : dy == 5 ? 8 : dy + 4; }
__device__ __forceinline__ constexpr int crn_row_dy(int r) { return r == 0 ? -5 : r == 8 ? 5 : r - 4; }

// the byte at column x + K + DX of ring row DY, out of the lane's dwords w[ring row][dword]: every index is a constant
template <int DY, int DX, int K>
__device__ __forceinline__ uint32_t crn_px(const uint32_t (&w)[9][5]) {
    constexpr int o = 8 + DX + K;
    return (w[crn_row(DY)][o >> 2] >> (8 * (o & 3))) & 0xffu;
}

// the response of the lane's pixel K (column x + K), 0 in the border
template <int K>
__device__ __forceinline__ int crn_pixel(const uint32_t (&w)[9][5], int x, int y, int W, int H) {
    const uint32_t I0 = crn_px<-5, 0, K>(w), I1 = crn_px<-5, 2, K>(w), I2 = crn_px<-3, 3, K>(w), I3 = crn_px<-2, 5, K>(w);
    const uint32_t I4 = crn_px<0, 5, K>(w), I5 = crn_px<2, 5, K>(w), I6 = crn_px<3, 3, K>(w), I7 = crn_px<5, 2, K>(w);
    const uint32_t I8 = crn_px<5, 0, K>(w), I9 = crn_px<5, -2, K>(w), I10 = crn_px<3, -3, K>(w), I11 = crn_px<2, -5, K>(w);
    const uint32_t I12 = crn_px<0, -5, K>(w), I13 = crn_px<-2, -5, K>(w), I14 = crn_px<-3, -3, K>(w), I15 = crn_px<-5, -2, K>(w);
    const uint32_t P0 = I0 | I1 << 8 | I2 << 16 | I3 << 24, P1 = I4 | I5 << 8 | I6 << 16 | I7 << 24;
    const uint32_t P2 = I8 | I9 << 8 | I10 << 16 | I11 << 24, P3 = I12 | I13 << 8 | I14 << 16 | I15 << 24;
    const int dr = static_cast<int>(__builtin_amdgcn_sad_u8(P0, P2, __builtin_amdgcn_sad_u8(P1, P3, 0u)));
    const int s16 = static_cast<int>(
        __builtin_amdgcn_sad_u8(P0, 0u, __builtin_amdgcn_sad_u8(P1, 0u, __builtin_amdgcn_sad_u8(P2, 0u, __builtin_amdgcn_sad_u8(P3, 0u, 0u)))));
    const int sr = corner_iabs(static_cast<int>(I0 + I8) - static_cast<int>(I4 + I12)) +
                   corner_iabs(static_cast<int>(I1 + I9) - static_cast<int>(I5 + I13)) +
                   corner_iabs(static_cast<int>(I2 + I10) - static_cast<int>(I6 + I14)) +
                   corner_iabs(static_cast<int>(I3 + I11) - static_cast<int>(I7 + I15));
    const int s5 = static_cast<int>(crn_px<0, 0, K>(w) + crn_px<0, -1, K>(w) + crn_px<0, 1, K>(w) + crn_px<-1, 0, K>(w) + crn_px<1, 0, K>(w));
    const int R = 5 * sr - 5 * dr - corner_iabs(5 * s16 - 16 * s5);
    const int xk = x + K;
    const bool inner = xk >= CORNER_BORDER && xk <= W - 1 - CORNER_BORDER && y >= CORNER_BORDER && y <= H - 1 - CORNER_BORDER;
    return inner ? R : 0;
}

template <bool WIDE>
__global__ __launch_bounds__(CRN_BLOCK) void k_corner_response(CornerRespArgs a) {
    __shared__ __align__(16) uint8_t tile[CRN_ROWS * CRN_PITCH];
    const int W = a.W, H = a.H;
    int b = blockIdx.x;
    const int tx = b % a.tiles_x;
    b /= a.tiles_x;
    const int ty = b % a.tiles_y, im = b / a.tiles_y;
    const int x0 = tx * CRN_TX, y0 = ty * CRN_TY;
    const int64_t fbase = static_cast<int64_t>(im) * W * H;
    const int tid = static_cast<int>(threadIdx.x);
    if constexpr (WIDE) {
        constexpr int VPR = CRN_PITCH / 16;
        for (int i = tid; i < CRN_ROWS * VPR; i += CRN_BLOCK) {
            const int row = i / VPR, v = i - row * VPR;
            const int y = y0 - CORNER_BORDER + row, x = x0 - CRN_LEFT + 16 * v;  // x and W are multiples of 16: all in or all out
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (y >= 0 && y < H && x >= 0 && x < W) q = *reinterpret_cast<const uint4*>(a.img + fbase + static_cast<int64_t>(y) * W + x);
            *reinterpret_cast<uint4*>(tile + row * CRN_PITCH + 16 * v) = q;
        }
    } else {
        constexpr int COLS = CRN_TX + 16, C0 = CRN_LEFT - 8;  // the columns the dword reads below touch: x0 - 8 .. x0 + 71
        for (int i = tid; i < CRN_ROWS * COLS; i += CRN_BLOCK) {
            const int row = i / COLS, c = i - row * COLS;
            const int y = y0 - CORNER_BORDER + row, x = x0 - 8 + c;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            tile[row * CRN_PITCH + C0 + c] = in ? a.img[fbase + static_cast<int64_t>(y) * W + x] : uint8_t(0);
        }
    }
    __syncthreads();
    const int ry = tid >> 4, l4 = tid & 15;
    const int x = x0 + 4 * l4, y = y0 + ry;
    if (x >= W || y >= H) return;
    // w[r][j]: dword j of ring row r, columns x - 8 + 4 j .. x - 5 + 4 j
    uint32_t w[9][5];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(tile + (ry + CORNER_BORDER + crn_row_dy(r)) * CRN_PITCH + CRN_LEFT + 4 * l4 - 8);
#pragma unroll
        for (int j = 0; j < 5; ++j) w[r][j] = p[j];
    }
    const int o0 = crn_pixel<0>(w, x, y, W, H), o1 = crn_pixel<1>(w, x, y, W, H), o2 = crn_pixel<2>(w, x, y, W, H),
              o3 = crn_pixel<3>(w, x, y, W, H);
    int16_t* dst = a.resp + fbase + static_cast<int64_t>(y) * W + x;
    if ((W & 3) == 0) {  // x + 3 < W, and the address is a multiple of 8 bytes
        uint2 q;
        q.x = (static_cast<uint32_t>(o0) & 0xffffu) | static_cast<uint32_t>(o1) << 16;
        q.y = (static_cast<uint32_t>(o2) & 0xffffu) | static_cast<uint32_t>(o3) << 16;
        *reinterpret_cast<uint2*>(dst) = q;
    } else {
        dst[0] = static_cast<int16_t>(o0);
        if (x + 1 < W) dst[1] = static_cast<int16_t>(o1);
        if (x + 2 < W) dst[2] = static_cast<int16_t>(o2);
        if (x + 3 < W) dst[3] = static_cast<int16_t>(o3);
    }
}

struct CornerRefineArgs {
    const uint8_t* img;
    const int16_t* resp;
    int W, H, n_slots, max_corners, cog_radius, refine, w, iters;
    const int32_t* count;
    const int32_t* peak_px;
    const double* wt;    // (2w + 1)^2
    const double* trig;  // [16]
    double* xy;          // [n_slots][2]
    double* sums;        // [n_slots][2]
    int32_t* response;   // [n_slots]
    int32_t* flags;      // [n_slots]
};

__global__ __launch_bounds__(CRN_BLOCK) void k_corner_refine(CornerRefineArgs a) {
    for (int i = blockIdx.x * CRN_BLOCK + threadIdx.x; i < a.n_slots; i += gridDim.x * CRN_BLOCK) {
        const int im = i / a.max_corners, slot = i - im * a.max_corners;
        double xy[2] = {NAN, NAN}, sums[2] = {NAN, NAN};
        int flags = 0, response = 0;
        if (slot < min(a.count[im], a.max_corners)) {
            const int p = a.peak_px[i], py = p / a.W, px = p - py * a.W;
            const int64_t fbase = static_cast<int64_t>(im) * a.W * a.H;
            corner_refine_one(a.img + fbase, a.resp + fbase, a.W, a.H, px, py, a.cog_radius, a.refine, a.w, a.iters, a.wt, a.trig, xy, sums,
                              &flags);
            response = a.resp[fbase + p];
        }
        a.xy[2 * i] = xy[0];
        a.xy[2 * i + 1] = xy[1];
        a.sums[2 * i] = sums[0];
        a.sums[2 * i + 1] = sums[1];
        a.response[i] = response;
        a.flags[i] = flags;
    }
}

// ---- host glue ---------------------------------------------------------------------------------------------------------------------
// The detector: options fixed at create, every buffer (the host staging of the angle sums included) sized for max_images there.  Every
// call ends with its stream synchronised.
struct CornerDetector : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    cba_corner_options opts;
    int W = 0, H = 0, max_images = 0, max_corners = 0;
    int tiles_x = 0, tiles_y = 0, strips = 0;
    DevBuf<uint8_t> img;
    DevBuf<int16_t> resp;
    DevBuf<int32_t> strip_count, strip_off, count, status, peak_px, response, flags;
    DevBuf<double> wt, trig, xy, sums;
    std::vector<double> h_sums;
    std::vector<int32_t> h_count;
};
static_assert(!std::is_copy_constructible_v<CornerDetector> && !std::is_copy_assignable_v<CornerDetector>, "a handle owns its stream and buffers");

CornerDetector* corner_detector_create(int W, int H, int max_images, int max_corners, const cba_corner_options& o, int device) {
    auto h = std::make_unique<CornerDetector>(device);
    h->opts = o;
    h->W = W; h->H = H; h->max_images = max_images; h->max_corners = max_corners;
    h->tiles_x = (W + CRN_TX - 1) / CRN_TX;
    h->tiles_y = (H + CRN_TY - 1) / CRN_TY;
    h->strips = (H + CRN_SH - 1) / CRN_SH;
    const size_t px = static_cast<size_t>(max_images) * W * H, slots = static_cast<size_t>(max_images) * max_corners;
    h->img.alloc(px);
    h->resp.alloc(px);
    h->strip_count.alloc(static_cast<size_t>(max_images) * h->strips);
    h->strip_off.alloc(static_cast<size_t>(max_images) * h->strips);
    h->count.alloc(max_images);
    h->status.alloc(max_images);
    h->peak_px.alloc(slots);
    h->response.alloc(slots);
    h->flags.alloc(slots);
    h->xy.alloc(2 * slots);
    h->sums.alloc(2 * slots);
    h->h_sums.resize(2 * slots);
    h->h_count.resize(max_images);
    const int w = o.refine_half_window, side = 2 * w + 1;
    std::vector<double> wt(static_cast<size_t>(side) * side), trig(16);
    corner_weight_table(w, wt.data());
    corner_trig_table(trig.data());
    const hipStream_t s = h->lease;
    h->wt.assign(wt.data(), wt.size(), s);
    h->trig.assign(trig.data(), trig.size(), s);
    CBA_HIP(hipStreamSynchronize(s));
    return h.release();
}

int corner_detector_max_images(const CornerDetector* h) { return h->max_images; }

// stage_ms [5] (experiment builds): upload, response, peaks, refine, download
void corner_detector_process(CornerDetector* h, int n_images, const uint8_t* images, int32_t* out_count, int32_t* out_status, double* out_xy,
                             double* out_angle, int32_t* out_response, int32_t* out_flags, double* stage_ms) {
    const hipStream_t s = h->begin();
    const size_t px = static_cast<size_t>(n_images) * h->W * h->H, slots = static_cast<size_t>(n_images) * h->max_corners;
    StageTimer<6> tm(s, stage_ms != nullptr);
    tm.mark(0);
    h->img.upload(images, px, s);
    tm.mark(1);
    CornerRespArgs ra{h->img.p, h->resp.p, h->W, h->H, h->tiles_x, h->tiles_y};
    const dim3 rgrid(static_cast<unsigned>(n_images * h->tiles_x * h->tiles_y));
    if (h->W % 16 == 0) hipLaunchKernelGGL(k_corner_response<true>, rgrid, dim3(CRN_BLOCK), 0, s, ra);
    else hipLaunchKernelGGL(k_corner_response<false>, rgrid, dim3(CRN_BLOCK), 0, s, ra);
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    PeakArgs<int16_t> pa{h->resp.p, h->W, h->H, h->strips, CORNER_BORDER, h->opts.min_response, h->opts.nms_radius, h->max_corners,
                         h->strip_count.p, h->strip_off.p, h->peak_px.p};
    peak_walk_launch<int16_t, CRN_SH>(s, n_images, pa, h->count.p, h->status.p);
    tm.mark(3);
    CornerRefineArgs fa{h->img.p, h->resp.p, h->W, h->H, static_cast<int>(slots), h->max_corners, h->opts.cog_radius, h->opts.refine,
                        h->opts.refine_half_window, h->opts.refine_iterations, h->count.p, h->peak_px.p, h->wt.p, h->trig.p, h->xy.p,
                        h->sums.p, h->response.p, h->flags.p};
    const int fgrid = launch_grid(static_cast<int64_t>(slots), CRN_BLOCK, CRN_GRID);
    hipLaunchKernelGGL(k_corner_refine, dim3(fgrid), dim3(CRN_BLOCK), 0, s, fa);
    CBA_HIP(hipGetLastError());
    tm.mark(4);
    h->count.download(h->h_count.data(), n_images, s);
    if (out_status) h->status.download(out_status, n_images, s);
    if (out_xy) h->xy.download(out_xy, 2 * slots, s);
    if (out_angle) h->sums.download(h->h_sums.data(), 2 * slots, s);
    if (out_response) h->response.download(out_response, slots, s);
    if (out_flags) h->flags.download(out_flags, slots, s);
    tm.mark(5);
    CBA_HIP(hipStreamSynchronize(s));
    for (int im = 0; im < n_images; ++im) {
        if (out_count) out_count[im] = h->h_count[im];
        if (!out_angle) continue;
        const int kept = std::min(h->h_count[im], h->max_corners);
        for (int c = 0; c < h->max_corners; ++c) {
            const size_t i = static_cast<size_t>(im) * h->max_corners + c;
            out_angle[i] = c < kept ? corner_angle(&h->h_sums[2 * i]) : static_cast<double>(NAN);
        }
    }
    tm.report(stage_ms);
}

void corner_detector_destroy(CornerDetector* h) noexcept { destroy_handle(h); }

}  // namespace cba
