// corner_detect.hip — chessboard corner detection on the GPU (corner_math.hpp, calibba.h: cba_corner_detector).  One stream and one
// synchronise per call:
//   k_corner_response<WIDE>  a workgroup of four wavefronts owns a tile of CRN_TX x CRN_TY pixels of one image and stages the tile and
//                            its 5-pixel halo as bytes in LDS (stage_tile of image_tile.hpp; the byte path stages only the columns
//                            read below).  A lane owns 4 adjacent pixels of a row: it reads the dwords of the 9 ring rows that cover
//                            columns -8 .. +11 around its first pixel once and cuts every ring sample out of them with constant
//                            shifts.  The ring samples of a pixel are packed four to a dword: DR is two v_sad_u8, S16 four more
//                            against zero.  The response leaves as int16 (store4), 0 in the border.
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
#include "image_tile.hpp"
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
    const auto [x0, y0, im, fbase] = tile_decode<CRN_TX, CRN_TY>(a.tiles_x, a.tiles_y, W, H);
    const int tid = static_cast<int>(threadIdx.x);
    // the byte path stages only the columns the dword reads below touch: x0 - 8 .. x0 + 71
    stage_tile<CRN_TX, CRN_TY, CORNER_BORDER, CRN_LEFT, CRN_PITCH, CRN_BLOCK, WIDE, CRN_LEFT - 8, CRN_TX + 16>(tile, a.img, fbase, x0, y0, W, H, tid);
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
    store4(x, W, Px4<int16_t, int>{a.resp + fbase + static_cast<int64_t>(y) * W + x, {o0, o1, o2, o3}});
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
        const SlotAt s = slot_at(i, a.max_corners, a.count, a.peak_px, a.W, a.H);
        double xy[2] = {NAN, NAN}, sums[2] = {NAN, NAN};
        int flags = 0, response = 0;
        if (s.kept) {
            corner_refine_one(a.img + s.fbase, a.resp + s.fbase, a.W, a.H, s.px, s.py, a.cog_radius, a.refine, a.w, a.iters, a.wt, a.trig, xy,
                              sums, &flags);
            response = a.resp[s.fbase + s.p];
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
struct CornerDetector : DetectorFrame {
    using DetectorFrame::DetectorFrame;
    cba_corner_options opts;
    DevBuf<int16_t> resp;
    DevBuf<double> wt, trig, sums;
    std::vector<double> h_sums;
};
static_assert(!std::is_copy_constructible_v<CornerDetector> && !std::is_copy_assignable_v<CornerDetector>, "a handle owns its stream and buffers");

CornerDetector* corner_detector_create(int W, int H, int max_images, int max_corners, const cba_corner_options& o, int device) {
    auto h = std::make_unique<CornerDetector>(device);
    h->opts = o;
    h->alloc(W, H, max_images, max_corners, CRN_TX, CRN_TY, CRN_SH);
    const size_t slots = static_cast<size_t>(max_images) * max_corners;
    h->resp.alloc(static_cast<size_t>(max_images) * W * H);
    h->sums.alloc(2 * slots);
    h->h_sums.resize(2 * slots);
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
CornerDeviceView corner_detector_view(const CornerDetector* h) { return {h->img.p, h->xy.p, h->count.p, h->peak_px.p}; }

// stage_ms [5] (experiment builds): upload, response, peaks, refine, download
void corner_detector_process(CornerDetector* h, int n_images, const uint8_t* images, int32_t* out_count, int32_t* out_status, double* out_xy,
                             double* out_angle, int32_t* out_response, int32_t* out_flags, double* stage_ms) {
    const hipStream_t s = h->begin();
    const size_t slots = static_cast<size_t>(n_images) * h->max_items;
    StageTimer<6> tm(s, stage_ms != nullptr);
    const CornerRespArgs ra{h->img.p, h->resp.p, h->W, h->H, h->tiles_x, h->tiles_y};
    const PeakArgs<int16_t> pa{h->resp.p, h->W, h->H, h->strips, CORNER_BORDER, h->opts.min_response, h->opts.nms_radius, h->max_items,
                               h->strip_count.p, h->strip_off.p, h->peak_px.p};
    h->find_peaks<CRN_SH>(tm, s, n_images, images, k_corner_response<true>, k_corner_response<false>, CRN_BLOCK, ra, pa);
    CornerRefineArgs fa{h->img.p, h->resp.p, h->W, h->H, static_cast<int>(slots), h->max_items, h->opts.cog_radius, h->opts.refine,
                        h->opts.refine_half_window, h->opts.refine_iterations, h->count.p, h->peak_px.p, h->wt.p, h->trig.p, h->xy.p,
                        h->sums.p, h->response.p, h->flags.p};
    hipLaunchKernelGGL(k_corner_refine, dim3(launch_grid(static_cast<int64_t>(slots), CRN_BLOCK, CRN_GRID)), dim3(CRN_BLOCK), 0, s, fa);
    CBA_HIP(hipGetLastError());
    h->fetch_counts(tm, s, n_images, out_status);
    if (out_xy) h->xy.download(out_xy, 2 * slots, s);
    if (out_angle) h->sums.download(h->h_sums.data(), 2 * slots, s);
    if (out_response) h->response.download(out_response, slots, s);
    if (out_flags) h->flags.download(out_flags, slots, s);
    h->finish(tm, s, n_images, out_count, stage_ms);
    for (int im = 0; out_angle && im < n_images; ++im) {
        const int kept = std::min(h->h_count[im], h->max_items);
        for (int c = 0; c < h->max_items; ++c) {
            const size_t i = static_cast<size_t>(im) * h->max_items + c;
            out_angle[i] = c < kept ? corner_angle(&h->h_sums[2 * i]) : static_cast<double>(NAN);
        }
    }
}

void corner_detector_destroy(CornerDetector* h) noexcept { destroy_handle(h); }

}  // namespace cba
