// blob_detect.hip — circle (blob) detection on the GPU (blob_math.hpp, calibba.h: cba_blob_detector).  One stream and one synchronise
// per call:
//   k_blob_response<WIDE>  a workgroup of four wavefronts owns a tile of BLB_TX x BLB_TY pixels of one image and stages the tile and its
//                          15-pixel halo as bytes in LDS (stage_tile of image_tile.hpp, the whole pitch).  Horizontal pass: a lane
//                          owns 4 adjacent pixels of a staged row; the first pixel's two window sums are v_sad_u8 against zero over
//                          the masked dwords of the window (a loop over LDS with run-time bounds), the other three slide by one byte
//                          in and one out; the sums go back to LDS as uint16 (8-byte stores).  Vertical pass: a lane owns 4 adjacent
//                          pixels of a tile row and adds the rows -b .. b of the outer sums and -a .. a of the inner ones (8-byte LDS
//                          reads).  R leaves as int32 and S_in as uint16 (store4).
//   k_peak_walk, k_peak_prefix  the row-major peak list of peak_walk.hpp (shared with corner_detect.hip), instantiated for int32
//                          responses, strips of BLB_SH rows and the border outer_half.
//   k_blob_refine          one lane per slot (image, blob), grid-stride: blob_refine_one; slots past the kept blobs get NaN / 0.
// The host sets the flags that follow from the numbers (blob_number_flags) after the download.  No scratch, no dynamically indexed
// private array.
#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

#include "pipelines.hpp"
#include "blob_math.hpp"
#include "image_tile.hpp"
#include "peak_walk.hpp"

namespace cba {

constexpr int BLB_BLOCK = 256;
constexpr int BLB_TX = 64, BLB_TY = 16;              // the tile: 16 lanes x 4 pixels wide, 16 rows
constexpr int BLB_HALO = BLOB_MAX_OUTER;              // staged rows above and below the tile
constexpr int BLB_ROWS = BLB_TY + 2 * BLB_HALO;       // 46 staged rows
constexpr int BLB_LEFT = 16;                          // LDS column of the tile's first pixel
constexpr int BLB_PITCH = BLB_TX + 2 * BLB_LEFT;      // 96 bytes: six 16-byte vectors
constexpr int BLB_SH = 16;                            // strip height of the peak passes
constexpr int BLB_GRID = 4096;                        // grid-stride cap of k_blob_refine
static_assert(BLB_LEFT >= BLB_HALO + 1 && BLB_TX == 4 * 16 && BLB_BLOCK == 16 * BLB_TY, "the lane layout of k_blob_response");

struct BlobRespArgs {
    const uint8_t* img;  // [n_images][H][W]
    int32_t* resp;       // [n_images][H][W]
    uint16_t* s_in;      // [n_images][H][W]
    int W, H, tiles_x, tiles_y, a, b, polarity;
};

// sum of the bytes of LDS columns c0 .. c1 of one staged row (0 <= c0 <= c1 < BLB_PITCH): whole dwords, the first and last masked
__device__ __forceinline__ uint32_t blb_window(const uint8_t* row, int c0, int c1) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(row);
    const int j0 = c0 >> 2, j1 = c1 >> 2;
    const uint32_t m0 = 0xffffffffu << (8 * (c0 & 3)), m1 = 0xffffffffu >> (8 * (3 - (c1 & 3)));
    uint32_t s = 0;
#pragma unroll 1
    for (int j = j0; j <= j1; ++j) {
        uint32_t v = w[j];
        v = j == j0 ? v & m0 : v;
        v = j == j1 ? v & m1 : v;
        s = __builtin_amdgcn_sad_u8(v, 0u, s);
    }
    return s;
}

template <bool WIDE>
__global__ __launch_bounds__(BLB_BLOCK) void k_blob_response(BlobRespArgs a) {
    __shared__ __align__(16) uint8_t tile[BLB_ROWS * BLB_PITCH];
    __shared__ __align__(8) uint16_t hin[BLB_ROWS * BLB_TX], hout[BLB_ROWS * BLB_TX];
    const int W = a.W, H = a.H, ha = a.a, hb = a.b;
    const auto [x0, y0, im, fbase] = tile_decode<BLB_TX, BLB_TY>(a.tiles_x, a.tiles_y, W, H);
    const int tid = static_cast<int>(threadIdx.x);
    stage_tile<BLB_TX, BLB_TY, BLB_HALO, BLB_LEFT, BLB_PITCH, BLB_BLOCK, WIDE>(tile, a.img, fbase, x0, y0, W, H, tid);  // the whole pitch
    __syncthreads();
    // horizontal sums of the staged rows BLB_HALO - b .. BLB_HALO + BLB_TY - 1 + b, 16 lanes x 4 pixels each
    const int r_lo = BLB_HALO - hb, n_items = (BLB_TY + 2 * hb) * 16;
    for (int i = tid; i < n_items; i += BLB_BLOCK) {
        const int row = r_lo + (i >> 4), g = i & 15;
        const uint8_t* rp = tile + row * BLB_PITCH;
        const int c = BLB_LEFT + 4 * g;  // LDS column of the lane's first pixel; every column below lies in 1 .. 94
        uint32_t so = blb_window(rp, c - hb, c + hb), si = blb_window(rp, c - ha, c + ha);
        const uint32_t o0 = so, i0 = si;
        so = so + rp[c + hb + 1] - rp[c - hb];
        si = si + rp[c + ha + 1] - rp[c - ha];
        const uint32_t o1 = so, i1 = si;
        so = so + rp[c + hb + 2] - rp[c - hb + 1];
        si = si + rp[c + ha + 2] - rp[c - ha + 1];
        const uint32_t o2 = so, i2 = si;
        so = so + rp[c + hb + 3] - rp[c - hb + 2];
        si = si + rp[c + ha + 3] - rp[c - ha + 2];
        *reinterpret_cast<uint2*>(hout + row * BLB_TX + 4 * g) = make_uint2(o0 | o1 << 16, o2 | so << 16);
        *reinterpret_cast<uint2*>(hin + row * BLB_TX + 4 * g) = make_uint2(i0 | i1 << 16, i2 | si << 16);
    }
    __syncthreads();
    const int ry = tid >> 4, l4 = tid & 15;
    const int x = x0 + 4 * l4, y = y0 + ry;
    if (x >= W || y >= H) return;
    uint32_t ob0 = 0, ob1 = 0, ob2 = 0, ob3 = 0, in0 = 0, in1 = 0, in2 = 0, in3 = 0;
#pragma unroll 1
    for (int dy = -hb; dy <= hb; ++dy) {
        const uint2 q = *reinterpret_cast<const uint2*>(hout + (ry + BLB_HALO + dy) * BLB_TX + 4 * l4);
        ob0 += q.x & 0xffffu;
        ob1 += q.x >> 16;
        ob2 += q.y & 0xffffu;
        ob3 += q.y >> 16;
    }
#pragma unroll 1
    for (int dy = -ha; dy <= ha; ++dy) {
        const uint2 q = *reinterpret_cast<const uint2*>(hin + (ry + BLB_HALO + dy) * BLB_TX + 4 * l4);
        in0 += q.x & 0xffffu;
        in1 += q.x >> 16;
        in2 += q.y & 0xffffu;
        in3 += q.y >> 16;
    }
    const int n_in = blob_n_in(ha), n_ring = blob_n_ring(ha, hb);
    const bool rows_in = y >= hb && y <= H - 1 - hb;
    const int sign = a.polarity == BLOB_DARK ? 1 : -1;
    auto resp = [&](uint32_t so, uint32_t si, int xk) {
        const int r = n_in * static_cast<int>(so - si) - n_ring * static_cast<int>(si);
        return rows_in && xk >= hb && xk <= W - 1 - hb ? sign * r : 0;
    };
    const int o0 = resp(ob0, in0, x), o1 = resp(ob1, in1, x + 1), o2 = resp(ob2, in2, x + 2), o3 = resp(ob3, in3, x + 3);
    const int64_t at = fbase + static_cast<int64_t>(y) * W + x;
    store4(x, W, Px4<int32_t, int>{a.resp + at, {o0, o1, o2, o3}}, Px4<uint16_t, uint32_t>{a.s_in + at, {in0, in1, in2, in3}});
}

struct BlobRefineArgs {
    const uint8_t* img;
    const int32_t* resp;
    const uint16_t* s_in;
    int W, H, n_slots, max_blobs, a, b, polarity, max_radius, rounds;
    const int32_t* count;
    const int32_t* peak_px;
    const double* rays;  // [64]
    double* xy;          // [n_slots][2]
    double* shape;       // [n_slots][3]
    double* fit_error;   // [n_slots]
    int32_t* response;   // [n_slots]
    int32_t* flags;      // [n_slots]
};

__global__ __launch_bounds__(BLB_BLOCK) void k_blob_refine(BlobRefineArgs a) {
    for (int i = blockIdx.x * BLB_BLOCK + threadIdx.x; i < a.n_slots; i += gridDim.x * BLB_BLOCK) {
        const SlotAt s = slot_at(i, a.max_blobs, a.count, a.peak_px, a.W, a.H);
        double xy[2] = {NAN, NAN}, shape[3] = {NAN, NAN, NAN}, err = NAN;
        int flags = 0, response = 0;
        if (s.kept) {
            response = a.resp[s.fbase + s.p];
            flags = blob_refine_one(a.img + s.fbase, a.W, a.H, s.px, s.py, response, a.s_in[s.fbase + s.p], a.a, a.b, a.polarity, a.max_radius,
                                    a.rounds, a.rays, xy, shape, &err);
        }
        a.xy[2 * i] = xy[0];
        a.xy[2 * i + 1] = xy[1];
        a.shape[3 * i] = shape[0];
        a.shape[3 * i + 1] = shape[1];
        a.shape[3 * i + 2] = shape[2];
        a.fit_error[i] = err;
        a.response[i] = response;
        a.flags[i] = flags;
    }
}

// ---- host glue ---------------------------------------------------------------------------------------------------------------------
// The detector: options fixed at create, every buffer (the host staging of what the number flags read included) sized for max_images
// there.  Every call ends with its stream synchronised.
struct BlobDetector : DetectorFrame {
    using DetectorFrame::DetectorFrame;
    cba_blob_options opts;
    DevBuf<int32_t> resp;
    DevBuf<uint16_t> s_in;
    DevBuf<double> rays, shape, fit_error;
    std::vector<double> h_xy, h_shape, h_fit;
    std::vector<int32_t> h_flags;
};
static_assert(!std::is_copy_constructible_v<BlobDetector> && !std::is_copy_assignable_v<BlobDetector>, "a handle owns its stream and buffers");

BlobDetector* blob_detector_create(int W, int H, int max_images, int max_blobs, const cba_blob_options& o, int device) {
    auto h = std::make_unique<BlobDetector>(device);
    h->opts = o;
    h->alloc(W, H, max_images, max_blobs, BLB_TX, BLB_TY, BLB_SH);
    const size_t px = static_cast<size_t>(max_images) * W * H, slots = static_cast<size_t>(max_images) * max_blobs;
    h->resp.alloc(px);
    h->s_in.alloc(px);
    h->shape.alloc(3 * slots);
    h->fit_error.alloc(slots);
    h->h_xy.resize(2 * slots);
    h->h_shape.resize(3 * slots);
    h->h_fit.resize(slots);
    h->h_flags.resize(slots);
    std::vector<double> rays(2 * BLOB_RAYS);
    blob_ray_table(rays.data());
    const hipStream_t s = h->lease;
    h->rays.assign(rays.data(), rays.size(), s);
    CBA_HIP(hipStreamSynchronize(s));
    return h.release();
}

int blob_detector_max_images(const BlobDetector* h) { return h->max_images; }

// stage_ms [5] (experiment builds): upload, response, peaks, refine, download
void blob_detector_process(BlobDetector* h, int n_images, const uint8_t* images, int32_t* out_count, int32_t* out_status, double* out_xy,
                           double* out_shape, double* out_fit_error, int32_t* out_response, int32_t* out_flags, double* stage_ms) {
    const hipStream_t s = h->begin();
    const cba_blob_options& o = h->opts;
    const size_t slots = static_cast<size_t>(n_images) * h->max_items;
    StageTimer<6> tm(s, stage_ms != nullptr);
    const BlobRespArgs ra{h->img.p, h->resp.p, h->s_in.p, h->W, h->H, h->tiles_x, h->tiles_y, o.inner_half, o.outer_half, o.polarity};
    const PeakArgs<int32_t> pa{h->resp.p, h->W, h->H, h->strips, o.outer_half, blob_threshold(o.inner_half, o.outer_half, o.min_contrast),
                               o.nms_radius, h->max_items, h->strip_count.p, h->strip_off.p, h->peak_px.p};
    h->find_peaks<BLB_SH>(tm, s, n_images, images, k_blob_response<true>, k_blob_response<false>, BLB_BLOCK, ra, pa);
    BlobRefineArgs fa{h->img.p, h->resp.p, h->s_in.p, h->W, h->H, static_cast<int>(slots), h->max_items, o.inner_half, o.outer_half,
                      o.polarity, o.max_radius, o.rounds, h->count.p, h->peak_px.p, h->rays.p, h->xy.p, h->shape.p, h->fit_error.p,
                      h->response.p, h->flags.p};
    hipLaunchKernelGGL(k_blob_refine, dim3(launch_grid(static_cast<int64_t>(slots), BLB_BLOCK, BLB_GRID)), dim3(BLB_BLOCK), 0, s, fa);
    CBA_HIP(hipGetLastError());
    h->fetch_counts(tm, s, n_images, out_status);
    if (out_response) h->response.download(out_response, slots, s);
    h->xy.download(h->h_xy.data(), 2 * slots, s);
    h->shape.download(h->h_shape.data(), 3 * slots, s);
    h->fit_error.download(h->h_fit.data(), slots, s);
    h->flags.download(h->h_flags.data(), slots, s);
    h->finish(tm, s, n_images, out_count, stage_ms);
    for (int im = 0; im < n_images; ++im) {
        const size_t at = static_cast<size_t>(im) * h->max_items;
        blob_number_flags(std::min(h->h_count[im], h->max_items), &h->h_xy[2 * at], &h->h_shape[3 * at], &h->h_fit[at], o.max_fit_error,
                          o.max_axis_ratio, o.min_radius, &h->h_flags[at]);
    }
    if (out_xy) std::copy(h->h_xy.begin(), h->h_xy.begin() + 2 * slots, out_xy);
    if (out_shape) std::copy(h->h_shape.begin(), h->h_shape.begin() + 3 * slots, out_shape);
    if (out_fit_error) std::copy(h->h_fit.begin(), h->h_fit.begin() + slots, out_fit_error);
    if (out_flags) std::copy(h->h_flags.begin(), h->h_flags.begin() + slots, out_flags);
}

void blob_detector_destroy(BlobDetector* h) noexcept { destroy_handle(h); }

}  // namespace cba
