// peak_walk.hpp — the row-major peak list both detectors share (corner_detect.hip: int16 responses, border 5; blob_detect.hip: int32
// responses, border outer_half).  peak_is_max is __host__ __device__ (corner_math.hpp and blob_math.hpp call it, and g++ compiles it for
// the host builds of the tests); the kernels below exist under hipcc only.
//   k_peak_walk<RT, SH, PLACE>  one workgroup per strip of SH rows of one image walks the strip in row-major chunks of 256 pixels; a
//                           lane tests its pixel (peak_is_max), the wavefront ballots, ranks come from popcounts and the four
//                           wavefront totals from LDS.  PLACE = false leaves the strip's count; k_peak_prefix turns the counts of an
//                           image into exclusive offsets, the true count and the status; PLACE = true repeats the walk and writes
//                           each peak's pixel index at offset + rank.  No atomic: the order is row-major by construction.
//   DetectorFrame           the host frame of the two detector handles: what they hold in common and the shared parts of a call.
#pragma once
#include <cstdint>

#include "camera_math.hpp"
#if defined(__HIPCC__)
#include <algorithm>
#include <vector>

#include "hip_glue.hpp"
#endif

namespace cba {

constexpr int PEAK_STATUS_OVERFLOW = 1;

// R: one image's responses [H][W].  A peak: R >= min_response, at least border + nms from every border, greater than every earlier and
// not less than every later response of its (2 nms + 1)^2 window.
template <typename RT>
CBA_HD bool peak_is_max(const RT* R, int W, int H, int x, int y, int min_response, int nms, int border) {
    const int b = border + nms;
    if (x < b || y < b || x > W - 1 - b || y > H - 1 - b) return false;
    const int v = R[y * W + x];
    if (v < min_response) return false;
    for (int dy = -nms; dy <= nms; ++dy)
        for (int dx = -nms; dx <= nms; ++dx) {
            const int q = R[(y + dy) * W + x + dx];
            const bool earlier = dy < 0 || (dy == 0 && dx < 0);
            if (earlier ? q >= v : q > v) return false;  // the pixel itself: q > v is false
        }
    return true;
}

#if defined(__HIPCC__)
constexpr int PEAK_BLOCK = 256;

template <typename RT>
struct PeakArgs {
    const RT* resp;
    int W, H, strips, border, min_response, nms, max_peaks;
    int32_t* strip_count;       // [n_images][strips] (PLACE = false)
    int32_t* strip_off;         // [n_images][strips] (k_peak_prefix writes it, PLACE = true reads it)
    int32_t* peak_px;           // [n_images][max_peaks]: y W + x
};

template <typename RT, int SH, bool PLACE>
__global__ __launch_bounds__(PEAK_BLOCK) void k_peak_walk(PeakArgs<RT> a) {
    __shared__ int wsum[PEAK_BLOCK / 64];
    const int W = a.W, H = a.H;
    const int im = static_cast<int>(blockIdx.x) / a.strips, st = static_cast<int>(blockIdx.x) - im * a.strips;
    const int y0 = st * SH, npx = min(SH, H - y0) * W;
    const RT* R = a.resp + static_cast<int64_t>(im) * W * H;
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    int running = PLACE ? a.strip_off[blockIdx.x] : 0;
    for (int base = 0; base < npx; base += PEAK_BLOCK) {  // uniform over the workgroup
        const int p = base + tid;
        bool flag = false;
        int x = 0, y = 0;
        if (p < npx) {
            const int ry = p / W;
            x = p - ry * W;
            y = y0 + ry;
            flag = peak_is_max<RT>(R, W, H, x, y, a.min_response, a.nms, a.border);
        }
        const unsigned long long m = __ballot(flag);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < PEAK_BLOCK / 64; ++v) {
            const int c = wsum[v];
            before += v < wave ? c : 0;
            total += c;
        }
        if constexpr (PLACE) {
            if (flag) {
                const int slot = running + before + __popcll(m & ((1ull << lane) - 1ull));
                if (slot < a.max_peaks) a.peak_px[static_cast<int64_t>(im) * a.max_peaks + slot] = y * W + x;
            }
        }
        running += total;
        __syncthreads();
    }
    if constexpr (!PLACE) {
        if (tid == 0) a.strip_count[blockIdx.x] = running;
    }
}

// one lane per image: the strips' counts -> exclusive offsets, the true count and the status (a template only so that the header can
// hold it: every translation unit that launches it gets its own copy)
template <typename RT>
__global__ __launch_bounds__(64) void k_peak_prefix(int n_images, PeakArgs<RT> a, int32_t* __restrict__ count, int32_t* __restrict__ status) {
    const int im = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (im >= n_images) return;
    int run = 0;
    for (int s = 0; s < a.strips; ++s) {
        a.strip_off[im * a.strips + s] = run;
        run += a.strip_count[im * a.strips + s];
    }
    count[im] = run;
    status[im] = run > a.max_peaks ? PEAK_STATUS_OVERFLOW : 0;
}

// the three launches of one peak list on stream s
template <typename RT, int SH>
inline void peak_walk_launch(hipStream_t s, int n_images, const PeakArgs<RT>& pa, int32_t* count, int32_t* status) {
    const dim3 pgrid(static_cast<unsigned>(n_images * pa.strips));
    hipLaunchKernelGGL((k_peak_walk<RT, SH, false>), pgrid, dim3(PEAK_BLOCK), 0, s, pa);
    CBA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_peak_prefix<RT>, dim3((n_images + 63) / 64), dim3(64), 0, s, n_images, pa, count, status);
    CBA_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_peak_walk<RT, SH, true>), pgrid, dim3(PEAK_BLOCK), 0, s, pa);
    CBA_HIP(hipGetLastError());
}

// The frame of a detector handle (corner_detect.hip, blob_detect.hip): the sizes, the buffers of the image, the peak list and the
// outputs every detector has, and the parts of a call round the detector's own two launches, its downloads and its host pass:
//   find_peaks  upload, the response kernel (wide when W % 16 == 0), the peak list; timer marks 0 .. 3
//   fetch_counts  after the refine launch: mark 4, count -> h_count and status queued
//   finish  mark 5, the call's one synchronise, out_count, the stage times
struct __attribute__((visibility("hidden"))) DetectorFrame : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    int W = 0, H = 0, max_images = 0, max_items = 0;
    int tiles_x = 0, tiles_y = 0, strips = 0;
    DevBuf<uint8_t> img;
    DevBuf<int32_t> strip_count, strip_off, count, status, peak_px, response, flags;
    DevBuf<double> xy;
    std::vector<int32_t> h_count;

    // tiles of tw x th pixels, strips of sh rows; returns the pixels and the slots of max_images_ images
    void alloc(int W_, int H_, int max_images_, int max_items_, int tw, int th, int sh) {
        W = W_; H = H_; max_images = max_images_; max_items = max_items_;
        tiles_x = (W + tw - 1) / tw;
        tiles_y = (H + th - 1) / th;
        strips = (H + sh - 1) / sh;
        const size_t slots = static_cast<size_t>(max_images) * max_items;
        img.alloc(static_cast<size_t>(max_images) * W * H);
        strip_count.alloc(static_cast<size_t>(max_images) * strips);
        strip_off.alloc(static_cast<size_t>(max_images) * strips);
        count.alloc(max_images);
        status.alloc(max_images);
        peak_px.alloc(slots);
        response.alloc(slots);
        flags.alloc(slots);
        xy.alloc(2 * slots);
        h_count.resize(max_images);
    }
    template <int SH, typename RT, typename RA>
    void find_peaks(StageTimer<6>& tm, hipStream_t s, int n_images, const uint8_t* images, void (*wide)(RA), void (*narrow)(RA), int block,
                    const RA& ra, const PeakArgs<RT>& pa) {
        tm.mark(0);
        img.upload(images, static_cast<size_t>(n_images) * W * H, s);
        tm.mark(1);
        hipLaunchKernelGGL(W % 16 == 0 ? wide : narrow, dim3(static_cast<unsigned>(n_images * tiles_x * tiles_y)), dim3(block), 0, s, ra);
        CBA_HIP(hipGetLastError());
        tm.mark(2);
        peak_walk_launch<RT, SH>(s, n_images, pa, count.p, status.p);
        tm.mark(3);
    }
    void fetch_counts(StageTimer<6>& tm, hipStream_t s, int n_images, int32_t* out_status) {
        tm.mark(4);
        count.download(h_count.data(), n_images, s);
        if (out_status) status.download(out_status, n_images, s);
    }
    void finish(StageTimer<6>& tm, hipStream_t s, int n_images, int32_t* out_count, double* stage_ms) {
        tm.mark(5);
        CBA_HIP(hipStreamSynchronize(s));
        if (out_count) std::copy(h_count.begin(), h_count.begin() + n_images, out_count);
        tm.report(stage_ms);
    }
};
#endif

}  // namespace cba
