// structured_light.hip — structured-light decoding on the GPU (structured_light_math.hpp, calibba.h: cba_sl_decoder).  One stream, one
// decode launch (and one points launch when points are asked for) and one synchronise per call:
//   k_sl_decode<NW, V2>  a lane owns NC = 4 NW adjacent columns of one row of one sequence and walks the sequence's image stack: white,
//                        black, then per axis the Gray pairs and the phase steps.  NW = 4 when the width is a multiple of 16: one
//                        aligned 16-byte load per image (every image base is then a multiple of 16 bytes); otherwise NW = 1: four
//                        columns cut out of the two aligned dwords that hold them, as k_laser_scan_cols does, which also serves odd
//                        image bases.  The two loads of a Gray pair are issued together and the next pair's before this pair's
//                        compares; the compares act on whole dwords (sl_gray_plane), only a pixel's code bit is extracted per pixel.
//                        The per-pixel state (code, S, C) lives in registers indexed by unrolled loops; the finish (sl_axis_finish:
//                        sqrt, atan2) runs once per pair of pixels in a rolled loop that rotates the state down by two, so the kernel
//                        holds one copy of it.  Coordinates leave as 16-byte vectors when the width is even (V2), status as the lane's
//                        packed bytes (one 16-byte or one dword store; byte stores where a group is cut by the row's end or is not
//                        dword-aligned).
//   k_sl_points<MODEL>   one lane per pixel, grid-stride, on the resident coordinate maps: uv = (column, row, x, y) in registers,
//                        tri_point<MODEL, false> with stride 2 on the two TriCamera records of the rig (wave-uniform loads).
// No atomics, no LDS, no scratch, no dynamically indexed private array.  Image loads never leave the decoder's image buffer: it is
// allocated SL_IMG_PAD bytes longer than the stacks, and a sample past a row's end is never used.
#include <memory>
#include <type_traits>

#include "pipelines.hpp"
#include "structured_light_math.hpp"
#include "tri_math.hpp"

namespace cba {

constexpr int SL_BLOCK = 256;
constexpr int SL_GRID = 8192;    // grid-stride cap of k_sl_points
constexpr int SL_IMG_PAD = 32;   // bytes after the last image that a funnel load may touch

struct SlArgs {
    const uint8_t* img;  // [n_seq][n_images][H][W]
    int W, H, n_seq, n_images;
    int groups;          // lanes of a row: ceil(W / NC)
    double* coord;       // [n_seq][n_axes][H][W]
    double* mod;         // the same, or null
    uint8_t* status;     // [n_seq][H][W]
};

// NC adjacent samples from byte index e: NW = 4: one aligned 16-byte load; NW = 1: the dword at e cut out of the two aligned dwords
// around it (one when e is aligned)
template <int NW>
__device__ __forceinline__ void sl_load(const uint8_t* __restrict__ img, int64_t e, uint32_t* w) {
    if constexpr (NW == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(img + e);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
        static_assert(NW == 1, "4 or 16 samples");
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(img + (e & ~int64_t(3)));
        const int s = static_cast<int>(e & 3) * 8;
        uint32_t v = wp[0];
        if (s) v = (v >> s) | (wp[1] << (32 - s));
        w[0] = v;
    }
}

__device__ __forceinline__ int64_t sl_at_most(int64_t e, int64_t last) { return e < last ? e : last; }

// grid = ceil(n_seq H groups / SL_BLOCK) workgroups, one lane per group of NC columns
template <int NW, bool V2>
__global__ __launch_bounds__(SL_BLOCK) void k_sl_decode(SlArgs a, SlRule r) {
    constexpr int NC = 4 * NW;
    const int64_t item = blockIdx.x * static_cast<int64_t>(SL_BLOCK) + threadIdx.x;
    const int64_t rows = static_cast<int64_t>(a.n_seq) * a.H;
    if (item >= rows * a.groups) return;
    const int64_t srow = item / a.groups;  // sequence * H + row
    const int c0 = static_cast<int>(item - srow * a.groups) * NC;
    const int seq = static_cast<int>(srow / a.H), row = static_cast<int>(srow - static_cast<int64_t>(seq) * a.H);
    const int64_t plane = static_cast<int64_t>(a.W) * a.H;
    int64_t e = static_cast<int64_t>(seq) * a.n_images * plane + static_cast<int64_t>(row) * a.W + c0;  // this lane's samples in image 0
    const int64_t last = e + static_cast<int64_t>(a.n_images - 1) * plane;  // ... in the sequence's last image

    uint32_t p[NW], q[NW], np[NW], nq[NW], st[NW];
    sl_load<NW>(a.img, e, p);
    sl_load<NW>(a.img, e + plane, q);
    e += 2 * plane;
    // the first pair of axis 0 is on its way before the contrast compares; a sequence has at least 4 images
    sl_load<NW>(a.img, e, np);
    sl_load<NW>(a.img, e + plane, nq);
#pragma unroll
    for (int w = 0; w < NW; ++w) st[w] = sl_low_contrast(p[w], q[w], r.min_contrast);

    const int64_t px0 = static_cast<int64_t>(row) * a.W + c0;  // in one map
#pragma unroll 1
    for (int ai = 0; ai < r.n_axes; ++ai) {
        const SlAxis ax = r.axis[ai];
        const int shift = 1 + 3 * (r.first_axis + ai);
        int code[NC];
        uint32_t bin[NW], unc[NW];
#pragma unroll
        for (int k = 0; k < NC; ++k) code[k] = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { bin[w] = 0u; unc[w] = 0u; }
#pragma unroll 1
        for (int b = 0; b < ax.nbits; ++b) {
#pragma unroll
            for (int w = 0; w < NW; ++w) { p[w] = np[w]; q[w] = nq[w]; }
            e += 2 * plane;
            // the next pair (after the last plane: the first phase steps, the next axis's first pair, or the last image again)
            sl_load<NW>(a.img, sl_at_most(e, last), np);
            sl_load<NW>(a.img, sl_at_most(e + plane, last), nq);
#pragma unroll
            for (int w = 0; w < NW; ++w) sl_gray_plane(p[w], q[w], r.min_bit_diff, &bin[w], &unc[w]);
#pragma unroll
            for (int k = 0; k < NC; ++k) sl_code_push(&code[k], bin[k >> 2], k & 3);
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) st[w] |= unc[w] << shift;
        double S[NC], C[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) { S[k] = 0.0; C[k] = 0.0; }
        // the phase steps: np holds step 0 (and nq step 1) already
#pragma unroll 1
        for (int k = 0; k < ax.N; ++k) {
#pragma unroll
            for (int w = 0; w < NW; ++w) { p[w] = np[w]; np[w] = nq[w]; }
            e += plane;
            sl_load<NW>(a.img, sl_at_most(e + plane, last), nq);
#pragma unroll
            for (int i = 0; i < NC; ++i) sl_phase_push(r, k, sl_byte(p[i >> 2], i & 3), &S[i], &C[i]);
        }
        // finish, two pixels at a time; the state and the status bytes rotate down by two pixels per round
        double* const cmap = a.coord + (static_cast<int64_t>(seq) * r.n_axes + ai) * plane + px0;
        double* const mmap = a.mod ? a.mod + (static_cast<int64_t>(seq) * r.n_axes + ai) * plane + px0 : nullptr;
#pragma unroll 1
        for (int k = 0; k < NC; k += 2) {
            double x[2], m[2];
            uint32_t bits = 0u;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t sb = sl_byte(st[0], i);
                const bool skip = (sb & (SL_LOW_CONTRAST | SL_UNCERTAIN << shift)) != 0u;
                bits |= (sb | sl_axis_finish(ax, skip, code[i], S[i], C[i], r.min_modulation, &x[i], &m[i]) << shift) << (8 * i);
            }
            if (V2) {
                if (c0 + k < a.W) {
                    reinterpret_cast<double2*>(cmap + k)[0] = make_double2(x[0], x[1]);
                    if (mmap) reinterpret_cast<double2*>(mmap + k)[0] = make_double2(m[0], m[1]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (c0 + k + i < a.W) {
                        cmap[k + i] = x[i];
                        if (mmap) mmap[k + i] = m[i];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i + 2 < NC; ++i) { code[i] = code[i + 2]; S[i] = S[i + 2]; C[i] = C[i + 2]; }
#pragma unroll
            for (int w = 0; w + 1 < NW; ++w) st[w] = st[w] >> 16 | st[w + 1] << 16;
            st[NW - 1] = st[NW - 1] >> 16 | bits << 16;
        }
    }
    // low contrast: bit 0 alone
#pragma unroll
    for (int w = 0; w < NW; ++w) st[w] &= ~((st[w] & SL_ONES) * 0xfeu);
    uint8_t* const sp = a.status + static_cast<int64_t>(seq) * plane + px0;
    if constexpr (NW == 4) {
        *reinterpret_cast<uint4*>(sp) = make_uint4(st[0], st[1], st[2], st[3]);  // W % 16 == 0: whole and aligned
    } else {
        if (c0 + NC <= a.W && (reinterpret_cast<uintptr_t>(sp) & 3u) == 0u) {
            *reinterpret_cast<uint32_t*>(sp) = st[0];
        } else {
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if (c0 + i < a.W) sp[i] = static_cast<uint8_t>(sl_byte(st[0], i));
        }
    }
}

// the points of the pixels of n_seq sequences from their coordinate maps
template <int MODEL>
__global__ __launch_bounds__(SL_BLOCK) void k_sl_points(int64_t n, int W, int H, const double* __restrict__ coord,
                                                        const TriCamera* __restrict__ cams, cba_triangulate_options o,
                                                        double* __restrict__ xyz, double* __restrict__ rms, int32_t* __restrict__ status) {
    const int64_t plane = static_cast<int64_t>(W) * H;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(SL_BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * SL_BLOCK) {
        const int64_t seq = i / plane, px = i - seq * plane;
        const int row = static_cast<int>(px / W), col = static_cast<int>(px - static_cast<int64_t>(row) * W);
        alignas(16) double uv[4];
        uv[0] = static_cast<double>(col);
        uv[1] = static_cast<double>(row);
        uv[2] = coord[2 * seq * plane + px];
        uv[3] = coord[(2 * seq + 1) * plane + px];
        TriResult t;
        tri_point<MODEL, false>(cams, 2, uv, 2, o, &t);
        xyz[3 * i] = t.X[0];
        xyz[3 * i + 1] = t.X[1];
        xyz[3 * i + 2] = t.X[2];
        rms[i] = t.rms;
        status[i] = t.status;
    }
}

// ---- host glue ---------------------------------------------------------------------------------------------------------------------
int sl_options_image_count(const cba_sl_options& o) {
    SlRule r;
    sl_fill_rule(o, &r);
    return sl_image_count(r);
}

void sl_patterns_host(const cba_sl_options& o, uint8_t* out) { sl_patterns(o, out); }

// The decoder: options fixed at create, every buffer sized for max_sequences there (the point buffers when a rig is set).  Every call
// ends with its stream synchronised.
struct SlDecoder : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    SlRule rule;
    int W = 0, H = 0, max_sequences = 0, n_images = 0;
    bool rig = false;
    int model = 0;
    cba_triangulate_options tri_opts{};
    DevBuf<uint8_t> img, status;
    DevBuf<double> coord, mod;
    DevBuf<TriCamera> cams;
    DevBuf<double> xyz, rms;
    DevBuf<int32_t> tri_status;
};
static_assert(!std::is_copy_constructible_v<SlDecoder> && !std::is_copy_assignable_v<SlDecoder>, "a handle owns its stream and buffers");

SlDecoder* sl_decoder_create(const cba_sl_options& o, int W, int H, int max_sequences, int device) {
    auto h = std::make_unique<SlDecoder>(device);
    sl_fill_rule(o, &h->rule);
    h->W = W; h->H = H; h->max_sequences = max_sequences;
    h->n_images = sl_image_count(h->rule);
    const size_t px = static_cast<size_t>(max_sequences) * W * H;
    h->img.alloc(px * h->n_images + SL_IMG_PAD);
    h->status.alloc(px);
    h->coord.alloc(px * h->rule.n_axes);
    h->mod.alloc(px * h->rule.n_axes);
    return h.release();
}

int sl_decoder_max_sequences(const SlDecoder* h) { return h->max_sequences; }
bool sl_decoder_can_point(const SlDecoder* h) {
    return h->rig && h->rule.n_axes == 2 && h->cams.p && h->xyz.p && h->rms.p && h->tri_status.p;
}

void sl_decoder_set_rig(SlDecoder* h, int model, const double* intr, int n_inv, const double* inv, const double* c_T_r,
                        const cba_triangulate_options& o) {
    const hipStream_t s = h->begin();
    const int ni = cam_intr_size(model);
    TriCamera hc[2];
    for (int c = 0; c < 2; ++c)
        tri_fill_camera(model, intr + static_cast<size_t>(c) * ni, n_inv, inv ? inv + static_cast<size_t>(c) * n_inv : nullptr,
                        c_T_r + 7 * static_cast<size_t>(c), &hc[c]);
    const size_t px = static_cast<size_t>(h->max_sequences) * h->W * h->H;
    // each buffer on its own: one that could not be had in an earlier call (out of memory) is asked for again, and rig stays false
    // until all four are there
    h->cams.ensure(2);
    h->xyz.ensure(3 * px);
    h->rms.ensure(px);
    h->tri_status.ensure(px);
    h->cams.upload(hc, 2, s);
    CBA_HIP(hipStreamSynchronize(s));  // hc goes out of scope
    h->model = model;
    h->tri_opts = o;
    h->rig = true;
}

template <int NW>
static void sl_launch(const SlArgs& a, const SlRule& r, hipStream_t s) {
    const int64_t items = static_cast<int64_t>(a.n_seq) * a.H * a.groups;
    const dim3 grid(static_cast<unsigned>((items + SL_BLOCK - 1) / SL_BLOCK));
    if (NW == 4 || a.W % 2 == 0) {  // a multiple of 16 is even
        hipLaunchKernelGGL((k_sl_decode<NW, true>), grid, dim3(SL_BLOCK), 0, s, a, r);
    } else if constexpr (NW == 1) {
        hipLaunchKernelGGL((k_sl_decode<NW, false>), grid, dim3(SL_BLOCK), 0, s, a, r);
    }
}

// stage_ms [4] (experiment builds): upload, decode, points, download
void sl_decoder_process(SlDecoder* h, int n_seq, const uint8_t* images, double* coord, double* modulation, uint8_t* status, double* xyz,
                        double* rms_px, int32_t* tri_status, double* stage_ms) {
    const hipStream_t s = h->begin();
    const size_t px = static_cast<size_t>(n_seq) * h->W * h->H;
    StageTimer<5> tm(s, stage_ms != nullptr);
    tm.mark(0);
    h->img.upload(images, px * h->n_images, s);
    tm.mark(1);
    SlArgs a;
    a.img = h->img.p;
    a.W = h->W; a.H = h->H; a.n_seq = n_seq; a.n_images = h->n_images;
    a.coord = h->coord.p;
    a.mod = modulation ? h->mod.p : nullptr;
    a.status = h->status.p;
    if (a.W % 16 == 0) {  // every row of every image starts on a 16-byte boundary
        a.groups = a.W / 16;
        sl_launch<4>(a, h->rule, s);
    } else {
        a.groups = (a.W + 3) / 4;
        sl_launch<1>(a, h->rule, s);
    }
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    const bool points = xyz || rms_px || tri_status;
    if (points) {
        const int64_t n = static_cast<int64_t>(px);
        const dim3 grid(launch_grid(n, SL_BLOCK, SL_GRID));
        if (h->model == CAM_SCHEIMPFLUG)
            hipLaunchKernelGGL((k_sl_points<CAM_SCHEIMPFLUG>), grid, dim3(SL_BLOCK), 0, s, n, h->W, h->H, h->coord.p, h->cams.p, h->tri_opts,
                               h->xyz.p, h->rms.p, h->tri_status.p);
        else
            hipLaunchKernelGGL((k_sl_points<CAM_PINHOLE_BC>), grid, dim3(SL_BLOCK), 0, s, n, h->W, h->H, h->coord.p, h->cams.p, h->tri_opts,
                               h->xyz.p, h->rms.p, h->tri_status.p);
        CBA_HIP(hipGetLastError());
    }
    tm.mark(3);
    if (coord) h->coord.download(coord, px * h->rule.n_axes, s);
    if (modulation) h->mod.download(modulation, px * h->rule.n_axes, s);
    if (status) h->status.download(status, px, s);
    if (xyz) h->xyz.download(xyz, 3 * px, s);
    if (rms_px) h->rms.download(rms_px, px, s);
    if (tri_status) h->tri_status.download(tri_status, px, s);
    tm.mark(4);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(stage_ms);
}

void sl_decoder_destroy(SlDecoder* h) noexcept { destroy_handle(h); }

}  // namespace cba
