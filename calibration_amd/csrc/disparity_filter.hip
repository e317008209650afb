// disparity_filter.hip — the median and speckle filters of a batch of disparity maps on the GPU (disparity_filter_math.hpp, calibba.h:
// cba_disparity_filter).  One device-side object, DispFilter (pipelines.hpp), serves the stand-alone handle of this file and the
// matchers of stereo_match.hip and stereo_sgm.hip; disp_filter_run is the only copy of the launch sequence, queued on the caller's
// stream.  A tile is DF_TW x DF_TH pixels of one image, one workgroup, one lane per pixel:
//   k_df_median<M>  stages the tile and its M-pixel halo in LDS through df_read (NaN outside the image), a lane selects the lower
//                   median of its window in registers (df_median, rank counting) and writes `med`; counts the valid pixels.
//   k_df_local      union-find of the tile in LDS (df_tile_link: left and upper neighbour), then every pixel's label = the batch-wide
//                   linear index of its tile-local root, -1 for an invalid pixel; zeroes the pixel's size.
//   k_df_merge      one lane per pixel on the left or upper edge of a tile: df_border_link on the labels in global memory.
//   k_df_flatten    label[i] = df_find(i): afterwards every label is the lowest linear index of its component.
//   k_df_sizes      size[label[i]] += 1; the lanes of a wavefront that share a root add once, a root that leads group after group once
//                   per wavefront.
//   k_df_apply      out = NaN where size[label] <= S, else med; counts the removed pixels and (at i == label[i]) components.
// With speckle_max_size == 0 the four middle kernels are not launched and k_df_apply copies med.  Kernel boundaries are the only
// grid-wide synchronisation: no workgroup waits for another one, and every loop ends by the argument written next to it.
// Atomics: atomicMin on labels and integer atomicAdd on counts, nothing else and no float atomic.  A minimum and an integer sum do not
// depend on the order their operands arrive in, and the labels after k_df_flatten are a function of the component alone (its lowest
// index), so the output is the same to the bit for every schedule.  Every index is checked against the image before it is used;
// n W H <= 2^31 - 1 (checked at create), so a linear index fits an int32 label; the index arithmetic itself is 64-bit.
#include <algorithm>
#include <memory>
#include <type_traits>

#include "pipelines.hpp"
#include "disparity_filter_math.hpp"

namespace cba {

static_assert(DF_TILE == 256 && DF_TW == 32, "one lane per pixel of a tile, a tile row is half a wavefront");
constexpr int64_t DF_GRID = 1 << 22;  // workgroups of a tile or chunk launch at most: DF_GRID * DF_TILE lanes stay below 2^32

struct DfLdsOps {  // labels of a tile in LDS
    int* L;
    __device__ int load(int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ int min(int i, int v) { return atomicMin(L + i, v); }
};
struct DfGlobalOps {  // labels of the batch in global memory
    int* L;
    __device__ int load(int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ int min(int i, int v) { return atomicMin(L + i, v); }
};

struct DfTile {
    int img, x0, y0;
};
// tile b of the n * tiles_y * tiles_x tiles of a batch
__device__ __forceinline__ DfTile df_tile_of(int64_t b, int tiles_x, int tiles_y) {
    DfTile t;
    const int64_t q = b / tiles_x;
    t.x0 = static_cast<int>(b - q * tiles_x) * DF_TW;
    t.img = static_cast<int>(q / tiles_y);
    t.y0 = static_cast<int>(q - static_cast<int64_t>(t.img) * tiles_y) * DF_TH;
    return t;
}

// Counts per image.  Atomic adds to one address take their turns, so a workgroup of the median and apply kernels owns a contiguous run
// of tiles or chunks, which lie in one image or in few, sums the flags of a run's image in LDS (one ballot and one LDS add per
// wavefront) and adds to the image's count in global memory once per image of its run.
__device__ __forceinline__ void df_count(bool flag, int* lds_counter) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(lds_counter, __popcll(m));
}
__device__ __forceinline__ void df_flush(int* lds_counter, int64_t* dst) {  // one lane
    if (*lds_counter) atomicAdd(reinterpret_cast<unsigned long long*>(dst), static_cast<unsigned long long>(*lds_counter));
    *lds_counter = 0;
}

// Workgroup b takes the tiles [b per, (b + 1) per) of the batch; the loop is counted, and every lane of a workgroup runs the same
// number of passes, so its barriers are uniform.
template <int M>
__global__ __launch_bounds__(DF_TILE) void k_df_median(const float* __restrict__ in, float* __restrict__ med, int W, int H, int tiles_x,
                                                       int tiles_y, int64_t n_tiles, int per, int64_t* __restrict__ stats) {
    constexpr int PW = DF_TW + 2 * M, PH = DF_TH + 2 * M;
    __shared__ float tile[PW * PH];
    __shared__ int n_valid;
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * per, b1 = b0 + per < n_tiles ? b0 + per : n_tiles;
    int cur = -1;  // the image n_valid counts
    if (tid == 0) n_valid = 0;
    for (int64_t b = b0; b < b1; ++b) {
        const DfTile t = df_tile_of(b, tiles_x, tiles_y);
        const int64_t base = static_cast<int64_t>(t.img) * W * H;
        __syncthreads();  // the previous pass has read its tile and added its count
        if (t.img != cur) {
            if (tid == 0 && cur >= 0) df_flush(&n_valid, stats + 3 * cur);
            cur = t.img;
        }
        for (int i = tid; i < PW * PH; i += DF_TILE) {
            const int r = i / PW, c = i - r * PW;
            const int y = t.y0 - M + r, x = t.x0 - M + c;
            const bool in_image = y >= 0 && y < H && x >= 0 && x < W;
            tile[i] = in_image ? df_read(in[base + static_cast<int64_t>(y) * W + x]) : df_nan();
        }
        __syncthreads();
        const int lx = tid % DF_TW, ly = tid / DF_TW, x = t.x0 + lx, y = t.y0 + ly;
        const float* centre = tile + (ly + M) * PW + lx + M;
        const float out = df_median<M>([&](int i, int j) { return centre[j * PW + i]; });
        const bool inside = x < W && y < H;
        if (inside) med[base + static_cast<int64_t>(y) * W + x] = out;
        df_count(inside && *centre == *centre, &n_valid);
    }
    __syncthreads();
    if (tid == 0 && cur >= 0) df_flush(&n_valid, stats + 3 * cur);
}

// the tiles grid-stride (DF_GRID caps the grid: degenerate shapes such as W = 1 have far more tile lanes than pixels); a counted loop
// with uniform barriers
__global__ __launch_bounds__(DF_TILE) void k_df_local(const float* __restrict__ med, int32_t* __restrict__ label, int32_t* __restrict__ size,
                                                      int W, int H, int tiles_x, int tiles_y, int64_t n_tiles, double diff) {
    __shared__ float val[DF_TILE];
    __shared__ int lab[DF_TILE];
    const int tid = static_cast<int>(threadIdx.x);
    for (int64_t b = blockIdx.x; b < n_tiles; b += gridDim.x) {
        const DfTile t = df_tile_of(b, tiles_x, tiles_y);
        const int64_t base = static_cast<int64_t>(t.img) * W * H;
        const int lx = tid % DF_TW, ly = tid / DF_TW, x = t.x0 + lx, y = t.y0 + ly;
        const bool inside = x < W && y < H;
        const int64_t i = base + static_cast<int64_t>(y) * W + x;
        const float v = inside ? med[i] : df_nan();
        __syncthreads();  // the previous pass has read its labels
        val[tid] = v;
        lab[tid] = tid;
        __syncthreads();
        DfLdsOps ops = {lab};
        if (v == v) df_tile_link(ops, val, lx, ly, diff);
        __syncthreads();
        if (inside) {
            int32_t l = -1;
            if (v == v) {
                const int r = df_find(ops, tid);  // the lowest local index of the component's part in this tile: also its lowest linear index
                l = static_cast<int32_t>(base + static_cast<int64_t>(t.y0 + r / DF_TW) * W + t.x0 + r % DF_TW);
            }
            label[i] = l;
            size[i] = 0;
        }
    }
}

// one lane per pixel of the batch; a lane off the tile edges has nothing to do
__global__ __launch_bounds__(DF_TILE) void k_df_merge(const float* __restrict__ med, int32_t* __restrict__ label, int64_t n_px, int W, int H,
                                                      double diff) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(DF_TILE) + threadIdx.x;
    if (i >= n_px) return;
    const int64_t row = i / W;
    const int x = static_cast<int>(i - row * W), y = static_cast<int>(row % H);
    if (x % DF_TW != 0 && y % DF_TH != 0) return;
    DfGlobalOps ops = {label};
    df_border_link(ops, med, i - (static_cast<int64_t>(y) * W + x), W, x, y, diff);
}

__global__ __launch_bounds__(DF_TILE) void k_df_flatten(int32_t* __restrict__ label, int64_t n_px) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(DF_TILE) + threadIdx.x;
    if (i >= n_px) return;
    DfGlobalOps ops = {label};
    const int l = ops.load(static_cast<int>(i));
    if (l < 0 || l == i) return;
    // no union runs in this launch, so the roots are fixed; a label another lane rewrites meanwhile moves from one ancestor to the root
    __hip_atomic_store(label + i, df_find(ops, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A wavefront walks DF_SEG consecutive groups of 64 pixels.  The lanes of a group that share a root add their count once, and the root
// of a group's first valid lane is carried to the next group: a large component, which fills most groups of its rows, costs one add
// per wavefront instead of one per group (adds to one address take their turns).
constexpr int DF_SEG = 16;
__global__ __launch_bounds__(DF_TILE) void k_df_sizes(const int32_t* __restrict__ label, int32_t* __restrict__ size, int64_t n_px) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t wave = blockIdx.x * static_cast<int64_t>(DF_TILE / 64) + (threadIdx.x >> 6);
    int carry = -1, carried = 0;  // wave-uniform: a root and the pixels counted for it so far
    for (int k = 0; k < DF_SEG; ++k) {
        const int64_t i = (wave * DF_SEG + k) * 64 + lane;
        const int r = i < n_px ? label[i] : -1;
        const unsigned long long valid = __ballot(r >= 0);
        if (!valid) continue;  // wave-uniform
        const int lead = __shfl(r, __ffsll(static_cast<long long>(valid)) - 1);
        const int n_lead = __popcll(__ballot(r == lead));
        if (lead != carry) {
            if (lane == 0 && carry >= 0) atomicAdd(size + carry, carried);
            carry = lead;
            carried = 0;
        }
        carried += n_lead;
        bool todo = r >= 0 && r != lead;
        // Termination: every pass retires the first lane still in the loop and all lanes with its root, so there are at most 64 passes.
        while (todo) {
            const int first = __builtin_amdgcn_readfirstlane(r);
            const bool mine = r == first;
            const unsigned long long m = __ballot(mine);
            if (mine) {
                if (lane == __ffsll(static_cast<long long>(m)) - 1) atomicAdd(size + first, __popcll(m));
                todo = false;
            }
        }
    }
    if (lane == 0 && carry >= 0) atomicAdd(size + carry, carried);
}

// Workgroup b takes the chunks [b per, (b + 1) per) of the n * chunks chunks of DF_TILE pixels (chunks = ceil(frame / DF_TILE)); a chunk
// stays inside one image, whose counts it adds to (df_count above).  label == nullptr: no speckle step.
__global__ __launch_bounds__(DF_TILE) void k_df_apply(const float* __restrict__ med, const int32_t* __restrict__ label,
                                                      const int32_t* __restrict__ size, float* __restrict__ out, int max_size, int64_t frame,
                                                      int64_t chunks, int64_t n_chunks, int per, int64_t* __restrict__ stats) {
    __shared__ int n_comp, n_pix;
    const int64_t c0 = static_cast<int64_t>(blockIdx.x) * per, c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
    int64_t cur = -1;  // the image n_comp and n_pix count
    if (threadIdx.x == 0) { n_comp = 0; n_pix = 0; }
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t img = c / chunks, j = (c - img * chunks) * DF_TILE + threadIdx.x, i = img * frame + j;
        bool removed = false, root = false;
        if (j < frame) {
            float v = med[i];
            if (label) {
                const int r = label[i];
                if (r >= 0 && size[r] <= max_size) {
                    v = df_nan();
                    removed = true;
                    root = r == i;
                }
            }
            out[i] = v;
        }
        if (!label) continue;  // uniform over the grid
        __syncthreads();       // the previous pass has added its counts; the first: the counts are zeroed
        if (img != cur) {
            if (threadIdx.x == 0 && cur >= 0) {
                df_flush(&n_comp, stats + 3 * cur + 1);
                df_flush(&n_pix, stats + 3 * cur + 2);
            }
            cur = img;
            __syncthreads();
        }
        df_count(root, &n_comp);
        df_count(removed, &n_pix);
    }
    __syncthreads();
    if (threadIdx.x == 0 && cur >= 0) {
        df_flush(&n_comp, stats + 3 * cur + 1);
        df_flush(&n_pix, stats + 3 * cur + 2);
    }
}

// ---- host glue ---------------------------------------------------------------------------------------------------------------------
// tiles or chunks of a workgroup's run: 1 up to DF_RUN_GRID of them, then as many as keep the grid at DF_RUN_GRID workgroups (the counts
// then cost DF_RUN_GRID adds per image at most); never a grid above DF_GRID
constexpr int64_t DF_RUN_GRID = 4096;
static int df_run(int64_t items) {
    const int64_t per = std::max<int64_t>((items + DF_RUN_GRID - 1) / DF_RUN_GRID, 1);
    return static_cast<int>(std::min<int64_t>(per, 0x7fffffff));
}

void disp_filter_init(DispFilter& f, int W, int H, int max_images, const cba_disparity_filter_options& o) {
    f.opts = o;
    f.W = W; f.H = H; f.max_images = max_images;
    const size_t px = static_cast<size_t>(max_images) * W * H;
    f.med.alloc(px);
    if (o.speckle_max_size > 0) {
        f.label.alloc(px);
        f.size.alloc(px);
    }
    f.stats.alloc(3 * static_cast<size_t>(max_images));
}

// stage_ms [DISP_FILTER_STAGES] (experiment builds): median, local labels, merge, flatten, sizes, apply; the stream is then synchronised
// here.  in == out is allowed: the first kernel reads `in` into f.med and only the last one writes `out`.
void disp_filter_run(DispFilter& f, hipStream_t s, int n, const float* in, float* out, double* stage_ms) {
    const int W = f.W, H = f.H, S = f.opts.speckle_max_size;
    const int64_t frame = static_cast<int64_t>(W) * H, n_px = frame * n;
    const int tiles_x = (W + DF_TW - 1) / DF_TW, tiles_y = (H + DF_TH - 1) / DF_TH;
    const int64_t n_tiles = static_cast<int64_t>(n) * tiles_y * tiles_x;
    const dim3 block(DF_TILE), tiles(static_cast<unsigned>(std::min<int64_t>(n_tiles, DF_GRID)));
    const int per_tiles = df_run(n_tiles);
    const dim3 tile_runs(static_cast<unsigned>((n_tiles + per_tiles - 1) / per_tiles));
    const dim3 flat(static_cast<unsigned>((n_px + DF_TILE - 1) / DF_TILE));
    StageTimer<DISP_FILTER_STAGES + 1> tm(s, stage_ms != nullptr);
    CBA_HIP(hipMemsetAsync(f.stats.p, 0, 3 * static_cast<size_t>(n) * sizeof(int64_t), s));
    tm.mark(0);
    switch (f.opts.median_half) {
    case 0: hipLaunchKernelGGL(k_df_median<0>, tile_runs, block, 0, s, in, f.med.p, W, H, tiles_x, tiles_y, n_tiles, per_tiles, f.stats.p); break;
    case 1: hipLaunchKernelGGL(k_df_median<1>, tile_runs, block, 0, s, in, f.med.p, W, H, tiles_x, tiles_y, n_tiles, per_tiles, f.stats.p); break;
    default: hipLaunchKernelGGL(k_df_median<2>, tile_runs, block, 0, s, in, f.med.p, W, H, tiles_x, tiles_y, n_tiles, per_tiles, f.stats.p); break;
    }
    CBA_HIP(hipGetLastError());
    tm.mark(1);
    if (S > 0) {
        const double diff = f.opts.speckle_max_diff;
        hipLaunchKernelGGL(k_df_local, tiles, block, 0, s, f.med.p, f.label.p, f.size.p, W, H, tiles_x, tiles_y, n_tiles, diff);
        CBA_HIP(hipGetLastError());
        tm.mark(2);
        hipLaunchKernelGGL(k_df_merge, flat, block, 0, s, f.med.p, f.label.p, n_px, W, H, diff);
        CBA_HIP(hipGetLastError());
        tm.mark(3);
        hipLaunchKernelGGL(k_df_flatten, flat, block, 0, s, f.label.p, n_px);
        CBA_HIP(hipGetLastError());
        tm.mark(4);
        hipLaunchKernelGGL(k_df_sizes, dim3(static_cast<unsigned>((n_px + DF_TILE * DF_SEG - 1) / (DF_TILE * DF_SEG))), block, 0, s, f.label.p,
                           f.size.p, n_px);
        CBA_HIP(hipGetLastError());
    } else {
        for (int k = 2; k <= 4; ++k) tm.mark(k);
    }
    tm.mark(5);
    const int64_t chunks = (frame + DF_TILE - 1) / DF_TILE, n_chunks = chunks * n;
    const int per_chunks = df_run(n_chunks);
    hipLaunchKernelGGL(k_df_apply, dim3(static_cast<unsigned>((n_chunks + per_chunks - 1) / per_chunks)), block, 0, s, f.med.p,
                       S > 0 ? f.label.p : nullptr, S > 0 ? f.size.p : nullptr, out, S, frame, chunks, n_chunks, per_chunks, f.stats.p);
    CBA_HIP(hipGetLastError());
    tm.mark(6);
    if (stage_ms) {
        CBA_HIP(hipStreamSynchronize(s));
        tm.report(stage_ms);
    }
}

// The stand-alone handle: the filter and one buffer the maps are uploaded into, filtered in and downloaded from.
struct DisparityFilter : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    DispFilter f;
    DevBuf<float> io;
};
static_assert(!std::is_copy_constructible_v<DisparityFilter> && !std::is_copy_assignable_v<DisparityFilter>, "a handle owns its stream and buffers");

DisparityFilter* disparity_filter_create(int W, int H, int max_images, const cba_disparity_filter_options& o, int device) {
    auto h = std::make_unique<DisparityFilter>(device);
    disp_filter_init(h->f, W, H, max_images, o);
    h->io.alloc(static_cast<size_t>(max_images) * W * H);
    return h.release();
}

int disparity_filter_max_images(const DisparityFilter* h) { return h->f.max_images; }

void disparity_filter_process(DisparityFilter* h, int n, const float* in, float* out, int64_t* stats, double* stage_ms) {
    const hipStream_t s = h->begin();
    const size_t px = static_cast<size_t>(n) * h->f.W * h->f.H;
    h->io.upload(in, px, s);
    disp_filter_run(h->f, s, n, h->io.p, h->io.p, stage_ms);
    h->io.download(out, px, s);
    if (stats) h->f.stats.download(stats, 3 * static_cast<size_t>(n), s);
    CBA_HIP(hipStreamSynchronize(s));
}

void disparity_filter_destroy(DisparityFilter* h) noexcept { destroy_handle(h); }

}  // namespace cba
