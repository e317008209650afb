// image_tile.hpp — the device pieces the image detectors share (corner_detect.hip, blob_detect.hip): which tile a workgroup owns, the
// staging of a tile and its halo as bytes in LDS, the store of a lane's four adjacent pixels and the frame of a refine slot.  The
// response arithmetic between staging and store, and the bodies of the refine kernels, stay in the .hip files.  hipcc only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace cba {

// The tile of workgroup blockIdx.x = (im tiles_y + ty) tiles_x + tx: its first pixel (x0, y0), its image and that image's first
// element in an [n_images][H][W] array.
struct TileAt {
    int x0, y0, im;
    int64_t fbase;
};
template <int TX, int TY>
__device__ __forceinline__ TileAt tile_decode(int tiles_x, int tiles_y, int W, int H) {
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, im = b / tiles_y;
    return {tx * TX, ty * TY, im, static_cast<int64_t>(im) * W * H};
}

// Stages rows y0 - HALO .. y0 + TY - 1 + HALO of one image (img + fbase) into tile [TY + 2 HALO][PITCH] bytes, LDS column LEFT being
// image column x0; zeros outside the image.  Every read lies inside the image, so inside [0, n_images W H).  The caller synchronises.
//   WIDE (W % 16 == 0, so every row starts on a 16-byte boundary): 16-byte loads of the PITCH / 16 aligned vectors of a row.
//   otherwise: single bytes of the LDS columns C0 .. C0 + COLS - 1 (the columns the caller reads; the rest stay unwritten).
template <int TX, int TY, int HALO, int LEFT, int PITCH, int BLOCK, bool WIDE, int C0 = 0, int COLS = PITCH>
__device__ __forceinline__ void stage_tile(uint8_t* tile, const uint8_t* img, int64_t fbase, int x0, int y0, int W, int H, int tid) {
    constexpr int ROWS = TY + 2 * HALO;
    static_assert(TX % 16 == 0 && LEFT % 16 == 0 && PITCH % 16 == 0 && PITCH >= LEFT + TX, "x0 - LEFT + 16 v is a multiple of 16");
    static_assert(C0 >= 0 && COLS >= 1 && C0 + COLS <= PITCH, "the byte window lies in the pitch");
    if constexpr (WIDE) {
        constexpr int VPR = PITCH / 16;
        for (int i = tid; i < ROWS * VPR; i += BLOCK) {
            const int row = i / VPR, v = i - row * VPR;
            const int y = y0 - HALO + row, x = x0 - LEFT + 16 * v;  // x and W are multiples of 16: all in or all out
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (y >= 0 && y < H && x >= 0 && x < W) q = *reinterpret_cast<const uint4*>(img + fbase + static_cast<int64_t>(y) * W + x);
            *reinterpret_cast<uint4*>(tile + row * PITCH + 16 * v) = q;
        }
    } else {
        for (int i = tid; i < ROWS * COLS; i += BLOCK) {
            const int row = i / COLS, c = i - row * COLS;
            const int y = y0 - HALO + row, x = x0 - LEFT + C0 + c;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            tile[row * PITCH + C0 + c] = in ? img[fbase + static_cast<int64_t>(y) * W + x] : uint8_t(0);
        }
    }
}

// A lane's four adjacent pixels v[0] .. v[3] of a row of one array, dst pointing at the first (T: int16, uint16 or int32).
template <typename T, typename V>
struct Px4 {
    T* dst;
    V v[4];
    static_assert(sizeof(T) == 2 || sizeof(T) == 4, "int16, uint16 or int32");
    // one vector store: 16 bytes for 32-bit T, 8 for 16-bit T (signed values cut to their low halves; unsigned ones are below 2^16)
    __device__ __forceinline__ void vec() const {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<int4*>(dst) = make_int4(v[0], v[1], v[2], v[3]);
        } else {
            constexpr uint32_t lo = std::is_signed_v<V> ? 0xffffu : 0xffffffffu;
            uint2 q;
            q.x = (static_cast<uint32_t>(v[0]) & lo) | static_cast<uint32_t>(v[1]) << 16;
            q.y = (static_cast<uint32_t>(v[2]) & lo) | static_cast<uint32_t>(v[3]) << 16;
            *reinterpret_cast<uint2*>(dst) = q;
        }
    }
    __device__ __forceinline__ void put(int k) const { dst[k] = static_cast<T>(v[k]); }
};
// Stores the lane's pixels of columns x .. x + 3 (x < W, x a multiple of 4) of every array given.  W % 4 == 0: x + 3 < W and every dst
// is a multiple of 4 sizeof(T) bytes, so one vector store each; otherwise scalar stores, guarded.  A kernel with two outputs passes
// both, so that it branches once.
template <typename... P>
__device__ __forceinline__ void store4(int x, int W, const P&... p) {
    if ((W & 3) == 0) {
        (p.vec(), ...);
    } else {
        (p.put(0), ...);
        if (x + 1 < W) (p.put(1), ...);
        if (x + 2 < W) (p.put(2), ...);
        if (x + 3 < W) (p.put(3), ...);
    }
}

// Slot i = im max_items + slot of a refine kernel: kept when slot < min(count[im], max_items); then p = peak_px[i] = py W + px and
// fbase is the image's first element.  A slot that is not kept reads no peak.
struct SlotAt {
    int im, p, px, py;
    int64_t fbase;
    bool kept;
};
__device__ __forceinline__ SlotAt slot_at(int i, int max_items, const int32_t* count, const int32_t* peak_px, int W, int H) {
    SlotAt s{};
    s.im = i / max_items;
    s.kept = i - s.im * max_items < min(count[s.im], max_items);
    if (s.kept) {
        s.p = peak_px[i];
        s.py = s.p / W;
        s.px = s.p - s.py * W;
        s.fbase = static_cast<int64_t>(s.im) * W * H;
    }
    return s;
}

}  // namespace cba
