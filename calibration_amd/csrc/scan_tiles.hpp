// scan_tiles.hpp — the tiled exclusive scan of int32 counts on the device, shared by cloud_register.hip (cell counts -> cell starts) and
// tsdf_fusion.hip (edge counts per tile -> the first place of each tile).  Tiles of SCAN_TILE = 1024 entries (256 lanes, 4 entries
// each, the lanes' sums scanned in LDS); the tile sums are scanned by the same kernels, level after level.  Integers: any order of
// addition gives the same result.  The kernels are static: each translation unit that includes this gets its own copy.
#pragma once
#include "hip_glue.hpp"

namespace cba {

constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_TILE = 1024;  // entries per workgroup of the scan

// v [n] -> its exclusive scan inside each tile of SCAN_TILE entries; sums [tiles]: each tile's total.  One workgroup per tile.
static __global__ __launch_bounds__(SCAN_BLOCK) void k_scan_tiles(int64_t n, int32_t* __restrict__ v, int32_t* __restrict__ sums) {
    __shared__ int32_t part[SCAN_BLOCK];
    const int t = threadIdx.x;
    const int64_t at = static_cast<int64_t>(blockIdx.x) * SCAN_TILE + 4 * t;
    int32_t a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = at + k < n ? v[at + k] : 0;
    const int32_t mine = (a[0] + a[1]) + (a[2] + a[3]);
    part[t] = mine;
    __syncthreads();
    // inclusive scan of the 256 lane sums (integers: any order gives the same)
    for (int d = 1; d < SCAN_BLOCK; d <<= 1) {
        const int32_t add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int32_t run = part[t] - mine;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (at + k < n) v[at + k] = run;
        run += a[k];
    }
    if (t == SCAN_BLOCK - 1) sums[blockIdx.x] = part[t];
}

// v [n] += the scanned total of the tiles before its own
static __global__ __launch_bounds__(SCAN_BLOCK) void k_scan_add(int64_t n, int32_t* __restrict__ v, const int32_t* __restrict__ sums) {
    const int64_t at = static_cast<int64_t>(blockIdx.x) * SCAN_TILE + 4 * threadIdx.x;
    const int32_t add = sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (at + k < n) v[at + k] += add;
}

// the int32 entries scan_exclusive needs in tmp for n entries: the tile sums of every level, and one
__attribute__((visibility("hidden"))) inline size_t scan_tmp_size(int64_t n) {
    size_t tmp_n = 0;
    for (int64_t t = n; t > 1;) {
        t = (t + SCAN_TILE - 1) / SCAN_TILE;
        tmp_n += static_cast<size_t>(t);
    }
    return tmp_n + 1;
}

// exclusive scan of v [n] in place on s; tmp: scan_tmp_size(n) entries
static void scan_exclusive(hipStream_t s, int32_t* v, int64_t n, int32_t* tmp) {
    const int64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(k_scan_tiles, dim3(static_cast<unsigned>(tiles)), dim3(SCAN_BLOCK), 0, s, n, v, tmp);
    if (tiles > 1) {
        scan_exclusive(s, tmp, tiles, tmp + tiles);
        hipLaunchKernelGGL(k_scan_add, dim3(static_cast<unsigned>(tiles)), dim3(SCAN_BLOCK), 0, s, n, v, tmp);
    }
}

}  // namespace cba
