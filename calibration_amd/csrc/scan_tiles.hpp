// scan_tiles.hpp — the tiled exclusive scan of int32 counts on the device, shared by cloud_register.hip (cell counts -> cell starts) and
// tsdf_fusion.hip (edge counts per tile -> the first place of each tile).  Tiles of SCAN_TILE = 1024 entries (256 lanes, 4 entries
// each, the lanes' sums scanned in LDS); the tile sums are scanned by the same kernels, level after level.  Integers: any order of
// addition gives the same result.  The kernels are static: each translation unit that includes this gets its own copy.
// For kernels that count per tile and then place: scan_counts (host) and wave_counts_prefix (a wave among its workgroup's).
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

// count [n], which a kernel queued on s fills -> its exclusive scan in place and the total: entry n is zeroed and scanned with the
// counts, so it receives the total.  tmp: scan_tmp_size(n + 1) entries; total_h: one pinned entry.  Ends with s synchronised.
[[maybe_unused]] static int64_t scan_counts(hipStream_t s, int32_t* count, int64_t n, int32_t* tmp, int32_t* total_h) {
    CBA_HIP(hipMemsetAsync(count + n, 0, sizeof(int32_t), s));
    scan_exclusive(s, count, n + 1, tmp);
    CBA_HIP(hipGetLastError());
    CBA_HIP(hipMemcpyAsync(total_h, count + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CBA_HIP(hipStreamSynchronize(s));
    return total_h[0];
}

// total: the wave's count, taken from lane 0 and exchanged through four entries of LDS.  -> the count of the workgroup (SCAN_BLOCK
// lanes); *before <- that of the waves before this one.  Two barriers: every lane of the workgroup must reach the call.
__device__ __forceinline__ int32_t wave_counts_prefix(int32_t total, int lane, int wave, int32_t* before) {
    __shared__ int32_t wave_total[SCAN_BLOCK / 64];
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    int32_t all = 0, b = 0;
#pragma unroll
    for (int w = 0; w < SCAN_BLOCK / 64; ++w) {
        const int32_t t = wave_total[w];
        b += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();  // the next call writes wave_total again
    *before = b;
    return all;
}

}  // namespace cba
