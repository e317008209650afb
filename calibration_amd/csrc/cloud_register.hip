// cloud_register.hip — scan registration on the GPU (cloud_math.hpp, calibba.h: cba_point_normals, cba_cloud_index, cba_cloud_nearest,
// cba_cloud_register).
//   k_point_normals     one lane per pixel: the centre and its four neighbours straight from global memory (a row is read by three
//                       rows of lanes, which the caches serve), cloud_normal.
//   k_cloud_count       one lane per target point: its cell into cell_of (-1: invalid), integer atomicAdd on the cell's count.
//   k_scan_tiles / k_scan_add   (scan_tiles.hpp) exclusive scan of the counts in tiles of CLOUD_SCAN_TILE = 1024 cells (256 lanes, 4 cells
//                       each, the lanes' sums scanned in LDS); the tile sums are scanned by the same kernels, up to three levels at the cap.
//   k_cloud_scatter     one lane per valid point: its place by integer atomicAdd on the cell's start, the 32-byte record and the
//                       normal into cell order.  The starts live at start + 1 while they are bumped: afterwards start[c + 1] is the
//                       end of cell c, which is the start of cell c + 1, and start[0] = 0 was never touched.
//   k_cloud_nearest     one lane per query, grid-stride: cloud_nearest_point.  No LDS.
//   k_icp_accumulate    ICP_BLOCKS workgroups per source, grid-striding its points: transform, search, rows, 29 sums in registers;
//                       wave_transpose_sum inside the wave, LDS across the four waves, one slab row per (source, block).
//   k_icp_step          one wavefront per source: lane e adds entry e of the source's slab rows in block order; lane 0 runs
//                       icp_advance (Cholesky, update, stop tests) and writes pose, phase and, when the source ends, the done count.
// The host queues max_iterations + 1 rounds of the two ICP kernels without reading values; every ICP_POLL rounds it reads the done
// count and stops when every source has ended.  A source that has ended is not touched again, so results do not depend on when the
// host looks.  No float atomics anywhere; integer atomics only for counts and places.
#include <memory>
#include <type_traits>

#include "pipelines.hpp"
#include "scan_tiles.hpp"
#include "wave_reduce.hpp"
#include "cloud_math.hpp"

namespace cba {

constexpr int CLOUD_BLOCK = 256;
constexpr int CLOUD_GRID = 8192;        // grid-stride cap
constexpr int CLOUD_SCAN_TILE = SCAN_TILE;  // cells per workgroup of the scan (scan_tiles.hpp)
constexpr int ICP_BLOCKS = 128;         // workgroups per source: fixed, so a source's sums do not depend on the call
constexpr int ICP_POLL = 4;             // rounds between two looks at the done count

// ---- normals ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CLOUD_BLOCK) void k_point_normals(int64_t n, int W, int H, const double* __restrict__ xyz, double vx, double vy,
                                                               double vz, double mj2, double* __restrict__ out) {
    const int64_t plane = static_cast<int64_t>(W) * H;
    const double vp[3] = {vx, vy, vz};
    for (int64_t i = blockIdx.x * static_cast<int64_t>(CLOUD_BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * CLOUD_BLOCK) {
        const int64_t px = i % plane;
        const int row = static_cast<int>(px / W), col = static_cast<int>(px - static_cast<int64_t>(row) * W);
        double P[3], R[3], L[3], D[3], U[3], nrm[3];
        const double* c = xyz + 3 * i;
        const bool r = col + 1 < W, l = col > 0, d = row + 1 < H, u = row > 0;
        const double* cr = r ? c + 3 : c;
        const double* cl = l ? c - 3 : c;
        const double* cd = d ? c + 3 * static_cast<int64_t>(W) : c;
        const double* cu = u ? c - 3 * static_cast<int64_t>(W) : c;
#pragma unroll
        for (int k = 0; k < 3; ++k) { P[k] = c[k]; R[k] = cr[k]; L[k] = cl[k]; D[k] = cd[k]; U[k] = cu[k]; }
        cloud_normal(P, R, L, D, U, (r ? 1 : 0) | (l ? 2 : 0) | (d ? 4 : 0) | (u ? 8 : 0), vp, mj2, nrm);
        out[3 * i] = nrm[0]; out[3 * i + 1] = nrm[1]; out[3 * i + 2] = nrm[2];
    }
}

void point_normals_gpu(int n_maps, int H, int W, const double* xyz, const double* viewpoint, double max_jump, double* normals, int device) {
    StreamLease s(device);
    const int64_t n = static_cast<int64_t>(n_maps) * H * W;
    DevBuf<double> in, out;
    in.assign(xyz, static_cast<size_t>(3 * n), s);
    out.alloc(static_cast<size_t>(3 * n));
    const double v[3] = {viewpoint ? viewpoint[0] : 0.0, viewpoint ? viewpoint[1] : 0.0, viewpoint ? viewpoint[2] : 0.0};
    hipLaunchKernelGGL(k_point_normals, dim3(launch_grid(n, CLOUD_BLOCK, CLOUD_GRID)), dim3(CLOUD_BLOCK), 0, s, n, W, H, in.p, v[0], v[1], v[2],
                       max_jump * max_jump, out.p);
    CBA_HIP(hipGetLastError());
    out.download(normals, static_cast<size_t>(3 * n), s);
    CBA_HIP(hipStreamSynchronize(s));
}

// ---- the index ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_count(int64_t n, const double* __restrict__ xyz, CloudGrid g, int32_t* __restrict__ cell_of,
                                                             int32_t* __restrict__ count) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(CLOUD_BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * CLOUD_BLOCK) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        int32_t c = -1;
        if (cloud_valid(x, y, z)) {
            c = cloud_point_cell(g, x, y, z);
            atomicAdd(&count[c], 1);
        }
        cell_of[i] = c;
    }
}

__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_scatter(int64_t n, const double* __restrict__ xyz, const double* __restrict__ normals,
                                                               const int32_t* __restrict__ cell_of, int32_t* __restrict__ bump,
                                                               CloudRec* __restrict__ rec, double* __restrict__ rec_normal) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(CLOUD_BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * CLOUD_BLOCK) {
        const int32_t c = cell_of[i];
        if (c < 0) continue;
        const int32_t at = atomicAdd(&bump[c], 1);
        CloudRec r;
        r.x = xyz[3 * i]; r.y = xyz[3 * i + 1]; r.z = xyz[3 * i + 2]; r.idx = i;
        rec[at] = r;
        if (normals) {
            rec_normal[3 * static_cast<int64_t>(at)] = normals[3 * i];
            rec_normal[3 * static_cast<int64_t>(at) + 1] = normals[3 * i + 1];
            rec_normal[3 * static_cast<int64_t>(at) + 2] = normals[3 * i + 2];
        }
    }
}

__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_nearest(int64_t m, const double* __restrict__ query, CloudGrid g,
                                                               const int32_t* __restrict__ start, const CloudRec* __restrict__ rec, double md,
                                                               int64_t* __restrict__ index, double* __restrict__ dist2) {
    const double md2 = md * md;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(CLOUD_BLOCK) + threadIdx.x; i < m; i += static_cast<int64_t>(gridDim.x) * CLOUD_BLOCK) {
        int32_t pos;
        double d2;
        index[i] = cloud_nearest_point(g, start, rec, query[3 * i], query[3 * i + 1], query[3 * i + 2], md, md2, &pos, &d2);
        dist2[i] = d2;
    }
}

// ---- ICP --------------------------------------------------------------------------------------------------------------------------
struct IcpArgs {
    CloudGrid g;
    const int32_t* start;
    const CloudRec* rec;
    const double* rec_normal;
    const int64_t* offset;   // [n_sources + 1]
    const double* src;       // [m][3]
    cba_icp_result* res;     // [n_sources]: pose7, iterations and status live here between the rounds
    int32_t* phase;          // [n_sources]
    double* slab;            // [n_sources][ICP_BLOCKS][ICP_ROW]
    int32_t* n_done;
    cba_icp_options o;
    double extent;
};

template <int METRIC>
__global__ __launch_bounds__(CLOUD_BLOCK) void k_icp_accumulate(IcpArgs a) {
    __shared__ double part[CLOUD_BLOCK / 64][ICP_ROW];
    const int s = blockIdx.x / ICP_BLOCKS, blk = blockIdx.x - s * ICP_BLOCKS;
    if (a.phase[s] == ICP_DONE) return;  // the whole workgroup
    const int64_t first = a.offset[s], m = a.offset[s + 1] - first;
    double R[9], t[3];
    {
        const double* pose = a.res[s].pose7;
        const double q[4] = {pose[0], pose[1], pose[2], pose[3]};
        icp_rotation(q, R);
        t[0] = pose[4]; t[1] = pose[5]; t[2] = pose[6];
    }
    const double md = a.o.max_distance, md2 = md * md;
    double acc[ICP_ROW];
#pragma unroll
    for (int e = 0; e < ICP_ROW; ++e) acc[e] = 0.0;
#pragma unroll 1
    for (int64_t i = static_cast<int64_t>(blk) * CLOUD_BLOCK + threadIdx.x; i < m; i += static_cast<int64_t>(ICP_BLOCKS) * CLOUD_BLOCK) {
        const double* pp = a.src + 3 * (first + i);
        const double p[3] = {pp[0], pp[1], pp[2]};
        if (!cloud_valid(p[0], p[1], p[2])) continue;
        double Q[3], d2;
        int32_t pos;
        icp_transform(R, t, p, Q);
        if (cloud_nearest_point(a.g, a.start, a.rec, Q[0], Q[1], Q[2], md, md2, &pos, &d2) < 0) continue;
        const CloudRec r = a.rec[pos];
        const double y[3] = {r.x, r.y, r.z};
        if (METRIC == 0) {
            const double* np = a.rec_normal + 3 * static_cast<int64_t>(pos);
            const double n[3] = {np[0], np[1], np[2]};
            if (n[0] != n[0]) continue;  // no normal: all three are NaN
            icp_add_plane(Q, y, n, acc);
        } else {
            icp_add_point(Q, y, acc);
        }
    }
    // every lane of every wave is here: the grid-stride loop has no early exit
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool owner;
    const int base = wave_transpose_sum<ICP_ROW>(acc, lane, &owner);
    static_assert(TransposeSum<ICP_ROW>::CNT == 1, "one finished sum per owning lane");
    if (owner) part[wave][base] = acc[0];
    __syncthreads();
    if (threadIdx.x < ICP_ROW) {
        double v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CLOUD_BLOCK / 64; ++w) v += part[w][threadIdx.x];
        a.slab[(static_cast<int64_t>(s) * ICP_BLOCKS + blk) * ICP_ROW + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void k_icp_step(IcpArgs a) {
    __shared__ double sums[ICP_ROW];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (a.phase[s] == ICP_DONE) return;
    if (lane < ICP_ROW) {
        const double* row = a.slab + static_cast<int64_t>(s) * ICP_BLOCKS * ICP_ROW + lane;
        double v = row[0];
#pragma unroll 1
        for (int b = 1; b < ICP_BLOCKS; ++b) v += row[static_cast<int64_t>(b) * ICP_ROW];
        sums[lane] = v;
    }
    __syncthreads();
    if (lane == 0) {
        double acc[ICP_SUMS];
        for (int e = 0; e < ICP_SUMS; ++e) acc[e] = sums[e];
        cba_icp_result r = a.res[s];
        int32_t phase = a.phase[s];
        icp_advance(acc, a.o, icp_min_pairs(a.o), a.extent, &r, &phase);
        a.res[s] = r;
        a.phase[s] = phase;
        if (phase == ICP_DONE) atomicAdd(a.n_done, 1);
    }
}

// The index: built once at create.  register grows src, offset, res, phase and slab when a call is larger than any before; every call
// ends with its stream synchronised.
struct CloudIndex : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    CloudGrid g{};
    double extent = 0.0;
    int64_t n = 0, n_cells = 0;
    bool has_normals = false;
    DevBuf<int32_t> start;     // [n_cells + 1]
    DevBuf<CloudRec> rec;      // [n]: the valid points in cell order
    DevBuf<double> rec_normal; // [n][3] with normals
    DevBuf<double> query, dist2, src, slab;
    DevBuf<int64_t> index, offset;
    DevBuf<cba_icp_result> res;
    DevBuf<int32_t> phase, n_done;
    PinnedBuf<int32_t> done_h;
};
static_assert(!std::is_copy_constructible_v<CloudIndex> && !std::is_copy_assignable_v<CloudIndex>, "a handle owns its stream and buffers");

int cloud_plan(int64_t n, const double* xyz, double cell_size, double* fit) {
    CloudGrid g;
    double extent;
    int64_t n_cells;
    return cloud_plan_grid(n, xyz, cell_size, &g, &extent, &n_cells, fit);
}

CloudIndex* cloud_index_create(int64_t n, const double* xyz, const double* normals, double cell_size, int device) {
    auto h = std::make_unique<CloudIndex>(device);
    double fit;
    if (cloud_plan_grid(n, xyz, cell_size, &h->g, &h->extent, &h->n_cells, &fit) != 0) throw std::invalid_argument("no grid for these points");
    const hipStream_t s = h->begin();
    h->n = n;
    h->has_normals = normals != nullptr;
    DevBuf<double> pts, nrm;
    DevBuf<int32_t> cell_of, tmp;
    pts.assign(xyz, static_cast<size_t>(3 * n), s);
    if (normals) nrm.assign(normals, static_cast<size_t>(3 * n), s);
    cell_of.alloc(static_cast<size_t>(n));
    tmp.alloc(scan_tmp_size(h->n_cells));
    h->start.alloc(static_cast<size_t>(h->n_cells) + 1);
    h->start.zero(s);
    h->rec.alloc(static_cast<size_t>(n));
    if (normals) h->rec_normal.alloc(static_cast<size_t>(3 * n));
    h->n_done.alloc(1);
    h->done_h.reserve(1);
    const dim3 grid(launch_grid(n, CLOUD_BLOCK, CLOUD_GRID));
    hipLaunchKernelGGL(k_cloud_count, grid, dim3(CLOUD_BLOCK), 0, s, n, pts.p, h->g, cell_of.p, h->start.p + 1);
    scan_exclusive(s, h->start.p + 1, h->n_cells, tmp.p);
    hipLaunchKernelGGL(k_cloud_scatter, grid, dim3(CLOUD_BLOCK), 0, s, n, pts.p, normals ? nrm.p : nullptr, cell_of.p, h->start.p + 1, h->rec.p,
                       h->rec_normal.p);
    CBA_HIP(hipGetLastError());
    CBA_HIP(hipStreamSynchronize(s));  // the build's buffers go out of scope
    return h.release();
}

double cloud_index_cell_size(const CloudIndex* h) { return h->g.cell; }
bool cloud_index_has_normals(const CloudIndex* h) { return h->has_normals; }

void cloud_index_nearest(CloudIndex* h, int64_t m, const double* query, double max_distance, int64_t* index, double* dist2) {
    const hipStream_t s = h->begin();
    h->query.ensure(static_cast<size_t>(3 * m));
    h->index.ensure(static_cast<size_t>(m));
    h->dist2.ensure(static_cast<size_t>(m));
    h->query.upload(query, static_cast<size_t>(3 * m), s);
    hipLaunchKernelGGL(k_cloud_nearest, dim3(launch_grid(m, CLOUD_BLOCK, CLOUD_GRID)), dim3(CLOUD_BLOCK), 0, s, m, h->query.p, h->g, h->start.p,
                       h->rec.p, max_distance, h->index.p, h->dist2.p);
    CBA_HIP(hipGetLastError());
    h->index.download(index, static_cast<size_t>(m), s);
    if (dist2) h->dist2.download(dist2, static_cast<size_t>(m), s);
    CBA_HIP(hipStreamSynchronize(s));
}

// init: [n_sources] results with the normalised initial pose, iterations 0 and the rest zero.  stage_ms [3] optional: upload, the
// rounds, download
void cloud_index_register(CloudIndex* h, int n_sources, const int64_t* source_offset, const double* source_xyz, const cba_icp_options& o,
                          cba_icp_result* results, double* stage_ms) {
    const hipStream_t s = h->begin();
    const size_t m = static_cast<size_t>(source_offset[n_sources]);  // the offsets start at 0 (checked by the caller)
    StageTimer<4> tm(s, stage_ms != nullptr);
    tm.mark(0);
    h->src.ensure(3 * m);
    h->offset.ensure(static_cast<size_t>(n_sources) + 1);
    h->res.ensure(static_cast<size_t>(n_sources));
    h->phase.ensure(static_cast<size_t>(n_sources));
    h->slab.ensure(static_cast<size_t>(n_sources) * ICP_BLOCKS * ICP_ROW);
    h->src.upload(source_xyz, 3 * m, s);
    h->offset.upload(source_offset, static_cast<size_t>(n_sources) + 1, s);
    h->res.upload(results, static_cast<size_t>(n_sources), s);
    CBA_HIP(hipMemsetAsync(h->phase.p, 0, static_cast<size_t>(n_sources) * sizeof(int32_t), s));  // ICP_RUN
    CBA_HIP(hipMemsetAsync(h->n_done.p, 0, sizeof(int32_t), s));
    tm.mark(1);
    IcpArgs a;
    a.g = h->g; a.start = h->start.p; a.rec = h->rec.p; a.rec_normal = h->rec_normal.p;
    a.offset = h->offset.p; a.src = h->src.p; a.res = h->res.p; a.phase = h->phase.p; a.slab = h->slab.p; a.n_done = h->n_done.p;
    a.o = o; a.extent = h->extent;
    const dim3 grid(static_cast<unsigned>(n_sources) * ICP_BLOCKS);
    for (int round = 0; round <= o.max_iterations; ++round) {
        if (o.metric == 0)
            hipLaunchKernelGGL(k_icp_accumulate<0>, grid, dim3(CLOUD_BLOCK), 0, s, a);
        else
            hipLaunchKernelGGL(k_icp_accumulate<1>, grid, dim3(CLOUD_BLOCK), 0, s, a);
        hipLaunchKernelGGL(k_icp_step, dim3(static_cast<unsigned>(n_sources)), dim3(64), 0, s, a);
        CBA_HIP(hipGetLastError());
        if (round % ICP_POLL == ICP_POLL - 1 && round < o.max_iterations) {
            h->n_done.download(h->done_h.p, 1, s);
            CBA_HIP(hipStreamSynchronize(s));
            if (h->done_h.p[0] == n_sources) break;
        }
    }
    tm.mark(2);
    h->res.download(results, static_cast<size_t>(n_sources), s);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(stage_ms);
}

void cloud_index_destroy(CloudIndex* h) noexcept { destroy_handle(h); }

}  // namespace cba
