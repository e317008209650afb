// cloud_register.hip — scan registration on the GPU (cloud_math.hpp, calibba.h: cba_point_normals, cba_cloud_index, cba_cloud_nearest,
// cba_cloud_register).
//   k_point_normals     one lane per pixel: the centre and its four neighbours straight from global memory (a row is read by three
//                       rows of lanes, which the caches serve), cloud_normal.
//   k_cloud_count       one lane per target point: its cell into cell_of (-1: invalid), integer atomicAdd on the cell's count.
//   k_scan_tiles / k_scan_add   (scan_tiles.hpp) exclusive scan of the counts in tiles of SCAN_TILE = 1024 cells, up to three levels at the cap.
//   k_cloud_scatter     one lane per valid point: its place by integer atomicAdd on the cell's start, the 32-byte record and the
//                       normal into cell order.  The starts live at start + 1 while they are bumped: afterwards start[c + 1] is the
//                       end of cell c, which is the start of cell c + 1, and start[0] = 0 was never touched.
//   k_cloud_nearest     one lane per query, grid-stride: cloud_nearest_point.  No LDS.
//   k_icp_accumulate    ICP_BLOCKS workgroups per source, grid-striding its points: the point rule (icp_add_source_point), 29 sums in
//                       registers; wave_transpose_sum inside the wave, LDS across the four waves, one slab row per (source, block).
//   k_icp_step          one wavefront per source: lane e adds entry e of the source's slab rows in block order (icp_slab_entry); lane 0
//                       runs icp_advance (Cholesky, update, stop tests) and writes pose, phase and, when the source ends, the done count.
// The host builds a grid by cloud_build_grid and runs both pipelines by icp_rounds: max_iterations + 1 rounds of the two kernels queued
// without reading values; every ICP_POLL rounds it reads the done count (the set: the state) and stops when every system has ended.  One
// that has ended is not touched again, so results do not depend on when the host looks.  No float atomics; integer ones for counts and places.
// cba_cloud_set / cba_cloud_align (the alignment of many scans over a graph of pairs):
//   k_align_accumulate  ICP_BLOCKS workgroups per edge (a, b): k_icp_accumulate's body (icp_accumulate_block, one copy for both) on scan
//                       a's points at T_b^-1 T_a against scan b (a CloudTarget); the edge, the scans' table rows and the poses from blockIdx.
//   k_align_step        one workgroup per call: the edges' slab rows in workgroup order, their statistics and blocks M = A^T H A,
//                       c = A^T g, the system of all scans but the fixed one in a global workspace (every entry walks the edges in list
//                       order), the width-n Cholesky by columns with two barriers each, both substitutions, the updates, the state.
#include <memory>
#include <type_traits>
#include <vector>

#include "pipelines.hpp"
#include "scan_tiles.hpp"
#include "wave_reduce.hpp"
#include "cloud_math.hpp"

namespace cba {

constexpr int CLOUD_BLOCK = 256;
constexpr int CLOUD_GRID = 8192;        // grid-stride cap
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

__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_nearest(int64_t m, const double* __restrict__ query, CloudTarget t, double md,
                                                               int64_t* __restrict__ index, double* __restrict__ dist2) {
    const double md2 = md * md;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(CLOUD_BLOCK) + threadIdx.x; i < m; i += static_cast<int64_t>(gridDim.x) * CLOUD_BLOCK) {
        int32_t pos;
        double d2;
        index[i] = cloud_nearest_point(t.g, t.start, t.rec, query[3 * i], query[3 * i + 1], query[3 * i + 2], md, md2, &pos, &d2);
        dist2[i] = d2;
    }
}

// ---- ICP --------------------------------------------------------------------------------------------------------------------------
struct IcpArgs {
    CloudTarget target;
    const int64_t* offset;   // [n_sources + 1]
    const double* src;       // [m][3]
    cba_icp_result* res;     // [n_sources]: pose7, iterations and status live here between the rounds
    int32_t* phase;          // [n_sources]
    double* slab;            // [n_sources][ICP_BLOCKS][ICP_ROW]
    int32_t* n_done;
    cba_icp_options o;
    double extent;
};

// The body of both accumulate kernels (k_icp_accumulate, k_align_accumulate): workgroup blockIdx.x is one of the ICP_BLOCKS of system
// blockIdx.x / ICP_BLOCKS; the m points at src at the pose (R, t) against one target; the sums of the workgroup go to its row of
// slab [systems][ICP_BLOCKS][ICP_ROW].  Every value that selects the system is wave-uniform.
template <int METRIC>
__device__ __forceinline__ void icp_accumulate_block(const CloudTarget& target, const double* __restrict__ src, int64_t m, const double* R,
                                                     const double* t, double md, int blk, double* __restrict__ slab_row,
                                                     double (*part)[ICP_ROW]) {
    const double md2 = md * md;
    double acc[ICP_ROW];
#pragma unroll
    for (int e = 0; e < ICP_ROW; ++e) acc[e] = 0.0;
#pragma unroll 1
    for (int64_t i = static_cast<int64_t>(blk) * CLOUD_BLOCK + threadIdx.x; i < m; i += static_cast<int64_t>(ICP_BLOCKS) * CLOUD_BLOCK)
        icp_add_source_point<METRIC>(target, R, t, src + 3 * i, md, md2, acc);
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
        slab_row[threadIdx.x] = v;
    }
}

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
    icp_accumulate_block<METRIC>(a.target, a.src + 3 * first, m, R, t, a.o.max_distance, blk,
                                 a.slab + (static_cast<int64_t>(s) * ICP_BLOCKS + blk) * ICP_ROW, part);
}

// entry c of a system's sums: its ICP_BLOCKS slab rows (slab: the first) added in block order from row 0 on; the order is the result
__device__ __forceinline__ double icp_slab_entry(const double* __restrict__ slab, int c) {
    const double* row = slab + c;
    double v = row[0];
#pragma unroll 4
    for (int b = 1; b < ICP_BLOCKS; ++b) v += row[static_cast<int64_t>(b) * ICP_ROW];
    return v;
}

__global__ __launch_bounds__(64) void k_icp_step(IcpArgs a) {
    __shared__ double sums[ICP_ROW];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (a.phase[s] == ICP_DONE) return;
    if (lane < ICP_ROW) sums[lane] = icp_slab_entry(a.slab + static_cast<int64_t>(s) * ICP_BLOCKS * ICP_ROW, lane);
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
    CloudTarget target{};      // the grid, and the three buffers below as the kernels read them
    double extent = 0.0;
    int64_t n_cells = 0;
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

// The target of grid g queued on s from its n points on the device (normals NULL: none): count into start + 1, scan, scatter.
// start [n_cells + 1] comes zeroed; cell_of [n] and tmp [scan_tmp_size(n_cells)] are work.
static CloudTarget cloud_build_grid(hipStream_t s, const CloudGrid& g, int64_t n_cells, int64_t n, const double* pts, const double* normals,
                                    int32_t* cell_of, int32_t* tmp, int32_t* start, CloudRec* rec, double* rec_normal) {
    const dim3 grid(launch_grid(n, CLOUD_BLOCK, CLOUD_GRID));
    hipLaunchKernelGGL(k_cloud_count, grid, dim3(CLOUD_BLOCK), 0, s, n, pts, g, cell_of, start + 1);
    scan_exclusive(s, start + 1, n_cells, tmp);
    hipLaunchKernelGGL(k_cloud_scatter, grid, dim3(CLOUD_BLOCK), 0, s, n, pts, normals, cell_of, start + 1, rec, rec_normal);
    CBA_HIP(hipGetLastError());
    return CloudTarget{g, start, rec, rec_normal};
}

// The rounds of an ICP call: queue_round() queues one; all_done() reads back, synchronised, whether every system has ended.
template <class Queue, class Done>
static void icp_rounds(int max_iterations, Queue queue_round, Done all_done) {
    for (int round = 0; round <= max_iterations; ++round) {
        queue_round();
        CBA_HIP(hipGetLastError());
        if (round % ICP_POLL == ICP_POLL - 1 && round < max_iterations && all_done()) break;
    }
}

CloudIndex* cloud_index_create(int64_t n, const double* xyz, const double* normals, double cell_size, int device) {
    auto h = std::make_unique<CloudIndex>(device);
    double fit;
    if (cloud_plan_grid(n, xyz, cell_size, &h->target.g, &h->extent, &h->n_cells, &fit) != 0) throw std::invalid_argument("no grid for these points");
    const hipStream_t s = h->begin();
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
    h->target = cloud_build_grid(s, h->target.g, h->n_cells, n, pts.p, normals ? nrm.p : nullptr, cell_of.p, tmp.p, h->start.p, h->rec.p,
                                 h->rec_normal.p);
    CBA_HIP(hipStreamSynchronize(s));  // the build's buffers go out of scope
    return h.release();
}

double cloud_index_cell_size(const CloudIndex* h) { return h->target.g.cell; }
bool cloud_index_has_normals(const CloudIndex* h) { return h->has_normals; }

void cloud_index_nearest(CloudIndex* h, int64_t m, const double* query, double max_distance, int64_t* index, double* dist2) {
    const hipStream_t s = h->begin();
    h->query.ensure(static_cast<size_t>(3 * m));
    h->index.ensure(static_cast<size_t>(m));
    h->dist2.ensure(static_cast<size_t>(m));
    h->query.upload(query, static_cast<size_t>(3 * m), s);
    hipLaunchKernelGGL(k_cloud_nearest, dim3(launch_grid(m, CLOUD_BLOCK, CLOUD_GRID)), dim3(CLOUD_BLOCK), 0, s, m, h->query.p, h->target,
                       max_distance, h->index.p, h->dist2.p);
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
    a.target = h->target; a.offset = h->offset.p; a.src = h->src.p; a.res = h->res.p; a.phase = h->phase.p; a.slab = h->slab.p; a.n_done = h->n_done.p;
    a.o = o; a.extent = h->extent;
    const dim3 grid(static_cast<unsigned>(n_sources) * ICP_BLOCKS);
    const auto queue_round = [&] {
        hipLaunchKernelGGL(o.metric == 0 ? k_icp_accumulate<0> : k_icp_accumulate<1>, grid, dim3(CLOUD_BLOCK), 0, s, a);
        hipLaunchKernelGGL(k_icp_step, dim3(static_cast<unsigned>(n_sources)), dim3(64), 0, s, a);
    };
    icp_rounds(o.max_iterations, queue_round, [&] {
        h->n_done.download(h->done_h.p, 1, s);
        CBA_HIP(hipStreamSynchronize(s));
        return h->done_h.p[0] == n_sources;
    });
    tm.mark(2);
    h->res.download(results, static_cast<size_t>(n_sources), s);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(stage_ms);
}

void cloud_index_destroy(CloudIndex* h) noexcept { destroy_handle(h); }

// ---- alignment of many scans (calibba.h: cba_cloud_align) -------------------------------------------------------------------------
// a scan of the set: its grid and sorted records (it is a target) and its points in original order (it is a source)
struct AlignScan {
    CloudTarget target;
    int64_t first, count;  // its points are xyz[first .. first + count)
};

constexpr int ALIGN_BLOCK = 256;
constexpr int ALIGN_WIDTH = 6 * (CBA_ALIGN_MAX_SCANS - 1);
static_assert(ALIGN_WIDTH <= 2 * ALIGN_BLOCK, "k_align_step: a lane owns at most two rows of a column");

struct AlignArgs {
    const AlignScan* scan;   // [n_scans]
    const double* xyz;       // [m][3]
    const int32_t* edge;     // [n_edges][2]
    double* pose;            // [n_scans][7]
    AlignState* st;
    double* slab;            // [n_edges][ICP_BLOCKS][ICP_ROW]
    double* sums;            // [n_edges][ICP_ROW]
    cba_align_edge* edge_out;  // [n_edges]
    double* adj;             // [n_scans][36]
    double* blocks;          // [n_edges][ALIGN_EDGE]
    double* H;               // [n][n], n = 6 (n_scans - 1)
    cba_icp_options o;
    double extent;
    int32_t n_scans, n_edges, fixed;
};

// ICP_BLOCKS workgroups per edge (a, b): scan a's points at T_b^-1 T_a against scan b's grid.  The edge, both table rows and both
// poses are indexed by blockIdx alone.
template <int METRIC>
__global__ __launch_bounds__(CLOUD_BLOCK) void k_align_accumulate(AlignArgs a) {
    __shared__ double part[CLOUD_BLOCK / 64][ICP_ROW];
    const int e = blockIdx.x / ICP_BLOCKS, blk = blockIdx.x - e * ICP_BLOCKS;
    if (a.st->phase == ICP_DONE) return;  // the whole workgroup
    const int sa = a.edge[2 * e], sb = a.edge[2 * e + 1];
    const AlignScan& A = a.scan[sa];
    const AlignScan& B = a.scan[sb];
    double R[9], t[3];
    {
        const double* pa = a.pose + 7 * sa;
        const double* pb = a.pose + 7 * sb;
        const double qa[4] = {pa[0], pa[1], pa[2], pa[3]}, qb[4] = {pb[0], pb[1], pb[2], pb[3]};
        const double ta[3] = {pa[4], pa[5], pa[6]}, tb[3] = {pb[4], pb[5], pb[6]};
        double Ra[9], Rb[9];
        icp_rotation(qa, Ra);
        icp_rotation(qb, Rb);
        align_relative(Ra, ta, Rb, tb, R, t);
    }
    icp_accumulate_block<METRIC>(B.target, a.xyz + 3 * A.first, A.count, R, t, a.o.max_distance, blk,
                                 a.slab + (static_cast<int64_t>(e) * ICP_BLOCKS + blk) * ICP_ROW, part);
}

// One workgroup per call: the edges' sums, statistics and blocks, the system of all scans, its solve, the updates, the state.  Every
// branch around a barrier is taken by the whole workgroup (its condition is read from LDS or the arguments), and every loop bound
// comes from n_scans, n_edges and constants.
__global__ __launch_bounds__(ALIGN_BLOCK) void k_align_step(AlignArgs a) {
    __shared__ double l_ss[CBA_ALIGN_MAX_EDGES], l_np[CBA_ALIGN_MAX_EDGES];  // l_np < 0: the edge is not used
    __shared__ int32_t l_row[2 * CBA_ALIGN_MAX_EDGES];                       // the row blocks of a and b in the reduced system, -1: fixed
    __shared__ double l_g[ALIGN_WIDTH], l_s[ALIGN_WIDTH], l_z[ALIGN_WIDTH], l_xi[ALIGN_WIDTH];
    __shared__ AlignState l_st;
    __shared__ double l_pivot;
    __shared__ int32_t l_solve, l_ok, l_small[CBA_ALIGN_MAX_SCANS];
    const int tid = threadIdx.x;
    if (a.st->phase == ICP_DONE) return;  // the whole workgroup
    const int E = a.n_edges, N = a.n_scans, n = 6 * (N - 1);
    const int32_t min_pairs = icp_min_pairs(a.o);
    // 1. entry c of edge e: its slab rows in workgroup order; a scan's adjoint
    for (int it = tid; it < E * ICP_ROW; it += ALIGN_BLOCK) {
        const int e = it / ICP_ROW, c = it - e * ICP_ROW;
        a.sums[it] = icp_slab_entry(a.slab + static_cast<int64_t>(e) * ICP_BLOCKS * ICP_ROW, c);
    }
    for (int p = tid; p < N; p += ALIGN_BLOCK) {
        const double* pose = a.pose + 7 * p;
        const double q[4] = {pose[0], pose[1], pose[2], pose[3]}, t[3] = {pose[4], pose[5], pose[6]};
        double R[9];
        icp_rotation(q, R);
        align_adjoint(R, t, a.adj + 36 * p);
    }
    __syncthreads();
    // 2. an edge's statistics
    for (int e = tid; e < E; e += ALIGN_BLOCK) {
        const double* s = a.sums + static_cast<int64_t>(e) * ICP_ROW;
        cba_align_edge* eo = a.edge_out + e;
        int at = 0;
        for (int k = 0; k < 6; ++k)
            for (int l = k; l < 6; ++l) {
                const double v = s[at++];
                eo->H[6 * k + l] = v;
                eo->H[6 * l + k] = v;
            }
        for (int k = 0; k < 6; ++k) eo->g[k] = s[21 + k];
        const int64_t np = static_cast<int64_t>(s[ICP_NP]);
        const bool used = np >= min_pairs;
        eo->ss = s[ICP_SS];
        eo->n_pairs = np;
        eo->used = used ? 1 : 0;
        l_ss[e] = s[ICP_SS];
        l_np[e] = used ? s[ICP_NP] : -1.0;
        const int sa = a.edge[2 * e], sb = a.edge[2 * e + 1];
        l_row[2 * e] = sa == a.fixed ? -1 : sa < a.fixed ? sa : sa - 1;
        l_row[2 * e + 1] = sb == a.fixed ? -1 : sb < a.fixed ? sb : sb - 1;
    }
    __syncthreads();
    // 3. entry r of edge e's blocks M and c; the totals in list order and the tests before the solve
    for (int it = tid; it < E * ALIGN_EDGE; it += ALIGN_BLOCK) {
        const int e = it / ALIGN_EDGE, r = it - e * ALIGN_EDGE;
        const cba_align_edge* eo = a.edge_out + e;
        const double* A = a.adj + 36 * a.edge[2 * e + 1];
        a.blocks[it] = r < 36 ? align_block_entry(eo->H, A, r / 6, r % 6) : align_block_gradient(eo->g, A, r - 36);
    }
    if (tid == 0) {
        AlignState st = *a.st;
        double ss = 0.0, np = 0.0;
        int32_t used = 0;
        for (int e = 0; e < E; ++e)
            if (l_np[e] >= 0.0) {
                ss += l_ss[e];
                np += l_np[e];
                ++used;
            }
        st.res.n_pairs = static_cast<int64_t>(np);
        st.res.n_used_edges = used;
        st.res.rms = np > 0.0 ? std::sqrt(ss / np) : std::numeric_limits<double>::quiet_NaN();
        l_solve = align_begin(a.o, &st) ? 1 : 0;
        l_ok = 1;
        l_st = st;
    }
    __syncthreads();
    if (l_solve != 0) {  // the whole workgroup
        // 4. the system: zero, then entry r of scan p's row of blocks walks the edges in list order
        for (int64_t it = tid; it < static_cast<int64_t>(n) * n; it += ALIGN_BLOCK) a.H[it] = 0.0;
        for (int it = tid; it < n; it += ALIGN_BLOCK) l_g[it] = 0.0;
        __syncthreads();
        for (int it = tid; it < N * ALIGN_EDGE; it += ALIGN_BLOCK) {
            const int p = it / ALIGN_EDGE, r = it - p * ALIGN_EDGE;
            const int rp = p == a.fixed ? -1 : p < a.fixed ? p : p - 1;
            if (rp < 0) continue;
            for (int e = 0; e < E; ++e)
                if (l_np[e] >= 0.0) align_assemble_entry(n, a.H, l_g, rp, r, l_row[2 * e], l_row[2 * e + 1], a.blocks + static_cast<int64_t>(e) * ALIGN_EDGE);
        }
        __syncthreads();
        // 5. align_cholesky's sequence: column k, a lane per row (two beyond ALIGN_BLOCK rows)
        for (int k = 0; k < n; ++k) {
            const int i0 = k + tid, i1 = i0 + ALIGN_BLOCK;
            double s0 = 0.0, s1 = 0.0;
            if (i0 < n) s0 = align_cholesky_entry(n, a.H, i0, k);
            if (i1 < n) s1 = align_cholesky_entry(n, a.H, i1, k);
            if (tid == 0) {
                if (!align_pivot_ok(s0, a.H[static_cast<int64_t>(k) * n + k])) l_ok = 0;
                l_pivot = std::sqrt(s0);
            }
            __syncthreads();
            const double lkk = l_pivot;
            if (i0 < n) a.H[static_cast<int64_t>(i0) * n + k] = tid == 0 ? lkk : s0 / lkk;
            if (i1 < n) a.H[static_cast<int64_t>(i1) * n + k] = s1 / lkk;
            __syncthreads();
        }
        for (int i = tid; i < n; i += ALIGN_BLOCK) l_s[i] = -l_g[i];
        __syncthreads();
        for (int j = 0; j < n; ++j) {  // forward: once z_j is known every later row subtracts its product, j ascending
            const double zj = l_s[j] / a.H[static_cast<int64_t>(j) * n + j];
            if (tid == 0) l_z[j] = zj;
            for (int i = j + 1 + tid; i < n; i += ALIGN_BLOCK) l_s[i] -= a.H[static_cast<int64_t>(i) * n + j] * zj;
            __syncthreads();
        }
        for (int i = n - 1; i >= 0; --i) {  // back: the products of row i's chain side by side, the chain itself in j ascending
            for (int j = i + 1 + tid; j < n; j += ALIGN_BLOCK) l_s[j] = a.H[static_cast<int64_t>(j) * n + i] * l_xi[j];
            __syncthreads();
            if (tid == 0) {
                double s = l_z[i];
                for (int j = i + 1; j < n; ++j) s -= l_s[j];
                l_xi[i] = s / a.H[static_cast<int64_t>(i) * n + i];
            }
            __syncthreads();
        }
        // 6. the updates and the stop tests
        const bool ok = l_ok != 0;
        for (int p = tid; p < N; p += ALIGN_BLOCK) {
            int32_t small = 1;
            if (ok && p != a.fixed) {
                const int rp = p < a.fixed ? p : p - 1;
                double* gp = a.pose + 7 * p;
                double pose[7] = {gp[0], gp[1], gp[2], gp[3], gp[4], gp[5], gp[6]};
                const double xi[6] = {l_xi[6 * rp], l_xi[6 * rp + 1], l_xi[6 * rp + 2], l_xi[6 * rp + 3], l_xi[6 * rp + 4], l_xi[6 * rp + 5]};
                small = align_update(pose, xi, a.o, a.extent) ? 1 : 0;
#pragma unroll
                for (int k = 0; k < 7; ++k) gp[k] = pose[k];
            }
            l_small[p] = small;
        }
        __syncthreads();
        if (tid == 0) {
            bool all = true;
            for (int p = 0; p < N; ++p) all = all && l_small[p] != 0;
            align_advance(ok, all, a.o, &l_st);
        }
    }
    if (tid == 0) *a.st = l_st;
}

// The set: every scan's index built at create with the kernels of cba_cloud_index into shared arrays; align grows the edge buffers
// and the system when a call is larger than any before; every call ends with its stream synchronised.
struct CloudSet : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    int n_scans = 0;
    double cell = 0.0, extent = 0.0;
    bool has_normals = false;
    DevBuf<double> xyz, rec_normal;  // [m][3]: the sources in original order; the normals in cell order
    DevBuf<CloudRec> rec;            // [m]: scan k's valid points in cell order from first_k on
    DevBuf<int32_t> start;           // every scan's n_cells + 1 starts, one scan after the other
    DevBuf<AlignScan> scan;
    DevBuf<double> pose, slab, sums, adj, blocks, H;
    DevBuf<int32_t> edge;
    DevBuf<cba_align_edge> edge_out;
    DevBuf<AlignState> st;
    PinnedBuf<AlignState> st_h;
};
static_assert(!std::is_copy_constructible_v<CloudSet> && !std::is_copy_assignable_v<CloudSet>, "a handle owns its stream and buffers");

int cloud_set_plan(int n_scans, const int64_t* offset, const double* xyz, double cell_size, int* scan, double* fit) {
    for (int k = 0; k < n_scans; ++k) {
        const int plan = cloud_plan(offset[k + 1] - offset[k], xyz + 3 * offset[k], cell_size, fit);
        if (plan != 0) {
            *scan = k;
            return plan;
        }
    }
    return 0;
}

CloudSet* cloud_set_create(int n_scans, const int64_t* offset, const double* xyz, const double* normals, double cell_size, int device) {
    auto h = std::make_unique<CloudSet>(device);
    const hipStream_t s = h->begin();
    const int64_t m = offset[n_scans];
    h->n_scans = n_scans;
    h->cell = cell_size;
    h->has_normals = normals != nullptr;
    std::vector<AlignScan> table(static_cast<size_t>(n_scans));
    std::vector<int64_t> start_at(static_cast<size_t>(n_scans)), cells(static_cast<size_t>(n_scans));
    int64_t n_start = 0, most_cells = 0, most_points = 0;
    for (int k = 0; k < n_scans; ++k) {
        double fit, extent;
        AlignScan& t = table[k];
        t.first = offset[k];
        t.count = offset[k + 1] - offset[k];
        if (cloud_plan_grid(t.count, xyz + 3 * t.first, cell_size, &t.target.g, &extent, &cells[k], &fit) != 0)
            throw std::invalid_argument("no grid for these points");
        h->extent = std::max(h->extent, extent);
        start_at[k] = n_start;
        n_start += cells[k] + 1;
        most_cells = std::max(most_cells, cells[k]);
        most_points = std::max(most_points, t.count);
    }
    DevBuf<double> nrm;
    DevBuf<int32_t> cell_of, tmp;
    h->xyz.assign(xyz, static_cast<size_t>(3 * m), s);
    if (normals) nrm.assign(normals, static_cast<size_t>(3 * m), s);
    cell_of.alloc(static_cast<size_t>(most_points));
    tmp.alloc(scan_tmp_size(most_cells));
    h->start.alloc(static_cast<size_t>(n_start));
    h->start.zero(s);
    h->rec.alloc(static_cast<size_t>(m));
    if (normals) h->rec_normal.alloc(static_cast<size_t>(3 * m));
    h->st.alloc(1);
    h->st_h.reserve(1);
    for (int k = 0; k < n_scans; ++k) {
        AlignScan& t = table[k];
        t.target = cloud_build_grid(s, t.target.g, cells[k], t.count, h->xyz.p + 3 * t.first, normals ? nrm.p + 3 * t.first : nullptr, cell_of.p, tmp.p,
                                    h->start.p + start_at[k], h->rec.p + t.first, normals ? h->rec_normal.p + 3 * t.first : nullptr);
    }
    h->scan.assign(table.data(), table.size(), s);
    CBA_HIP(hipStreamSynchronize(s));  // the build's buffers and the host table go out of scope
    return h.release();
}

int cloud_set_scans(const CloudSet* h) { return h->n_scans; }
double cloud_set_cell_size(const CloudSet* h) { return h->cell; }
bool cloud_set_has_normals(const CloudSet* h) { return h->has_normals; }

// pose7 [n_scans][7]: in: the normalised initial poses, out: the result's.  stage_ms [3] optional: upload, the rounds, download
void cloud_set_align(CloudSet* h, int n_edges, const int32_t* edges, const cba_icp_options& o, int fixed, double* pose7, cba_align_edge* edge_out,
                     cba_align_result* result, double* stage_ms) {
    const hipStream_t s = h->begin();
    const size_t E = static_cast<size_t>(n_edges), N = static_cast<size_t>(h->n_scans), n = 6 * (N - 1);
    StageTimer<4> tm(s, stage_ms != nullptr);
    tm.mark(0);
    h->pose.ensure(7 * N);
    h->adj.ensure(36 * N);
    h->H.ensure(n * n);
    h->edge.ensure(2 * E);
    h->slab.ensure(E * ICP_BLOCKS * ICP_ROW);
    h->sums.ensure(E * ICP_ROW);
    h->blocks.ensure(E * ALIGN_EDGE);
    h->edge_out.ensure(E);
    AlignState st{};
    st.res.status = CBA_ICP_NOT_CONVERGED;
    st.phase = ICP_RUN;
    h->pose.upload(pose7, 7 * N, s);
    h->edge.upload(edges, 2 * E, s);
    h->st.upload(&st, 1, s);
    tm.mark(1);
    AlignArgs a;
    a.scan = h->scan.p; a.xyz = h->xyz.p; a.edge = h->edge.p; a.pose = h->pose.p; a.st = h->st.p; a.slab = h->slab.p; a.sums = h->sums.p;
    a.edge_out = h->edge_out.p; a.adj = h->adj.p; a.blocks = h->blocks.p; a.H = h->H.p;
    a.o = o; a.extent = h->extent; a.n_scans = h->n_scans; a.n_edges = n_edges; a.fixed = fixed;
    const dim3 grid(static_cast<unsigned>(n_edges) * ICP_BLOCKS);
    const auto queue_round = [&] {
        hipLaunchKernelGGL(o.metric == 0 ? k_align_accumulate<0> : k_align_accumulate<1>, grid, dim3(CLOUD_BLOCK), 0, s, a);
        hipLaunchKernelGGL(k_align_step, dim3(1), dim3(ALIGN_BLOCK), 0, s, a);
    };
    icp_rounds(o.max_iterations, queue_round, [&] {
        h->st.download(h->st_h.p, 1, s);
        CBA_HIP(hipStreamSynchronize(s));
        return h->st_h.p[0].phase == ICP_DONE;
    });
    tm.mark(2);
    h->pose.download(pose7, 7 * N, s);
    if (edge_out) h->edge_out.download(edge_out, E, s);
    h->st.download(h->st_h.p, 1, s);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));
    *result = h->st_h.p[0].res;
    tm.report(stage_ms);
}

void cloud_set_destroy(CloudSet* h) noexcept { destroy_handle(h); }

}  // namespace cba
