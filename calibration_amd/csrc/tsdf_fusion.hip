// tsdf_fusion.hip — scan fusion on the GPU (tsdf_math.hpp, tsdf_mesh_math.hpp, tsdf_ray_math.hpp, tsdf_colour_math.hpp, calibba.h:
// cba_tsdf_volume, cba_tsdf_integrate, cba_tsdf_integrate_colour, cba_tsdf_extract, cba_tsdf_mesh, cba_tsdf_raycast).
//   k_tsdf_fill         D = 1, W = 0 in every stored voxel (create, reset).
//   k_tsdf_integrate    one launch per call.  A lane owns two adjacent x voxels, one aligned 16-byte {D, W, D, W} word that it loads
//                       once, keeps in registers while it walks the call's maps in order, and stores once: the whole word when both
//                       voxels were updated, 8 bytes when one was, nothing otherwise.  The camera and the pose of map m are tables
//                       indexed by wave-uniform values alone (scalar loads, as in k_triangulate).  Per voxel and map: tsdf_update,
//                       one fp64 projection and one 8-byte gather from the map; neighbouring voxels gather neighbouring pixels.  No
//                       LDS, no atomics; no lane reads another's voxel.
//   k_tsdf_integrate_colour   the same ownership and the same steps 1 to 6 (tsdf_update_at), with the {R, G, B, Wc} words of the lane's two
//                       voxels beside them.  A voxel's colour word is loaded at its first step-7 update and stored once at the end, and
//                       only then: the voxels outside the band, nearly all of them, cost no colour traffic.  The colour sample is one
//                       4-byte gather at the pixel index of the depth gather.
//   k_tsdf_planes       the interleaved rows <-> dense [nz][ny][nx] planes of D and of W (fetch, upload).
//   k_tsdf_colour_planes   the colour rows <-> dense [nz][ny][nx][4] records, one 16-byte word per lane and step.
//   k_tsdf_extract<0>   one workgroup per tile of TSDF_EXTRACT_TILE voxels of the dense order, in four rounds of 256 voxels: each lane
//                       tests the three edges of its voxel; ballots and popcounts give the wave's total, wave_counts_prefix the workgroup's.
//   k_scan_tiles / k_scan_add   (scan_tiles.hpp: scan_counts) the exclusive scan of the tile counts; one extra entry receives the total.
//   k_tsdf_extract<1>   the same walk again: an edge's place is its tile's start, the rounds and waves before it, and the popcount of
//                       the ballots below its lane, so the order is the visiting order whatever the arrival order; tsdf_edge_point.
//   k_tsdf_extract<1,1> the place pass of cba_tsdf_mesh: it also writes, per wave and round, the record {first place, three ballots} of
//                       its 64 voxels (tsdf_mesh_math.hpp: TsdfEdgeGroup), from which an edge's place follows by popcounts.
//   k_tsdf_extract<1,R,1>   the place pass on a handle with colour: it also writes the colour of each point (tsdf_colour_edge), one
//                       4-byte store.  A handle without colour launches the instantiations above.
//   k_tsdf_mesh<0/1>    the same tiles: a lane owns the cell at its voxel.  It loads the {D, W} words of its voxel in the four rows
//                       (j, k) .. (j + 1, k + 1), forms sign and weight bits and takes the +x neighbour's from the next lane (the last lane
//                       of a wave loads its own): four 8-byte loads per cell.  The table of triangles per case (2 KiB, generated from
//                       the rule at compile time) is staged in LDS.  Ballots of the three bits of a lane's triangle count give the
//                       wave's prefix; count, scan and place as above.  A triangle is three lookups in the records.
//   k_tsdf_rays         the rays table of a ray cast: one lane per pixel, ls_unproject as it is, one 16-byte store.
//   k_tsdf_raycast      one launch per call over views x pixel tiles.  A wavefront owns a compact 8 x 8 block of pixels of one view, so its
//                       64 rays walk neighbouring cells and share cache lines; the view is a table indexed by a wave-uniform value
//                       alone.  A lane marches its ray by tsdf_ray_pixel: per sample four rows of two {D, W} pairs, one 16-byte load
//                       per row where the cell's x is even, two 8-byte loads where it is odd; every decision in fp64.  The loop has
//                       the rule's exits and no other (hit, behind, past the range, no progress, the sample cap).  No LDS, no
//                       atomics, no scratch; a lane writes its own pixel only.
//   k_tsdf_raycast_colour   after k_tsdf_raycast on a handle with colour: one lane per pixel reads its status, depth and ray and the view,
//                       and stores the hit's colour (tsdf_colour_hit: eight 16-byte loads for a hit, none otherwise), one 4-byte store.
// The handle owns one stream and every buffer; a call grows a buffer that is too small and allocates nothing else; every call ends
// with the stream synchronised.  No float atomics, and no integer ones either.
#include <memory>
#include <type_traits>
#include <vector>

#include "pipelines.hpp"
#include "scan_tiles.hpp"
#include "tsdf_colour_math.hpp"
#include "tsdf_math.hpp"
#include "tsdf_mesh_math.hpp"
#include "tsdf_ray_math.hpp"

namespace cba {

constexpr int TSDF_BLOCK = 256;
constexpr int TSDF_GRID = 8192;  // grid-stride cap of the fill and plane kernels
static_assert(TSDF_EXTRACT_TILE == 4 * TSDF_BLOCK, "k_tsdf_extract walks a tile in four rounds");
static_assert(TSDF_BLOCK == 256, "k_tsdf_mesh stages one table word per lane");
static_assert(TSDF_BLOCK == SCAN_BLOCK, "wave_counts_prefix adds up the waves of a workgroup of SCAN_BLOCK lanes");
static_assert(TSDF_MESH_GROUP == 64 && TSDF_EXTRACT_TILE % TSDF_MESH_GROUP == 0, "a record is one wave of one round of k_tsdf_extract");

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_fill(int64_t n_stored, float2* __restrict__ vol) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(TSDF_BLOCK) + threadIdx.x; i < n_stored; i += static_cast<int64_t>(gridDim.x) * TSDF_BLOCK)
        vol[i] = make_float2(1.0f, 0.0f);
}

template <int MODEL>
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_integrate(TsdfGrid g, const TsdfCam* __restrict__ cam, const TsdfPose* __restrict__ poses,
                                                               const double* __restrict__ depth, int n_maps, TsdfRule r, float* __restrict__ vol) {
    const int64_t pair = blockIdx.x * static_cast<int64_t>(TSDF_BLOCK) + threadIdx.x;
    const int half = g.pitch >> 1;
    const int64_t row = pair / half;
    if (row >= static_cast<int64_t>(g.ny) * g.nz) return;
    const int i = 2 * static_cast<int>(pair - row * half), k = static_cast<int>(row / g.ny), j = static_cast<int>(row - static_cast<int64_t>(k) * g.ny);
    float4* at = reinterpret_cast<float4*>(vol) + pair;  // rows are pitch / 2 words long: the pair's number is its word's
    float4 q = *at;
    const double xa = tsdf_coord(g.o[0], i, g.vs), xb = tsdf_coord(g.o[0], i + 1, g.vs);
    const double y = tsdf_coord(g.o[1], j, g.vs), z = tsdf_coord(g.o[2], k, g.vs);
    const bool second = i + 1 < g.nx;
    const int64_t plane = static_cast<int64_t>(r.W) * r.H;
    bool ca = false, cb = false;
#pragma unroll 1
    for (int m = 0; m < n_maps; ++m) {
        const double* map = depth + m * plane;
        ca |= tsdf_update<MODEL>(*cam, poses[m], map, r, xa, y, z, &q.x, &q.y);
        if (second) cb |= tsdf_update<MODEL>(*cam, poses[m], map, r, xb, y, z, &q.z, &q.w);
    }
    if (ca && cb)
        *at = q;
    else if (ca)
        *reinterpret_cast<float2*>(at) = make_float2(q.x, q.y);
    else if (cb)
        *(reinterpret_cast<float2*>(at) + 1) = make_float2(q.z, q.w);
}

// EAGER: both colour words loaded up front (instantiated by the experiment builds: what the lazy load is worth)
template <int MODEL, bool EAGER = false>
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_integrate_colour(TsdfGrid g, const TsdfCam* __restrict__ cam, const TsdfPose* __restrict__ poses,
                                                                      const double* __restrict__ depth, const uint32_t* __restrict__ rgba, int n_maps,
                                                                      TsdfRule r, float* __restrict__ vol, float* __restrict__ col) {
    const int64_t pair = blockIdx.x * static_cast<int64_t>(TSDF_BLOCK) + threadIdx.x;
    const int half = g.pitch >> 1;
    const int64_t row = pair / half;
    if (row >= static_cast<int64_t>(g.ny) * g.nz) return;
    const int i = 2 * static_cast<int>(pair - row * half), k = static_cast<int>(row / g.ny), j = static_cast<int>(row - static_cast<int64_t>(k) * g.ny);
    float4* at = reinterpret_cast<float4*>(vol) + pair;
    float4* cat = reinterpret_cast<float4*>(col) + 2 * pair;  // a voxel's colour word has the number of its voxel
    float4 q = *at;
    const double xa = tsdf_coord(g.o[0], i, g.vs), xb = tsdf_coord(g.o[0], i + 1, g.vs);
    const double y = tsdf_coord(g.o[1], j, g.vs), z = tsdf_coord(g.o[2], k, g.vs);
    const bool second = i + 1 < g.nx;
    const int64_t plane = static_cast<int64_t>(r.W) * r.H;
    bool ca = false, cb = false;
    float Ca[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Cb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool have_a = false, have_b = false;  // the word is in registers
    bool took_a = false, took_b = false;  // and step 7 changed it
    if (EAGER) {
        const float4 wa = cat[0], wb = cat[1];  // the padding voxel's word exists: rows are pitch words long
        Ca[0] = wa.x; Ca[1] = wa.y; Ca[2] = wa.z; Ca[3] = wa.w;
        Cb[0] = wb.x; Cb[1] = wb.y; Cb[2] = wb.z; Cb[3] = wb.w;
        have_a = have_b = true;
    }
#pragma unroll 1
    for (int m = 0; m < n_maps; ++m) {
        const double* map = depth + m * plane;
        const uint32_t* image = rgba + m * plane;
        int64_t px;
        double s;
        if (tsdf_update_at<MODEL>(*cam, poses[m], map, r, xa, y, z, &q.x, &q.y, &px, &s)) {
            ca = true;
            const uint32_t c = image[px];
            if (tsdf_colour_takes(s, r.trunc, c)) {
                if (!have_a) {
                    const float4 w = cat[0];
                    Ca[0] = w.x; Ca[1] = w.y; Ca[2] = w.z; Ca[3] = w.w;
                    have_a = true;
                }
                tsdf_colour_blend(Ca, c, r.max_weight);
                took_a = true;
            }
        }
        if (second && tsdf_update_at<MODEL>(*cam, poses[m], map, r, xb, y, z, &q.z, &q.w, &px, &s)) {
            cb = true;
            const uint32_t c = image[px];
            if (tsdf_colour_takes(s, r.trunc, c)) {
                if (!have_b) {
                    const float4 w = cat[1];
                    Cb[0] = w.x; Cb[1] = w.y; Cb[2] = w.z; Cb[3] = w.w;
                    have_b = true;
                }
                tsdf_colour_blend(Cb, c, r.max_weight);
                took_b = true;
            }
        }
    }
    if (ca && cb)
        *at = q;
    else if (ca)
        *reinterpret_cast<float2*>(at) = make_float2(q.x, q.y);
    else if (cb)
        *(reinterpret_cast<float2*>(at) + 1) = make_float2(q.z, q.w);
    if (took_a) cat[0] = make_float4(Ca[0], Ca[1], Ca[2], Ca[3]);
    if (took_b) cat[1] = make_float4(Cb[0], Cb[1], Cb[2], Cb[3]);
}

// TO_DENSE: tsdf [n], weight [n] <- the volume; else the volume <- the planes.  Either plane may be NULL.
template <bool TO_DENSE>
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_planes(TsdfGrid g, float* __restrict__ vol, float* __restrict__ tsdf, float* __restrict__ weight) {
    const int64_t n = static_cast<int64_t>(g.nx) * g.ny * g.nz;
    for (int64_t l = blockIdx.x * static_cast<int64_t>(TSDF_BLOCK) + threadIdx.x; l < n; l += static_cast<int64_t>(gridDim.x) * TSDF_BLOCK) {
        const int64_t row = l / g.nx;
        float* v = vol + 2 * (row * g.pitch + (l - row * g.nx));
        if (TO_DENSE) {
            if (tsdf) tsdf[l] = v[0];
            if (weight) weight[l] = v[1];
        } else {
            if (tsdf) v[0] = tsdf[l];
            if (weight) v[1] = weight[l];
        }
    }
}

// TO_DENSE: dense [n] <- the colour rows; else the colour rows <- dense: {R, G, B, Wc} records as they are
template <bool TO_DENSE>
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_colour_planes(TsdfGrid g, float4* __restrict__ col, float4* __restrict__ dense) {
    const int64_t n = static_cast<int64_t>(g.nx) * g.ny * g.nz;
    for (int64_t l = blockIdx.x * static_cast<int64_t>(TSDF_BLOCK) + threadIdx.x; l < n; l += static_cast<int64_t>(gridDim.x) * TSDF_BLOCK) {
        const int64_t row = l / g.nx;
        float4* v = col + (row * g.pitch + (l - row * g.nx));
        if (TO_DENSE)
            dense[l] = *v;
        else
            *v = dense[l];
    }
}

// PLACE false: count [tile] <- the tile's qualifying edges.  PLACE true: count holds the scanned starts; xyz, nrm [n_points][3] written.
// RECORD (with PLACE): rec [tiles * TSDF_EXTRACT_TILE / 64] written, one per wave and round.  COLOUR (with PLACE): rgba [n_points]
// written from the colour rows col.
template <bool PLACE, bool RECORD = false, bool COLOUR = false>
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_extract(TsdfGrid g, const float* __restrict__ vol, double min_weight, int32_t* __restrict__ count,
                                                             double* __restrict__ xyz, double* __restrict__ nrm, TsdfEdgeGroup* __restrict__ rec,
                                                             const float* __restrict__ col, uint32_t* __restrict__ rgba) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = static_cast<int64_t>(g.nx) * g.ny * g.nz;
    int32_t base = PLACE ? count[blockIdx.x] : 0;
#pragma unroll 1
    for (int round = 0; round < TSDF_EXTRACT_TILE / TSDF_BLOCK; ++round) {
        const int64_t l = static_cast<int64_t>(blockIdx.x) * TSDF_EXTRACT_TILE + round * TSDF_BLOCK + threadIdx.x;
        int i = 0, j = 0, k = 0, mask = 0;
        if (l < n) {
            tsdf_voxel_of(g, l, &i, &j, &k);
            mask = tsdf_edge_mask(vol, g, i, j, k, min_weight);
        }
        // every lane of the workgroup is here: the ballots and the barriers see all of them
        const uint64_t b0 = __ballot(mask & 1), b1 = __ballot(mask & 2), b2 = __ballot(mask & 4);
        const uint64_t below = (1ull << lane) - 1;
        int32_t before;
        const int32_t all = wave_counts_prefix(__popcll(b0) + __popcll(b1) + __popcll(b2), lane, wave, &before);
        if (RECORD && lane == 0) {  // l is a multiple of 64 here
            TsdfEdgeGroup r;
            r.ballot[0] = b0; r.ballot[1] = b1; r.ballot[2] = b2;
            r.start = base + before;
            r.pad = 0;
            rec[l / TSDF_MESH_GROUP] = r;
        }
        if (PLACE && mask) {
            int64_t at = base + before + __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below);
#pragma unroll
            for (int axis = 0; axis < 3; ++axis) {
                double Da, Db;
                if (!tsdf_edge(vol, g, i, j, k, axis, min_weight, &Da, &Db)) continue;
                double pt[3], nn[3];
                tsdf_edge_point(vol, g, i, j, k, axis, Da, Db, pt, nn);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xyz[3 * at + c] = pt[c];
                    nrm[3 * at + c] = nn[c];
                }
                if (COLOUR) rgba[at] = tsdf_colour_edge(col, g, i, j, k, axis, Da, Db);
                ++at;
            }
        }
        base += all;
    }
    if (!PLACE && threadIdx.x == 0) count[blockIdx.x] = base;
}

__constant__ TsdfMeshTable d_tsdf_mesh_table = TSDF_MESH_TABLE;

// PLACE false: count [tile] <- the triangles of the tile's cells.  PLACE true: count holds the scanned starts; tri [n_triangles][3]
// written from the records of the extract at the same min_weight.
template <bool PLACE>
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_mesh(TsdfGrid g, const float* __restrict__ vol, double min_weight,
                                                          const TsdfEdgeGroup* __restrict__ rec, int32_t* __restrict__ count, int32_t* __restrict__ tri) {
    __shared__ uint64_t table[256];
    table[threadIdx.x] = d_tsdf_mesh_table.w[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = static_cast<int64_t>(g.nx) * g.ny * g.nz;
    int32_t base = PLACE ? count[blockIdx.x] : 0;
#pragma unroll 1
    for (int round = 0; round < TSDF_EXTRACT_TILE / TSDF_BLOCK; ++round) {
        const int64_t l = static_cast<int64_t>(blockIdx.x) * TSDF_EXTRACT_TILE + round * TSDF_BLOCK + threadIdx.x;
        int i = 0, j = 0, k = 0, own = 0;
        bool rows = false;
        if (l < n) {
            tsdf_voxel_of(g, l, &i, &j, &k);
            rows = tsdf_mesh_has_rows(g, j, k);
            if (rows) own = tsdf_mesh_rows(vol, g, i, j, k, min_weight);
        }
        // every lane of the workgroup is here: the shuffle, the ballots and the barriers see all of them.  A cell's +x neighbour is the
        // next voxel of its row, so the next lane holds it, and has loaded it: it shares j and k.
        int next = __shfl_down(own, 1);
        const bool cell = rows && i + 1 < g.nx;
        if (cell && lane == 63) next = tsdf_mesh_rows(vol, g, i + 1, j, k, min_weight);
        uint64_t word = 0;
        if (cell && tsdf_mesh_live(own, next)) word = table[tsdf_mesh_case(own, next)];
        const int mine = tsdf_mesh_word_count(word);  // 0 .. 5: three bits
        const uint64_t c0 = __ballot(mine & 1), c1 = __ballot(mine & 2), c2 = __ballot(mine & 4);
        const uint64_t below = (1ull << lane) - 1;
        int32_t before;
        const int32_t all = wave_counts_prefix(__popcll(c0) + 2 * __popcll(c1) + 4 * __popcll(c2), lane, wave, &before);
        if (PLACE && mine) {
            int64_t at = base + before + __popcll(c0 & below) + 2 * __popcll(c1 & below) + 4 * __popcll(c2 & below);
#pragma unroll 1
            for (int t = 0; t < mine; ++t, ++at)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int e = tsdf_mesh_word_edge(word, 3 * t + c);
                    tri[3 * at + c] = tsdf_mesh_edge_index(rec, tsdf_mesh_edge_voxel(g, i, j, k, e), e >> 2);
                }
        }
        base += all;
    }
    if (!PLACE && threadIdx.x == 0) count[blockIdx.x] = base;
}

constexpr int TSDF_RAY_BLOCK = 256;  // four wavefronts, each with a block of pixels of its own
constexpr int TSDF_RAY_WAVE_W = 8;   // a wavefront's pixels are TSDF_RAY_WAVE_W x (64 / TSDF_RAY_WAVE_W)

// rays [H][W][2] <- ls_unproject(c, col, row)
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_rays(int H, int W, double* __restrict__ rays, LsCamera c) {
    const int64_t n = static_cast<int64_t>(H) * W;
    for (int64_t l = blockIdx.x * static_cast<int64_t>(TSDF_BLOCK) + threadIdx.x; l < n; l += static_cast<int64_t>(gridDim.x) * TSDF_BLOCK) {
        const int64_t row = l / W;
        double2 o;
        ls_unproject(c, static_cast<double>(l - row * W), static_cast<double>(row), &o.x, &o.y);
        reinterpret_cast<double2*>(rays)[l] = o;
    }
}

// BW: the width of a wavefront's pixel block (8: compact; 64: one row segment, instantiated by the experiment builds for the comparison)
template <int BW>
__global__ __launch_bounds__(TSDF_RAY_BLOCK) void k_tsdf_raycast(TsdfGrid g, const float* __restrict__ vol, const TsdfRayView* __restrict__ views,
                                                                 const double* __restrict__ rays, int n_views, int H, int W, TsdfRayRule r,
                                                                 double* __restrict__ depth, double* __restrict__ xyz, double* __restrict__ nrm,
                                                                 uint8_t* __restrict__ status) {
    constexpr int BH = 64 / BW;
    const int tiles_x = (W + BW - 1) / BW, tiles_y = (H + BH - 1) / BH;
    const int64_t tiles = static_cast<int64_t>(tiles_x) * tiles_y;
    const int64_t wave = blockIdx.x * static_cast<int64_t>(TSDF_RAY_BLOCK / 64) + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    if (wave >= tiles * n_views) return;
    const int view = static_cast<int>(wave / tiles);  // wave-uniform: the view is read with scalar loads
    const int tile = static_cast<int>(wave - view * tiles);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int lane = threadIdx.x & 63;
    const int col = tx * BW + lane % BW, row = ty * BH + lane / BW;
    if (col >= W || row >= H) return;
    const int64_t px = static_cast<int64_t>(row) * W + col;
    const double2 ray = reinterpret_cast<const double2*>(rays)[px];
    TsdfRayOut o;
    tsdf_ray_pixel(vol, g, views[view], r, ray.x, ray.y, &o);
    const int64_t at = static_cast<int64_t>(view) * H * W + px;
    depth[at] = o.depth;  // NaN unless the ray hit, and then NaN times the ray is NaN
    xyz[3 * at] = ray.x * o.depth;
    xyz[3 * at + 1] = ray.y * o.depth;
    xyz[3 * at + 2] = o.depth;
#pragma unroll
    for (int c = 0; c < 3; ++c) nrm[3 * at + c] = o.nrm[c];
    status[at] = static_cast<uint8_t>(o.status);
}

// rgba [n_views][H][W] <- tsdf_colour_hit of the stored outputs of k_tsdf_raycast
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_raycast_colour(TsdfGrid g, const float* __restrict__ col, const TsdfRayView* __restrict__ views,
                                                                    const double* __restrict__ rays, int64_t plane, int64_t n_px,
                                                                    const double* __restrict__ depth, const uint8_t* __restrict__ status,
                                                                    uint32_t* __restrict__ rgba) {
    const int64_t at = blockIdx.x * static_cast<int64_t>(TSDF_BLOCK) + threadIdx.x;
    if (at >= n_px) return;
    const int64_t view = at / plane;
    const double2 ray = reinterpret_cast<const double2*>(rays)[at - view * plane];
    rgba[at] = tsdf_colour_hit(col, g, views[view], status[at], depth[at], ray.x, ray.y);
}

struct TsdfVolume : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    TsdfGrid g{};
    cba_tsdf_options o{};
    int64_t n_voxels = 0, n_stored = 0, n_tiles = 0;
    int64_t n_points = -1;     // of the last extract; -1: none yet
    int64_t n_triangles = -1;  // of the handle's mesh; -1: there is none (no mesh call yet, or a later call made it stale)
    DevBuf<float> vol;         // [nz][ny][pitch][2]
    DevBuf<float> planes;      // [2][n_voxels]: the staging of fetch and upload
    DevBuf<TsdfCam> cam;
    DevBuf<TsdfPose> poses;
    DevBuf<double> depth;
    DevBuf<int32_t> count, tmp;  // [n_tiles + 1] and the scan's levels
    DevBuf<double> xyz, nrm;     // [n_points][3] of the last extract
    DevBuf<TsdfEdgeGroup> rec;   // [n_tiles * TSDF_EXTRACT_TILE / 64], from the first mesh call on
    DevBuf<int32_t> tcount;      // [n_tiles + 1] triangles per tile, from the first mesh call on
    DevBuf<int32_t> tri;         // [n_triangles][3] of the mesh
    PinnedBuf<int32_t> total_h;
    // the last ray cast: ray_views < 0: none yet
    int64_t ray_views = -1;
    int ray_H = 0, ray_W = 0;
    DevBuf<TsdfRayView> views;       // [ray_views]
    DevBuf<double> rays;             // [ray_H][ray_W][2]
    DevBuf<double> rdepth, rxyz, rnrm;  // [ray_views][ray_H][ray_W] ([3])
    DevBuf<uint8_t> rstatus;
    // colour: nothing below is allocated before the first cba_tsdf_integrate_colour or cba_tsdf_colour_upload
    bool has_colour = false;
    DevBuf<float> col;        // [nz][ny][pitch][4], zeros at first
    DevBuf<float> cplanes;    // [n_voxels][4]: the staging of the colour fetch and upload
    DevBuf<uint32_t> image;   // [n_maps][H][W] of a call
    DevBuf<uint32_t> prgba;   // [n_points] of the last extract, when it ran with colour
    DevBuf<uint32_t> rrgba;   // [ray_views][ray_H][ray_W] of the last ray cast, when it ran with colour
    bool points_coloured = false, rays_coloured = false;
};
static_assert(!std::is_copy_constructible_v<TsdfVolume> && !std::is_copy_assignable_v<TsdfVolume>, "a handle owns its stream and buffers");

static void tsdf_fill(TsdfVolume* h, hipStream_t s) {
    hipLaunchKernelGGL(k_tsdf_fill, dim3(launch_grid(h->n_stored, TSDF_BLOCK, TSDF_GRID)), dim3(TSDF_BLOCK), 0, s, h->n_stored,
                       reinterpret_cast<float2*>(h->vol.p));
    CBA_HIP(hipGetLastError());
}

TsdfVolume* tsdf_volume_create(int nx, int ny, int nz, const double* origin, const cba_tsdf_options& o, int device) {
    auto h = std::make_unique<TsdfVolume>(device);
    const hipStream_t s = h->begin();
    h->g.nx = nx; h->g.ny = ny; h->g.nz = nz; h->g.pitch = (nx + 1) & ~1;
    for (int c = 0; c < 3; ++c) h->g.o[c] = origin[c];
    h->g.vs = o.voxel_size;
    h->o = o;
    h->n_voxels = static_cast<int64_t>(nx) * ny * nz;
    h->n_stored = static_cast<int64_t>(h->g.pitch) * ny * nz;
    h->n_tiles = (h->n_voxels + TSDF_EXTRACT_TILE - 1) / TSDF_EXTRACT_TILE;
    h->vol.alloc(2 * static_cast<size_t>(h->n_stored));
    h->cam.alloc(1);
    h->count.alloc(static_cast<size_t>(h->n_tiles) + 1);
    h->tmp.alloc(scan_tmp_size(h->n_tiles + 1));
    h->total_h.reserve(1);
    tsdf_fill(h.get(), s);
    CBA_HIP(hipStreamSynchronize(s));
    return h.release();
}

void tsdf_volume_reset(TsdfVolume* h) {
    const hipStream_t s = h->begin();
    h->n_triangles = -1;
    tsdf_fill(h, s);
    if (h->has_colour) h->col.zero(s);
    CBA_HIP(hipStreamSynchronize(s));
}

// The colour volume of a handle that has none yet, all zeros.  An allocation failure throws with the handle as it was: without colour.
static void tsdf_colour_ensure(TsdfVolume* h, hipStream_t s) {
    if (h->has_colour) return;
    h->col.alloc(4 * static_cast<size_t>(h->n_stored));
    h->col.zero(s);
    h->has_colour = true;
}

bool tsdf_volume_has_colour(const TsdfVolume* h) { return h->has_colour; }
bool tsdf_volume_points_coloured(const TsdfVolume* h) { return h->points_coloured; }
bool tsdf_volume_rays_coloured(const TsdfVolume* h) { return h->rays_coloured; }

int64_t tsdf_volume_points(const TsdfVolume* h) { return h->n_points; }
double tsdf_volume_voxel_size(const TsdfVolume* h) { return h->g.vs; }
int64_t tsdf_volume_triangles(const TsdfVolume* h) { return h->n_triangles; }

// rgba: uint8 [n_maps][H][W][4] for cba_tsdf_integrate_colour (the first such call allocates the colour volume), NULL for
// cba_tsdf_integrate.  eager: the experiment builds' kernel that loads every colour word.  stage_ms [2] optional: upload, kernel
void tsdf_volume_integrate(TsdfVolume* h, int model, const double* intr, int n_maps, int H, int W, const double* depth, const uint8_t* rgba,
                           const double* c_T_v, bool eager, double* stage_ms) {
    const hipStream_t s = h->begin();
    h->n_triangles = -1;
    TsdfCam cam;
    double intr12[12];
    ls_fill_intr(model, intr, intr12, cam.sd);
    for (int k = 0; k < 12; ++k) cam.intr[k] = intr12[k];
    std::vector<TsdfPose> poses(static_cast<size_t>(n_maps));
    for (int m = 0; m < n_maps; ++m) {
        quat_to_rotmat(c_T_v + 7 * static_cast<size_t>(m), poses[m].R);
        for (int c = 0; c < 3; ++c) poses[m].t[c] = c_T_v[7 * static_cast<size_t>(m) + 4 + c];
    }
    const size_t n_px = static_cast<size_t>(n_maps) * H * W;
    StageTimer<3> tm(s, stage_ms != nullptr);
    h->poses.ensure(static_cast<size_t>(n_maps));
    h->depth.ensure(n_px);
    if (rgba) {
        h->image.ensure(n_px);
        tsdf_colour_ensure(h, s);  // last: a buffer that could not grow leaves the handle without colour, as it was
    }
    tm.mark(0);
    h->cam.upload(&cam, 1, s);
    h->poses.upload(poses.data(), static_cast<size_t>(n_maps), s);
    h->depth.upload(depth, n_px, s);
    if (rgba) h->image.upload(reinterpret_cast<const uint32_t*>(rgba), n_px, s);  // hipMemcpyAsync takes any alignment
    tm.mark(1);
    TsdfRule r;
    r.trunc = h->o.truncation; r.max_depth = h->o.max_depth; r.max_weight = h->o.max_weight; r.W = W; r.H = H;
    const dim3 grid(static_cast<unsigned>((h->n_stored / 2 + TSDF_BLOCK - 1) / TSDF_BLOCK));
    if (!rgba)
        hipLaunchKernelGGL(model == CAM_SCHEIMPFLUG ? k_tsdf_integrate<CAM_SCHEIMPFLUG> : k_tsdf_integrate<CAM_PINHOLE_BC>, grid, dim3(TSDF_BLOCK), 0, s,
                           h->g, h->cam.p, h->poses.p, h->depth.p, n_maps, r, h->vol.p);
#ifdef CBA_EXPERIMENTS
    else if (eager)
        hipLaunchKernelGGL((model == CAM_SCHEIMPFLUG ? k_tsdf_integrate_colour<CAM_SCHEIMPFLUG, true> : k_tsdf_integrate_colour<CAM_PINHOLE_BC, true>), grid,
                           dim3(TSDF_BLOCK), 0, s, h->g, h->cam.p, h->poses.p, h->depth.p, h->image.p, n_maps, r, h->vol.p, h->col.p);
#endif
    else
        hipLaunchKernelGGL((model == CAM_SCHEIMPFLUG ? k_tsdf_integrate_colour<CAM_SCHEIMPFLUG> : k_tsdf_integrate_colour<CAM_PINHOLE_BC>), grid,
                           dim3(TSDF_BLOCK), 0, s, h->g, h->cam.p, h->poses.p, h->depth.p, h->image.p, n_maps, r, h->vol.p, h->col.p);
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    CBA_HIP(hipStreamSynchronize(s));  // cam and poses go out of scope
    tm.report(stage_ms);
}

static void tsdf_planes(TsdfVolume* h, hipStream_t s, bool to_dense, float* tsdf, float* weight) {
    const dim3 grid(launch_grid(h->n_voxels, TSDF_BLOCK, TSDF_GRID));
    hipLaunchKernelGGL(to_dense ? k_tsdf_planes<true> : k_tsdf_planes<false>, grid, dim3(TSDF_BLOCK), 0, s, h->g, h->vol.p, tsdf, weight);
    CBA_HIP(hipGetLastError());
}

void tsdf_volume_fetch(TsdfVolume* h, float* tsdf, float* weight) {
    const hipStream_t s = h->begin();
    const size_t n = static_cast<size_t>(h->n_voxels);
    h->planes.ensure(2 * n);
    tsdf_planes(h, s, true, tsdf ? h->planes.p : nullptr, weight ? h->planes.p + n : nullptr);
    if (tsdf) h->planes.download(tsdf, n, s);
    if (weight) h->planes.download(weight, n, s, n);
    CBA_HIP(hipStreamSynchronize(s));
}

void tsdf_volume_upload(TsdfVolume* h, const float* tsdf, const float* weight) {
    const hipStream_t s = h->begin();
    h->n_triangles = -1;
    const size_t n = static_cast<size_t>(h->n_voxels);
    h->planes.ensure(2 * n);
    if (tsdf) h->planes.upload(tsdf, n, s);
    if (weight) h->planes.upload(weight, n, s, n);
    tsdf_planes(h, s, false, tsdf ? h->planes.p : nullptr, weight ? h->planes.p + n : nullptr);
    CBA_HIP(hipStreamSynchronize(s));
}

static void tsdf_colour_planes(TsdfVolume* h, hipStream_t s, bool to_dense) {
    const dim3 grid(launch_grid(h->n_voxels, TSDF_BLOCK, TSDF_GRID));
    hipLaunchKernelGGL(to_dense ? k_tsdf_colour_planes<true> : k_tsdf_colour_planes<false>, grid, dim3(TSDF_BLOCK), 0, s, h->g,
                       reinterpret_cast<float4*>(h->col.p), reinterpret_cast<float4*>(h->cplanes.p));
    CBA_HIP(hipGetLastError());
}

// colour [nz][ny][nx][4]; the handle has colour (checked by the caller)
void tsdf_volume_colour_fetch(TsdfVolume* h, float* colour) {
    const hipStream_t s = h->begin();
    const size_t n = 4 * static_cast<size_t>(h->n_voxels);
    h->cplanes.ensure(n);
    tsdf_colour_planes(h, s, true);
    h->cplanes.download(colour, n, s);
    CBA_HIP(hipStreamSynchronize(s));
}

void tsdf_volume_colour_upload(TsdfVolume* h, const float* colour) {
    const hipStream_t s = h->begin();
    h->n_triangles = -1;
    const size_t n = 4 * static_cast<size_t>(h->n_voxels);
    h->cplanes.ensure(n);
    tsdf_colour_ensure(h, s);  // after the staging: an allocation failure leaves the handle without colour, as it was
    h->cplanes.upload(colour, n, s);
    tsdf_colour_planes(h, s, false);
    CBA_HIP(hipStreamSynchronize(s));
}

// The extract on s, ending synchronised; tm marks 0, 1, 2 around count and scan, and place.  record: the place pass also writes h->rec.
template <class Timer>
static int64_t tsdf_extract_run(TsdfVolume* h, hipStream_t s, double min_weight, bool record, Timer& tm) {
    const dim3 grid(static_cast<unsigned>(h->n_tiles));
    tm.mark(0);
    hipLaunchKernelGGL((k_tsdf_extract<false>), grid, dim3(TSDF_BLOCK), 0, s, h->g, h->vol.p, min_weight, h->count.p, nullptr, nullptr, nullptr, nullptr,
                       nullptr);
    const int64_t total = scan_counts(s, h->count.p, h->n_tiles, h->tmp.p, h->total_h.p);
    tm.mark(1);
    h->n_points = -1;
    h->points_coloured = false;
    const bool colour = h->has_colour;  // a handle without colour launches what it always has
    if (total > 0) {
        h->xyz.ensure(3 * static_cast<size_t>(total));
        h->nrm.ensure(3 * static_cast<size_t>(total));
        if (colour) {
            h->prgba.ensure(static_cast<size_t>(total));
            hipLaunchKernelGGL((record ? k_tsdf_extract<true, true, true> : k_tsdf_extract<true, false, true>), grid, dim3(TSDF_BLOCK), 0, s, h->g,
                               h->vol.p, min_weight, h->count.p, h->xyz.p, h->nrm.p, record ? h->rec.p : nullptr, h->col.p, h->prgba.p);
        } else {
            hipLaunchKernelGGL((record ? k_tsdf_extract<true, true> : k_tsdf_extract<true, false>), grid, dim3(TSDF_BLOCK), 0, s, h->g, h->vol.p,
                               min_weight, h->count.p, h->xyz.p, h->nrm.p, record ? h->rec.p : nullptr, nullptr, nullptr);
        }
        CBA_HIP(hipGetLastError());
    }
    tm.mark(2);
    CBA_HIP(hipStreamSynchronize(s));
    h->n_points = total;
    h->points_coloured = colour;
    return total;
}

// stage_ms [2] optional: count and scan, place
void tsdf_volume_extract(TsdfVolume* h, double min_weight, int64_t* n_points, double* stage_ms) {
    const hipStream_t s = h->begin();
    h->n_triangles = -1;
    StageTimer<3> tm(s, stage_ms != nullptr);
    *n_points = tsdf_extract_run(h, s, min_weight, false, tm);
    tm.report(stage_ms);
}

// stage_ms [4] optional: the extract's count and scan, its place with the records, the triangles' count and scan, their place
void tsdf_volume_mesh(TsdfVolume* h, double min_weight, int64_t* n_points, int64_t* n_triangles, double* stage_ms) {
    const hipStream_t s = h->begin();
    h->n_triangles = -1;
    StageTimer<5> tm(s, stage_ms != nullptr);
    h->rec.ensure(static_cast<size_t>(h->n_tiles) * (TSDF_EXTRACT_TILE / TSDF_MESH_GROUP));
    h->tcount.ensure(static_cast<size_t>(h->n_tiles) + 1);
    const int64_t points = tsdf_extract_run(h, s, min_weight, true, tm);
    int64_t total = 0;
    if (points > 0) {  // a triangle needs three points, and only then were the records written
        const dim3 grid(static_cast<unsigned>(h->n_tiles));
        hipLaunchKernelGGL(k_tsdf_mesh<false>, grid, dim3(TSDF_BLOCK), 0, s, h->g, h->vol.p, min_weight, h->rec.p, h->tcount.p, nullptr);
        total = scan_counts(s, h->tcount.p, h->n_tiles, h->tmp.p, h->total_h.p);
        tm.mark(3);
        if (total > 0) {
            h->tri.ensure(3 * static_cast<size_t>(total));
            hipLaunchKernelGGL(k_tsdf_mesh<true>, grid, dim3(TSDF_BLOCK), 0, s, h->g, h->vol.p, min_weight, h->rec.p, h->tcount.p, h->tri.p);
            CBA_HIP(hipGetLastError());
        }
        tm.mark(4);
        CBA_HIP(hipStreamSynchronize(s));
    }
    h->n_triangles = total;
    *n_points = points;
    *n_triangles = total;
    tm.report(stage_ms);
}

void tsdf_volume_mesh_fetch(TsdfVolume* h, int32_t* triangles) {
    const hipStream_t s = h->begin();
    h->tri.download(triangles, 3 * static_cast<size_t>(h->n_triangles), s);
    CBA_HIP(hipStreamSynchronize(s));
}

// rgba uint8 [n_points][4]; the last extract ran with colour and gave points (checked by the caller)
void tsdf_volume_extract_fetch_colour(TsdfVolume* h, uint8_t* rgba) {
    const hipStream_t s = h->begin();
    h->prgba.download(reinterpret_cast<uint32_t*>(rgba), static_cast<size_t>(h->n_points), s);
    CBA_HIP(hipStreamSynchronize(s));
}

void tsdf_volume_extract_fetch(TsdfVolume* h, double* xyz, double* normals) {
    const hipStream_t s = h->begin();
    const size_t n = 3 * static_cast<size_t>(h->n_points);
    h->xyz.download(xyz, n, s);
    if (normals) h->nrm.download(normals, n, s);
    CBA_HIP(hipStreamSynchronize(s));
}

int64_t tsdf_volume_ray_views(const TsdfVolume* h) { return h->ray_views; }

// The ray cast reads the volume and writes only its own buffers: the extract's points and the mesh stay as they are.
// wave_w: TSDF_RAY_WAVE_W; the experiment builds also take 64 for the comparison.  stage_ms [2] optional: upload and the rays table, the cast;
// colour_ms optional, with stage_ms: the colour pass (0 on a handle without colour)
void tsdf_volume_raycast(TsdfVolume* h, int model, const double* intr, int n_views, int H, int W, const double* c_T_v,
                         const cba_tsdf_raycast_options& o, int wave_w, double* stage_ms, double* colour_ms) {
    const hipStream_t s = h->begin();
    LsCamera cam;
    ls_fill_camera(model, intr, 0, nullptr, &cam);
    std::vector<TsdfRayView> views(static_cast<size_t>(n_views));
    for (int m = 0; m < n_views; ++m) tsdf_ray_view(c_T_v + 7 * static_cast<size_t>(m), &views[m]);
    TsdfRayRule r;
    r.step = o.step > 0.0 ? o.step : 0.5 * h->g.vs;
    r.skip = o.skip; r.near_depth = o.near_depth; r.far_depth = o.far_depth; r.min_weight = o.min_weight; r.trunc = h->o.truncation;
    const size_t plane = static_cast<size_t>(H) * W, n_px = plane * n_views;
    StageTimer<4> tm(s, stage_ms != nullptr);
    h->ray_views = -1;  // a buffer that grows loses its contents: an allocation failure leaves the handle without a ray cast
    h->views.ensure(static_cast<size_t>(n_views));
    h->rays.ensure(2 * plane);
    h->rdepth.ensure(n_px);
    h->rxyz.ensure(3 * n_px);
    h->rnrm.ensure(3 * n_px);
    h->rstatus.ensure(n_px);
    const bool colour = h->has_colour;
    h->rays_coloured = false;
    if (colour) h->rrgba.ensure(n_px);
    tm.mark(0);
    h->views.upload(views.data(), static_cast<size_t>(n_views), s);
    hipLaunchKernelGGL(k_tsdf_rays, dim3(launch_grid(static_cast<int64_t>(plane), TSDF_BLOCK, TSDF_GRID)), dim3(TSDF_BLOCK), 0, s, H, W, h->rays.p, cam);
    CBA_HIP(hipGetLastError());
    tm.mark(1);
    const int wave_h = 64 / wave_w;
    const int64_t waves = static_cast<int64_t>((W + wave_w - 1) / wave_w) * ((H + wave_h - 1) / wave_h) * n_views;
    const dim3 grid(static_cast<unsigned>((waves + TSDF_RAY_BLOCK / 64 - 1) / (TSDF_RAY_BLOCK / 64)));
#ifdef CBA_EXPERIMENTS
    if (wave_w == 64)
        hipLaunchKernelGGL(k_tsdf_raycast<64>, grid, dim3(TSDF_RAY_BLOCK), 0, s, h->g, h->vol.p, h->views.p, h->rays.p, n_views, H, W, r, h->rdepth.p,
                           h->rxyz.p, h->rnrm.p, h->rstatus.p);
    else
#endif
        hipLaunchKernelGGL(k_tsdf_raycast<TSDF_RAY_WAVE_W>, grid, dim3(TSDF_RAY_BLOCK), 0, s, h->g, h->vol.p, h->views.p, h->rays.p, n_views, H, W, r,
                           h->rdepth.p, h->rxyz.p, h->rnrm.p, h->rstatus.p);
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    if (colour) {  // a function of the cast's stored outputs and the colour volume alone: a pass of its own is exact
        hipLaunchKernelGGL(k_tsdf_raycast_colour, dim3(static_cast<unsigned>((n_px + TSDF_BLOCK - 1) / TSDF_BLOCK)), dim3(TSDF_BLOCK), 0, s, h->g, h->col.p,
                           h->views.p, h->rays.p, static_cast<int64_t>(plane), static_cast<int64_t>(n_px), h->rdepth.p, h->rstatus.p, h->rrgba.p);
        CBA_HIP(hipGetLastError());
    }
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));  // views goes out of scope
    h->rays_coloured = colour;
    h->ray_views = n_views;
    h->ray_H = H;
    h->ray_W = W;
    if (stage_ms) {
        stage_ms[0] = tm.ms(0, 1);
        stage_ms[1] = tm.ms(1, 2);
        if (colour_ms) *colour_ms = tm.ms(2, 3);
    }
}

// each pointer may be NULL
void tsdf_volume_raycast_fetch(TsdfVolume* h, double* depth, double* xyz, double* normals, uint8_t* status, double* rays) {
    const hipStream_t s = h->begin();
    const size_t plane = static_cast<size_t>(h->ray_H) * h->ray_W, n = plane * static_cast<size_t>(h->ray_views);
    if (depth) h->rdepth.download(depth, n, s);
    if (xyz) h->rxyz.download(xyz, 3 * n, s);
    if (normals) h->rnrm.download(normals, 3 * n, s);
    if (status) h->rstatus.download(status, n, s);
    if (rays) h->rays.download(rays, 2 * plane, s);
    CBA_HIP(hipStreamSynchronize(s));
}

// rgba uint8 [ray_views][ray_H][ray_W][4]; the last ray cast ran with colour (checked by the caller)
void tsdf_volume_raycast_fetch_colour(TsdfVolume* h, uint8_t* rgba) {
    const hipStream_t s = h->begin();
    h->rrgba.download(reinterpret_cast<uint32_t*>(rgba), static_cast<size_t>(h->ray_H) * h->ray_W * static_cast<size_t>(h->ray_views), s);
    CBA_HIP(hipStreamSynchronize(s));
}

void tsdf_volume_destroy(TsdfVolume* h) noexcept { destroy_handle(h); }

}  // namespace cba
