// tsdf_mesh_math.hpp — scan meshing (calibba.h: cba_tsdf_mesh, item 4 of the scan-fusion block) as __host__ __device__ code: the table of
// triangles per sign pattern, generated from the rule at compile time, and what one cell needs: the sign and weight bits of its corners,
// its case, whether it is live, the voxel and axis of a local edge, and the place of that edge in the extract's point list.  The kernels
// of tsdf_fusion.hip call it per lane; tests/mesh_cpu compiles the same header with g++.  No table is typed in: tsdf_mesh_case_word is
// the only copy of the rule, and every output is an integer.
//
//   corners   q = dx + 2 dy + 4 dz at lattice point (i + dx, j + dy, k + dz)
//   edges     e = 4 axis + u + 2 v, (u, v) the offsets of the lower end along the other two axes in ascending axis order
//   a word    TSDF_MESH_SLOTS four-bit edge numbers, three per triangle, slot s in bits [4 s, 4 s + 4); the triangle count in bits 60-63
//   a record  per aligned group of 64 consecutive l (one wave of the extract): the place of its first point and the three ballots of
//             its qualifying +x, +y, +z edges; an edge's place follows from popcounts (tsdf_mesh_edge_index), one 32-byte load
#pragma once
#include <cstdint>

#include "tsdf_math.hpp"

namespace cba {

constexpr int TSDF_MESH_SLOTS = 15;  // edge numbers per word: five triangles at most
constexpr int TSDF_MESH_GROUP = 64;  // consecutive l per record: the lanes of a wave

struct TsdfMeshTable {
    uint64_t w[256];
};

struct alignas(32) TsdfEdgeGroup {
    uint64_t ballot[3];  // bit lane: voxel (group 64 + lane) has a qualifying edge along +axis
    int32_t start;       // the place of the group's first point
    int32_t pad;
};
static_assert(sizeof(TsdfEdgeGroup) == 32, "one 32-byte load per lookup");

// ---- the rule -----------------------------------------------------------------------------------------------------------------------
// the local edge between two corners that differ along one axis
constexpr int tsdf_mesh_edge_between(int p, int q) {
    const int d = p ^ q, lo = p & q;
    const int axis = d == 1 ? 0 : (d == 2 ? 1 : 2);
    const int first = axis == 0 ? 1 : 0, second = axis == 2 ? 1 : 2;  // the other two axes, ascending
    return 4 * axis + ((lo >> first) & 1) + 2 * ((lo >> second) & 1);
}

// corner p = 0..3 of the cycle of the face across axis a on side s: (b, c) = (0,0), (1,0), (1,1), (0,1) with b = a + 1, c = a + 2 (mod 3),
// counter-clockwise seen from outside for s = 1, reversed for s = 0
constexpr int tsdf_mesh_face_corner(int a, int s, int p) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    const int at = s ? (p & 3) : ((4 - p) & 3);
    const int ub = (at == 1 || at == 2) ? 1 : 0, uc = at >= 2 ? 1 : 0;
    return (s << a) | (ub << b) | (uc << c);
}

// the word of one sign pattern (bit q: corner q is negative)
constexpr uint64_t tsdf_mesh_case_word(int pattern) {
    int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    for (int a = 0; a < 3; ++a)
        for (int s = 0; s < 2; ++s)
            for (int p = 0; p < 4; ++p) {
                const int c0 = tsdf_mesh_face_corner(a, s, p), c1 = tsdf_mesh_face_corner(a, s, p + 1);
                if (((pattern >> c0) & 1) || !((pattern >> c1) & 1)) continue;  // the cycle enters a run of negative corners here
                int r = p + 1;                                                   // c0 is positive: the run ends before it comes round
                while ((pattern >> tsdf_mesh_face_corner(a, s, r + 1)) & 1) ++r;
                next[tsdf_mesh_edge_between(c0, c1)] = tsdf_mesh_edge_between(tsdf_mesh_face_corner(a, s, r), tsdf_mesh_face_corner(a, s, r + 1));
            }
    bool done[12] = {false, false, false, false, false, false, false, false, false, false, false, false};
    uint64_t word = 0;
    int slots = 0;
    for (int e0 = 0; e0 < 12; ++e0) {
        if (next[e0] < 0 || done[e0]) continue;
        done[e0] = true;
        int prev = next[e0];
        done[prev] = true;
        for (int cur = next[prev]; cur != e0; prev = cur, cur = next[cur]) {  // the fan (e0, e_i, e_i+1)
            done[cur] = true;
            word |= static_cast<uint64_t>(e0) << (4 * slots) | static_cast<uint64_t>(prev) << (4 * slots + 4) |
                    static_cast<uint64_t>(cur) << (4 * slots + 8);
            slots += 3;
        }
    }
    return word | static_cast<uint64_t>(slots / 3) << 60;
}

constexpr TsdfMeshTable tsdf_mesh_make_table() {
    TsdfMeshTable t{};
    for (int c = 0; c < 256; ++c) t.w[c] = tsdf_mesh_case_word(c);
    return t;
}
inline constexpr TsdfMeshTable TSDF_MESH_TABLE = tsdf_mesh_make_table();  // 2 KiB
static_assert(TSDF_MESH_TABLE.w[0] == 0 && TSDF_MESH_TABLE.w[255] == 0, "cases 0 and 255 give nothing");
static_assert(TSDF_MESH_TABLE.w[1] == (1ull << 60 | 0x840ull), "case 1 is (0, 4, 8)");

CBA_HD int tsdf_mesh_word_count(uint64_t word) { return static_cast<int>(word >> 60); }
CBA_HD int tsdf_mesh_word_edge(uint64_t word, int slot) { return static_cast<int>(word >> (4 * slot)) & 15; }

// ---- one cell ---------------------------------------------------------------------------------------------------------------------------
// whether voxel (i, j, k) has the rows (j, k), (j + 1, k), (j, k + 1), (j + 1, k + 1), and whether it is corner 0 of a cell
CBA_HD bool tsdf_mesh_has_rows(const TsdfGrid& g, int j, int k) { return j + 1 < g.ny && k + 1 < g.nz; }
CBA_HD bool tsdf_mesh_has_cell(const TsdfGrid& g, int i, int j, int k) { return i + 1 < g.nx && tsdf_mesh_has_rows(g, j, k); }

// The bits of the voxels (i, j + dy, k + dz), r = dy + 2 dz: bit r = (D < 0), bit 4 + r = (W >= min_weight).  Needs tsdf_mesh_has_rows.
CBA_HD int tsdf_mesh_rows(const float* vol, const TsdfGrid& g, int i, int j, int k, double min_weight) {
    int bits = 0;
    for (int r = 0; r < 4; ++r) {
        const float* v = vol + tsdf_at(g, i, j + (r & 1), k + (r >> 1));
        bits |= (static_cast<double>(v[0]) < 0.0 ? 1 : 0) << r;
        bits |= (static_cast<double>(v[1]) >= min_weight ? 1 : 0) << (4 + r);
    }
    return bits;
}

// own: tsdf_mesh_rows of corner 0's voxel, next: of its +x neighbour's
CBA_HD bool tsdf_mesh_live(int own, int next) { return ((own & next) >> 4) == 15; }
CBA_HD int tsdf_mesh_case(int own, int next) {
    int c = 0;
    for (int r = 0; r < 4; ++r) c |= ((own >> r) & 1) << (2 * r) | ((next >> r) & 1) << (2 * r + 1);
    return c;
}

// the dense l of the voxel at the lower end of local edge e of cell (i, j, k); the edge's axis is e >> 2
CBA_HD int64_t tsdf_mesh_edge_voxel(const TsdfGrid& g, int i, int j, int k, int e) {
    const int axis = e >> 2, u = e & 1, v = (e >> 1) & 1;
    const int di = axis == 0 ? 0 : u, dj = axis == 0 ? u : (axis == 1 ? 0 : v), dk = axis == 2 ? 0 : v;
    return (static_cast<int64_t>(k + dk) * g.ny + (j + dj)) * g.nx + (i + di);
}

// The place in the extract's point list of the qualifying edge from voxel l along +axis: the group's start, the points of the lanes
// below, the lower axes of the voxel itself.
CBA_HD int32_t tsdf_mesh_edge_index(const TsdfEdgeGroup* rec, int64_t l, int axis) {
    const TsdfEdgeGroup r = rec[l / TSDF_MESH_GROUP];
    const int lane = static_cast<int>(l % TSDF_MESH_GROUP);
    const uint64_t below = (1ull << lane) - 1;
    int32_t at = r.start + __builtin_popcountll(r.ballot[0] & below) + __builtin_popcountll(r.ballot[1] & below) +
                 __builtin_popcountll(r.ballot[2] & below);
    if (axis > 0) at += static_cast<int32_t>((r.ballot[0] >> lane) & 1);
    if (axis > 1) at += static_cast<int32_t>((r.ballot[1] >> lane) & 1);
    return at;
}

}  // namespace cba
