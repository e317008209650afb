// mesh_driver.cpp — TEST-ONLY: extern "C" wrapper of tsdf_mesh_math.hpp for ctypes (tests/test_mesh_cpu.py).  The volume is kept as the
// device keeps it ({D, W} pairs in rows of an even pitch); the edge records are built per group of 64 voxels as the extract's waves
// build them, and the cells are walked in ascending l with the functions every lane runs.  Built with -DCBA_HOST_DRIVER_MAIN it is a
// stand-alone program (for the sanitizers): it checks the table's counts and named cases, meshes a sphere and a volume whose rows
// straddle the groups, and checks that every index is a point and every directed edge of the closed sphere has its reverse.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "../../calibration_amd/csrc/tsdf_mesh_math.hpp"
#include "../host_volume.hpp"

using namespace cba;

// the records of every group, as k_tsdf_extract's waves write them -> the number of points
static int64_t host_records(const HostVolume& v, double min_weight, std::vector<TsdfEdgeGroup>& rec) {
    const int64_t n = static_cast<int64_t>(v.g.nx) * v.g.ny * v.g.nz;
    rec.assign(static_cast<size_t>((n + TSDF_MESH_GROUP - 1) / TSDF_MESH_GROUP), TsdfEdgeGroup{});
    int64_t at = 0;
    for (int64_t l = 0; l < n; ++l) {
        TsdfEdgeGroup& r = rec[static_cast<size_t>(l / TSDF_MESH_GROUP)];
        if (l % TSDF_MESH_GROUP == 0) r.start = static_cast<int32_t>(at);
        int i, j, k;
        tsdf_voxel_of(v.g, l, &i, &j, &k);
        const int mask = tsdf_edge_mask(v.vol.data(), v.g, i, j, k, min_weight);
        for (int axis = 0; axis < 3; ++axis)
            if (mask >> axis & 1) {
                r.ballot[axis] |= 1ull << (l % TSDF_MESH_GROUP);
                ++at;
            }
    }
    return at;
}

// -> the number of triangles; the first `cap` of them written
static int64_t host_triangles(const HostVolume& v, double min_weight, int64_t* n_points, int64_t cap, int32_t* tri) {
    std::vector<TsdfEdgeGroup> rec;
    *n_points = host_records(v, min_weight, rec);
    int64_t m = 0;
    for (int k = 0; k < v.g.nz; ++k)
        for (int j = 0; j < v.g.ny; ++j)
            for (int i = 0; i < v.g.nx; ++i) {
                if (!tsdf_mesh_has_cell(v.g, i, j, k)) continue;
                const int own = tsdf_mesh_rows(v.vol.data(), v.g, i, j, k, min_weight), next = tsdf_mesh_rows(v.vol.data(), v.g, i + 1, j, k, min_weight);
                if (!tsdf_mesh_live(own, next)) continue;
                const uint64_t word = TSDF_MESH_TABLE.w[tsdf_mesh_case(own, next)];
                for (int t = 0; t < tsdf_mesh_word_count(word); ++t, ++m) {
                    if (m >= cap) continue;
                    for (int c = 0; c < 3; ++c) {
                        const int e = tsdf_mesh_word_edge(word, 3 * t + c);
                        tri[3 * m + c] = tsdf_mesh_edge_index(rec.data(), tsdf_mesh_edge_voxel(v.g, i, j, k, e), e >> 2);
                    }
                }
            }
    return m;
}

extern "C" {

void mesh_host_table(uint64_t* words) {
    for (int c = 0; c < 256; ++c) words[c] = TSDF_MESH_TABLE.w[c];
}

int64_t mesh_host_triangles(int nx, int ny, int nz, const float* D, const float* W, double min_weight, int64_t* n_points, int64_t cap, int32_t* tri) {
    const double origin[3] = {0.0, 0.0, 0.0};
    HostVolume v(nx, ny, nz, origin, 1.0, D, W);
    return host_triangles(v, min_weight, n_points, cap, tri);
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
static bool word_is(uint64_t word, std::vector<int> edges) {
    if (tsdf_mesh_word_count(word) * 3 != static_cast<int>(edges.size())) return false;
    for (size_t s = 0; s < edges.size(); ++s)
        if (tsdf_mesh_word_edge(word, static_cast<int>(s)) != edges[s]) return false;
    return true;
}

int main() {
    int bad = 0;
    // 1. the table: 820 triangles, the histogram, the named cases
    int hist[6] = {0, 0, 0, 0, 0, 0}, total = 0;
    for (int c = 0; c < 256; ++c) {
        const int n = tsdf_mesh_word_count(TSDF_MESH_TABLE.w[c]);
        if (n > 5) { ++bad; continue; }
        ++hist[n];
        total += n;
    }
    const int want[6] = {2, 16, 50, 80, 76, 32};
    for (int n = 0; n < 6; ++n) bad += hist[n] != want[n];
    bad += total != 820;
    bad += !word_is(TSDF_MESH_TABLE.w[1], {0, 4, 8});
    bad += !word_is(TSDF_MESH_TABLE.w[5], {0, 1, 10, 0, 10, 8});
    bad += !word_is(TSDF_MESH_TABLE.w[0x69], {0, 4, 8, 1, 5, 11, 2, 7, 9, 3, 6, 10});
    bad += !word_is(TSDF_MESH_TABLE.w[0x96], {0, 9, 5, 1, 10, 4, 2, 8, 6, 3, 11, 7});
    std::printf("mesh_driver: table of %d triangles, histogram %d %d %d %d %d %d\n", total, hist[0], hist[1], hist[2], hist[3], hist[4], hist[5]);
    // 2. a sphere (closed: every directed edge has its reverse) and a shifted one in a volume whose rows straddle the groups of 64
    const int shapes[2][3] = {{20, 20, 20}, {67, 9, 7}};
    for (int s = 0; s < 2; ++s) {
        const int nx = shapes[s][0], ny = shapes[s][1], nz = shapes[s][2];
        const double centre[3] = {0.47 * nx, 0.49 * ny, 0.51 * nz}, radius = s == 0 ? 6.0 : 2.2;
        std::vector<float> D(static_cast<size_t>(nx) * ny * nz), W(D.size(), 1.0f);
        for (int k = 0; k < nz; ++k)
            for (int j = 0; j < ny; ++j)
                for (int i = 0; i < nx; ++i) {
                    const double r = std::sqrt((i - centre[0]) * (i - centre[0]) + (j - centre[1]) * (j - centre[1]) + (k - centre[2]) * (k - centre[2]));
                    D[(static_cast<size_t>(k) * ny + j) * nx + i] = static_cast<float>(std::fmax(-1.0, std::fmin(1.0, (r - radius) / 3.0)));
                }
        int64_t n_points = 0;
        const int64_t m = mesh_host_triangles(nx, ny, nz, D.data(), W.data(), 1.0, &n_points, 0, nullptr);
        std::vector<int32_t> tri(3 * static_cast<size_t>(m) + 1);
        if (mesh_host_triangles(nx, ny, nz, D.data(), W.data(), 1.0, &n_points, m, tri.data()) != m || m < 20) ++bad;
        std::map<std::pair<int32_t, int32_t>, int> net;
        for (int64_t t = 0; t < m; ++t)
            for (int c = 0; c < 3; ++c) {
                const int32_t a = tri[3 * t + c], b = tri[3 * t + (c + 1) % 3];
                if (a < 0 || a >= n_points) ++bad;
                ++net[{a, b}];
                --net[{b, a}];
            }
        int open = 0;
        for (const auto& kv : net) open += kv.second != 0;
        std::printf("mesh_driver: %d x %d x %d: %lld points, %lld triangles, %d unbalanced directed edges\n", nx, ny, nz, static_cast<long long>(n_points),
                    static_cast<long long>(m), open);
        if (open != 0 || 2 * n_points - 4 != m) ++bad;  // a closed surface of genus 0: F = 2 V - 4
        // with a weight of 0 in one voxel the cells around it are not live: fewer triangles, a boundary, the points stay
        W[(static_cast<size_t>(nz / 2) * ny + ny / 2) * nx + static_cast<size_t>(centre[0] + radius)] = 0.0f;
        int64_t n2 = 0;
        if (mesh_host_triangles(nx, ny, nz, D.data(), W.data(), 1.0, &n2, 0, nullptr) >= m || n2 >= n_points) ++bad;
    }
    // 3. one cell
    {
        float D[8] = {-0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f}, W[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        int64_t n_points = 0;
        int32_t tri[3] = {-1, -1, -1};
        if (mesh_host_triangles(2, 2, 2, D, W, 1.0, &n_points, 1, tri) != 1 || n_points != 3 || tri[0] != 0 || tri[1] != 1 || tri[2] != 2) ++bad;
        W[7] = 0.0f;
        if (mesh_host_triangles(2, 2, 2, D, W, 1.0, &n_points, 1, tri) != 0 || n_points != 3) ++bad;
    }
    std::printf("mesh_driver: %d mismatches\n", bad);
    return bad != 0;
}
#endif
