// align_driver.cpp — TEST-ONLY: extern "C" wrapper of cloud_math.hpp's alignment of many scans for ctypes (tests/test_align_cpu.py).
// Every scan's grid is built on the host (tests/host_cloud.hpp); an edge's sums are added in index order into one accumulator, by the
// point rule every lane runs or, its search replaced, by brute force over the scan's valid points; the relative pose, the adjoint, the blocks, their places in the system, the width-n Cholesky, the stop tests and the
// updates are the functions the device runs.  Built with -DCBA_HOST_DRIVER_MAIN it is a stand-alone program (for the sanitizers):
// the planted statuses, 2 and 64 scans, 1 and 1024 edges, the last scan fixed, duplicate and two-way edges.  Every buffer is
// sized exactly.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../host_cloud.hpp"

using namespace cba;

struct HostScan {
    HostCloud cloud;
    int64_t first = 0, count = 0;
};

// brute force's rule over all valid points of the scan, in the records' order: -> the record's place or -1
static int32_t brute_nearest(const HostCloud& ix, const double* Q, double md2) {
    int32_t pos = -1;
    int64_t best = -1;
    double bd = 0.0;
    if (!cloud_valid(Q[0], Q[1], Q[2])) return -1;
    for (size_t k = 0; k < ix.rec.size(); ++k) {
        const CloudRec& r = ix.rec[k];
        const double dx = Q[0] - r.x, dy = Q[1] - r.y, dz = Q[2] - r.z;
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d <= md2 && (best < 0 || d < bd || (d == bd && r.idx < best))) {
            best = r.idx;
            bd = d;
            pos = static_cast<int32_t>(k);
        }
    }
    return pos;
}

// the sums of edge (a, b) at the poses: scan a's m points src at (R, t) against scan b
template <int METRIC>
static void host_edge_sums(const HostCloud& b, int64_t m, const double* src, const double* R, const double* t, const cba_icp_options& o,
                           bool brute, double* acc) {
    for (int e = 0; e < ICP_SUMS; ++e) acc[e] = 0.0;
    const double md = o.max_distance, md2 = md * md;
    const CloudTarget target = b.target();
    for (int64_t i = 0; i < m; ++i) {
        const double* p = src + 3 * i;
        if (!brute) {
            icp_add_source_point<METRIC>(target, R, t, p, md, md2, acc);
            continue;
        }
        if (!cloud_valid(p[0], p[1], p[2])) continue;
        double Q[3];
        icp_transform(R, t, p, Q);
        const int32_t pos = brute_nearest(b, Q, md2);
        if (pos >= 0) icp_add_match<METRIC>(Q, target.rec, target.rec_normal, pos, acc);
    }
}

extern "C" {

// The width of one edge in edge_out: H [36], g [6], ss, n_pairs, used
enum { EDGE_OUT = 45 };

// cba_cloud_set_create + cba_cloud_align in one call.  pose7 [n_scans][7] out; edge_out [n_edges][45]; result [5]: rms, n_pairs,
// n_used_edges, iterations, status.  -> 0, or 10 + the grid plan's answer for the first scan without a grid
int align_host(int n_scans, const int64_t* offset, const double* xyz, const double* normals, double cell, int n_edges, const int32_t* edges,
               const double* init_pose7, int metric, double max_distance, int max_iterations, double step_tolerance, int min_pairs, int fixed,
               int brute, double* pose7, double* edge_out, double* result) {
    std::vector<HostScan> scan(static_cast<size_t>(n_scans));
    double extent = 0.0;
    for (int k = 0; k < n_scans; ++k) {
        HostScan& s = scan[k];
        s.first = offset[k];
        s.count = offset[k + 1] - offset[k];
        const int plan = host_build(s.count, xyz + 3 * s.first, normals ? normals + 3 * s.first : nullptr, cell, &s.cloud);
        if (plan != 0) return 10 + plan;
        extent = std::max(extent, s.cloud.extent);
    }
    cba_icp_options o;
    o.metric = metric; o.max_distance = max_distance; o.max_iterations = max_iterations; o.step_tolerance = step_tolerance; o.min_pairs = min_pairs;
    const int32_t bar = icp_min_pairs(o);
    const int n = 6 * (n_scans - 1);
    for (int k = 0; k < n_scans; ++k) {
        double* p = pose7 + 7 * k;
        for (int j = 0; j < 7; ++j) p[j] = init_pose7 ? init_pose7[7 * k + j] : (j == 0 ? 1.0 : 0.0);
        icp_normalise(p);
    }
    std::vector<double> adj(36 * static_cast<size_t>(n_scans)), blocks(static_cast<size_t>(ALIGN_EDGE) * n_edges);
    std::vector<double> H(static_cast<size_t>(n) * n), g(static_cast<size_t>(n)), z(static_cast<size_t>(n)), xi(static_cast<size_t>(n));
    std::vector<int32_t> row(2 * static_cast<size_t>(n_edges));
    std::vector<char> used(static_cast<size_t>(n_edges));
    auto reduced = [&](int s) { return s == fixed ? -1 : s < fixed ? s : s - 1; };
    AlignState st{};
    st.res.status = CBA_ICP_NOT_CONVERGED;
    st.phase = ICP_RUN;
    while (st.phase != ICP_DONE) {
        for (int k = 0; k < n_scans; ++k) {
            double R[9];
            icp_rotation(pose7 + 7 * k, R);
            align_adjoint(R, pose7 + 7 * k + 4, &adj[36 * static_cast<size_t>(k)]);
        }
        double ss = 0.0, np = 0.0;
        int32_t n_used = 0;
        for (int e = 0; e < n_edges; ++e) {
            const int a = edges[2 * e], b = edges[2 * e + 1];
            double Ra[9], Rb[9], R[9], t[3], acc[ICP_SUMS];
            icp_rotation(pose7 + 7 * a, Ra);
            icp_rotation(pose7 + 7 * b, Rb);
            align_relative(Ra, pose7 + 7 * a + 4, Rb, pose7 + 7 * b + 4, R, t);
            (metric == 0 ? host_edge_sums<0> : host_edge_sums<1>)(scan[b].cloud, scan[a].count, xyz + 3 * scan[a].first, R, t, o, brute != 0, acc);
            double* w = edge_out + static_cast<size_t>(EDGE_OUT) * e;
            icp_mirror(acc, w);
            for (int k = 0; k < 6; ++k) w[36 + k] = acc[21 + k];
            used[e] = static_cast<int64_t>(acc[ICP_NP]) >= bar;
            w[42] = acc[ICP_SS]; w[43] = acc[ICP_NP]; w[44] = used[e] ? 1.0 : 0.0;
            row[2 * e] = reduced(a);
            row[2 * e + 1] = reduced(b);
            align_edge_blocks(w, w + 36, &adj[36 * static_cast<size_t>(b)], &blocks[static_cast<size_t>(ALIGN_EDGE) * e]);
            if (used[e]) {
                ss += acc[ICP_SS];
                np += acc[ICP_NP];
                ++n_used;
            }
        }
        st.res.n_pairs = static_cast<int64_t>(np);
        st.res.n_used_edges = n_used;
        st.res.rms = np > 0.0 ? std::sqrt(ss / np) : std::numeric_limits<double>::quiet_NaN();
        if (!align_begin(o, &st)) break;
        std::fill(H.begin(), H.end(), 0.0);
        std::fill(g.begin(), g.end(), 0.0);
        for (int p = 0; p < n_scans; ++p)
            for (int r = 0; r < ALIGN_EDGE; ++r)
                for (int e = 0; e < n_edges; ++e)
                    if (used[e]) align_assemble_entry(n, H.data(), g.data(), reduced(p), r, row[2 * e], row[2 * e + 1], &blocks[static_cast<size_t>(ALIGN_EDGE) * e]);
        const bool solved = align_cholesky(n, H.data(), g.data(), z.data(), xi.data());
        bool all_small = true;
        if (solved)
            for (int p = 0; p < n_scans; ++p)
                if (p != fixed && !align_update(pose7 + 7 * p, &xi[6 * static_cast<size_t>(reduced(p))], o, extent)) all_small = false;
        align_advance(solved, all_small, o, &st);
    }
    result[0] = st.res.rms; result[1] = static_cast<double>(st.res.n_pairs); result[2] = st.res.n_used_edges;
    result[3] = st.res.iterations; result[4] = st.res.status;
    return 0;
}

// M [36] and c [6] of H [36], g [6] under the adjoint of pose7 (for the finite-difference check of the blocks and their signs)
void align_host_blocks(const double* H, const double* g, const double* pose7_b, double* A, double* out) {
    double q[7], R[9];
    for (int k = 0; k < 7; ++k) q[k] = pose7_b[k];
    icp_normalise(q);
    icp_rotation(q, R);
    align_adjoint(R, q + 4, A);
    align_edge_blocks(H, g, A, out);
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
// scan k of a chain: a W x H patch of the bumpy surface z = 1 + ..., its window moved by `shift` in x, with the plane's rough normals
static void patch(int W, int H, double shift, std::vector<double>* xyz, std::vector<double>* nrm) {
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            const double x = (u - 0.5 * W) / 40.0 + shift, y = (v - 0.5 * H) / 40.0;
            const double z = 1.0 + 0.1 * std::sin(4.0 * x) * std::cos(3.0 * y) + 0.05 * std::cos(5.0 * x * y + y);
            const double zx = 0.4 * std::cos(4.0 * x) * std::cos(3.0 * y) - 0.25 * y * std::sin(5.0 * x * y + y);
            const double zy = -0.3 * std::sin(4.0 * x) * std::sin(3.0 * y) - 0.05 * (5.0 * x + 1.0) * std::sin(5.0 * x * y + y);
            const double len = std::sqrt(zx * zx + zy * zy + 1.0);
            xyz->insert(xyz->end(), {x, y, z});
            nrm->insert(nrm->end(), {zx / len, zy / len, -1.0 / len});
        }
}

struct Run {
    std::vector<double> pose, edge, result;
    int rc;
};

static Run run(int n_scans, const std::vector<int64_t>& off, const std::vector<double>& xyz, const std::vector<double>& nrm, const std::vector<int32_t>& edges,
               const std::vector<double>* init, int metric, int max_it, double tol, int fixed, int brute) {
    Run r;
    const int E = static_cast<int>(edges.size() / 2);
    r.pose.resize(7 * static_cast<size_t>(n_scans));
    r.edge.resize(static_cast<size_t>(EDGE_OUT) * E);
    r.result.resize(5);
    r.rc = align_host(n_scans, off.data(), xyz.data(), nrm.data(), 0.0201, E, edges.data(), init ? init->data() : nullptr, metric, 0.02, max_it, tol, 6, fixed,
                      brute, r.pose.data(), r.edge.data(), r.result.data());
    return r;
}

int main() {
    int bad = 0;
    // a chain of n scans: windows 0.1 apart (16 x 12 points each, 0.025 apart, so neighbours share lattice points); the gate of 0.02
    // is below the spacing, so a point beyond a neighbour's border finds no pair
    auto chain = [&](int n_scans, std::vector<int64_t>* off, std::vector<double>* xyz, std::vector<double>* nrm) {
        off->assign(1, 0);
        for (int k = 0; k < n_scans; ++k) {
            patch(16, 12, 0.1 * k, xyz, nrm);
            off->push_back(static_cast<int64_t>(xyz->size() / 3));
        }
    };
    // 1. two scans, one edge; two-way and duplicate edges; the last scan fixed; brute force and the grid agree to the bit
    {
        std::vector<int64_t> off;
        std::vector<double> xyz, nrm;
        chain(2, &off, &xyz, &nrm);
        for (size_t i = static_cast<size_t>(3 * off[1]); i < xyz.size(); i += 3) xyz[i] += 0.004;  // scan 1 is off by 0.004 in x
        const Run one = run(2, off, xyz, nrm, {1, 0}, nullptr, 0, 30, 1e-10, 0, 0);
        const Run brute = run(2, off, xyz, nrm, {1, 0}, nullptr, 0, 30, 1e-10, 0, 1);
        const Run both = run(2, off, xyz, nrm, {1, 0, 0, 1, 1, 0}, nullptr, 0, 30, 1e-10, 1, 0);
        std::printf("align_driver: two scans: status %d iterations %d tx %.6g; fixed last: status %d tx0 %.6g\n", static_cast<int>(one.result[4]),
                    static_cast<int>(one.result[3]), one.pose[7 + 4], static_cast<int>(both.result[4]), both.pose[4]);
        if (one.rc || one.result[4] != CBA_ICP_OK || !(std::fabs(one.pose[7 + 4] + 0.004) < 1e-4)) ++bad;
        if (std::memcmp(one.pose.data(), brute.pose.data(), one.pose.size() * sizeof(double)) != 0) ++bad;
        if (both.rc || both.result[4] != CBA_ICP_OK || both.result[2] != 3 || !(std::fabs(both.pose[4] - 0.004) < 1e-4) || both.pose[7 + 4] != 0.0) ++bad;
        // max_iterations = 0: the statistics at the start; a scan no edge connects: degenerate; scans far apart: too few
        const Run zero = run(2, off, xyz, nrm, {1, 0}, nullptr, 1, 0, 1e-10, 0, 0);
        if (zero.result[4] != CBA_ICP_NOT_CONVERGED || zero.result[3] != 0 || !(zero.result[1] > 0)) ++bad;
        std::vector<double> far(14, 0.0);
        far[0] = far[7] = 1.0;
        far[7 + 6] = 3.0;
        const Run few = run(2, off, xyz, nrm, {1, 0, 0, 1}, &far, 0, 30, 1e-10, 0, 0);
        if (few.result[4] != CBA_ICP_TOO_FEW || few.result[2] != 0 || few.result[0] == few.result[0]) ++bad;
    }
    {
        std::vector<int64_t> off;
        std::vector<double> xyz, nrm;
        chain(3, &off, &xyz, &nrm);
        const Run apart = run(3, off, xyz, nrm, {1, 0}, nullptr, 0, 30, 1e-10, 0, 0);  // scan 2 has no edge
        if (apart.result[4] != CBA_ICP_DEGENERATE || apart.result[3] != 0) ++bad;
        const Run on = run(3, off, xyz, nrm, {1, 0, 2, 1}, nullptr, 0, 30, 1e-6, 0, 0);  // every scan lies on its neighbour already
        if (on.result[4] != CBA_ICP_OK || on.result[3] != 1) ++bad;
    }
    // 2. 64 scans in a chain, fixed in the middle, 1024 edges: the 126 neighbours both ways, repeated
    {
        std::vector<int64_t> off;
        std::vector<double> xyz, nrm;
        chain(64, &off, &xyz, &nrm);
        std::vector<int32_t> edges;
        for (int e = 0; e < 1024; ++e) {
            const int k = (e / 2) % 63;
            if (e % 2) { edges.push_back(k); edges.push_back(k + 1); } else { edges.push_back(k + 1); edges.push_back(k); }
        }
        const Run big = run(64, off, xyz, nrm, edges, nullptr, 0, 2, 1e-6, 31, 0);
        std::printf("align_driver: 64 scans, 1024 edges: status %d iterations %d used %d\n", static_cast<int>(big.result[4]),
                    static_cast<int>(big.result[3]), static_cast<int>(big.result[2]));
        if (big.rc || big.result[4] != CBA_ICP_OK || big.result[2] != 1024) ++bad;
        const Run chain1 = run(64, off, xyz, nrm, std::vector<int32_t>(edges.begin(), edges.begin() + 2), nullptr, 0, 2, 1e-6, 63, 0);
        if (chain1.result[4] != CBA_ICP_DEGENERATE) ++bad;  // one edge cannot hold 63 scans
    }
    std::printf("align_driver: %d mismatches\n", bad);
    return bad != 0;
}
#endif
