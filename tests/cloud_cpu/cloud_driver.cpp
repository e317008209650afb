// cloud_driver.cpp — TEST-ONLY: extern "C" wrapper of cloud_math.hpp for ctypes (tests/test_cloud_cpu.py).  The grid is built on the
// host (tests/host_cloud.hpp); the point rule, the search, the normal, the rows, the Cholesky and the update are the functions every
// lane runs.  A source's sums are added in index order into one accumulator.  Built
// with -DCBA_HOST_DRIVER_MAIN it is a stand-alone program (for the sanitizers): it checks the grid search against brute force on a
// scattered cloud with planted ties and invalid points, the normals of a plane, and that both metrics recover a known small motion.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../host_cloud.hpp"

using namespace cba;

// the sums of the system of one source at res->pose7
static void host_system(const HostCloud& ix, int64_t m, const double* src, const cba_icp_options& o, const cba_icp_result& res, double* acc) {
    for (int e = 0; e < ICP_SUMS; ++e) acc[e] = 0.0;
    double R[9];
    icp_rotation(res.pose7, R);
    const double md = o.max_distance, md2 = md * md;
    const CloudTarget target = ix.target();
    for (int64_t i = 0; i < m; ++i) {
        if (o.metric == 0)
            icp_add_source_point<0>(target, R, res.pose7 + 4, src + 3 * i, md, md2, acc);
        else
            icp_add_source_point<1>(target, R, res.pose7 + 4, src + 3 * i, md, md2, acc);
    }
}

static void host_register_one(const HostCloud& ix, int64_t m, const double* src, const double* init, const cba_icp_options& o,
                              cba_icp_result* res) {
    *res = cba_icp_result{};
    res->pose7[0] = 1.0;
    if (init) {
        for (int k = 0; k < 7; ++k) res->pose7[k] = init[k];
        icp_normalise(res->pose7);
    }
    res->status = CBA_ICP_NOT_CONVERGED;
    int32_t phase = ICP_RUN;
    double acc[ICP_SUMS];
    while (phase != ICP_DONE) {
        host_system(ix, m, src, o, *res, acc);
        icp_advance(acc, o, icp_min_pairs(o), ix.extent, res, &phase);
    }
}

extern "C" {

void cloud_host_normals(int n_maps, int H, int W, const double* xyz, const double* viewpoint, double max_jump, double* out) {
    const double origin[3] = {0.0, 0.0, 0.0};
    const double* vp = viewpoint ? viewpoint : origin;
    const double mj2 = max_jump * max_jump;
    for (int64_t i = 0; i < static_cast<int64_t>(n_maps) * H * W; ++i) {
        const int64_t px = i % (static_cast<int64_t>(W) * H);
        const int row = static_cast<int>(px / W), col = static_cast<int>(px % W);
        const double* c = xyz + 3 * i;
        const bool r = col + 1 < W, l = col > 0, d = row + 1 < H, u = row > 0;
        cloud_normal(c, r ? c + 3 : c, l ? c - 3 : c, d ? c + 3 * static_cast<int64_t>(W) : c, u ? c - 3 * static_cast<int64_t>(W) : c,
                     (r ? 1 : 0) | (l ? 2 : 0) | (d ? 4 : 0) | (u ? 8 : 0), vp, mj2, out + 3 * i);
    }
}

// cba_cloud_index_create + cba_cloud_nearest in one call; -> the grid plan's answer (0: done)
int cloud_host_nearest(int64_t n, const double* xyz, double cell, int64_t m, const double* query, double md, int64_t* index, double* dist2) {
    HostCloud ix;
    const int plan = host_build(n, xyz, nullptr, cell, &ix);
    if (plan != 0) return plan;
    const double md2 = md * md;
    for (int64_t i = 0; i < m; ++i) {
        int32_t pos;
        index[i] = cloud_nearest_point(ix.g, ix.start.data(), ix.rec.data(), query[3 * i], query[3 * i + 1], query[3 * i + 2], md, md2, &pos,
                                       &dist2[i]);
    }
    return 0;
}

// cba_cloud_index_create + cba_cloud_register in one call; out [n_sources][53]: pose7, rms, H, g, n_pairs, iterations, status
int cloud_host_register(int64_t n, const double* xyz, const double* normals, double cell, int n_sources, const int64_t* offset,
                        const double* src, const double* init_pose7, int metric, double max_distance, int max_iterations,
                        double step_tolerance, int min_pairs, double* out) {
    HostCloud ix;
    const int plan = host_build(n, xyz, normals, cell, &ix);
    if (plan != 0) return plan;
    cba_icp_options o;
    o.metric = metric; o.max_distance = max_distance; o.max_iterations = max_iterations; o.step_tolerance = step_tolerance; o.min_pairs = min_pairs;
    for (int s = 0; s < n_sources; ++s) {
        cba_icp_result r;
        host_register_one(ix, offset[s + 1] - offset[s], src + 3 * offset[s], init_pose7 ? init_pose7 + 7 * s : nullptr, o, &r);
        double* w = out + 53 * static_cast<size_t>(s);
        std::memcpy(w, r.pose7, 7 * sizeof(double));
        w[7] = r.rms;
        std::memcpy(w + 8, r.H, 36 * sizeof(double));
        std::memcpy(w + 44, r.g, 6 * sizeof(double));
        w[50] = static_cast<double>(r.n_pairs); w[51] = r.iterations; w[52] = r.status;
    }
    return 0;
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
static double unit(uint64_t* s) {  // a fixed sequence in [0, 1)
    *s = *s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<double>(*s >> 11) / 9007199254740992.0;
}

int main() {
    int bad = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    uint64_t seed = 12345;
    // 1. the grid search against brute force: a scattered cloud on a 1/64 lattice (so that ties occur), with invalid points
    {
        const int n = 700, m = 400;
        std::vector<double> T(3 * n), Q(3 * m);
        for (double& v : T) v = std::floor(unit(&seed) * 64.0) / 64.0;
        for (double& v : Q) v = std::floor(unit(&seed) * 160.0 - 16.0) / 128.0;
        for (int i = 0; i < n; i += 37) T[3 * i + (i % 3)] = nan;
        Q[5] = nan;
        const double cell = 0.125, md = 0.12;
        std::vector<int64_t> index(m);
        std::vector<double> dist2(m);
        if (cloud_host_nearest(n, T.data(), cell, m, Q.data(), md, index.data(), dist2.data()) != 0) ++bad;
        for (int i = 0; i < m; ++i) {
            int64_t best = -1;
            double bd = nan;
            if (cloud_valid(Q[3 * i], Q[3 * i + 1], Q[3 * i + 2]))
                for (int j = 0; j < n; ++j) {
                    if (!cloud_valid(T[3 * j], T[3 * j + 1], T[3 * j + 2])) continue;
                    const double dx = Q[3 * i] - T[3 * j], dy = Q[3 * i + 1] - T[3 * j + 1], dz = Q[3 * i + 2] - T[3 * j + 2];
                    const double d = (dx * dx + dy * dy) + dz * dz;
                    if (d <= md * md && (best < 0 || d < bd)) { best = j; bd = d; }
                }
            if (index[i] != best || (best >= 0 ? dist2[i] != bd : dist2[i] == dist2[i])) ++bad;
        }
    }
    // 2. normals of the plane z = 1 + x / 4 seen from the origin, with a hole; 3. both metrics recover a small motion on a bumpy map
    {
        const int W = 24, H = 18;
        std::vector<double> map(3 * W * H), nrm(3 * W * H), bumpy(3 * W * H), bn(3 * W * H);
        for (int v = 0; v < H; ++v)
            for (int u = 0; u < W; ++u) {
                double* p = &map[3 * (v * W + u)];
                p[0] = (u - 11.5) / 16.0; p[1] = (v - 8.5) / 16.0; p[2] = 1.0 + p[0] / 4.0;
                double* b = &bumpy[3 * (v * W + u)];
                b[0] = p[0]; b[1] = p[1]; b[2] = 1.0 + 0.1 * std::sin(4.0 * p[0]) * std::cos(3.0 * p[1]) + 0.05 * std::cos(5.0 * p[0] * p[1] + p[1]);
            }
        map[3 * (5 * W + 7)] = nan;
        cloud_host_normals(1, H, W, map.data(), nullptr, 1e300, nrm.data());
        const double inv = 1.0 / std::sqrt(1.0 + 1.0 / 16.0);
        for (int v = 0; v < H; ++v)
            for (int u = 0; u < W; ++u) {
                const double* q = &nrm[3 * (v * W + u)];
                const bool hole = v == 5 && u == 7;
                if (hole ? q[0] == q[0] : !(std::fabs(q[0] - 0.25 * inv) < 1e-12 && std::fabs(q[1]) < 1e-12 && std::fabs(q[2] + inv) < 1e-12)) ++bad;
            }
        cloud_host_normals(1, H, W, bumpy.data(), nullptr, 1e300, bn.data());
        const double truth[7] = {std::cos(0.01), std::sin(0.01) * 0.6, 0.0, std::sin(0.01) * 0.8, 0.01, -0.008, 0.005};
        // source = truth^-1 applied to the target's points, so the exact answer is truth
        std::vector<double> src(bumpy.size());
        double R[9];
        icp_rotation(truth, R);
        for (int i = 0; i < W * H; ++i) {
            const double d[3] = {bumpy[3 * i] - truth[4], bumpy[3 * i + 1] - truth[5], bumpy[3 * i + 2] - truth[6]};
            for (int k = 0; k < 3; ++k) src[3 * i + k] = R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2];
        }
        const int64_t off[3] = {0, W * H, W * H};
        for (int metric = 0; metric < 2; ++metric) {
            double out[2 * 53];
            if (cloud_host_register(W * H, bumpy.data(), bn.data(), 0.11, 2, off, src.data(), nullptr, metric, 0.1, 60, 1e-10, 6, out) != 0) ++bad;
            double err = 0.0;
            for (int k = 0; k < 7; ++k) err = std::fmax(err, std::fabs(out[k] - truth[k]));
            std::printf("cloud_driver: metric %d status %d iterations %d pairs %d pose error %.3g rms %.3g\n", metric, static_cast<int>(out[52]),
                        static_cast<int>(out[51]), static_cast<int>(out[50]), err, out[7]);
            if (out[52] != CBA_ICP_OK || !(err < 1e-6) || !(out[7] < 1e-6)) ++bad;
            if (out[53 + 52] != CBA_ICP_TOO_FEW || out[53 + 50] != 0.0) ++bad;  // the empty source
        }
    }
    std::printf("cloud_driver: %d mismatches\n", bad);
    return bad != 0;
}
#endif
