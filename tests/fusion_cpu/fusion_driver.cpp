// fusion_driver.cpp — TEST-ONLY: extern "C" wrapper of tsdf_math.hpp for ctypes (tests/test_fusion_cpu.py).  The volume is kept as the
// device keeps it ({D, W} pairs in rows of an even pitch); the update and the edges are the functions every lane runs, walked here in
// the order the rule states.  Built with -DCBA_HOST_DRIVER_MAIN it is a stand-alone program (for the sanitizers): it fuses four
// views of the plane z = 1 with both camera models, checks the extracted surface against the plane, and runs the planted edge cases.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../host_volume.hpp"

using namespace cba;

static void host_integrate(HostVolume& v, int model, const double* intr, int n_maps, int H, int W, const double* depth, const double* poses,
                           const TsdfRule& r) {
    TsdfCam cam;
    double intr12[12];
    ls_fill_intr(model, intr, intr12, cam.sd);
    for (int k = 0; k < 12; ++k) cam.intr[k] = intr12[k];
    for (int m = 0; m < n_maps; ++m) {
        TsdfPose p;
        quat_to_rotmat(poses + 7 * m, p.R);
        for (int c = 0; c < 3; ++c) p.t[c] = poses[7 * m + 4 + c];
        const double* map = depth + static_cast<int64_t>(m) * W * H;
        for (int k = 0; k < v.g.nz; ++k)
            for (int j = 0; j < v.g.ny; ++j)
                for (int i = 0; i < v.g.nx; ++i) {
                    float* at = &v.vol[tsdf_at(v.g, i, j, k)];
                    const double X0 = tsdf_coord(v.g.o[0], i, v.g.vs), X1 = tsdf_coord(v.g.o[1], j, v.g.vs), X2 = tsdf_coord(v.g.o[2], k, v.g.vs);
                    if (model == CAM_SCHEIMPFLUG)
                        tsdf_update<CAM_SCHEIMPFLUG>(cam, p, map, r, X0, X1, X2, at, at + 1);
                    else
                        tsdf_update<CAM_PINHOLE_BC>(cam, p, map, r, X0, X1, X2, at, at + 1);
                }
    }
}

// -> the number of qualifying edges; the first `cap` of them written
static int64_t host_extract(const HostVolume& v, double min_weight, int64_t cap, double* xyz, double* nrm) {
    int64_t n = 0;
    for (int k = 0; k < v.g.nz; ++k)
        for (int j = 0; j < v.g.ny; ++j)
            for (int i = 0; i < v.g.nx; ++i)
                for (int axis = 0; axis < 3; ++axis) {
                    double Da, Db;
                    if (!tsdf_edge(v.vol.data(), v.g, i, j, k, axis, min_weight, &Da, &Db)) continue;
                    if (n < cap) tsdf_edge_point(v.vol.data(), v.g, i, j, k, axis, Da, Db, xyz + 3 * n, nrm + 3 * n);
                    ++n;
                }
    return n;
}

extern "C" {

// D, W [nz][ny][nx]: in and out
void fusion_host_integrate(int nx, int ny, int nz, const double* origin, double vs, double trunc, double max_weight, double max_depth, int model,
                           const double* intr, int n_maps, int H, int W, const double* depth, const double* poses, float* D, float* Wt) {
    HostVolume v(nx, ny, nz, origin, vs, D, Wt);
    TsdfRule r;
    r.trunc = trunc; r.max_depth = max_depth; r.max_weight = max_weight; r.W = W; r.H = H;
    host_integrate(v, model, intr, n_maps, H, W, depth, poses, r);
    v.planes(D, Wt);
}

int64_t fusion_host_extract(int nx, int ny, int nz, const double* origin, double vs, const float* D, const float* Wt, double min_weight, int64_t cap,
                            double* xyz, double* nrm) {
    HostVolume v(nx, ny, nz, origin, vs, D, Wt);
    return host_extract(v, min_weight, cap, xyz, nrm);
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
int main() {
    int bad = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // 1. four views of the plane z = 1 from the origin side, both models: the crossings lie on the plane, the normals point to -z
    for (int model = 0; model < 2; ++model) {
        const int nx = 13, ny = 10, nz = 12, W = 40, H = 30, n_maps = 4;
        const double origin[3] = {-0.3, -0.22, 0.74}, vs = 0.046875, intr[12] = {60.0, 58.0, 19.5, 14.5, 0.0, -0.05, 0.01, 0.0, 0.0005, -0.0003, 0.02, -0.01};
        std::vector<double> depth(static_cast<size_t>(n_maps) * W * H), poses(7 * n_maps, 0.0);
        for (int m = 0; m < n_maps; ++m) {
            poses[7 * m] = 1.0;
            poses[7 * m + 4] = 0.01 * m;  // the camera moves along x: the plane keeps z = 1 in every view
            for (int px = 0; px < W * H; ++px) depth[static_cast<size_t>(m) * W * H + px] = 1.0;
            depth[static_cast<size_t>(m) * W * H + 7 * m] = nan;
            depth[static_cast<size_t>(m) * W * H + 9 * m + 1] = -1.0;
        }
        HostVolume v(nx, ny, nz, origin, vs, nullptr, nullptr);
        TsdfRule r;
        r.trunc = 3 * vs; r.max_depth = std::numeric_limits<double>::infinity(); r.max_weight = 3.0; r.W = W; r.H = H;
        host_integrate(v, model, intr, n_maps, H, W, depth.data(), poses.data(), r);
        const int64_t n = host_extract(v, 1.0, 0, nullptr, nullptr);
        std::vector<double> xyz(3 * static_cast<size_t>(n) + 1), nrm(3 * static_cast<size_t>(n) + 1);
        if (host_extract(v, 1.0, n, xyz.data(), nrm.data()) != n || n < 50) ++bad;
        int with_normal = 0;
        double worst = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            worst = std::fmax(worst, std::fabs(xyz[3 * i + 2] - 1.0));
            if (nrm[3 * i] == nrm[3 * i]) {
                ++with_normal;
                if (!(nrm[3 * i + 2] < -0.99)) ++bad;
            }
        }
        float wmax = 0.0f;
        for (size_t i = 1; i < v.vol.size(); i += 2) wmax = std::fmax(wmax, v.vol[i]);
        std::printf("fusion_driver: model %d: %lld points, %d with a normal, largest |z - 1| %.3g, largest W %g\n", model, static_cast<long long>(n),
                    with_normal, worst, static_cast<double>(wmax));
        if (!(worst < 1e-6) || with_normal == 0 || wmax != 3.0f) ++bad;
    }
    // 2. planted edges: one crossing between two observed voxels of an otherwise unobserved 2 x 2 x 2 volume (no normal: the point is
    // kept); D_a = 0 and -0.0 against a negative neighbour (t = 0, both count as non-negative); an end below min_weight
    {
        const double origin[3] = {0.0, 0.0, 0.0};
        float D[8] = {-0.5f, 0.5f, 1, 1, 1, 1, 1, 1}, W[8] = {1, 1, 0, 0, 0, 0, 0, 0};
        double xyz[9], nrm[9];
        if (fusion_host_extract(2, 2, 2, origin, 0.5, D, W, 1.0, 3, xyz, nrm) != 1 || xyz[0] != 0.25 || xyz[1] != 0.0 || nrm[0] == nrm[0]) ++bad;
        if (fusion_host_extract(2, 2, 2, origin, 0.5, D, W, 2.0, 3, xyz, nrm) != 0) ++bad;
        D[0] = 0.0f; D[1] = -0.5f;
        if (fusion_host_extract(2, 2, 2, origin, 0.5, D, W, 1.0, 3, xyz, nrm) != 1 || xyz[0] != 0.0) ++bad;
        D[0] = -0.0f;
        if (fusion_host_extract(2, 2, 2, origin, 0.5, D, W, 1.0, 3, xyz, nrm) != 1 || xyz[0] != 0.0) ++bad;
        D[1] = 0.5f;
        if (fusion_host_extract(2, 2, 2, origin, 0.5, D, W, 1.0, 3, xyz, nrm) != 0) ++bad;
    }
    std::printf("fusion_driver: %d mismatches\n", bad);
    return bad != 0;
}
#endif
