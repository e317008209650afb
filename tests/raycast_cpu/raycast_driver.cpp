// raycast_driver.cpp — TEST-ONLY: extern "C" wrapper of tsdf_ray_math.hpp for ctypes (tests/test_raycast_cpu.py).  The volume is kept as
// the device keeps it ({D, W} pairs in rows of an even pitch, the padding voxel of an odd row poisoned with NaN so that a read of it
// shows); tsdf_ray_pixel is the function every lane runs.  Built with -DCBA_HOST_DRIVER_MAIN it is a stand-alone program (for the
// sanitizers): it runs the planted cases of the rule - rays parallel to an axis, through lattice points and along the last lattice
// plane, a camera inside the volume and one 1e17 away, the depth range, exact and negative zeros, voxels below min_weight, both routes
// to BEHIND, the step's lower bound along the longest side - and random fields with odd rows, and checks what the rule gives by hand.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../calibration_amd/csrc/tsdf_ray_math.hpp"
#include "../host_volume.hpp"

using namespace cba;

static TsdfRayRule make_rule(double vs, double trunc, const double* opts) {
    TsdfRayRule r;
    r.step = opts[0] > 0.0 ? opts[0] : 0.5 * vs;
    r.skip = opts[1]; r.near_depth = opts[2]; r.far_depth = opts[3]; r.min_weight = opts[4]; r.trunc = trunc;
    return r;
}

extern "C" {

// One view: rays [n_px][2], pose7, opts = {step, skip, near_depth, far_depth, min_weight} -> depth [n_px], xyz, nrm [n_px][3],
// status [n_px], count [n_px]
void raycast_host_cast(int nx, int ny, int nz, const double* origin, double vs, double trunc, const float* D, const float* W, int64_t n_px,
                       const double* rays, const double* pose7, const double* opts, double* depth, double* xyz, double* nrm, uint8_t* status,
                       int32_t* count) {
    const HostVolume v(nx, ny, nz, origin, vs, D, W);
    TsdfRayView view;
    tsdf_ray_view(pose7, &view);
    const TsdfRayRule r = make_rule(vs, trunc, opts);
    for (int64_t p = 0; p < n_px; ++p) {
        TsdfRayOut o;
        tsdf_ray_pixel(v.vol.data(), v.g, view, r, rays[2 * p], rays[2 * p + 1], &o);
        depth[p] = o.depth;
        xyz[3 * p] = rays[2 * p] * o.depth;
        xyz[3 * p + 1] = rays[2 * p + 1] * o.depth;
        xyz[3 * p + 2] = o.depth;
        for (int c = 0; c < 3; ++c) nrm[3 * p + c] = o.nrm[c];
        status[p] = static_cast<uint8_t>(o.status);
        count[p] = o.count;
    }
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
// The planted volume: 9 x 9 x 9 voxels of 1/8 at (-0.5, -0.5, 1), D = (4 - k) / 4 (zero on the plane z = 1.5), W = 1
struct Planted {
    std::vector<float> D, W;
    double origin[3] = {-0.5, -0.5, 1.0};
    Planted() : D(729), W(729, 1.0f) {
        for (int l = 0; l < 729; ++l) D[l] = static_cast<float>(4 - l / 81) / 4.0f;
    }
    float& d(int i, int j, int k) { return D[(k * 9 + j) * 9 + i]; }
    float& w(int i, int j, int k) { return W[(k * 9 + j) * 9 + i]; }
    TsdfRayOut cast(double x, double y, const double* pose7, double step, double skip, double near_depth, double far_depth, double min_weight) {
        const double opts[5] = {step, skip, near_depth, far_depth, min_weight}, ray[2] = {x, y};
        double depth, xyz[3];
        TsdfRayOut o;
        uint8_t st;
        raycast_host_cast(9, 9, 9, origin, 0.125, 0.5, D.data(), W.data(), 1, ray, pose7, opts, &depth, xyz, o.nrm, &st, &o.count);
        o.depth = depth;
        o.status = st;
        return o;
    }
};

static int expect(const char* name, const TsdfRayOut& o, int status, double depth, int count, int normal /*1: (0,0,-1); 0: NaN; -1: any*/) {
    bool ok = o.status == status && (count < 0 || o.count == count);
    ok = ok && (status == TSDF_RAY_HIT ? o.depth == depth : o.depth != o.depth);
    if (normal == 1) ok = ok && o.nrm[0] == 0.0 && o.nrm[1] == 0.0 && o.nrm[2] == -1.0;
    if (normal == 0) ok = ok && o.nrm[0] != o.nrm[0] && o.nrm[1] != o.nrm[1] && o.nrm[2] != o.nrm[2];
    if (!ok)
        std::printf("raycast_driver: %s: status %d, depth %.17g, count %d, normal %g %g %g\n", name, o.status, o.depth, o.count, o.nrm[0], o.nrm[1],
                    o.nrm[2]);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double id[7] = {1, 0, 0, 0, 0, 0, 0};
    {
        Planted p;
        // along z through the lattice points (4, 4, k): parallel to x and y inside the slab; sixteenths from z = 1: the ninth sample is F = 0
        // exactly, the tenth is negative: the hit is at the zero
        bad += expect("axis", p.cast(0, 0, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_HIT, 1.5, 10, 1);
        bad += expect("axis skip 1", p.cast(0, 0, id, 0.0, 1.0, 0.0, inf, 1.0), TSDF_RAY_HIT, 1.5, -1, 1);
        p.d(4, 4, 4) = -0.0f;
        bad += expect("minus zero", p.cast(0, 0, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_HIT, 1.5, 10, -1);
        p.d(4, 4, 4) = 0.0f;
        const double out_x[7] = {1, 0, 0, 0, -1.0, 0, 0}, last_x[7] = {1, 0, 0, 0, -0.5, 0, 0}, inside[7] = {1, 0, 0, 0, 0, 0, -1.25};
        bad += expect("outside the slab", p.cast(0, 0, out_x, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_MISS, nan, 0, 0);
        bad += expect("last lattice plane", p.cast(0, 0, last_x, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_HIT, 1.5, 10, 0);  // no +x neighbour
        bad += expect("edge of the view", p.cast(-0.5, 0, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_MISS, nan, 1, 0);  // z0 == z1 == 1
        bad += expect("camera inside", p.cast(0, 0, inside, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_HIT, 0.25, 6, 1);
        bad += expect("near cuts", p.cast(0, 0, id, 0.0, 0.0, 1.625, inf, 1.0), TSDF_RAY_BEHIND, nan, 1, 0);
        bad += expect("far cuts", p.cast(0, 0, id, 0.0, 0.0, 0.0, 1.4375, 1.0), TSDF_RAY_MISS, nan, 8, 0);
        bad += expect("no ray", p.cast(nan, 0, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_NO_RAY, nan, 0, 0);
        bad += expect("no ray", p.cast(0, inf, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_NO_RAY, nan, 0, 0);
        const double away[7] = {1, 0, 0, 0, 0, 0, 1e17};  // the centre at z = -1e17: z0 = z1 = 1e17, and z + step == z
        bad += expect("far camera", p.cast(0, 0, away, 0.0, 0.5, 0.0, inf, 1.0), TSDF_RAY_MISS, nan, 1, 0);
        const double back[7] = {0, 1, 0, 0, 0, 0, 0};  // half a turn about x: the camera looks along -z, away from the volume
        bad += expect("looking away", p.cast(0, 0, back, 0.0, 0.5, 0.0, inf, 1.0), TSDF_RAY_MISS, nan, 0, 0);
    }
    {
        Planted p;  // a voxel of a normal's cell below min_weight: +x of the hit samples cell (5, 4, 4), which holds voxel (6, 4, 4)
        p.w(6, 4, 4) = 0.0f;
        bad += expect("normal's cell", p.cast(0, 0, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_HIT, 1.5, 10, 0);
        p.w(6, 4, 4) = 1.0f;
        bad += expect("min_weight 2", p.cast(0, 0, id, 0.0, 0.0, 0.0, inf, 2.0), TSDF_RAY_MISS, nan, 17, 0);
        // a voxel before the surface: the cells k = 2, 3 are invalid, the sample on the zero is valid again, the next one hits
        p.w(4, 4, 3) = 0.0f;
        bad += expect("hole before the surface", p.cast(0, 0, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_HIT, 1.5, 10, 0);
        p.w(4, 4, 3) = 1.0f;
        // the voxel on the surface: the cells k = 3, 4 are invalid, "previous" is reset, the first valid sample after them is negative
        p.w(4, 4, 4) = 0.0f;
        bad += expect("hole at the surface", p.cast(0, 0, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_BEHIND, nan, 11, 0);
    }
    {
        Planted p;  // the second route: D is NaN in the planes k = 0, 1, negative in k = 2, positive from k = 3 on
        for (int l = 0; l < 729; ++l) p.D[l] = l / 81 < 2 ? std::numeric_limits<float>::quiet_NaN() : l / 81 == 2 ? -0.5f : 0.5f;
        bad += expect("behind, second route", p.cast(0, 0, id, 0.0, 0.0, 0.0, inf, 1.0), TSDF_RAY_BEHIND, nan, 6, 0);
    }
    {
        // the step's lower bound along the longest side: 1024 x 2 x 2 free voxels, a camera that looks along +x: 1023 x 16 + 1 samples
        const int nx = 1024;
        std::vector<float> D(4 * nx, 1.0f), W(4 * nx, 1.0f);
        const double origin[3] = {1.0, 0.0, 0.0}, pose[7] = {0.5, -0.5, -0.5, -0.5, 0, 0, 0}, ray[2] = {0.0, 0.0};
        const double opts[5] = {0.125 / 16, 0.0, 0.0, inf, 1.0};
        double depth, xyz[3], nrm[3];
        uint8_t st;
        int32_t count;
        raycast_host_cast(nx, 2, 2, origin, 0.125, 0.5, D.data(), W.data(), 1, ray, pose, opts, &depth, xyz, nrm, &st, &count);
        std::printf("raycast_driver: lower-bound step: status %d, %d samples\n", st, count);
        if (st != TSDF_RAY_MISS || count != 1023 * 16 + 1 || depth == depth) ++bad;  // under CBA_TSDF_RAY_MAX_SAMPLES
    }
    {
        // random fields with odd rows (the padding voxel is NaN here): every ray ends, hits have finite depths inside the range
        uint64_t s = 12345;
        auto rnd = [&] { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<int>((s >> 33) % 17); };
        const int shapes[5][3] = {{2, 2, 2}, {3, 2, 2}, {5, 4, 3}, {64, 3, 2}, {65, 3, 2}};
        for (const auto& sh : shapes) {
            const int n = sh[0] * sh[1] * sh[2];
            std::vector<float> D(n), W(n);
            for (int l = 0; l < n; ++l) {
                D[l] = static_cast<float>(rnd() - 8) / 8.0f;
                W[l] = static_cast<float>(rnd() % 8 ? 1 : 0);
            }
            const double origin[3] = {-0.125 * (sh[0] - 1) / 2, -0.125 * (sh[1] - 1) / 2, 1.0}, opts[5] = {0.0, 0.5, 0.0, inf, 1.0};
            int hits = 0;
            for (int py = 0; py < 9; ++py)
                for (int px = 0; px < 33; ++px) {
                    const double ray[2] = {(px - 16) / 16.0 * 0.06 * sh[0], (py - 4) / 4.0 * 0.06 * sh[1]};
                    double depth, xyz[3], nrm[3];
                    uint8_t st;
                    int32_t count;
                    raycast_host_cast(sh[0], sh[1], sh[2], origin, 0.125, 0.375, D.data(), W.data(), 1, ray, id, opts, &depth, xyz, nrm, &st, &count);
                    if (st == TSDF_RAY_HIT) {
                        ++hits;
                        if (!(depth >= 1.0 && depth <= 1.0 + 0.125 * (sh[2] - 1))) ++bad;
                    } else if (depth == depth) {
                        ++bad;
                    }
                    if (count > 64) ++bad;
                }
            std::printf("raycast_driver: random %d x %d x %d: %d hits of 297 rays\n", sh[0], sh[1], sh[2], hits);
        }
    }
    std::printf("raycast_driver: %d mismatches\n", bad);
    return bad != 0;
}
#endif
