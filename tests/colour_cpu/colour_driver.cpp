// colour_driver.cpp — TEST-ONLY: extern "C" wrapper of tsdf_colour_math.hpp for ctypes (tests/test_colour_cpu.py).  The volume and the
// colour records are kept as the device keeps them (rows of an even pitch, the padding voxel of an odd row poisoned with NaN); the
// update, the point colours and the hit colours are the functions every lane runs, walked here in the order the rule states.  Built
// with -DCBA_HOST_DRIVER_MAIN it is a stand-alone program (for the sanitizers): it fuses three painted views of the plane z = 1, reads
// the colours of the extract's points and of a ray cast's hits, and runs the planted blend and rounding cases.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../calibration_amd/csrc/tsdf_colour_math.hpp"
#include "../host_volume.hpp"

using namespace cba;

// the colour records beside a HostVolume: exactly the stored rows, so that a read past them is the sanitizer's to find
struct HostColour {
    std::vector<float> col;
    // colour [nz][ny][nx][4]: the dense records; NULL: all zeros
    HostColour(const TsdfGrid& g, const float* colour) {
        col.assign(4 * static_cast<size_t>(g.pitch) * g.ny * g.nz, std::numeric_limits<float>::quiet_NaN());
        for (int64_t l = 0; l < static_cast<int64_t>(g.nx) * g.ny * g.nz; ++l) {
            int i, j, k;
            tsdf_voxel_of(g, l, &i, &j, &k);
            for (int c = 0; c < 4; ++c) col[tsdf_colour_at(g, i, j, k) + c] = colour ? colour[4 * l + c] : 0.0f;
        }
    }
    void records(const TsdfGrid& g, float* colour) const {
        for (int64_t l = 0; l < static_cast<int64_t>(g.nx) * g.ny * g.nz; ++l) {
            int i, j, k;
            tsdf_voxel_of(g, l, &i, &j, &k);
            for (int c = 0; c < 4; ++c) colour[4 * l + c] = col[tsdf_colour_at(g, i, j, k) + c];
        }
    }
};

static void host_integrate(HostVolume& v, HostColour& hc, int model, const double* intr, int n_maps, int H, int W, const double* depth,
                           const uint32_t* rgba, const double* poses, const TsdfRule& r) {
    TsdfCam cam;
    double intr12[12];
    ls_fill_intr(model, intr, intr12, cam.sd);
    for (int k = 0; k < 12; ++k) cam.intr[k] = intr12[k];
    for (int m = 0; m < n_maps; ++m) {
        TsdfPose p;
        quat_to_rotmat(poses + 7 * m, p.R);
        for (int c = 0; c < 3; ++c) p.t[c] = poses[7 * m + 4 + c];
        const double* map = depth + static_cast<int64_t>(m) * W * H;
        const uint32_t* image = rgba + static_cast<int64_t>(m) * W * H;
        for (int k = 0; k < v.g.nz; ++k)
            for (int j = 0; j < v.g.ny; ++j)
                for (int i = 0; i < v.g.nx; ++i) {
                    float* at = &v.vol[tsdf_at(v.g, i, j, k)];
                    float* C = &hc.col[tsdf_colour_at(v.g, i, j, k)];
                    const double X0 = tsdf_coord(v.g.o[0], i, v.g.vs), X1 = tsdf_coord(v.g.o[1], j, v.g.vs), X2 = tsdf_coord(v.g.o[2], k, v.g.vs);
                    if (model == CAM_SCHEIMPFLUG)
                        tsdf_colour_update<CAM_SCHEIMPFLUG>(cam, p, map, image, r, X0, X1, X2, at, at + 1, C);
                    else
                        tsdf_colour_update<CAM_PINHOLE_BC>(cam, p, map, image, r, X0, X1, X2, at, at + 1, C);
                }
    }
}

// -> the number of qualifying edges; the colours of the first `cap` of them written
static int64_t host_points(const HostVolume& v, const HostColour& hc, double min_weight, int64_t cap, uint32_t* rgba) {
    int64_t n = 0;
    for (int k = 0; k < v.g.nz; ++k)
        for (int j = 0; j < v.g.ny; ++j)
            for (int i = 0; i < v.g.nx; ++i)
                for (int axis = 0; axis < 3; ++axis) {
                    double Da, Db;
                    if (!tsdf_edge(v.vol.data(), v.g, i, j, k, axis, min_weight, &Da, &Db)) continue;
                    if (n < cap) rgba[n] = tsdf_colour_edge(hc.col.data(), v.g, i, j, k, axis, Da, Db);
                    ++n;
                }
    return n;
}

// ctypes hands over byte arrays: the words are copied in and out, whatever their alignment
static std::vector<uint32_t> words_of(const uint8_t* bytes, size_t n) {
    std::vector<uint32_t> w(n);
    if (n) std::memcpy(w.data(), bytes, 4 * n);
    return w;
}

extern "C" {

// D, W [nz][ny][nx] and colour [nz][ny][nx][4]: in and out; rgba uint8 [n_maps][H][W][4]
void colour_host_integrate(int nx, int ny, int nz, const double* origin, double vs, double trunc, double max_weight, double max_depth, int model,
                           const double* intr, int n_maps, int H, int W, const double* depth, const uint8_t* rgba, const double* poses, float* D,
                           float* Wt, float* colour) {
    HostVolume v(nx, ny, nz, origin, vs, D, Wt);
    HostColour hc(v.g, colour);
    TsdfRule r;
    r.trunc = trunc; r.max_depth = max_depth; r.max_weight = max_weight; r.W = W; r.H = H;
    const std::vector<uint32_t> image = words_of(rgba, static_cast<size_t>(n_maps) * H * W);
    host_integrate(v, hc, model, intr, n_maps, H, W, depth, image.data(), poses, r);
    v.planes(D, Wt);
    hc.records(v.g, colour);
}

int64_t colour_host_points(int nx, int ny, int nz, const double* origin, double vs, const float* D, const float* Wt, const float* colour,
                           double min_weight, int64_t cap, uint8_t* rgba) {
    HostVolume v(nx, ny, nz, origin, vs, D, Wt);
    HostColour hc(v.g, colour);
    std::vector<uint32_t> out(static_cast<size_t>(cap));
    const int64_t n = host_points(v, hc, min_weight, cap, out.data());
    if (cap) std::memcpy(rgba, out.data(), 4 * static_cast<size_t>(cap < n ? cap : n));
    return n;
}

// rays [n_px][2], status uint8 [n_px], depth [n_px] of one view at pose7 -> rgba uint8 [n_px][4]
void colour_host_hits(int nx, int ny, int nz, const double* origin, double vs, const float* colour, int64_t n_px, const double* rays,
                      const double* pose7, const uint8_t* status, const double* depth, uint8_t* rgba) {
    HostVolume v(nx, ny, nz, origin, vs, nullptr, nullptr);
    HostColour hc(v.g, colour);
    TsdfRayView view;
    tsdf_ray_view(pose7, &view);
    for (int64_t l = 0; l < n_px; ++l) {
        const uint32_t c = tsdf_colour_hit(hc.col.data(), v.g, view, status[l], depth[l], rays[2 * l], rays[2 * l + 1]);
        std::memcpy(rgba + 4 * l, &c, 4);
    }
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
int main() {
    int bad = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // 1. three views of the plane z = 1 painted {10, 20, 40}, odd nx: every point of the extract has that colour, and so has every
    // coloured hit of a ray cast from the first pose
    {
        const int nx = 13, ny = 10, nz = 12, W = 40, H = 30, n_maps = 3;
        const double origin[3] = {-0.3, -0.22, 0.74}, vs = 0.046875, intr[10] = {60.0, 58.0, 19.5, 14.5, 0.0, -0.05, 0.01, 0.0, 0.0005, -0.0003};
        std::vector<double> depth(static_cast<size_t>(n_maps) * W * H, 1.0), poses(7 * n_maps, 0.0);
        std::vector<uint32_t> image(static_cast<size_t>(n_maps) * W * H, 10u | 20u << 8 | 40u << 16 | 255u << 24);
        for (int m = 0; m < n_maps; ++m) {
            poses[7 * m] = 1.0;
            poses[7 * m + 4] = 0.01 * m;
            depth[static_cast<size_t>(m) * W * H + 7 * m] = nan;
            image[static_cast<size_t>(m) * W * H + 11 * m + 3] = 0u;  // A == 0: D moves, the colour stays
        }
        HostVolume v(nx, ny, nz, origin, vs, nullptr, nullptr);
        HostColour hc(v.g, nullptr);
        TsdfRule r;
        r.trunc = 3 * vs; r.max_depth = std::numeric_limits<double>::infinity(); r.max_weight = 2.0; r.W = W; r.H = H;
        host_integrate(v, hc, 0, intr, n_maps, H, W, depth.data(), image.data(), poses.data(), r);
        const int64_t n = host_points(v, hc, 1.0, 0, nullptr);
        std::vector<uint32_t> rgba(static_cast<size_t>(n) + 1);
        if (host_points(v, hc, 1.0, n, rgba.data()) != n || n < 50) ++bad;
        int coloured = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (rgba[i] == 0u) continue;
            ++coloured;
            if (rgba[i] != (10u | 20u << 8 | 40u << 16 | 255u << 24)) ++bad;
        }
        TsdfRayView view;
        tsdf_ray_view(poses.data(), &view);
        TsdfRayRule rr;
        rr.step = 0.5 * vs; rr.skip = 0.5; rr.near_depth = 0.0; rr.far_depth = std::numeric_limits<double>::infinity(); rr.min_weight = 1.0; rr.trunc = r.trunc;
        int hits = 0, hit_colours = 0;
        for (int py = 0; py < H; py += 3)
            for (int px = 0; px < W; px += 3) {
                const double x = (px - intr[2]) / intr[0], y = (py - intr[3]) / intr[1];
                TsdfRayOut o;
                tsdf_ray_pixel(v.vol.data(), v.g, view, rr, x, y, &o);
                const uint32_t c = tsdf_colour_hit(hc.col.data(), v.g, view, o.status, o.depth, x, y);
                if (o.status != TSDF_RAY_HIT) {
                    if (c != 0u) ++bad;
                    continue;
                }
                ++hits;
                if (c == 0u) continue;
                ++hit_colours;
                if (c != (10u | 20u << 8 | 40u << 16 | 255u << 24)) ++bad;
            }
        std::printf("colour_driver: %lld points, %d with a colour; %d hits, %d with a colour\n", static_cast<long long>(n), coloured, hits, hit_colours);
        if (coloured < n / 2 || hits < 10 || hit_colours == 0) ++bad;
    }
    // 2. the blend by hand: bytes 10, 20, 40 give 10, 15, float32(70 / 3) under max_weight = 2, and Wc stays at 2
    {
        float C[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        tsdf_colour_blend(C, 10u | 255u << 24, 2.0);
        if (C[0] != 10.0f || C[3] != 1.0f) ++bad;
        tsdf_colour_blend(C, 20u | 255u << 24, 2.0);
        if (C[0] != 15.0f || C[3] != 2.0f) ++bad;
        tsdf_colour_blend(C, 40u | 255u << 24, 2.0);
        if (C[0] != static_cast<float>(70.0 / 3.0) || C[3] != 2.0f || C[1] != 0.0f) ++bad;
        if (!tsdf_colour_takes(0.25, 0.25, 1u << 24) || tsdf_colour_takes(0.2500000000000001, 0.25, 1u << 24) || tsdf_colour_takes(0.0, 0.25, 0xffffffu)) ++bad;
    }
    // 3. rounding: x.5 goes up, the ends clamp, NaN gives 0
    if (tsdf_colour_byte(0.5) != 1u || tsdf_colour_byte(0.49999) != 0u || tsdf_colour_byte(254.5) != 255u || tsdf_colour_byte(300.0) != 255u ||
        tsdf_colour_byte(-3.0) != 0u || tsdf_colour_byte(nan) != 0u || tsdf_colour_byte(127.5) != 128u)
        ++bad;
    std::printf("colour_driver: %d mismatches\n", bad);
    return bad != 0;
}
#endif
