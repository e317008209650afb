// stereo_driver.cpp — TEST-ONLY: extern "C" wrapper of stereo_math.hpp for ctypes (tests/test_stereo_cpu.py) and, built with
// -DCBA_HOST_DRIVER_MAIN, a stand-alone program whose main checks itself (for the sanitizers).  It fills the geometry as
// stereo_match.hip's host glue does and walks every pixel with stereo_match_pair (the naive window sum that every tiling of the
// kernels must reproduce).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../calibration_amd/csrc/stereo_math.hpp"

using namespace cba;

extern "C" {

// the arguments of cba_stereo_rectify after its pointer and size checks; 0 on success
int st_rectify(const double* intr, int ni, const double* c_T_r, int W, int H, double focal, double cx, double cy, double* R, double* new_k5,
               double* baseline, double* r_T_rect) {
    return stereo_rectify(intr, ni, c_T_r, W, H, focal, cx, cy, R, new_k5, baseline, r_T_rect) ? 1 : 0;
}

// cba_stereo_matcher_create + _process in one call; geom [4] = f, cx, cy, B or null; pose7 or null
void st_match(int W, int H, int n_pairs, int dmin, int D, int r, int uniqueness_percent, int lr_max_diff, int subpixel, const uint8_t* left,
              const uint8_t* right, const double* geom, const double* pose7, float* disparity, int32_t* cost, float* xyz) {
    StereoGeom g;
    if (geom) stereo_fill_geom(geom[0], geom[1], geom[2], geom[3], pose7, &g);
    const StereoMatchParams p = {W, H, dmin, D, r, uniqueness_percent, lr_max_diff, subpixel};
    const size_t px = static_cast<size_t>(W) * H;
    for (int i = 0; i < n_pairs; ++i)
        stereo_match_pair(p, left + i * px, right + i * px, geom ? &g : nullptr, disparity + i * px, cost ? cost + i * px : nullptr,
                          xyz ? xyz + 3 * i * px : nullptr);
}

void st_points(const double* geom, const double* pose7, int64_t n, const double* uvd, double* xyz) {
    StereoGeom g;
    stereo_fill_geom(geom[0], geom[1], geom[2], geom[3], pose7, &g);
    for (int64_t i = 0; i < n; ++i) stereo_point(g, uvd[3 * i], uvd[3 * i + 1], uvd[3 * i + 2], xyz + 3 * i);
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
// Self-check: a textured pair moved by 5 columns must come back as disparity 5 wherever 5 is admissible, at every window size and
// with every switch on; rectification of a toe-in rig must give orthonormal rotations; the error paths return an error.
int main() {
    const int W = 67, H = 29, shift = 5;
    std::vector<uint8_t> T(static_cast<size_t>(H) * (W + shift)), L(static_cast<size_t>(W) * H), R(L.size());
    uint32_t s = 12345u;
    for (auto& t : T) { s = s * 1664525u + 1013904223u; t = static_cast<uint8_t>(s >> 24); }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            R[y * W + x] = T[y * (W + shift) + x + shift];
            L[y * W + x] = T[y * (W + shift) + x];  // L(x) = R(x - shift)
        }
    int bad = 0;
    const double geom[4] = {100.0, 33.0, 14.0, 0.1}, pose[7] = {1.0, 0.0, 0.0, 0.0, 0.1, 0.2, 0.3};
    for (int r : {1, 4, 10})
        for (int lr : {-1, 1}) {
            std::vector<float> disp(L.size()), xyz(3 * L.size());
            std::vector<int32_t> cost(L.size());
            st_match(W, H, 1, -3, 40, r, 10, lr, 1, L.data(), R.data(), geom, pose, disp.data(), cost.data(), xyz.data());
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const bool adm = y >= r && y <= H - 1 - r && x >= r && x <= W - 1 - r && x - r - shift >= 0;
                    const float d = disp[y * W + x];
                    if (adm && !(std::fabs(d - 5.0f) < 0.5f && cost[y * W + x] == 0 && xyz[3 * (y * W + x) + 2] > 0.3f)) ++bad;
                    if (!(y >= r && y <= H - 1 - r && x >= r && x <= W - 1 - r) && (d == d || cost[y * W + x] != -1)) ++bad;
                }
        }
    const double intr[20] = {800, 790, 320, 240, 0, 0, 0, 0, 0, 0, 810, 805, 315, 236, 0, 0, 0, 0, 0, 0};
    double c_T_r[14] = {1, 0, 0, 0, 0, 0, 0, 0.999, 0.0, 0.04, 0.0, -0.2, 0.01, 0.0};
    double Ro[18], K[10], B, rt[7];
    if (st_rectify(intr, 10, c_T_r, 640, 480, 0, 0, 0, Ro, K, &B, rt)) ++bad;
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double dot = 0.0;
                for (int k = 0; k < 3; ++k) dot += Ro[9 * c + 3 * i + k] * Ro[9 * c + 3 * j + k];
                if (std::fabs(dot - (i == j)) > 1e-12) ++bad;
            }
    c_T_r[11] = 0.0; c_T_r[12] = 0.0;
    if (!st_rectify(intr, 10, c_T_r, 640, 480, 0, 0, 0, Ro, K, &B, rt)) ++bad;  // no baseline
    c_T_r[13] = 0.5; c_T_r[9] = 0.0;
    if (!st_rectify(intr, 10, c_T_r, 640, 480, 0, 0, 0, Ro, K, &B, rt)) ++bad;  // the axes along the baseline
    std::printf("stereo self-check: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
