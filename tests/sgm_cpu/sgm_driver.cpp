// sgm_driver.cpp — TEST-ONLY: extern "C" wrapper of sgm_math.hpp for ctypes (tests/sgm_ref.py) and, built with
// -DCBA_HOST_DRIVER_MAIN, a stand-alone program whose main checks itself (for the sanitizers).  It fills the geometry as the host glue
// of stereo_sgm.hip does and walks every path of every pair with sgm_match_pair (the scalar recurrence that the packed kernel must
// reproduce).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../calibration_amd/csrc/sgm_math.hpp"

using namespace cba;

extern "C" {

// cba_sgm_matcher_create + _process in one call; geom [4] = f, cx, cy, B or null; pose7 or null
void sgm_match(int W, int H, int n_pairs, int dmin, int D, int p1, int p2, int paths, int uniqueness_percent, int lr_max_diff, int subpixel,
               const uint8_t* left, const uint8_t* right, const double* geom, const double* pose7, float* disparity, int32_t* cost, float* xyz) {
    StereoGeom g;
    if (geom) stereo_fill_geom(geom[0], geom[1], geom[2], geom[3], pose7, &g);
    const SgmParams p = {W, H, dmin, D, p1, p2, paths, uniqueness_percent, lr_max_diff, subpixel};
    const size_t px = static_cast<size_t>(W) * H;
    for (int i = 0; i < n_pairs; ++i)
        sgm_match_pair(p, left + i * px, right + i * px, geom ? &g : nullptr, disparity + i * px, cost ? cost + i * px : nullptr,
                       xyz ? xyz + 3 * i * px : nullptr);
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
// Self-check: a textured pair moved by 5 columns must come back as disparity 5 in the interior (where no census window sees an image
// border; the path sums there need not be 0, since a path carries what it met at the border), for 4 and 8 paths, an odd size and a D
// that is no multiple of 16.
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
    for (int paths : {4, 8})
        for (int lr : {-1, 1}) {
            std::vector<float> disp(L.size()), xyz(3 * L.size());
            std::vector<int32_t> cost(L.size());
            sgm_match(W, H, 1, -3, 37, 4, 32, paths, 10, lr, 1, L.data(), R.data(), geom, pose, disp.data(), cost.data(), xyz.data());
            for (int y = SGM_CENSUS_HY; y < H - SGM_CENSUS_HY; ++y)
                for (int x = shift + SGM_CENSUS_HX; x < W - SGM_CENSUS_HX; ++x) {
                    const float d = disp[y * W + x];
                    if (!(std::fabs(d - 5.0f) < 0.5f && cost[y * W + x] >= 0 && xyz[3 * (y * W + x) + 2] > 0.3f)) ++bad;
                }
        }
    // one row, one column, one pixel: whole path families have no predecessor
    for (int w : {1, 9})
        for (int h : {1, 7}) {
            std::vector<float> disp(static_cast<size_t>(w) * h);
            std::vector<int32_t> cost(disp.size());
            sgm_match(w, h, 1, 0, 17, 1023, 1023, 8, 0, 1, 1, L.data(), R.data(), nullptr, nullptr, disp.data(), cost.data(), nullptr);
            for (size_t i = 0; i < disp.size(); ++i)
                if (cost[i] < 0) ++bad;  // d = 0 is admissible everywhere
        }
    std::printf("sgm self-check: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
