// circle_driver.cpp — TEST-ONLY: extern "C" wrapper of blob_math.hpp and circle_grid.hpp for ctypes (tests/test_circle_cpu.py) and,
// built with -DCBA_HOST_DRIVER_MAIN, a stand-alone program whose main checks itself (for the sanitizers).  It makes the ray table as
// blob_detect.hip's host glue does and walks every pixel with blob_detect_image.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../calibration_amd/csrc/blob_math.hpp"
#include "../../calibration_amd/csrc/circle_grid.hpp"

using namespace cba;

extern "C" {

// cba_blob_detector_create + _process in one call; resp [n][H][W] and s_in [n][H][W] optional
void cc_detect(int W, int H, int n_images, int max_blobs, int polarity, int a, int b, int min_contrast, int nms, int max_radius, int rounds,
               double max_fit_error, double max_axis_ratio, double min_radius, const uint8_t* images, int32_t* count, int32_t* status,
               double* xy, double* shape, double* fit_error, int32_t* response, int32_t* flags, int32_t* resp, uint16_t* s_in) {
    const BlobParams p = {W, H, max_blobs, polarity, a, b, min_contrast, nms, max_radius, rounds, max_fit_error, max_axis_ratio, min_radius};
    std::vector<double> rays(2 * BLOB_RAYS);
    blob_ray_table(rays.data());
    const size_t px = static_cast<size_t>(W) * H;
    std::vector<int32_t> R(px);
    std::vector<uint16_t> S(px);
    for (int i = 0; i < n_images; ++i) {
        const size_t s = static_cast<size_t>(i) * max_blobs;
        blob_detect_image(p, images + i * px, rays.data(), R.data(), S.data(), count + i, status + i, xy + 2 * s, shape + 3 * s, fit_error + s,
                          response + s, flags + s);
        if (resp) std::copy(R.begin(), R.end(), resp + i * px);
        if (s_in) std::copy(S.begin(), S.end(), s_in + i * px);
    }
}

void cc_rays(double* rays) { blob_ray_table(rays); }

int cc_order(int n, const double* xy, const double* shape, int pattern, int rows, int cols, int32_t* index, int32_t* unique) {
    int u = 0;
    const int found = circle_grid_order(n, xy, shape, pattern, rows, cols, index, &u);
    *unique = u;
    return found;
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
// Self-check: an ideal asymmetric 5 x 3 grid of dark discs of radius 5 at pitch 14 must give its 15 blobs without a flag, every centre
// within 0.1 px of the truth, one labelling (unique) equal to the construction; one blob less is not found; max_blobs = 3 overflows;
// a constant image has no peak.
int main() {
    const int W = 141, H = 117, rows = 5, cols = 3, d = 14, ox = 30, oy = 30;
    const double rad = 5.0;
    const int ss = 8;
    std::vector<uint8_t> img(static_cast<size_t>(W) * H);
    std::vector<double> truth;
    for (int j = 0; j < rows; ++j)
        for (int i = 0; i < cols; ++i) {
            truth.push_back(ox + (2 * i + (j & 1)) * d);
            truth.push_back(oy + j * d);
        }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int in = 0;
            for (int sy = 0; sy < ss; ++sy)
                for (int sx = 0; sx < ss; ++sx) {
                    const double u = x + (sx + 0.5) / ss - 0.5, v = y + (sy + 0.5) / ss - 0.5;
                    for (size_t c = 0; c < truth.size(); c += 2)
                        if ((u - truth[c]) * (u - truth[c]) + (v - truth[c + 1]) * (v - truth[c + 1]) <= rad * rad) { ++in; break; }
                }
            img[y * W + x] = static_cast<uint8_t>(210 - (170 * in + ss * ss / 2) / (ss * ss));
        }
    int bad = 0;
    const int M = 32, need = rows * cols;
    std::vector<double> xy(2 * M), shape(3 * M), fit(M);
    std::vector<int32_t> response(M), flags(M), index(need);
    int32_t count = 0, status = 0, unique = 0;
    cc_detect(W, H, 1, M, BLOB_DARK, 2, 9, 30, 3, 12, 3, 0.2, 3.0, 1.5, img.data(), &count, &status, xy.data(), shape.data(), fit.data(),
              response.data(), flags.data(), nullptr, nullptr);
    if (count != need || status != 0) ++bad;
    else {
        for (int c = 0; c < need; ++c)
            if (flags[c] || std::fabs(xy[2 * c] - truth[2 * c]) > 0.1 || std::fabs(xy[2 * c + 1] - truth[2 * c + 1]) > 0.1) ++bad;
        if (!cc_order(count, xy.data(), shape.data(), CIRCLES_ASYMMETRIC, rows, cols, index.data(), &unique) || !unique) ++bad;
        else
            for (int c = 0; c < need; ++c)
                if (index[c] != c) ++bad;
        if (!cc_order(count, xy.data(), nullptr, CIRCLES_ASYMMETRIC, rows, cols, index.data(), &unique)) ++bad;
        if (cc_order(count - 1, xy.data() + 2, shape.data() + 3, CIRCLES_ASYMMETRIC, rows, cols, index.data(), &unique)) ++bad;
        if (cc_order(count, xy.data(), shape.data(), CIRCLES_SYMMETRIC, rows, cols, index.data(), &unique)) ++bad;
    }
    cc_detect(W, H, 1, 3, BLOB_DARK, 2, 9, 30, 3, 12, 3, 0.2, 3.0, 1.5, img.data(), &count, &status, xy.data(), shape.data(), fit.data(),
              response.data(), flags.data(), nullptr, nullptr);
    if (count != need || status != BLOB_STATUS_OVERFLOW) ++bad;
    std::vector<uint8_t> flat(static_cast<size_t>(W) * H, 77);
    cc_detect(W, H, 1, M, BLOB_BRIGHT, 7, 15, 1, 10, 32, 8, 0.2, 3.0, 1.5, flat.data(), &count, &status, xy.data(), shape.data(), fit.data(),
              response.data(), flags.data(), nullptr, nullptr);
    if (count != 0 || status != 0 || xy[0] == xy[0]) ++bad;
    std::printf("circle self-check: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
