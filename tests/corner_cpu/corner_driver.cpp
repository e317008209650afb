// corner_driver.cpp — TEST-ONLY: extern "C" wrapper of corner_math.hpp and corner_grid.hpp for ctypes (tests/test_corner_cpu.py) and,
// built with -DCBA_HOST_DRIVER_MAIN, a stand-alone program whose main checks itself (for the sanitizers).  It makes the tables as
// corner_detect.hip's host glue does and walks every pixel with corner_detect_image.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../calibration_amd/csrc/corner_math.hpp"
#include "../../calibration_amd/csrc/corner_grid.hpp"

using namespace cba;

extern "C" {

// cba_corner_detector_create + _process in one call; resp [n][H][W] optional
void cr_detect(int W, int H, int n_images, int max_corners, int min_response, int nms, int cog, int refine, int w, int iters,
               const uint8_t* images, int32_t* count, int32_t* status, double* xy, double* angle, int32_t* response, int32_t* flags,
               int16_t* resp) {
    const CornerParams p = {W, H, max_corners, min_response, nms, cog, refine, w, iters};
    std::vector<double> wt(static_cast<size_t>(2 * w + 1) * (2 * w + 1)), trig(16);
    corner_weight_table(w, wt.data());
    corner_trig_table(trig.data());
    const size_t px = static_cast<size_t>(W) * H;
    std::vector<int16_t> R(px);
    for (int i = 0; i < n_images; ++i) {
        const size_t s = static_cast<size_t>(i) * max_corners;
        corner_detect_image(p, images + i * px, wt.data(), trig.data(), R.data(), count + i, status + i, xy + 2 * s, angle + s, response + s,
                            flags + s);
        if (resp) std::copy(R.begin(), R.end(), resp + i * px);
    }
}

void cr_tables(int w, double* wt, double* trig) {
    corner_weight_table(w, wt);
    corner_trig_table(trig);
}

int cr_order(int n, const double* xy, const double* angle, int rows, int cols, int32_t* index) {
    return chessboard_order(n, xy, angle, rows, cols, index);
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
// Self-check: an ideal board of 14-pixel squares must give its 5 x 4 inner corners, every refinement within 0.6 px of the truth, and
// the grid order must be the identity of the row-major list; a constant image has no peak; max_corners = 3 overflows; a lattice with
// one corner missing is not found.
int main() {
    const int W = 131, H = 97, sq = 14, cols = 5, rows = 4, ox = 20, oy = 15;
    std::vector<uint8_t> img(static_cast<size_t>(W) * H, 128);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int i = (x - ox + sq) / sq, j = (y - oy + sq) / sq;  // squares (cols + 1) x (rows + 1), the first starts at ox - sq
            if (x >= ox - sq && y >= oy - sq && i <= cols && j <= rows) img[y * W + x] = (i + j) & 1 ? 210 : 40;
        }
    int bad = 0;
    const int M = 64;
    std::vector<double> xy(2 * M), angle(M);
    std::vector<int32_t> response(M), flags(M), index(rows * cols);
    int32_t count = 0, status = 0;
    for (int refine = 0; refine < 3; ++refine) {
        cr_detect(W, H, 1, M, 400, 3, 2, refine, 5, 5, img.data(), &count, &status, xy.data(), angle.data(), response.data(), flags.data(),
                  nullptr);
        if (count != rows * cols || status != 0) { ++bad; continue; }
        for (int c = 0; c < count; ++c) {
            const double tx = ox + sq * (c % cols) - 0.5, ty = oy + sq * (c / cols) - 0.5;  // the corner lies between two pixels
            if (std::fabs(xy[2 * c] - tx) > 0.6 || std::fabs(xy[2 * c + 1] - ty) > 0.6 || flags[c]) ++bad;
        }
        if (!cr_order(count, xy.data(), angle.data(), rows, cols, index.data())) { ++bad; continue; }
        for (int c = 0; c < count; ++c)
            if (index[c] != c) ++bad;
        if (cr_order(count - 1, xy.data(), angle.data(), rows, cols, index.data())) ++bad;
        if (cr_order(count - 1, xy.data() + 2, angle.data() + 1, rows, cols - 1, index.data())) ++bad;
    }
    cr_detect(W, H, 1, 3, 400, 3, 2, 2, 5, 5, img.data(), &count, &status, xy.data(), angle.data(), response.data(), flags.data(), nullptr);
    if (count != rows * cols || status != CORNER_STATUS_OVERFLOW) ++bad;
    std::vector<uint8_t> flat(static_cast<size_t>(W) * H, 77);
    cr_detect(W, H, 1, M, 1, 1, 1, 2, 1, 1, flat.data(), &count, &status, xy.data(), angle.data(), response.data(), flags.data(), nullptr);
    if (count != 0 || status != 0 || xy[0] == xy[0]) ++bad;
    std::printf("corner self-check: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
