// sl_driver.cpp — TEST-ONLY: extern "C" wrapper of structured_light_math.hpp for ctypes (tests/test_structured_light_cpu.py).  It
// fills the rule as the library's host glue does, generates the patterns with the library's generator and decodes every pixel with
// the functions every lane runs, four pixels of a row at a time and one image after the other.  Built with -DCBA_HOST_DRIVER_MAIN it is
// a stand-alone program (for the sanitizers): it generates a sequence, decodes it as a camera that is the projector and checks that
// every pixel decodes to its own index.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../calibration_amd/csrc/structured_light_math.hpp"

using namespace cba;

static cba_sl_options sl_opts(int pw, int ph, int axes, int s, int N, int T, int min_contrast, int min_bit_diff, double min_modulation) {
    cba_sl_options o;
    o.proj_width = pw; o.proj_height = ph; o.axes = axes; o.gray_skip_bits = s; o.phase_steps = N; o.phase_period = T;
    o.min_contrast = min_contrast; o.min_bit_diff = min_bit_diff; o.min_modulation = min_modulation;
    return o;
}

// four pixels of row `row` from column c0 of image `img` (zeros past the row's end)
static uint32_t pack_at(const uint8_t* img, int W, int row, int c0) {
    uint32_t w = 0;
    for (int i = 0; i < 4 && c0 + i < W; ++i) w |= static_cast<uint32_t>(img[static_cast<size_t>(row) * W + c0 + i]) << (8 * i);
    return w;
}

extern "C" {

void sl_host_patterns(int pw, int ph, int axes, int s, int N, int T, int min_contrast, int min_bit_diff, double min_modulation, uint8_t* out) {
    sl_patterns(sl_opts(pw, ph, axes, s, N, T, min_contrast, min_bit_diff, min_modulation), out);
}

// cba_sl_decoder_create + _process in one call: images [n_seq][n_images][H][W]
void sl_host_decode(int pw, int ph, int axes, int s, int N, int T, int min_contrast, int min_bit_diff, double min_modulation, int W, int H,
                    int n_seq, const uint8_t* images, double* coord, double* modulation, uint8_t* status) {
    SlRule r;
    sl_fill_rule(sl_opts(pw, ph, axes, s, N, T, min_contrast, min_bit_diff, min_modulation), &r);
    const int n_images = sl_image_count(r);
    const size_t plane = static_cast<size_t>(W) * H;
    for (int q = 0; q < n_seq; ++q) {
        const uint8_t* stack = images + static_cast<size_t>(q) * n_images * plane;
        for (int row = 0; row < H; ++row)
            for (int c0 = 0; c0 < W; c0 += 4) {
                uint32_t st = sl_low_contrast(pack_at(stack, W, row, c0), pack_at(stack + plane, W, row, c0), r.min_contrast);
                const uint8_t* img = stack + 2 * plane;
                for (int ai = 0; ai < r.n_axes; ++ai) {
                    const SlAxis& ax = r.axis[ai];
                    const int shift = 1 + 3 * (r.first_axis + ai);
                    int code[4] = {0, 0, 0, 0};
                    uint32_t bin = 0, unc = 0;
                    for (int b = 0; b < ax.nbits; ++b, img += 2 * plane) {
                        sl_gray_plane(pack_at(img, W, row, c0), pack_at(img + plane, W, row, c0), r.min_bit_diff, &bin, &unc);
                        for (int i = 0; i < 4; ++i) sl_code_push(&code[i], bin, i);
                    }
                    st |= unc << shift;
                    double S[4] = {0, 0, 0, 0}, C[4] = {0, 0, 0, 0};
                    for (int k = 0; k < ax.N; ++k, img += plane) {
                        const uint32_t w = pack_at(img, W, row, c0);
                        for (int i = 0; i < 4; ++i) sl_phase_push(r, k, sl_byte(w, i), &S[i], &C[i]);
                    }
                    for (int i = 0; i < 4 && c0 + i < W; ++i) {
                        const uint32_t sb = sl_byte(st, i);
                        const bool skip = (sb & (SL_LOW_CONTRAST | SL_UNCERTAIN << shift)) != 0u;
                        const size_t at = (static_cast<size_t>(q) * r.n_axes + ai) * plane + static_cast<size_t>(row) * W + c0 + i;
                        st |= (sl_axis_finish(ax, skip, code[i], S[i], C[i], r.min_modulation, &coord[at], &modulation[at]) << shift) << (8 * i);
                    }
                }
                st &= ~((st & SL_ONES) * 0xfeu);  // low contrast: bit 0 alone
                for (int i = 0; i < 4 && c0 + i < W; ++i) status[static_cast<size_t>(q) * plane + static_cast<size_t>(row) * W + c0 + i] = static_cast<uint8_t>(sl_byte(st, i));
            }
    }
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
int main() {
    int bad = 0;
    const int cases[][5] = {{37, 21, 0, 0, 16}, {37, 21, 0, 4, 16}, {200, 120, 3, 3, 16}, {2, 2, 0, 0, 16}, {33, 5, 2, 8, 8}};  // pw ph s N T
    for (const auto& c : cases) {
        const cba_sl_options o = sl_opts(c[0], c[1], 3, c[2], c[3], c[4], 10, 4, 5.0);
        SlRule r;
        sl_fill_rule(o, &r);
        const int n = sl_image_count(r);
        const size_t plane = static_cast<size_t>(c[0]) * c[1];
        std::vector<uint8_t> pats(n * plane), status(plane);
        std::vector<double> coord(2 * plane), mod(2 * plane);
        sl_patterns(o, pats.data());
        sl_host_decode(c[0], c[1], 3, c[2], c[3], c[4], 10, 4, 5.0, c[0], c[1], 1, pats.data(), coord.data(), mod.data(), status.data());
        const double half = 0.5 * ((1 << c[2]) - 1), bar = c[3] ? 0.05 : 0.0;  // Gray only: the stripe's centre, exactly
        for (int y = 0; y < c[1]; ++y)
            for (int x = 0; x < c[0]; ++x) {
                const size_t i = static_cast<size_t>(y) * c[0] + x;
                const double wx = c[3] ? x : ((x >> c[2]) << c[2]) + half, wy = c[3] ? y : ((y >> c[2]) << c[2]) + half;
                // a stripe that reaches past the panel's end has its centre outside: those pixels are "outside" by the rule
                const bool out_x = ((x >> c[2]) << c[2]) + half > c[0] - 1, out_y = ((y >> c[2]) << c[2]) + half > c[1] - 1;
                const int want = (out_x ? 4 : 0) | (out_y ? 32 : 0);
                if (status[i] != want) ++bad;
                if (!out_x && !(std::fabs(coord[i] - wx) <= bar)) ++bad;
                if (!out_y && !(std::fabs(coord[plane + i] - wy) <= bar)) ++bad;
            }
    }
    std::printf("sl_driver: %d mismatches\n", bad);
    return bad != 0;
}
#endif
