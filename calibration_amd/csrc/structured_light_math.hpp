// structured_light_math.hpp — structured-light decoding (calibba.h: cba_sl_patterns, cba_sl_decoder) as __host__ __device__ code: the
// value of a pattern pixel and the decode of one axis of a camera pixel by the rule calibba.h states (Gray bits, prefix XOR, coarse
// coordinate, phase sums, unwrap, status bits).  k_sl_decode (structured_light.hip), the host generator behind cba_sl_patterns and
// tests/sl_cpu (the same header under g++) all call these functions: there is one copy of the rule.
// The reference has no counterpart.
//
//   packs          the uint8 compares act on a dword of four pixels at once (SWAR in plain C++, the same on host and device): a pack
//                  is split into its even and odd bytes, each in a 16-bit field, where 512 + a - b - d keeps bit 9 exactly when
//                  a >= b + d (all of a, b, d in 0..255: the field holds 2..767).  A mask has 0x01 in the byte of every pixel it names.
//   Gray planes    sl_gray_plane folds one (pattern, inverse) pair into the pack's running binary bit (the prefix XOR from the MSB)
//                  and its "uncertain" mask; sl_code_push appends a pixel's bit to its code
//   phase sums     sl_phase_push: S += I ws[k], C += I wc[k], products rounded before adding
//   finish         sl_axis_finish: coarse coordinate, outside test, modulation, unwrap
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "camera_math.hpp"

namespace cba {

constexpr int SL_MAX_STEPS = 8;
// status bits of one axis, before the shift by 1 + 3 axis; bit 0 of the status byte is SL_LOW_CONTRAST
enum : uint32_t { SL_LOW_CONTRAST = 1u, SL_UNCERTAIN = 1u, SL_OUTSIDE = 2u, SL_LOW_MODULATION = 4u };
constexpr uint32_t SL_ONES = 0x01010101u;

// one decoded axis: P projector pixels, nbits Gray planes, stripes of 2^s pixels, N phase steps of period T (N == 0: none)
struct SlAxis {
    int P, nbits, s, N, T;
};

// what the kernel needs of the options: a kernel argument, wave-uniform
struct SlRule {
    SlAxis axis[2];  // the selected axes in order; n_axes of them
    int n_axes;
    int first_axis;  // 0 or 1: the projector axis of axis[0] (its status bits are 1 + 3 first_axis ...)
    int min_contrast, min_bit_diff;
    double min_modulation;
    double ws[SL_MAX_STEPS], wc[SL_MAX_STEPS];  // sin / cos (2 pi k / N), formed on the host by the C library
};

// max(1, ceil(log2 P)) - s
CBA_HD int sl_nbits(int P, int s) {
    int b = 1;
    while ((1 << b) < P) ++b;
    return b - s;
}

// images of a sequence for these axes: white, black, then 2 nbits + N per axis
CBA_HD int sl_image_count(const SlRule& r) {
    int n = 2;
    for (int a = 0; a < r.n_axes; ++a) n += 2 * r.axis[a].nbits + r.axis[a].N;
    return n;
}

// ---- patterns ------------------------------------------------------------------------------------------------------------------------
// Gray plane b (0 = MSB) at projector index j: 255 or 0
CBA_HD int sl_pattern_gray(const SlAxis& ax, int b, int j) {
    const int c = j >> ax.s, g = c ^ (c >> 1);
    return (g >> (ax.nbits - 1 - b)) & 1 ? 255 : 0;
}

// phase step k at projector index j: m = (j N - k T) mod (N T); cos(2 pi m / (N T)) with its two zeros exact
CBA_HD int sl_pattern_phase(const SlAxis& ax, int k, int j) {
    const int64_t NT = static_cast<int64_t>(ax.N) * ax.T;
    int64_t m = (static_cast<int64_t>(j) * ax.N - static_cast<int64_t>(k) * ax.T) % NT;
    if (m < 0) m += NT;
    const double c = (4 * m == NT || 4 * m == 3 * NT) ? 0.0 : cos(2.0 * 3.14159265358979323846 * static_cast<double>(m) / static_cast<double>(NT));
    const double v = floor(127.5 * (1.0 + c) + 0.5);
    return v < 0.0 ? 0 : v > 255.0 ? 255 : static_cast<int>(v);
}

// the options as the kernel reads them (checked by the caller); host only: the weights come from the C library
inline void sl_fill_rule(const cba_sl_options& o, SlRule* r) {
    *r = SlRule{};
    r->first_axis = (o.axes & 1) ? 0 : 1;
    for (int a = 0; a < 2; ++a) {
        if (!(o.axes >> a & 1)) continue;
        SlAxis& ax = r->axis[r->n_axes++];
        ax.P = a == 0 ? o.proj_width : o.proj_height;
        ax.s = o.gray_skip_bits;
        ax.nbits = sl_nbits(ax.P, ax.s);
        ax.N = o.phase_steps;
        ax.T = o.phase_period;
    }
    r->min_contrast = o.min_contrast;
    r->min_bit_diff = o.min_bit_diff;
    r->min_modulation = o.min_modulation;
    for (int k = 0; k < o.phase_steps; ++k) {
        r->ws[k] = std::sin(2.0 * 3.14159265358979323846 * k / o.phase_steps);
        r->wc[k] = std::cos(2.0 * 3.14159265358979323846 * k / o.phase_steps);
    }
}

// the generator behind cba_sl_patterns: out [n_images][proj_height][proj_width]; host only
inline void sl_patterns(const cba_sl_options& o, uint8_t* out) {
    SlRule r;
    sl_fill_rule(o, &r);
    const int PW = o.proj_width, PH = o.proj_height;
    const size_t plane = static_cast<size_t>(PW) * PH;
    uint8_t* img = out;
    for (size_t i = 0; i < plane; ++i) { img[i] = 255; img[plane + i] = 0; }
    img += 2 * plane;
    for (int ai = 0; ai < r.n_axes; ++ai) {
        const SlAxis& ax = r.axis[ai];
        const bool cols = r.first_axis + ai == 0;
        for (int i = 0; i < 2 * ax.nbits + ax.N; ++i, img += plane) {
            for (int y = 0; y < PH; ++y)
                for (int x = 0; x < PW; ++x) {
                    const int j = cols ? x : y;
                    int v;
                    if (i < 2 * ax.nbits) {
                        v = sl_pattern_gray(ax, i >> 1, j);
                        if (i & 1) v = 255 - v;
                    } else {
                        v = sl_pattern_phase(ax, i - 2 * ax.nbits, j);
                    }
                    img[static_cast<size_t>(y) * PW + x] = static_cast<uint8_t>(v);
                }
        }
    }
}

// ---- packs of four pixels ------------------------------------------------------------------------------------------------------------
// the mask of the bytes with a >= b + d; d in 0..255
CBA_HD uint32_t sl_ge(uint32_t a, uint32_t b, uint32_t d) {
    const uint32_t F = 0x00ff00ffu, D = d * 0x00010001u, K = 0x02000200u;
    const uint32_t e = ((a & F) + K - (b & F) - D) >> 9 & 0x00010001u;
    const uint32_t o = (((a >> 8) & F) + K - ((b >> 8) & F) - D) >> 9 & 0x00010001u;
    return e | o << 8;
}

// white - black < min_contrast
CBA_HD uint32_t sl_low_contrast(uint32_t white, uint32_t black, int min_contrast) {
    return ~sl_ge(white, black, static_cast<uint32_t>(min_contrast)) & SL_ONES;
}

// one Gray plane p with its inverse q: the bit p > q enters the running binary bit `bin`; |p - q| < min_bit_diff marks the pixel
CBA_HD void sl_gray_plane(uint32_t p, uint32_t q, int min_bit_diff, uint32_t* bin, uint32_t* uncertain) {
    const uint32_t d = static_cast<uint32_t>(min_bit_diff);
    *bin ^= sl_ge(p, q, 1u);
    *uncertain |= ~(sl_ge(p, q, d) | sl_ge(q, p, d)) & SL_ONES;
}

// byte i (0..3) of a pack
CBA_HD uint32_t sl_byte(uint32_t w, int i) { return w >> (8 * i) & 0xffu; }

// pixel i's binary bit joins its code, MSB first
CBA_HD void sl_code_push(int* c, uint32_t bin, int i) { *c = *c << 1 | static_cast<int>(sl_byte(bin, i) & 1u); }

// ---- one pixel -----------------------------------------------------------------------------------------------------------------------
// sample I of phase step k
CBA_HD void sl_phase_push(const SlRule& r, int k, uint32_t I, double* S, double* C) {
    CBA_NO_CONTRACT
    const double v = static_cast<double>(I);
    const double ps = v * r.ws[k], pc = v * r.wc[k];
    *S = *S + ps;
    *C = *C + pc;
}

// The axis of one pixel after its planes and steps.  skip: low contrast or an uncertain bit (nothing is evaluated).  Returns SL_OUTSIDE,
// SL_LOW_MODULATION or 0; *coord is finite exactly when it returns 0 and skip is false; *mod is the modulation where it was evaluated
// (low modulation included), NaN otherwise and without phase steps.
CBA_HD uint32_t sl_axis_finish(const SlAxis& ax, bool skip, int c, double S, double C, double min_modulation, double* coord, double* mod) {
    CBA_NO_CONTRACT
    *coord = NAN;
    *mod = NAN;
    if (skip) return 0u;
    const double xg = static_cast<double>(static_cast<int64_t>(c) << ax.s) + 0.5 * static_cast<double>((1 << ax.s) - 1);
    if (xg > static_cast<double>(ax.P - 1)) return SL_OUTSIDE;
    if (ax.N == 0) {
        *coord = xg;
        return 0u;
    }
    const double ss = S * S, cc = C * C;
    const double m = (2.0 / static_cast<double>(ax.N)) * sqrt(ss + cc);
    *mod = m;
    if (m < min_modulation) return SL_LOW_MODULATION;
    const double two_pi = 2.0 * 3.14159265358979323846, T = static_cast<double>(ax.T);
    double phi = atan2(S, C);
    if (phi < 0.0) phi = phi + two_pi;
    const double f = phi * T / two_pi;
    const double kk = rint((xg - f) / T);
    const double kT = kk * T;
    *coord = kT + f;
    return 0u;
}

}  // namespace cba
