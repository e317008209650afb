// marker_math.hpp — the per-corner and per-cell pieces of ChArUco detection (calibba.h: cba_charuco_detector) as __host__ __device__
// code.  The kernels of marker_read.hip call them; tests/charuco_cpu compiles the same header with g++.  Every sum has a fixed order and
// nothing is contracted into FMAs, so the host build and the device agree to the bit.
//
//   arms        corner_arms_one: the arm test of one corner from its 12 direction vectors (the host makes them with cos / sin)
//   homography  marker_homography: Heckbert's closed form, unit square -> quad
//   cells       marker_cell_mean: the mean of cell_samples^2 bilinear samples of one marker cell
//   codes       marker_code_of: the inner code out of the 128-bit mask of bright cells; marker_rotate; marker_border_mask
//   reading     marker_read_one: the whole rule for one lattice cell on the host (what one wavefront of k_marker_read must reproduce)
#pragma once
#include <cmath>
#include <cstdint>

#include "corner_math.hpp"

namespace cba {

constexpr int MARKER_FLAG_DEGENERATE = 1, MARKER_FLAG_WINDOW = 2, MARKER_FLAG_LOW_CONTRAST = 4, MARKER_FLAG_BORDER = 8,
              MARKER_FLAG_NO_MATCH = 16;
constexpr int MARKER_MAX_BITS = 7, MARKER_MAX_CELLS = (MARKER_MAX_BITS + 2) * (MARKER_MAX_BITS + 2);  // 81: a lane owns at most two
constexpr int MARKER_MAX_CODES = 16384;         // 4 id + rotation stays below 2^16
constexpr double MARKER_DEGENERATE_REL = 1e-12;
constexpr int MARKER_NO_KEY = 0x7fffffff;

// one record per lattice cell, as cba_marker_reading
struct MarkerReading {
    uint64_t code;
    double level_min, level_max;
    int32_t flags, id, rotation, distance, second_distance, border_errors;
};

// (x, y) lies at least 1 px inside every border (false for NaN)
CBA_HD bool marker_inside(double x, double y, int W, int H) {
    return x >= 1.0 && x <= static_cast<double>(W - 2) && y >= 1.0 && y <= static_cast<double>(H - 2);
}

// the image at (x, y), marker_inside
CBA_HD double marker_sample(const uint8_t* img, int W, double x, double y) {
    CBA_NO_CONTRACT
    const double x0 = std::floor(x), y0 = std::floor(y);
    return corner_bilinear(img + static_cast<int>(y0) * W + static_cast<int>(x0), W, x - x0, y - y0);
}

// The arm test of the corner at (x, y).  dirs [12][2]: the unit vectors (c, s) of direction 3 k + f, arm k = 0..3, fan f = 0..2.
// len [2], off: the arm lengths and the offset across the edge.
CBA_HD double corner_arms_one(const uint8_t* img, int W, int H, double x, double y, const double* dirs, const double* len, double off) {
    CBA_NO_CONTRACT
    double score = 0.0;
#pragma unroll 1
    for (int l = 0; l < 2; ++l) {
        const double L = len[l];
        double plus = 0.0, minus = 0.0;  // the minimum over the counted arms, per polarity
        int counted = 0;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            bool ok = true;
            double best_p = 0.0, best_m = 0.0;
#pragma unroll 1
            for (int f = 0; f < 3; ++f) {
                const double c = dirs[2 * (3 * k + f)], s = dirs[2 * (3 * k + f) + 1];
                const double px = x + L * c, py = y + L * s;
                const double ax = px - off * s, ay = py + off * c, bx = px + off * s, by = py - off * c;
                if (!marker_inside(ax, ay, W, H) || !marker_inside(bx, by, W, H)) {
                    ok = false;
                    break;
                }
                const double d = marker_sample(img, W, ax, ay) - marker_sample(img, W, bx, by);
                const double sp = (k & 1) ? -d : d, sm = (k & 1) ? d : -d;
                best_p = f == 0 || sp > best_p ? sp : best_p;
                best_m = f == 0 || sm > best_m ? sm : best_m;
            }
            if (!ok) continue;
            plus = counted == 0 || best_p < plus ? best_p : plus;
            minus = counted == 0 || best_m < minus ? best_m : minus;
            ++counted;
        }
        if (counted < 2) return 0.0;
        const double sl = plus > minus ? plus : minus;
        score = l == 0 || sl < score ? sl : score;
    }
    return score;
}

// Unit square (0,0) (1,0) (1,1) (0,1) -> q [4][2]: x = (a u + b v + c) / (g u + h v + 1), y = (d u + e v + f) / (g u + h v + 1),
// hc = (a, b, c, d, e, f, g, h).  Returns false when the quad is degenerate.
CBA_HD bool marker_homography(const double* q, double* hc) {
    CBA_NO_CONTRACT
    const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
    const double sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3;
    const double dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
    const double den = dx1 * dy2 - dy1 * dx2;
    // the cross product of the two sides at every corner (den is the one at corner 2) against the longest side
    double longest = 0.0, smallest = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double ex = q[2 * ((k + 1) & 3)] - q[2 * k], ey = q[2 * ((k + 1) & 3) + 1] - q[2 * k + 1];
        const double fx = q[2 * ((k + 3) & 3)] - q[2 * k], fy = q[2 * ((k + 3) & 3) + 1] - q[2 * k + 1];
        const double l2 = ex * ex + ey * ey, cr = ex * fy - ey * fx, mag = cr < 0.0 ? -cr : cr;
        longest = l2 > longest ? l2 : longest;
        smallest = k == 0 || mag < smallest ? mag : smallest;
    }
    if (!(smallest > MARKER_DEGENERATE_REL * longest)) return false;
    const double g = (sx * dy2 - sy * dx2) / den, h = (dx1 * sy - dy1 * sx) / den;
    hc[0] = x1 - x0 + g * x1;
    hc[1] = x3 - x0 + h * x3;
    hc[2] = x0;
    hc[3] = y1 - y0 + g * y1;
    hc[4] = y3 - y0 + h * y3;
    hc[5] = y0;
    hc[6] = g;
    hc[7] = h;
    return true;
}

// The mean of marker cell `cell` = cy (bits + 2) + cx: samples^2 bilinear samples, row-major, divided once.  Returns false (and
// leaves *mean alone) when a sample is not marker_inside.
CBA_HD bool marker_cell_mean(const uint8_t* img, int W, int H, const double* hc, double ratio, int bits, int samples, int cell, double* mean) {
    CBA_NO_CONTRACT
    const int side = bits + 2, cy = cell / side, cx = cell - cy * side;
    const double m0 = 0.5 * (1.0 - ratio), ms = ratio / static_cast<double>(side);
    double sum = 0.0;
#pragma unroll 1
    for (int ky = 0; ky < samples; ++ky) {
        const double v = m0 + ms * (static_cast<double>(cy) + (0.25 + 0.5 * (static_cast<double>(ky) + 0.5) / static_cast<double>(samples)));
#pragma unroll 1
        for (int kx = 0; kx < samples; ++kx) {
            const double u = m0 + ms * (static_cast<double>(cx) + (0.25 + 0.5 * (static_cast<double>(kx) + 0.5) / static_cast<double>(samples)));
            const double w = hc[6] * u + hc[7] * v + 1.0;
            const double x = (hc[0] * u + hc[1] * v + hc[2]) / w, y = (hc[3] * u + hc[4] * v + hc[5]) / w;
            if (!marker_inside(x, y, W, H)) return false;
            sum = sum + marker_sample(img, W, x, y);
        }
    }
    *mean = sum / static_cast<double>(samples * samples);
    return true;
}

// bit `cell` of the 128-bit mask (lo: cells 0..63, hi: cells 64..)
CBA_HD int marker_mask_bit(uint64_t lo, uint64_t hi, int cell) {
    return static_cast<int>(((cell < 64 ? lo >> cell : hi >> (cell - 64))) & 1u);
}

// the inner bits^2 cells row-major, the first the most significant
CBA_HD uint64_t marker_code_of(uint64_t lo, uint64_t hi, int bits) {
    uint64_t code = 0;
    for (int iy = 0; iy < bits; ++iy)
        for (int ix = 0; ix < bits; ++ix) code = (code << 1) | static_cast<uint64_t>(marker_mask_bit(lo, hi, (iy + 1) * (bits + 2) + ix + 1));
    return code;
}

// the mask of the border cells
inline void marker_border_mask(int bits, uint64_t* lo, uint64_t* hi) {
    const int side = bits + 2;
    *lo = *hi = 0;
    for (int cy = 0; cy < side; ++cy)
        for (int cx = 0; cx < side; ++cx) {
            if (cx != 0 && cy != 0 && cx != side - 1 && cy != side - 1) continue;
            const int cell = cy * side + cx;
            (cell < 64 ? *lo : *hi) |= uint64_t(1) << (cell & 63);
        }
}

// a quarter-turn clockwise (x right, y down): new (y, x) = old (bits - 1 - x, y)
inline uint64_t marker_rotate(uint64_t code, int bits) {
    uint64_t out = 0;
    for (int y = 0; y < bits; ++y)
        for (int x = 0; x < bits; ++x) {
            const int src = (bits - 1 - x) * bits + y;
            out = (out << 1) | ((code >> (bits * bits - 1 - src)) & 1u);
        }
    return out;
}

// table [4 n][1]: entry 4 id + r = the code of marker id turned r quarter-turns
inline void marker_rotated_table(int bits, int n, const uint64_t* codes, uint64_t* table) {
    for (int id = 0; id < n; ++id) {
        uint64_t c = codes[id];
        for (int r = 0; r < 4; ++r) {
            table[4 * id + r] = c;
            c = marker_rotate(c, bits);
        }
    }
}

CBA_HD int marker_popcount(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

struct MarkerParams {
    int W, H, bits, samples, n_codes;  // n_codes = 4 n_markers
    int max_border_errors, max_correction;
    double ratio, min_contrast;
};

// flags, border errors and match of a reading whose cell levels are known (lane 0 of a wavefront, or the host)
CBA_HD void marker_finish(const MarkerParams& p, double lo_level, double hi_level, int border_errors, uint64_t code, int best_key,
                          int second_distance, MarkerReading* r) {
    int flags = 0;
    if (hi_level - lo_level < p.min_contrast) flags |= MARKER_FLAG_LOW_CONTRAST;
    if (border_errors > p.max_border_errors) flags |= MARKER_FLAG_BORDER;
    const int dist = best_key >> 16, e = best_key & 0xffff;
    if (dist > p.max_correction) flags |= MARKER_FLAG_NO_MATCH;
    r->code = code;
    r->level_min = lo_level;
    r->level_max = hi_level;
    r->flags = flags;
    r->id = e >> 2;
    r->rotation = e & 3;
    r->distance = dist;
    r->second_distance = second_distance;
    r->border_errors = border_errors;
}

CBA_HD void marker_unread(int flags, MarkerReading* r) {
    r->code = 0;
    r->level_min = r->level_max = 0.0;
    r->flags = flags;
    r->id = -1;
    r->rotation = 0;
    r->distance = r->second_distance = -1;
    r->border_errors = 0;
}

// The whole rule for one lattice cell on the host.  table: the 4 n_markers rotated codes; bmask: marker_border_mask.
inline void marker_read_one(const MarkerParams& p, const uint8_t* img, const double* quad, const uint64_t* table, MarkerReading* r) {
    double hc[8], mean[MARKER_MAX_CELLS] = {};
    if (!marker_homography(quad, hc)) return marker_unread(MARKER_FLAG_DEGENERATE, r);
    const int cells = (p.bits + 2) * (p.bits + 2);
    for (int c = 0; c < cells; ++c)
        if (!marker_cell_mean(img, p.W, p.H, hc, p.ratio, p.bits, p.samples, c, &mean[c])) return marker_unread(MARKER_FLAG_WINDOW, r);
    double lo_level = mean[0], hi_level = mean[0];
    for (int c = 1; c < cells; ++c) {
        lo_level = mean[c] < lo_level ? mean[c] : lo_level;
        hi_level = mean[c] > hi_level ? mean[c] : hi_level;
    }
    const double t = (lo_level + hi_level) / 2.0;
    uint64_t lo = 0, hi = 0, blo, bhi;
    for (int c = 0; c < cells; ++c)
        if (mean[c] > t) (c < 64 ? lo : hi) |= uint64_t(1) << (c & 63);
    marker_border_mask(p.bits, &blo, &bhi);
    const int border_errors = marker_popcount(lo & blo) + marker_popcount(hi & bhi);
    const uint64_t code = marker_code_of(lo, hi, p.bits);
    int best = MARKER_NO_KEY;
    for (int e = 0; e < p.n_codes; ++e) {
        const int key = (marker_popcount(code ^ table[e]) << 16) | e;
        best = key < best ? key : best;
    }
    int second = MARKER_NO_KEY;
    for (int e = 0; e < p.n_codes; ++e) {
        if ((e >> 2) == ((best & 0xffff) >> 2)) continue;
        const int d = marker_popcount(code ^ table[e]);
        second = d < second ? d : second;
    }
    marker_finish(p, lo_level, hi_level, border_errors, code, best, second == MARKER_NO_KEY ? -1 : second, r);
}

}  // namespace cba
