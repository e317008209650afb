// corner_math.hpp — chessboard corner detection (calibba.h: cba_corner_detector) as __host__ __device__ code.  The kernels of
// corner_detect.hip call the per-pixel pieces; tests/corner_cpu compiles the same header with g++ and walks every pixel.  The
// reference has no counterpart (its pipeline reads corners from JSON).
//
//   response   corner_response_ring / corner_response_at: exact integers from the 16 ring samples and the 5-pixel centre
//   peaks      corner_is_peak: threshold, border, non-maximum suppression with the lowest index winning among equals
//   COG        corner_cog: exact integer sums over the response window, one fp64 division per axis
//   angle      corner_angle_sums: the two fp64 sums whose atan2 the host halves (corner_angle)
//   GRADIENT   corner_refine_gradient: the cornerSubPix condition in fp64, fixed order, nothing contracted into FMAs
//   image      corner_detect_image: the whole rule for one image on the host (what the device must reproduce)
#pragma once
#include <cmath>
#include <cstdint>

#include "camera_math.hpp"
#include "peak_walk.hpp"

namespace cba {

constexpr int CORNER_BORDER = 5;         // the ring's radius: R is defined this far from every border
constexpr int CORNER_REFINE_NONE = 0, CORNER_REFINE_COG = 1, CORNER_REFINE_GRADIENT = 2;
constexpr int CORNER_FLAG_WINDOW = 1;    // GRADIENT: the window would leave the image; the last good position is kept
constexpr int CORNER_FLAG_DET = 2;       // GRADIENT: det <= CORNER_DET_REL (trace)^2; the last good position is kept
constexpr int CORNER_FLAG_DRIFT = 4;     // GRADIENT: ended further than cog_radius + 1 from its peak (either axis)
constexpr int CORNER_STATUS_OVERFLOW = PEAK_STATUS_OVERFLOW;
constexpr double CORNER_DET_REL = 1e-6;

// ring offset n = 0..15: (0,-5) (2,-5) (3,-3) (5,-2) (5,0) (5,2) (3,3) (2,5) (0,5) (-2,5) (-3,3) (-5,2) (-5,0) (-5,-2) (-3,-3) (-2,-5);
// dx + 5 packed one nibble per n, and dy(n) = -dx(n + 4)
CBA_HD constexpr int corner_dx(int n) { return static_cast<int>((0x3200023578AAA875ull >> (4 * n)) & 15u) - 5; }
CBA_HD constexpr int corner_dy(int n) { return -corner_dx((n + 4) & 15); }

CBA_HD int corner_iabs(int v) { return v < 0 ? -v : v; }

// R = 5 SR - 5 DR - |5 S16 - 16 S5| from the ring samples I[16] and S5 (centre + 4-neighbours)
CBA_HD int corner_response_ring(const int* I, int s5) {
    int sr = 0, dr = 0, s16 = 0;
    for (int n = 0; n < 4; ++n) sr += corner_iabs(I[n] + I[n + 8] - I[n + 4] - I[n + 12]);
    for (int n = 0; n < 8; ++n) dr += corner_iabs(I[n] - I[n + 8]);
    for (int n = 0; n < 16; ++n) s16 += I[n];
    return 5 * sr - 5 * dr - corner_iabs(5 * s16 - 16 * s5);
}

// R of pixel (x, y) of one image; 0 closer than CORNER_BORDER to a border
CBA_HD int corner_response_at(const uint8_t* img, int W, int H, int x, int y) {
    if (x < CORNER_BORDER || y < CORNER_BORDER || x > W - 1 - CORNER_BORDER || y > H - 1 - CORNER_BORDER) return 0;
    int I[16];
    for (int n = 0; n < 16; ++n) I[n] = img[(y + corner_dy(n)) * W + x + corner_dx(n)];
    const uint8_t* c = img + y * W + x;
    return corner_response_ring(I, c[0] + c[-1] + c[1] + c[-W] + c[W]);
}

// R: one image's responses [H][W]
CBA_HD bool corner_is_peak(const int16_t* R, int W, int H, int x, int y, int min_response, int nms) {
    return peak_is_max<int16_t>(R, W, H, x, y, min_response, nms, CORNER_BORDER);
}

// centre of gravity of max(R, 0) over the (2c + 1)^2 window of a peak (R(peak) >= 1, so the sum is positive)
CBA_HD void corner_cog(const int16_t* R, int W, int px, int py, int c, double* x, double* y) {
    int s = 0, sx = 0, sy = 0;
    for (int dy = -c; dy <= c; ++dy)
        for (int dx = -c; dx <= c; ++dx) {
            const int q = R[(py + dy) * W + px + dx];
            const int r = q > 0 ? q : 0;
            s += r;
            sx += r * dx;
            sy += r * dy;
        }
    *x = static_cast<double>(px) + static_cast<double>(sx) / static_cast<double>(s);
    *y = static_cast<double>(py) + static_cast<double>(sy) / static_cast<double>(s);
}

// trig [16]: cos 2 theta_n (n < 8), then sin 2 theta_n (n < 8); theta_{n+8} = theta_n + pi has the same double angle.  Rational in the
// offsets, so every host makes the same doubles: cos 2t = (dx^2 - dy^2) / (dx^2 + dy^2), sin 2t = 2 dx dy / (dx^2 + dy^2)
inline void corner_trig_table(double* trig) {
    for (int n = 0; n < 8; ++n) {
        const double dx = corner_dx(n), dy = corner_dy(n), q = dx * dx + dy * dy;
        trig[n] = (dx * dx - dy * dy) / q;
        trig[8 + n] = (2.0 * dx * dy) / q;
    }
}

// sums [2] = sum_n (I_n + I_{n+8}) cos 2 theta_n, ... sin 2 theta_n, n ascending
CBA_HD void corner_angle_sums(const uint8_t* img, int W, int x, int y, const double* trig, double* sums) {
    CBA_NO_CONTRACT
    double a = 0.0, b = 0.0;
    for (int n = 0; n < 8; ++n) {
        const int p = img[(y + corner_dy(n)) * W + x + corner_dx(n)] + img[(y - corner_dy(n)) * W + x - corner_dx(n)];
        const double pd = static_cast<double>(p);
        a = a + pd * trig[n];
        b = b + pd * trig[8 + n];
    }
    sums[0] = a;
    sums[1] = b;
}
inline double corner_angle(const double* sums) { return 0.5 * std::atan2(sums[1], sums[0]); }

// the Gaussian weights of GRADIENT, (2w + 1)^2 row-major
inline void corner_weight_table(int w, double* wt) {
    const double h = w / 2.0, den = 2.0 * (h * h);
    for (int dy = -w; dy <= w; ++dy)
        for (int dx = -w; dx <= w; ++dx) wt[(dy + w) * (2 * w + 1) + dx + w] = std::exp(-static_cast<double>(dx * dx + dy * dy) / den);
}

// the image at (ix + fx, iy + fy), 0 <= fx, fy < 1: rows first, then between the rows
CBA_HD double corner_bilinear(const uint8_t* p, int W, double fx, double fy) {
    CBA_NO_CONTRACT
    const double p00 = p[0], p01 = p[1], p10 = p[W], p11 = p[W + 1];
    const double top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10);
    return top + fy * (bot - top);
}

// GRADIENT from (*x, *y) (the COG result): returns the flags.  A round whose position (or whose result) lies closer than w + 2 to a
// border, or whose determinant is too small, ends the rounds: the position would not change any more.
CBA_HD int corner_refine_gradient(const uint8_t* img, int W, int H, int px, int py, int cog_radius, int w, int iters, const double* wt,
                                  double* x, double* y) {
    CBA_NO_CONTRACT
    int flags = 0;
    double cx = *x, cy = *y;
    const double lim = static_cast<double>(w + 2), xhi = static_cast<double>(W - 1) - lim, yhi = static_cast<double>(H - 1) - lim;
    if (!(cx >= lim && cx <= xhi && cy >= lim && cy <= yhi)) flags |= CORNER_FLAG_WINDOW;
#pragma unroll 1
    for (int it = 0; it < iters && !flags; ++it) {
        const double x0 = std::floor(cx), y0 = std::floor(cy);
        const double fx = cx - x0, fy = cy - y0;
        const uint8_t* c = img + static_cast<int>(y0) * W + static_cast<int>(x0);
        double a = 0.0, b = 0.0, cc = 0.0, bb1 = 0.0, bb2 = 0.0;
        const double* wp = wt;
#pragma unroll 1
        for (int dy = -w; dy <= w; ++dy) {
#pragma unroll 1
            for (int dx = -w; dx <= w; ++dx) {
                const uint8_t* q = c + dy * W + dx;
                const double gx = (corner_bilinear(q + 1, W, fx, fy) - corner_bilinear(q - 1, W, fx, fy)) * 0.5;
                const double gy = (corner_bilinear(q + W, W, fx, fy) - corner_bilinear(q - W, W, fx, fy)) * 0.5;
                const double m = *wp++;
                const double tgx = gx * m, tgy = gy * m;
                const double gxx = tgx * gx, gxy = tgx * gy, gyy = tgy * gy;
                const double ox = static_cast<double>(dx), oy = static_cast<double>(dy);
                a = a + gxx;
                b = b + gxy;
                cc = cc + gyy;
                bb1 = bb1 + (gxx * ox + gxy * oy);
                bb2 = bb2 + (gxy * ox + gyy * oy);
            }
        }
        const double det = a * cc - b * b, tr = a + cc;
        if (!(det > CORNER_DET_REL * (tr * tr))) {
            flags |= CORNER_FLAG_DET;
            break;
        }
        const double nx = cx + (cc * bb1 - b * bb2) / det, ny = cy + (a * bb2 - b * bb1) / det;
        if (!(nx >= lim && nx <= xhi && ny >= lim && ny <= yhi)) {
            flags |= CORNER_FLAG_WINDOW;
            break;
        }
        cx = nx;
        cy = ny;
    }
    const double lx = cx - static_cast<double>(px), ly = cy - static_cast<double>(py), far = static_cast<double>(cog_radius + 1);
    if (lx > far || lx < -far || ly > far || ly < -far) flags |= CORNER_FLAG_DRIFT;
    *x = cx;
    *y = cy;
    return flags;
}

// one kept peak -> position, angle sums, flags (what one lane of k_corner_refine does)
CBA_HD void corner_refine_one(const uint8_t* img, const int16_t* R, int W, int H, int px, int py, int cog_radius, int refine, int w,
                              int iters, const double* wt, const double* trig, double* xy, double* sums, int* flags) {
    double x = static_cast<double>(px), y = static_cast<double>(py);
    int f = 0;
    if (refine != CORNER_REFINE_NONE) corner_cog(R, W, px, py, cog_radius, &x, &y);
    if (refine == CORNER_REFINE_GRADIENT) f = corner_refine_gradient(img, W, H, px, py, cog_radius, w, iters, wt, &x, &y);
    corner_angle_sums(img, W, px, py, trig, sums);
    xy[0] = x;
    xy[1] = y;
    *flags = f;
}

struct CornerParams {
    int W, H, max_corners;
    int min_response, nms_radius, cog_radius, refine, refine_half_window, refine_iterations;
};

// The whole rule for one image on the host.  R: scratch [H][W]; wt, trig: the tables above.  Outputs as cba_corner_detector_process
// writes them for one image (entries past the kept corners: xy and angle NaN, response and flags 0).
inline void corner_detect_image(const CornerParams& p, const uint8_t* img, const double* wt, const double* trig, int16_t* R,
                                int32_t* count, int32_t* status, double* xy, double* angle, int32_t* response, int32_t* flags) {
    for (int y = 0; y < p.H; ++y)
        for (int x = 0; x < p.W; ++x) R[y * p.W + x] = static_cast<int16_t>(corner_response_at(img, p.W, p.H, x, y));
    int n = 0;
    for (int y = 0; y < p.H; ++y)
        for (int x = 0; x < p.W; ++x) {
            if (!corner_is_peak(R, p.W, p.H, x, y, p.min_response, p.nms_radius)) continue;
            if (n < p.max_corners) {
                double sums[2];
                corner_refine_one(img, R, p.W, p.H, x, y, p.cog_radius, p.refine, p.refine_half_window, p.refine_iterations, wt, trig,
                                  xy + 2 * n, sums, flags + n);
                angle[n] = corner_angle(sums);
                response[n] = R[y * p.W + x];
            }
            ++n;
        }
    *count = n;
    *status = n > p.max_corners ? CORNER_STATUS_OVERFLOW : 0;
    for (int i = n; i < p.max_corners; ++i) {
        xy[2 * i] = xy[2 * i + 1] = angle[i] = NAN;
        response[i] = flags[i] = 0;
    }
}

}  // namespace cba
