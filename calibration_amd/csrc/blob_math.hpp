// blob_math.hpp — circle (blob) detection (calibba.h: cba_blob_detector) as __host__ __device__ code.  The kernels of blob_detect.hip
// call the per-pixel and per-blob pieces; tests/circle_cpu compiles the same header with g++ and walks every pixel.  The reference has
// no counterpart (its pipeline reads features from JSON).
//
//   response   blob_response_at: exact integers from two centred box sums, R = n_in S_ring - n_ring S_in (DARK), and S_in next to it
//   peaks      blob_is_peak: peak_is_max of peak_walk.hpp with the border outer_half
//   refine     blob_refine_one: 32 rays from the centre to the half level, the polygon's centroid per round, its second moments and
//              the largest deviation from the moment ellipse after the last; fp64, fixed order, nothing contracted, only + - x /
//   flags      blob_number_flags: SHAPE, RATIO, SIZE and DUPLICATE from the downloaded numbers (host)
//   image      blob_detect_image: the whole rule for one image on the host (what the device must reproduce)
#pragma once
#include <cmath>
#include <cstdint>

#include "camera_math.hpp"
#include "peak_walk.hpp"

namespace cba {

constexpr int BLOB_RAYS = 32;
constexpr int BLOB_DARK = 0, BLOB_BRIGHT = 1;
constexpr int BLOB_FLAG_WINDOW = 1;      // a sample would leave [0, W-1) x [0, H-1); the last good centre is kept
constexpr int BLOB_FLAG_NO_EDGE = 2;     // the centre is not on the blob's side of the level, or a ray meets no edge by max_radius
constexpr int BLOB_FLAG_DEGENERATE = 4;  // the polygon's area or the determinant of its moments is not positive
constexpr int BLOB_FLAG_SHAPE = 8;       // fit_error > max_fit_error
constexpr int BLOB_FLAG_RATIO = 16;      // major / minor semi-axis > max_axis_ratio
constexpr int BLOB_FLAG_SIZE = 32;       // minor semi-axis < min_radius
constexpr int BLOB_FLAG_DUPLICATE = 64;  // an earlier unflagged blob's centre lies within this blob's minor semi-axis
constexpr int BLOB_STATUS_OVERFLOW = PEAK_STATUS_OVERFLOW;
constexpr int BLOB_MAX_OUTER = 15;

struct BlobParams {
    int W, H, max_blobs;
    int polarity, a, b, min_contrast, nms_radius, max_radius, rounds;
    double max_fit_error, max_axis_ratio, min_radius;
};

CBA_HD constexpr int blob_n_in(int a) { return (2 * a + 1) * (2 * a + 1); }
CBA_HD constexpr int blob_n_ring(int a, int b) { return (2 * b + 1) * (2 * b + 1) - blob_n_in(a); }
CBA_HD constexpr int blob_threshold(int a, int b, int min_contrast) { return min_contrast * blob_n_in(a) * blob_n_ring(a, b); }

// R and S_in of pixel (x, y) of one image; R is 0 closer than b to a border (S_in is the sum of what lies inside the image there)
CBA_HD int blob_response_at(const uint8_t* img, int W, int H, int x, int y, int a, int b, int polarity, int* s_in) {
    int sa = 0, sb = 0;
    for (int dy = -b; dy <= b; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -b; dx <= b; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const int v = img[yy * W + xx];
            sb += v;
            if (dy >= -a && dy <= a && dx >= -a && dx <= a) sa += v;
        }
    }
    *s_in = sa;
    if (x < b || y < b || x > W - 1 - b || y > H - 1 - b) return 0;
    const int r = blob_n_in(a) * (sb - sa) - blob_n_ring(a, b) * sa;
    return polarity == BLOB_DARK ? r : -r;
}

CBA_HD bool blob_is_peak(const int32_t* R, int W, int H, int x, int y, int min_response, int nms, int b) {
    return peak_is_max<int32_t>(R, W, H, x, y, min_response, nms, b);
}

// rays [64]: cos 2 pi k / 32 (k < 32), then sin 2 pi k / 32.  Made once on the host and uploaded, so the device never takes a cosine.
inline void blob_ray_table(double* rays) {
    for (int k = 0; k < BLOB_RAYS; ++k) {
        const double t = 2.0 * 3.14159265358979323846 * static_cast<double>(k) / static_cast<double>(BLOB_RAYS);
        rays[k] = std::cos(t);
        rays[BLOB_RAYS + k] = std::sin(t);
    }
}

// the image at (x, y) when 0 <= x < W - 1 and 0 <= y < H - 1 (returns false otherwise): rows first, then between the rows
CBA_HD bool blob_sample(const uint8_t* img, int W, int H, double x, double y, double* v) {
    CBA_NO_CONTRACT
    if (!(x >= 0.0 && y >= 0.0 && x < static_cast<double>(W - 1) && y < static_cast<double>(H - 1))) return false;
    const int ix = static_cast<int>(x), iy = static_cast<int>(y);  // x, y >= 0: truncation is the floor
    const double fx = x - static_cast<double>(ix), fy = y - static_cast<double>(iy);
    const uint8_t* p = img + iy * W + ix;
    const double p00 = p[0], p01 = p[1], p10 = p[W], p11 = p[W + 1];
    const double top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10);
    *v = top + fy * (bot - top);
    return true;
}

// the edge along (dx, dy) from (cx, cy), whose sample i0 lies on the blob's side: returns flags, *r the distance of the half level
CBA_HD int blob_ray_edge(const uint8_t* img, int W, int H, double cx, double cy, double dx, double dy, double i0, double thr, int polarity,
                         int max_radius, double* r) {
    CBA_NO_CONTRACT
    double prev = i0;
#pragma unroll 1
    for (int t = 1; t <= max_radius; ++t) {
        const double td = static_cast<double>(t);
        double cur;
        if (!blob_sample(img, W, H, cx + td * dx, cy + td * dy, &cur)) return BLOB_FLAG_WINDOW;
        if (polarity == BLOB_DARK ? cur >= thr : cur <= thr) {
            const double num = polarity == BLOB_DARK ? thr - prev : prev - thr;
            const double den = polarity == BLOB_DARK ? cur - prev : prev - cur;
            *r = (td - 1.0) + num / den;
            return 0;
        }
        prev = cur;
    }
    return BLOB_FLAG_NO_EDGE;
}

// one kept peak (px, py) with its stored R and S_in -> xy [2], shape [3] = (m_xx, m_xy, m_yy), fit_error; returns the flags WINDOW,
// NO_EDGE, DEGENERATE.  A flagged blob keeps its last good centre and has NaN shape and fit_error.
CBA_HD int blob_refine_one(const uint8_t* img, int W, int H, int px, int py, int R, int s_in, int a, int b, int polarity, int max_radius,
                           int rounds, const double* rays, double* xy, double* shape, double* fit_error) {
    CBA_NO_CONTRACT
    const int n_in = blob_n_in(a), n_ring = blob_n_ring(a, b);
    const int s_ring = (polarity == BLOB_DARK ? R + n_ring * s_in : n_ring * s_in - R) / n_in;  // exact
    const double lo = static_cast<double>(s_in) / static_cast<double>(n_in), hi = static_cast<double>(s_ring) / static_cast<double>(n_ring);
    const double thr = (lo + hi) / 2.0;
    double cx = static_cast<double>(px), cy = static_cast<double>(py);
    double mxx = NAN, mxy = NAN, myy = NAN, err = NAN;
    int flags = 0;
#pragma unroll 1
    for (int round = 0; round < rounds && !flags; ++round) {
        double i0;
        if (!blob_sample(img, W, H, cx, cy, &i0)) { flags |= BLOB_FLAG_WINDOW; break; }
        if (!(polarity == BLOB_DARK ? i0 < thr : i0 > thr)) { flags |= BLOB_FLAG_NO_EDGE; break; }
        // shoelace sums over the edge points e_k (relative to the centre), k = 0..31 and back to 0
        double s2 = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, sxy = 0.0, syy = 0.0;
        double x0 = 0.0, y0 = 0.0, xp = 0.0, yp = 0.0;
#pragma unroll 1
        for (int k = 0; k <= BLOB_RAYS && !flags; ++k) {
            double xk = x0, yk = y0;
            if (k < BLOB_RAYS) {
                double r;
                const double dx = rays[k], dy = rays[BLOB_RAYS + k];
                flags |= blob_ray_edge(img, W, H, cx, cy, dx, dy, i0, thr, polarity, max_radius, &r);
                if (flags) break;
                xk = r * dx;
                yk = r * dy;
            }
            if (k == 0) {
                x0 = xk;
                y0 = yk;
            } else {
                const double cr = xp * yk - xk * yp;
                s2 = s2 + cr;
                sx = sx + (xp + xk) * cr;
                sy = sy + (yp + yk) * cr;
                sxx = sxx + (xp * xp + xp * xk + xk * xk) * cr;
                syy = syy + (yp * yp + yp * yk + yk * yk) * cr;
                sxy = sxy + (xp * yk + 2.0 * (xp * yp) + 2.0 * (xk * yk) + xk * yp) * cr;
            }
            xp = xk;
            yp = yk;
        }
        if (flags) break;
        if (!(s2 > 0.0)) { flags |= BLOB_FLAG_DEGENERATE; break; }
        const double gx = sx / (3.0 * s2), gy = sy / (3.0 * s2);  // centroid: sum / (6 A), A = s2 / 2
        if (round == rounds - 1) {
            // central second moments over the area, times 4: the ellipse {d : d^T M^-1 d = 1} of equal moments
            const double axx = 4.0 * (sxx / (6.0 * s2) - gx * gx), ayy = 4.0 * (syy / (6.0 * s2) - gy * gy);
            const double axy = 4.0 * (sxy / (12.0 * s2) - gx * gy);
            const double det = axx * ayy - axy * axy;
            if (!(det > 0.0)) { flags |= BLOB_FLAG_DEGENERATE; break; }
            double worst = 0.0;
#pragma unroll 1
            for (int k = 0; k < BLOB_RAYS; ++k) {  // the same rays again: nothing is kept in a private array
                double r = 0.0;
                const double dx = rays[k], dy = rays[BLOB_RAYS + k];
                (void)blob_ray_edge(img, W, H, cx, cy, dx, dy, i0, thr, polarity, max_radius, &r);
                const double ex = r * dx - gx, ey = r * dy - gy;
                const double q = (ayy * (ex * ex) - 2.0 * (axy * (ex * ey)) + axx * (ey * ey)) / det - 1.0;
                const double aq = q < 0.0 ? -q : q;
                if (aq > worst) worst = aq;
            }
            mxx = axx; mxy = axy; myy = ayy; err = worst;
        }
        cx = cx + gx;
        cy = cy + gy;
    }
    xy[0] = cx;
    xy[1] = cy;
    shape[0] = flags ? static_cast<double>(NAN) : mxx;
    shape[1] = flags ? static_cast<double>(NAN) : mxy;
    shape[2] = flags ? static_cast<double>(NAN) : myy;
    *fit_error = flags ? static_cast<double>(NAN) : err;
    return flags;
}

// semi-axes (major, minor) of the ellipse M = shape: the square roots of its eigenvalues (host)
inline void blob_semi_axes(const double* shape, double* major, double* minor) {
    const double h = 0.5 * (shape[0] + shape[2]), d = 0.5 * (shape[0] - shape[2]);
    const double s = std::sqrt(d * d + shape[1] * shape[1]);
    *major = std::sqrt(h + s);
    *minor = std::sqrt(h - s);
}

// SHAPE, RATIO, SIZE and DUPLICATE of one image's kept blobs, from the downloaded numbers; flags [kept] in and out
inline void blob_number_flags(int kept, const double* xy, const double* shape, const double* fit_error, double max_fit_error,
                              double max_axis_ratio, double min_radius, int32_t* flags) {
    for (int i = 0; i < kept; ++i) {
        double major, minor;
        blob_semi_axes(shape + 3 * i, &major, &minor);
        if (fit_error[i] > max_fit_error) flags[i] |= BLOB_FLAG_SHAPE;
        if (major > max_axis_ratio * minor) flags[i] |= BLOB_FLAG_RATIO;
        if (minor < min_radius) flags[i] |= BLOB_FLAG_SIZE;
        for (int j = 0; j < i; ++j) {
            if (flags[j]) continue;
            const double dx = xy[2 * i] - xy[2 * j], dy = xy[2 * i + 1] - xy[2 * j + 1];
            if (dx * dx + dy * dy <= minor * minor) {
                flags[i] |= BLOB_FLAG_DUPLICATE;
                break;
            }
        }
    }
}

// The whole rule for one image on the host.  R [H][W] and S [H][W]: scratch that holds the responses afterwards; rays: blob_ray_table.
// Outputs as cba_blob_detector_process writes them for one image.
inline void blob_detect_image(const BlobParams& p, const uint8_t* img, const double* rays, int32_t* R, uint16_t* S, int32_t* count,
                              int32_t* status, double* xy, double* shape, double* fit_error, int32_t* response, int32_t* flags) {
    for (int y = 0; y < p.H; ++y)
        for (int x = 0; x < p.W; ++x) {
            int s;
            R[y * p.W + x] = blob_response_at(img, p.W, p.H, x, y, p.a, p.b, p.polarity, &s);
            S[y * p.W + x] = static_cast<uint16_t>(s);
        }
    const int thr = blob_threshold(p.a, p.b, p.min_contrast);
    int n = 0;
    for (int y = 0; y < p.H; ++y)
        for (int x = 0; x < p.W; ++x) {
            if (!blob_is_peak(R, p.W, p.H, x, y, thr, p.nms_radius, p.b)) continue;
            if (n < p.max_blobs) {
                flags[n] = blob_refine_one(img, p.W, p.H, x, y, R[y * p.W + x], S[y * p.W + x], p.a, p.b, p.polarity, p.max_radius, p.rounds,
                                           rays, xy + 2 * n, shape + 3 * n, fit_error + n);
                response[n] = R[y * p.W + x];
            }
            ++n;
        }
    *count = n;
    *status = n > p.max_blobs ? BLOB_STATUS_OVERFLOW : 0;
    const int kept = n < p.max_blobs ? n : p.max_blobs;
    blob_number_flags(kept, xy, shape, fit_error, p.max_fit_error, p.max_axis_ratio, p.min_radius, flags);
    for (int i = kept; i < p.max_blobs; ++i) {
        xy[2 * i] = xy[2 * i + 1] = shape[3 * i] = shape[3 * i + 1] = shape[3 * i + 2] = fit_error[i] = NAN;
        response[i] = flags[i] = 0;
    }
}

}  // namespace cba
