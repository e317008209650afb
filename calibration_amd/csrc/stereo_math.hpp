// stereo_math.hpp — stereo depth (calibba.h: cba_stereo_rectify, cba_stereo_matcher, cba_stereo_points) as __host__ __device__ code.
// The kernels of stereo_match.hip call the per-pixel pieces; tests/stereo_cpu compiles the same header with g++ and walks every pixel
// with the naive window sum.  The reference has no counterpart.
//
//   rectification  stereo_rectify: closed form, fp64, host only
//   selection      StereoSel: the state of one pixel while its admissible candidates arrive in ascending d (they form one interval):
//                  best cost and its lowest d, the costs next to it, and the lowest cost at distance > 1 on either side.  stereo_sel_push
//                  adds the next candidate; the result does not depend on how the costs were summed (they are exact integers)
//   sub-pixel      stereo_disparity: uniqueness, the parabola step, one rounding to float32
//   disparity->3D  stereo_point: the function both k_stereo_points and the matcher's xyz run; nothing is contracted into FMAs
#pragma once
#include <cmath>
#include <cstdint>

#include "camera_math.hpp"

namespace cba {

constexpr int STEREO_INF = 0x7fffffff;       // "no such candidate"
constexpr int STEREO_NO_DISP = -32768;       // int16 maps: no admissible candidate (an admissible |d| is below the image width)

// [f', cx', cy', baseline] and an optional [R | t] (has_pose)
struct StereoGeom {
    double f, cx, cy, B;
    double Rt[12];
    int has_pose;
};

CBA_HD void stereo_fill_geom(double f, double cx, double cy, double B, const double* pose7, StereoGeom* g) {
    g->f = f; g->cx = cx; g->cy = cy; g->B = B;
    g->has_pose = pose7 ? 1 : 0;
    for (int j = 0; j < 12; ++j) g->Rt[j] = 0.0;
    if (pose7) {
        quat_to_rotmat(pose7, g->Rt);
        for (int j = 0; j < 3; ++j) g->Rt[9 + j] = pose7[4 + j];
    }
}

// (u, v, d) -> P: s = B / d, P = ((u - cx) s, (v - cy) s, f s); d <= 0 or a non-finite input gives NaN; with a pose P <- R P + t, each
// row summed left to right, then + t
CBA_HD void stereo_point(const StereoGeom& g, double u, double v, double d, double* P) {
    CBA_NO_CONTRACT
    const double lim = 1.7976931348623157e308;
    const bool ok = d > 0.0 && d <= lim && u >= -lim && u <= lim && v >= -lim && v <= lim;
    const double nan = NAN;
    const double s = g.B / d;
    double P0 = ok ? (u - g.cx) * s : nan, P1 = ok ? (v - g.cy) * s : nan, P2 = ok ? g.f * s : nan;
    if (g.has_pose) {
        const double* Rt = g.Rt;
        const double Q0 = Rt[0] * P0 + Rt[1] * P1 + Rt[2] * P2 + Rt[9];
        const double Q1 = Rt[3] * P0 + Rt[4] * P1 + Rt[5] * P2 + Rt[10];
        const double Q2 = Rt[6] * P0 + Rt[7] * P1 + Rt[8] * P2 + Rt[11];
        P0 = Q0; P1 = Q1; P2 = Q2;
    }
    P[0] = P0; P[1] = P1; P[2] = P2;
}

// The admissible candidates of a pixel in column x: [lo, hi] (empty when lo > hi).  right == 0: a left pixel, candidate d pairs it
// with right column x - d; right != 0: a right pixel x', candidate d pairs it with left column x' + d (the left-right map).  The
// row condition r <= y <= H - 1 - r is the caller's.
CBA_HD void stereo_interval(int x, int W, int r, int dmin, int D, int right, int* lo, int* hi) {
    const int dmax = dmin + D - 1;
    int a, b;
    if (right) { a = r - x; b = W - 1 - r - x; }
    else { a = x + r - W + 1; b = x - r; }
    if (x < r || x > W - 1 - r) { a = 1; b = 0; }
    *lo = a > dmin ? a : dmin;
    *hi = b < dmax ? b : dmax;
}

struct StereoSel {
    int best, bestd;      // lowest cost, its lowest d (best == STEREO_INF: no candidate yet)
    int cm, cp;           // C(bestd - 1), C(bestd + 1), STEREO_INF where not admissible (or not seen yet)
    int before, after;    // lowest cost over d <= bestd - 2 / d >= bestd + 2
    int c1, c2, pm2;      // C(d - 1), C(d - 2) of the next candidate d, and the lowest cost over d' <= d - 3
};

CBA_HD void stereo_sel_init(StereoSel& s) {
    s.best = STEREO_INF; s.bestd = 0;
    s.cm = STEREO_INF; s.cp = STEREO_INF; s.before = STEREO_INF; s.after = STEREO_INF;
    s.c1 = STEREO_INF; s.c2 = STEREO_INF; s.pm2 = STEREO_INF;
}

// candidate d (the one after the last pushed, or the first) with cost c < STEREO_INF
CBA_HD void stereo_sel_push(StereoSel& s, int d, int c) {
    const int pm = s.c2 < s.pm2 ? s.c2 : s.pm2;  // the lowest cost over d' <= d - 2
    const bool take = c < s.best;
    const bool next = !take && d == s.bestd + 1;
    const bool far = !take && !next;             // d >= bestd + 2
    s.cp = take ? STEREO_INF : (next ? c : s.cp);
    s.after = take ? STEREO_INF : (far && c < s.after ? c : s.after);
    s.before = take ? pm : s.before;
    s.cm = take ? s.c1 : s.cm;
    s.bestd = take ? d : s.bestd;
    s.best = take ? c : s.best;
    s.pm2 = pm; s.c2 = s.c1; s.c1 = c;
}

// steps 3 and 5 of the rule: the float32 disparity of a pixel with at least one candidate
CBA_HD float stereo_disparity(const StereoSel& s, int uniqueness_percent, int subpixel) {
    if (uniqueness_percent > 0) {
        const int other = s.before < s.after ? s.before : s.after;
        if (other != STEREO_INF && 100 * other <= (100 + uniqueness_percent) * s.best) return NAN;
    }
    double d = static_cast<double>(s.bestd);
    if (subpixel && s.cm != STEREO_INF && s.cp != STEREO_INF) {
        const int den = s.cm - 2 * s.best + s.cp;
        if (den > 0) d = d + static_cast<double>(s.cm - s.cp) / static_cast<double>(2 * den);
    }
    return static_cast<float>(d);
}

// step 4: the left pixel's d* against the right map's entry at x - d*
CBA_HD bool stereo_lr_ok(int dstar, int dr, int lr_max_diff) {
    if (dr == STEREO_NO_DISP) return false;
    const int diff = dr > dstar ? dr - dstar : dstar - dr;
    return diff <= lr_max_diff;
}

// ---- rectification (host) ---------------------------------------------------------------------------------------------------------
// 0 on success; otherwise a message.  ni: 10 | 12 entries per camera.  focal, cx, cy: 0 or NaN selects the default.
inline const char* stereo_rectify(const double* intr, int ni, const double* c_T_r, int W, int H, double focal, double cx, double cy,
                                  double* R_out /*[2][9]*/, double* new_k5 /*[2][5]*/, double* baseline, double* r_T_rect /*[7]*/) {
    double R[2][9], o[2][3];
    for (int c = 0; c < 2; ++c) {
        const double* p = c_T_r + 7 * c;
        double n = 0.0;
        for (int k = 0; k < 4; ++k) n += p[k] * p[k];
        n = std::sqrt(n);
        if (!(n > 0.0) || !std::isfinite(n)) return "a quaternion of c_T_r is zero or not finite";
        const double q[4] = {p[0] / n, p[1] / n, p[2] / n, p[3] / n};
        quat_to_rotmat(q, R[c]);
        for (int i = 0; i < 3; ++i) o[c][i] = -(R[c][i] * p[4] + R[c][3 + i] * p[5] + R[c][6 + i] * p[6]);  // -R^T t
        if (intr[c * ni] == 0.0 || intr[c * ni + 1] == 0.0) return "fx and fy must not be 0";
    }
    if (focal < 0.0 || std::isinf(focal)) return "focal must be positive and finite (0 or NaN: the default)";
    double e1[3], no[2] = {0.0, 0.0}, B = 0.0;
    for (int i = 0; i < 3; ++i) {
        e1[i] = o[1][i] - o[0][i];
        B += e1[i] * e1[i];
        no[0] += o[0][i] * o[0][i];
        no[1] += o[1][i] * o[1][i];
    }
    B = std::sqrt(B);
    if (!(B > 1e-12 * (std::sqrt(no[0]) + std::sqrt(no[1]) + 1.0))) return "the two camera centres coincide";
    for (int i = 0; i < 3; ++i) e1[i] /= B;
    const double z[3] = {R[0][6] + R[1][6], R[0][7] + R[1][7], R[0][8] + R[1][8]};  // R_i^T e_z = row 2 of R_i
    double e2[3] = {z[1] * e1[2] - z[2] * e1[1], z[2] * e1[0] - z[0] * e1[2], z[0] * e1[1] - z[1] * e1[0]};
    const double n2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    if (!(n2 > 1e-6)) return "the optical axes lie along the baseline";
    for (int i = 0; i < 3; ++i) e2[i] /= n2;
    const double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double M[9] = {e1[0], e1[1], e1[2], e2[0], e2[1], e2[2], e3[0], e3[1], e3[2]};  // rect_R_r
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)  // M R_c^T
                R_out[9 * c + 3 * i + j] = M[3 * i] * R[c][3 * j] + M[3 * i + 1] * R[c][3 * j + 1] + M[3 * i + 2] * R[c][3 * j + 2];
    const bool fdef = !(focal > 0.0);
    const double f = fdef ? (intr[0] + intr[1] + intr[ni] + intr[ni + 1]) / 4.0 : focal;
    const double cxn = (cx == 0.0 || cx != cx) ? (W - 1) / 2.0 : cx, cyn = (cy == 0.0 || cy != cy) ? (H - 1) / 2.0 : cy;
    for (int c = 0; c < 2; ++c) {
        double* k = new_k5 + 5 * c;
        k[0] = f; k[1] = f; k[2] = cxn; k[3] = cyn; k[4] = 0.0;
    }
    *baseline = B;
    // the quaternion of rect_R_r^T (row-major T[i][j] = M[j][i]), w >= 0
    const double T[9] = {M[0], M[3], M[6], M[1], M[4], M[7], M[2], M[5], M[8]};
    double q[4];
    const double tr = T[0] + T[4] + T[8];
    if (tr > 0.0) {
        double t = std::sqrt(tr + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (T[7] - T[5]) * t; q[2] = (T[2] - T[6]) * t; q[3] = (T[3] - T[1]) * t;
    } else {
        int i = 0;
        if (T[4] > T[0]) i = 1;
        if (T[8] > T[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = std::sqrt(T[i * 3 + i] - T[j * 3 + j] - T[k * 3 + k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (T[k * 3 + j] - T[j * 3 + k]) * t;
        q[1 + j] = (T[j * 3 + i] + T[i * 3 + j]) * t;
        q[1 + k] = (T[k * 3 + i] + T[i * 3 + k]) * t;
    }
    double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (q[0] < 0.0) qn = -qn;
    for (int k = 0; k < 4; ++k) r_T_rect[k] = q[k] / qn;
    for (int k = 0; k < 3; ++k) r_T_rect[4 + k] = o[0][k];
    return nullptr;
}

// ---- one pair, every pixel walked with the naive window sum (the host build; the kernels do not call it) --------------------------
struct StereoMatchParams {
    int W, H, dmin, D, r, uniqueness_percent, lr_max_diff, subpixel;
};

inline int stereo_naive_cost(const uint8_t* L, const uint8_t* R, int W, int r, int xl, int xr, int y) {
    int c = 0;
    for (int j = -r; j <= r; ++j)
        for (int i = -r; i <= r; ++i) {
            const int a = L[(y + j) * W + xl + i], b = R[(y + j) * W + xr + i];
            c += a > b ? a - b : b - a;
        }
    return c;
}

// disparity [H][W] float32, cost [H][W] int32 or null, xyz [H][W][3] float32 or null (needs g)
inline void stereo_match_pair(const StereoMatchParams& p, const uint8_t* L, const uint8_t* R, const StereoGeom* g, float* disparity,
                              int32_t* cost, float* xyz) {
    const int W = p.W, H = p.H;
    int16_t* dl = new int16_t[static_cast<size_t>(W) * H];
    int16_t* dr = new int16_t[static_cast<size_t>(W) * H];
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = static_cast<size_t>(y) * W + x;
            const bool row = y >= p.r && y <= H - 1 - p.r;
            for (int right = 0; right < 2; ++right) {
                int lo, hi;
                stereo_interval(x, W, p.r, p.dmin, p.D, right, &lo, &hi);
                StereoSel s;
                stereo_sel_init(s);
                if (row)
                    for (int d = lo; d <= hi; ++d)
                        stereo_sel_push(s, d, right ? stereo_naive_cost(L, R, W, p.r, x + d, x, y) : stereo_naive_cost(L, R, W, p.r, x, x - d, y));
                const bool any = s.best != STEREO_INF;
                if (right) {
                    dr[i] = any ? static_cast<int16_t>(s.bestd) : static_cast<int16_t>(STEREO_NO_DISP);
                } else {
                    dl[i] = any ? static_cast<int16_t>(s.bestd) : static_cast<int16_t>(STEREO_NO_DISP);
                    disparity[i] = any ? stereo_disparity(s, p.uniqueness_percent, p.subpixel) : NAN;
                    if (cost) cost[i] = any ? s.best : -1;
                }
            }
        }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = static_cast<size_t>(y) * W + x;
            if (p.lr_max_diff >= 0 && dl[i] != STEREO_NO_DISP && !stereo_lr_ok(dl[i], dr[i - dl[i]], p.lr_max_diff)) disparity[i] = NAN;
            if (xyz) {
                double P[3];
                stereo_point(*g, x, y, static_cast<double>(disparity[i]), P);
                for (int k = 0; k < 3; ++k) xyz[3 * i + k] = static_cast<float>(P[k]);
            }
        }
    delete[] dl;
    delete[] dr;
}
}  // namespace cba
