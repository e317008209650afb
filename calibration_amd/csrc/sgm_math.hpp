// sgm_math.hpp — semi-global matching (calibba.h: cba_sgm_matcher) as __host__ __device__ code.  The kernels of stereo_sgm.hip call
// the census and cost pieces per pixel; tests/sgm_cpu compiles the same header with g++ and walks every path of a pair with the scalar
// recurrence.  The reference has no counterpart.
//
//   census     sgm_census_bit (the rule of one bit) and sgm_census_code: the 62 bits of a pixel in one uint64, row by row, the centre
//              left out.  Only the set of bits matters: both images are packed the same way
//   cost       sgm_cost: the Hamming distance of two codes; a right column outside the image has the code 0
//   path       sgm_path_step: L_r(p, .) from L_r(p - r, .) and C(p, .) on an array of D candidates.  The path kernel of stereo_sgm.hip
//              runs the same step on packed uint16 pairs spread over 16 lanes; every quantity is an exact integer, so the two agree
//   selection  StereoSel / stereo_disparity / stereo_lr_ok / stereo_point of stereo_math.hpp, with S for C and sgm_interval
#pragma once
#include <cstdint>
#include <vector>

#include "stereo_math.hpp"

namespace cba {

constexpr int SGM_CENSUS_HX = 4, SGM_CENSUS_HY = 3;  // the window is |i| <= 4, |j| <= 3
constexpr int SGM_PATH_INF = 0x7fff;                 // a path cost "no such candidate": no minimum picks it up, + p1 stays in 16 bits

CBA_HD bool sgm_census_bit(int neighbour, int centre) { return neighbour < centre; }

// img: one image [H][W]; pixels outside read 0
CBA_HD uint64_t sgm_census_code(const uint8_t* img, int W, int H, int x, int y) {
    const int c = img[static_cast<size_t>(y) * W + x];
    uint64_t code = 0;
    for (int j = -SGM_CENSUS_HY; j <= SGM_CENSUS_HY; ++j)
        for (int i = -SGM_CENSUS_HX; i <= SGM_CENSUS_HX; ++i) {
            if (i == 0 && j == 0) continue;
            const int xx = x + i, yy = y + j;
            const bool in = xx >= 0 && xx < W && yy >= 0 && yy < H;
            const int t = img[static_cast<size_t>(in ? yy : y) * W + (in ? xx : x)];  // always a load inside the image: no branch per bit
            const int v = in ? t : 0;
            code = (code << 1) | (sgm_census_bit(v, c) ? 1u : 0u);
        }
    return code;
}

CBA_HD int sgm_popcount64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

// C(x, y, d): codeR is the code of right pixel (x - d, y), or 0 when x - d lies outside the image
CBA_HD int sgm_cost(uint64_t codeL, uint64_t codeR) { return sgm_popcount64(codeL ^ codeR); }

// The directions r in the order of the rule: the first `paths` (4 or 8) are used
CBA_HD void sgm_direction(int k, int* dx, int* dy) {
    const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
    *dx = DX[k];
    *dy = DY[k];
}

// One step of a path: Lq[D] = L_r(q, .) of the predecessor, C[D] the pixel's costs, L[D] out (L may not alias Lq)
CBA_HD void sgm_path_step(const uint16_t* Lq, const uint8_t* C, int D, int p1, int p2, uint16_t* L) {
    int M = Lq[0];
    for (int k = 1; k < D; ++k) M = Lq[k] < M ? Lq[k] : M;
    for (int k = 0; k < D; ++k) {
        int m = Lq[k];
        const int far = M + p2;
        if (k > 0 && Lq[k - 1] + p1 < m) m = Lq[k - 1] + p1;
        if (k + 1 < D && Lq[k + 1] + p1 < m) m = Lq[k + 1] + p1;
        if (far < m) m = far;
        L[k] = static_cast<uint16_t>(C[k] + m - M);
    }
}

// The admissible candidates of a pixel in column x: [lo, hi] (empty when lo > hi).  right == 0: a left pixel, 0 <= x - d <= W - 1;
// right != 0: a right pixel x', 0 <= x' + d <= W - 1.  No window margin: the census is defined everywhere.
CBA_HD void sgm_interval(int x, int W, int dmin, int D, int right, int* lo, int* hi) {
    const int dmax = dmin + D - 1;
    const int a = right ? -x : x - W + 1, b = right ? W - 1 - x : x;
    *lo = a > dmin ? a : dmin;
    *hi = b < dmax ? b : dmax;
}

// ---- one pair on the host: every path walked with sgm_path_step (the host build; the kernels do not call it) --------------------
struct SgmParams {
    int W, H, dmin, D, p1, p2, paths, uniqueness_percent, lr_max_diff, subpixel;
};

// disparity [H][W] float32, cost [H][W] int32 or null, xyz [H][W][3] float32 or null (needs g)
inline void sgm_match_pair(const SgmParams& p, const uint8_t* L, const uint8_t* R, const StereoGeom* g, float* disparity, int32_t* cost,
                           float* xyz) {
    const int W = p.W, H = p.H, D = p.D;
    const size_t px = static_cast<size_t>(W) * H;
    std::vector<uint64_t> cl(px), cr(px);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            cl[static_cast<size_t>(y) * W + x] = sgm_census_code(L, W, H, x, y);
            cr[static_cast<size_t>(y) * W + x] = sgm_census_code(R, W, H, x, y);
        }
    std::vector<uint8_t> C(px * D);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < D; ++k) {
                const int xr = x - (p.dmin + k);
                const size_t i = static_cast<size_t>(y) * W + x;
                C[i * D + k] = static_cast<uint8_t>(sgm_cost(cl[i], xr >= 0 && xr < W ? cr[static_cast<size_t>(y) * W + xr] : 0));
            }
    std::vector<uint16_t> S(px * D, 0), Lq(D), Ln(D);
    for (int r = 0; r < p.paths; ++r) {
        int dx, dy;
        sgm_direction(r, &dx, &dy);
        for (int y0 = 0; y0 < H; ++y0)
            for (int x0 = 0; x0 < W; ++x0) {
                const int qx = x0 - dx, qy = y0 - dy;
                if (qx >= 0 && qx < W && qy >= 0 && qy < H) continue;  // not the first pixel of a line
                for (int x = x0, y = y0, first = 1; x >= 0 && x < W && y >= 0 && y < H; x += dx, y += dy, first = 0) {
                    const size_t i = (static_cast<size_t>(y) * W + x) * D;
                    if (first)
                        for (int k = 0; k < D; ++k) Ln[k] = C[i + k];
                    else
                        sgm_path_step(Lq.data(), &C[i], D, p.p1, p.p2, Ln.data());
                    for (int k = 0; k < D; ++k) S[i + k] = static_cast<uint16_t>(S[i + k] + Ln[k]);
                    Lq.swap(Ln);
                }
            }
    }
    std::vector<int16_t> dl(px), dr(px);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = static_cast<size_t>(y) * W + x;
            for (int right = 0; right < 2; ++right) {
                int lo, hi;
                sgm_interval(x, W, p.dmin, D, right, &lo, &hi);
                StereoSel s;
                stereo_sel_init(s);
                for (int d = lo; d <= hi; ++d) stereo_sel_push(s, d, S[(i + (right ? d : 0)) * D + (d - p.dmin)]);
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
}
}  // namespace cba
