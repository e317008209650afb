// camera_math.hpp — the camera models themselves (include/calib/models/) as __host__ __device__ code: the projection of a
// camera-frame point, the pixel of an undistortion / rectification map, and the bilinear resampling of apply.  The kernels of
// camera.hip call it per lane; tests/camera_cpu compiles the same header with g++.
//
//   projection     PinholeCamera::project (pinhole.h:96-107) and ScheimpflugCamera::project (scheimpflug.h:139-181), in
//                  reproj_residual's expression order (reproj_math.hpp): Horner radial polynomial, the Scheimpflug ray through
//                  scheimpflug_consts' Rs, the shift of the principal intersection m0 as su / sv.  reproj_residual and
//                  reproj_core are NOT written in terms of it: they are the LM's hot path and keep their own copy.
//   unprojection   ls_unproject (linescan_math.hpp), called where it is: the pinhole's normalise + undistort (BrownConrady's
//                  5-step fixed point or DualDistortion's one step) and the documented exact Scheimpflug inverse.
//   map pixel      (u', v') -> normalised with K' in ls_normalize's order -> R^T (x, y, 1) -> project, in fp64; NaN where the
//                  ray does not reach the image side (z <= 0 pinhole, sensor denominator <= 0 Scheimpflug).
//   resampling     bilinear with a constant border: uint8 by OpenCV's 5-bit fixed-point rule, float32 by fp32 lerps (calibba.h).
#pragma once
#include <cmath>
#include <cstdint>

#include "linescan_math.hpp"

// The projection's own arithmetic and the float32 blend are not contracted into FMAs, so the device rounds as the host build and
// the numpy restatement do: an identity map gives the pixel grid exactly (a fused fy y + cy leaves ~1e-15 where the grid has 0), and
// a float32 blend next to a large border value agrees to the bit (fused lerps differed by ~1e-6 at a border of 17).
#if defined(__clang__)
#define CBA_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CBA_NO_CONTRACT
#endif

namespace cba {

// project(xyz) of one camera-frame point.  intr: [fx fy cx cy skew k1 k2 k3 p1 p2 (tau_x tau_y)], sd: scheimpflug_consts(intr)
// (unused for the pinhole).  No masking: z <= 0 or a sensor denominator <= 0 gives whatever the division gives.
template <int MODEL>
CBA_HD void cam_project(const double* intr, const double* sd, double P0, double P1, double P2, double* u, double* v) {
    CBA_NO_CONTRACT
    double x, y, su = 0.0, sv = 0.0;
    if (MODEL == CAM_PINHOLE_BC) {
        const double iz = 1.0 / P2;
        x = P0 * iz; y = P1 * iz;
    } else {
        const double* Rs = sd + SD_RS;
        const double is = 1.0 / (Rs[2] * P0 + Rs[5] * P1 + Rs[8] * P2);
        x = (Rs[0] * P0 + Rs[3] * P1 + Rs[6] * P2) * is - sd[SD_M0];
        y = (Rs[1] * P0 + Rs[4] * P1 + Rs[7] * P2) * is - sd[SD_M0 + 1];
        su = intr[0] * sd[SD_M0] + intr[4] * sd[SD_M0 + 1];
        sv = intr[1] * sd[SD_M0 + 1];
    }
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (intr[5] + r2 * (intr[6] + r2 * intr[7]));
    const double xy = x * y;
    const double xd = x * rad + 2.0 * intr[8] * xy + intr[9] * (r2 + 2.0 * x * x);
    const double yd = y * rad + intr[8] * (r2 + 2.0 * y * y) + 2.0 * intr[9] * xy;
    *u = intr[0] * xd + intr[4] * yd + intr[2] + su;
    *v = intr[1] * yd + intr[3] + sv;
}

// The denominator whose sign decides whether a ray reaches the image side: z (pinhole), n_sensor . P (Scheimpflug)
template <int MODEL>
CBA_HD double cam_denominator(const double* sd, double P0, double P1, double P2) {
    CBA_NO_CONTRACT
    if (MODEL == CAM_PINHOLE_BC) return P2;
    const double* Rs = sd + SD_RS;
    return Rs[2] * P0 + Rs[5] * P1 + Rs[8] * P2;
}

// One camera of a map: its intrinsics, Scheimpflug constants, rectifying rotation R (row-major) and new camera matrix K'
struct CamMapCam {
    double intr[12];
    double sd[SD_SIZE];
    double R[9];
    double kp[5];  // fx' fy' cx' cy' skew'
};
static_assert(sizeof(CamMapCam) == 496, "CamMapCam is read by k_cam_map: its layout is fixed");

// The source pixel of output pixel (up, vp): the projection of P = R^T (x, y, 1), (x, y) = K'^-1 (up, vp) in ls_normalize's order,
// rounded to nearest float32; NaN in both where the denominator is not positive (or NaN)
template <int MODEL>
CBA_HD void cam_map_pixel(const CamMapCam& c, double up, double vp, float* mx, float* my) {
    double x, y;
    ls_normalize(c.kp, up, vp, &x, &y);
    const double q[3] = {x, y, 1.0};
    double P[3];
    mat3_tvec(c.R, q, P);
    if (!(cam_denominator<MODEL>(c.sd, P[0], P[1], P[2]) > 0.0)) {
        *mx = NAN;
        *my = NAN;
        return;
    }
    double u, v;
    cam_project<MODEL>(c.intr, c.sd, P[0], P[1], P[2], &u, &v);
    *mx = static_cast<float>(u);
    *my = static_cast<float>(v);
}

// ---- resampling (apply) ---------------------------------------------------------------------------------------------------
constexpr float CAM_COORD_MAX = 16777216.0f;  // 2^24: a map coordinate beyond it (or NaN) gives the border value

// uint8: OpenCV's fixed-point rule (INTER_BITS = 5).  X = rint(32 m) (half to even), tap = X >> 5, a = X & 31; weights
// (32-a)(32-b)32, a(32-b)32, (32-a)b32, ab32 of taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), summing to 2^15.
// Returns false where the pixel is all border.
CBA_HD bool cam_taps_u8(float mx, float my, int* x0, int* y0, int* w) {
    if (!(fabsf(mx) <= CAM_COORD_MAX && fabsf(my) <= CAM_COORD_MAX)) return false;
    const int X = static_cast<int>(rintf(mx * 32.0f)), Y = static_cast<int>(rintf(my * 32.0f));
    const int a = X & 31, b = Y & 31;
    *x0 = X >> 5;
    *y0 = Y >> 5;
    w[0] = (32 - a) * (32 - b) * 32;
    w[1] = a * (32 - b) * 32;
    w[2] = (32 - a) * b * 32;
    w[3] = a * b * 32;
    return true;
}

// (sum w p + 2^14) >> 15, saturated to [0, 255]
CBA_HD uint8_t cam_blend_u8(const int* w, int p00, int p01, int p10, int p11) {
    int r = (w[0] * p00 + w[1] * p01 + w[2] * p10 + w[3] * p11 + (1 << 14)) >> 15;
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    return static_cast<uint8_t>(r);
}

// float32: tap (x0, y0) = floor(m), fractional parts fx, fy (exact below 2^24)
CBA_HD bool cam_taps_f32(float mx, float my, int* x0, int* y0, float* fx, float* fy) {
    if (!(fabsf(mx) <= CAM_COORD_MAX && fabsf(my) <= CAM_COORD_MAX)) return false;
    const float fx0 = floorf(mx), fy0 = floorf(my);
    *x0 = static_cast<int>(fx0);
    *y0 = static_cast<int>(fy0);
    *fx = mx - fx0;
    *fy = my - fy0;
    return true;
}

// top = p00 + fx (p01 - p00), bottom = p10 + fx (p11 - p10), result = top + fy (bottom - top)
CBA_HD float cam_blend_f32(float fx, float fy, float p00, float p01, float p10, float p11) {
    CBA_NO_CONTRACT
    const float t = p00 + fx * (p01 - p00);
    const float b = p10 + fx * (p11 - p10);
    return t + fy * (b - t);
}

// One output pixel of channels ch (interleaved) from a source of sw x sh; taps outside the source read the border.
CBA_HD bool cam_in_source(int x, int y, int sw, int sh) {
    return x >= 0 && x < sw && y >= 0 && y < sh;
}

CBA_HD void cam_remap_u8(const uint8_t* src, int sw, int sh, int ch, float mx, float my, uint8_t border, uint8_t* out) {
    int x0, y0, w[4];
    if (!cam_taps_u8(mx, my, &x0, &y0, w)) {
        for (int k = 0; k < ch; ++k) out[k] = border;
        return;
    }
    const bool i00 = cam_in_source(x0, y0, sw, sh), i01 = cam_in_source(x0 + 1, y0, sw, sh);
    const bool i10 = cam_in_source(x0, y0 + 1, sw, sh), i11 = cam_in_source(x0 + 1, y0 + 1, sw, sh);
    const int64_t o = (static_cast<int64_t>(y0) * sw + x0) * ch, row = static_cast<int64_t>(sw) * ch;
    for (int k = 0; k < ch; ++k) {
        const int p00 = i00 ? src[o + k] : border, p01 = i01 ? src[o + ch + k] : border;
        const int p10 = i10 ? src[o + row + k] : border, p11 = i11 ? src[o + row + ch + k] : border;
        out[k] = cam_blend_u8(w, p00, p01, p10, p11);
    }
}

CBA_HD void cam_remap_f32(const float* src, int sw, int sh, int ch, float mx, float my, float border, float* out) {
    int x0, y0;
    float fx, fy;
    if (!cam_taps_f32(mx, my, &x0, &y0, &fx, &fy)) {
        for (int k = 0; k < ch; ++k) out[k] = border;
        return;
    }
    const bool i00 = cam_in_source(x0, y0, sw, sh), i01 = cam_in_source(x0 + 1, y0, sw, sh);
    const bool i10 = cam_in_source(x0, y0 + 1, sw, sh), i11 = cam_in_source(x0 + 1, y0 + 1, sw, sh);
    const int64_t o = (static_cast<int64_t>(y0) * sw + x0) * ch, row = static_cast<int64_t>(sw) * ch;
    for (int k = 0; k < ch; ++k) {
        const float p00 = i00 ? src[o + k] : border, p01 = i01 ? src[o + ch + k] : border;
        const float p10 = i10 ? src[o + row + k] : border, p11 = i11 ? src[o + row + ch + k] : border;
        out[k] = cam_blend_f32(fx, fy, p00, p01, p10, p11);
    }
}

}  // namespace cba
