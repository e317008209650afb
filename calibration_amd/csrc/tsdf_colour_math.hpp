// tsdf_colour_math.hpp — colour in scan fusion (calibba.h: cba_tsdf_integrate_colour, rules 6 to 8 of the scan-fusion section) as
// __host__ __device__ code: step 7 of the update of one voxel by one map, the colour of an extract's point and the colour of a ray
// cast's hit.  The kernels of tsdf_fusion.hip call it per lane; tests/colour_cpu compiles the same header with g++.  The reference has
// no fusion: the rule is this project's own and is stated in full in calibba.h.
//
//   storage      float32 {R, G, B, Wc} records, one aligned 16-byte word per voxel, in rows of the {D, W} volume's pitch: the word of
//                voxel (i, j, k) starts at float 2 tsdf_at(g, i, j, k); the padding voxel of an odd row is never read by a rule.
//   a pixel      uint8 {R, G, B, A} read as one little-endian 32-bit word: R in bits 0-7, A in bits 24-31; outputs are packed the same way.
//   arithmetic   fp64, rounded once on store; nothing is contracted into an FMA.
#pragma once
#include <cmath>
#include <cstdint>

#include "tsdf_ray_math.hpp"

namespace cba {

// the first float of the colour record of voxel (i, j, k): R, G, B, then Wc
CBA_HD int64_t tsdf_colour_at(const TsdfGrid& g, int i, int j, int k) { return 2 * tsdf_at(g, i, j, k); }

// the record at `at` -> w [4]: one 16-byte load on the device
CBA_HD void tsdf_colour_word(const float* at, float* w) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 q = *reinterpret_cast<const float4*>(at);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
#else
    w[0] = at[0]; w[1] = at[1]; w[2] = at[2]; w[3] = at[3];
#endif
}

// whether step 7 runs for a voxel that step 6 updated with the s of step 5 through a pixel rgba
CBA_HD bool tsdf_colour_takes(double s, double trunc, uint32_t rgba) { return s <= trunc && (rgba >> 24) != 0; }

// step 7: the running mean of C [4] = {R, G, B, Wc} takes the pixel; the three channels with the old Wc, then Wc
CBA_HD void tsdf_colour_blend(float* C, uint32_t rgba, double max_weight) {
    CBA_NO_CONTRACT
    const double w = static_cast<double>(C[3]);
    const double w1 = w + 1.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double c = static_cast<double>((rgba >> (8 * ch)) & 255u);
        C[ch] = static_cast<float>((w * static_cast<double>(C[ch]) + c) / w1);
    }
    C[3] = static_cast<float>(w1 < max_weight ? w1 : max_weight);
}

// One voxel at X through one map and its image (steps 1-7): D, Wt and C [4] in place.  Returns whether steps 1-6 updated the voxel.
template <int MODEL>
CBA_HD bool tsdf_colour_update(const TsdfCam& c, const TsdfPose& p, const double* depth, const uint32_t* rgba, const TsdfRule& r, double X0,
                               double X1, double X2, float* D, float* Wt, float* C) {
    int64_t pixel;
    double s;
    if (!tsdf_update_at<MODEL>(c, p, depth, r, X0, X1, X2, D, Wt, &pixel, &s)) return false;
    const uint32_t px = rgba[pixel];
    if (tsdf_colour_takes(s, r.trunc, px)) tsdf_colour_blend(C, px, r.max_weight);
    return true;
}

// q = floor(C + 0.5), 0 when q < 0 (and for NaN), 255 when q > 255
CBA_HD uint32_t tsdf_colour_byte(double C) {
    const double q = floor(C + 0.5);
    if (!(q >= 0.0)) return 0u;
    return q > 255.0 ? 255u : static_cast<uint32_t>(q);
}

CBA_HD uint32_t tsdf_colour_pack(double R, double G, double B) {
    return tsdf_colour_byte(R) | tsdf_colour_byte(G) << 8 | tsdf_colour_byte(B) << 16 | 255u << 24;
}

// Rule 7: the colour of the point of the qualifying edge from voxel (i, j, k) along +axis (tsdf_edge gave Da, Db); 0 where there is none
CBA_HD uint32_t tsdf_colour_edge(const float* col, const TsdfGrid& g, int i, int j, int k, int axis, double Da, double Db) {
    CBA_NO_CONTRACT
    float a[4], b[4];
    tsdf_colour_word(col + tsdf_colour_at(g, i, j, k), a);
    tsdf_colour_word(col + tsdf_colour_at(g, i + (axis == 0), j + (axis == 1), k + (axis == 2)), b);
    const bool has_a = a[3] > 0.0f, has_b = b[3] > 0.0f;
    if (!has_a && !has_b) return 0u;
    if (!has_b) return tsdf_colour_pack(static_cast<double>(a[0]), static_cast<double>(a[1]), static_cast<double>(a[2]));
    if (!has_a) return tsdf_colour_pack(static_cast<double>(b[0]), static_cast<double>(b[1]), static_cast<double>(b[2]));
    const double t = Da / (Da - Db);
    double C[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) C[ch] = tsdf_ray_lerp(static_cast<double>(a[ch]), static_cast<double>(b[ch]), t);
    return tsdf_colour_pack(C[0], C[1], C[2]);
}

// Rule 8: the colour of a pixel of a ray cast from its stored outputs: status, depth = z_hit and the ray (x, y) of the table through
// the view v; 0 unless the pixel is a hit whose cell has Wc > 0 in all eight voxels
CBA_HD uint32_t tsdf_colour_hit(const float* col, const TsdfGrid& g, const TsdfRayView& v, int status, double z_hit, double x, double y) {
    CBA_NO_CONTRACT
    if (status != TSDF_RAY_HIT) return 0u;
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double s = v.R[a] * x, t = v.R[3 + a] * y;
        const double d = (s + t) + v.R[6 + a];
        const double along = z_hit * d;
        p[a] = v.c[a] + along;
    }
    int cell[3];
    double f[3];
    if (!tsdf_ray_cell(g, p[0], p[1], p[2], cell, f)) return 0u;
    double c[4][3];
    bool all = true;
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // (y, z) = (0,0), (1,0), (0,1), (1,1)
        const float* row = col + tsdf_colour_at(g, cell[0], cell[1] + (r & 1), cell[2] + (r >> 1));
        float a[4], b[4];  // voxels i and i + 1 <= nx - 1
        tsdf_colour_word(row, a);
        tsdf_colour_word(row + 4, b);
        all = all && a[3] > 0.0f && b[3] > 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[r][ch] = tsdf_ray_lerp(static_cast<double>(a[ch]), static_cast<double>(b[ch]), f[0]);
    }
    if (!all) return 0u;
    double C[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) C[ch] = tsdf_ray_lerp(tsdf_ray_lerp(c[0][ch], c[1][ch], f[1]), tsdf_ray_lerp(c[2][ch], c[3][ch], f[1]), f[2]);
    return tsdf_colour_pack(C[0], C[1], C[2]);
}

}  // namespace cba
