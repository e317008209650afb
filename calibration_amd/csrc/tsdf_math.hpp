// tsdf_math.hpp — scan fusion (calibba.h: cba_tsdf_integrate, cba_tsdf_extract) as __host__ __device__ code: the update of one voxel
// by one depth map, and one lattice edge with its zero crossing, point and normal.  The kernels of tsdf_fusion.hip call it per lane;
// tests/fusion_cpu compiles the same header with g++.  The reference has no fusion: the rule is this project's own and is stated in
// full in calibba.h.
//
//   projection   cam_project / cam_denominator (camera_math.hpp), called where they are.
//   storage      float32 {D, W} pairs, x fastest, rows of `pitch` voxels (nx rounded up to even, so that two adjacent x voxels are one
//                aligned 16-byte word); the padding voxel of an odd row is never read by a rule.
//   arithmetic   fp64, rounded once on store; nothing is contracted into an FMA.
#pragma once
#include <cmath>
#include <cstdint>

#include "camera_math.hpp"

namespace cba {

constexpr int TSDF_EXTRACT_TILE = 1024;  // voxels (of the dense order l) per workgroup of the extraction

struct TsdfGrid {
    int32_t nx, ny, nz, pitch;
    double o[3];
    double vs;
};
// the camera of a call and the pose of one map: tables the kernel indexes with wave-uniform values only
struct TsdfCam {
    double intr[12];
    double sd[SD_SIZE];
};
struct TsdfPose {
    double R[9];
    double t[3];
};
struct TsdfRule {
    double trunc, max_depth, max_weight;
    int32_t W, H;
};
static_assert(sizeof(TsdfCam) == 384 && sizeof(TsdfPose) == 96, "read by k_tsdf_integrate: the layouts are fixed");

CBA_HD bool tsdf_finite(double a) { return fabs(a) <= 1.7976931348623157e308; }  // false for NaN and +-inf

// the position of lattice index i along one axis: the product rounded, then the sum
CBA_HD double tsdf_coord(double o, int i, double vs) {
    CBA_NO_CONTRACT
    const double step = static_cast<double>(i) * vs;
    return o + step;
}

// the first float of voxel (i, j, k): D, then W
CBA_HD int64_t tsdf_at(const TsdfGrid& g, int i, int j, int k) {
    return 2 * ((static_cast<int64_t>(k) * g.ny + j) * g.pitch + i);
}

// voxel l of the dense order [nz][ny][nx], x fastest -> (i, j, k)
CBA_HD void tsdf_voxel_of(const TsdfGrid& g, int64_t l, int* i, int* j, int* k) {
    const int64_t row = l / g.nx;
    *i = static_cast<int>(l - row * g.nx);
    *k = static_cast<int>(row / g.ny);
    *j = static_cast<int>(row - static_cast<int64_t>(*k) * g.ny);
}

// One voxel at X through one map (steps 1-6 of calibba.h).  depth: the map [H][W].  Returns whether the voxel was updated, and then
// *pixel = py W + px, the place of step 4's sample in the map, and *s of step 5 (what step 7 of tsdf_colour_math.hpp goes on from).
template <int MODEL>
CBA_HD bool tsdf_update_at(const TsdfCam& c, const TsdfPose& p, const double* depth, const TsdfRule& r, double X0, double X1, double X2, float* D,
                           float* Wt, int64_t* pixel, double* s_out) {
    CBA_NO_CONTRACT
    const double P0 = ((p.R[0] * X0 + p.R[1] * X1) + p.R[2] * X2) + p.t[0];
    const double P1 = ((p.R[3] * X0 + p.R[4] * X1) + p.R[5] * X2) + p.t[1];
    const double P2 = ((p.R[6] * X0 + p.R[7] * X1) + p.R[8] * X2) + p.t[2];
    if (!(P2 > 0.0) || !(cam_denominator<MODEL>(c.sd, P0, P1, P2) > 0.0)) return false;
    double u, v;
    cam_project<MODEL>(c.intr, c.sd, P0, P1, P2, &u, &v);
    const double px = floor(u + 0.5), py = floor(v + 0.5);
    if (!(px >= 0.0 && px <= static_cast<double>(r.W - 1) && py >= 0.0 && py <= static_cast<double>(r.H - 1))) return false;  // false for NaN
    const int64_t at = static_cast<int64_t>(static_cast<int>(py)) * r.W + static_cast<int>(px);
    const double d = depth[at];
    if (!(tsdf_finite(d) && d > 0.0 && d <= r.max_depth)) return false;
    const double s = d - P2;
    if (s < -r.trunc) return false;
    double f = s / r.trunc;
    if (f > 1.0) f = 1.0;
    const double w = static_cast<double>(*Wt);
    const double w1 = w + 1.0;
    *D = static_cast<float>((w * static_cast<double>(*D) + f) / w1);
    *Wt = static_cast<float>(w1 < r.max_weight ? w1 : r.max_weight);
    *pixel = at;
    *s_out = s;
    return true;
}

template <int MODEL>
CBA_HD bool tsdf_update(const TsdfCam& c, const TsdfPose& p, const double* depth, const TsdfRule& r, double X0, double X1, double X2, float* D,
                        float* Wt) {
    int64_t pixel;
    double s;
    return tsdf_update_at<MODEL>(c, p, depth, r, X0, X1, X2, D, Wt, &pixel, &s);
}

// The edge from voxel a = (i, j, k) along +axis: whether it exists and qualifies; Da, Db: its two distances
CBA_HD bool tsdf_edge(const float* vol, const TsdfGrid& g, int i, int j, int k, int axis, double min_weight, double* Da, double* Db) {
    const int bi = i + (axis == 0), bj = j + (axis == 1), bk = k + (axis == 2);
    if (bi >= g.nx || bj >= g.ny || bk >= g.nz) return false;
    const float* a = vol + tsdf_at(g, i, j, k);
    const float* b = vol + tsdf_at(g, bi, bj, bk);
    if (!(static_cast<double>(a[1]) >= min_weight && static_cast<double>(b[1]) >= min_weight)) return false;
    *Da = static_cast<double>(a[0]);
    *Db = static_cast<double>(b[0]);
    return (*Da < 0.0) != (*Db < 0.0);
}

// the three qualifying bits of a voxel: bit c = its +c edge
CBA_HD int tsdf_edge_mask(const float* vol, const TsdfGrid& g, int i, int j, int k, double min_weight) {
    double Da, Db;
    int m = 0;
    for (int axis = 0; axis < 3; ++axis)
        if (tsdf_edge(vol, g, i, j, k, axis, min_weight, &Da, &Db)) m |= 1 << axis;
    return m;
}

// central differences of D at a voxel; false when a neighbour is outside the grid or has W <= 0
CBA_HD bool tsdf_gradient(const float* vol, const TsdfGrid& g, int i, int j, int k, double* gr) {
    const int n[3] = {g.nx, g.ny, g.nz}, at[3] = {i, j, k};
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        gr[c] = 0.0;
        if (at[c] < 1 || at[c] + 1 >= n[c]) {
            ok = false;
            continue;
        }
        const float* hi = vol + tsdf_at(g, i + (c == 0), j + (c == 1), k + (c == 2));
        const float* lo = vol + tsdf_at(g, i - (c == 0), j - (c == 1), k - (c == 2));
        if (!(hi[1] > 0.0f && lo[1] > 0.0f)) ok = false;
        gr[c] = static_cast<double>(hi[0]) - static_cast<double>(lo[0]);
    }
    return ok;
}

// The point and the normal of a qualifying edge (tsdf_edge gave Da, Db): pt [3], nrm [3] (NaN in all three when there is none)
CBA_HD void tsdf_edge_point(const float* vol, const TsdfGrid& g, int i, int j, int k, int axis, double Da, double Db, double* pt, double* nrm) {
    CBA_NO_CONTRACT
    const double t = Da / (Da - Db);
    pt[0] = tsdf_coord(g.o[0], i, g.vs);
    pt[1] = tsdf_coord(g.o[1], j, g.vs);
    pt[2] = tsdf_coord(g.o[2], k, g.vs);
    const double along = t * g.vs;
    pt[axis] = pt[axis] + along;
    double ga[3], gb[3], n[3];
    const bool oka = tsdf_gradient(vol, g, i, j, k, ga);
    const bool okb = tsdf_gradient(vol, g, i + (axis == 0), j + (axis == 1), k + (axis == 2), gb);
    for (int c = 0; c < 3; ++c) {
        const double rise = t * (gb[c] - ga[c]);
        n[c] = ga[c] + rise;
    }
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool ok = oka && okb && len > 0.0 && tsdf_finite(len);
    for (int c = 0; c < 3; ++c) nrm[c] = ok ? n[c] / len : NAN;
}

}  // namespace cba
