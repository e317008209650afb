// tsdf_ray_math.hpp — the ray cast into a TSDF volume (calibba.h: cba_tsdf_raycast, rule 5 of the scan-fusion section) as
// __host__ __device__ code: the view of a pose, the range of a ray inside the volume, one trilinear sample, the march to the first
// zero crossing and the outputs of a pixel.  k_tsdf_raycast (tsdf_fusion.hip) calls tsdf_ray_pixel per lane; tests/raycast_cpu compiles
// the same header with g++.  The reference has no ray cast: the rule is this project's own and is stated in full in calibba.h.
//
//   rays         a table [H][W][2] of (x, y) = ls_unproject(camera, col, row), written by k_tsdf_rays before the cast; everything here is a
//                function of its stored values (the unprojection itself is compiled with contraction and is not held to the bit).
//   storage      the volume of tsdf_math.hpp.  A cell is four rows of two adjacent {D, W} pairs; on the device a row is one 16-byte load
//                where its first voxel is even (rows start 16-byte aligned: the pitch is even), two 8-byte loads where it is odd.  The
//                second voxel of a row is at most nx - 1: the padding voxel of an odd row is never read.
//   arithmetic   fp64, + - * / sqrt floor and comparisons, each rounded once in the order written; nothing is contracted into an FMA.
//   termination  the march ends by a hit, by "behind", or by one of the three guards of step 6; every index is formed from a lattice
//                coordinate that was compared against [0, n - 1] in fp64 first.
#pragma once
#include <cmath>
#include <cstdint>

#include "tsdf_math.hpp"

namespace cba {

constexpr int TSDF_RAY_MAX_SAMPLES = 65536;  // CBA_TSDF_RAY_MAX_SAMPLES
constexpr int TSDF_RAY_MISS = 0, TSDF_RAY_HIT = 1, TSDF_RAY_BEHIND = 2, TSDF_RAY_NO_RAY = 3;

// the view of one pose: R (volume frame -> camera, row-major) and the camera's centre in the volume frame; a table the kernel indexes
// with wave-uniform values only
struct TsdfRayView {
    double R[9];
    double c[3];
};
static_assert(sizeof(TsdfRayView) == 96, "read by k_tsdf_raycast: the layout is fixed");

// the options of a call with step already resolved (step_eff) and the volume's truncation beside them
struct TsdfRayRule {
    double step, skip, near_depth, far_depth, min_weight, trunc;
};

struct TsdfRayOut {
    double depth;   // z_hit; NaN unless status is HIT
    double nrm[3];  // camera frame; NaN where there is none
    int32_t status;
    int32_t count;  // samples taken by the march
};

CBA_HD void tsdf_ray_view(const double* pose7, TsdfRayView* v) {
    CBA_NO_CONTRACT
    quat_to_rotmat(pose7, v->R);
    const double* t = pose7 + 4;
    for (int r = 0; r < 3; ++r) {
        const double a = v->R[r] * t[0], b = v->R[3 + r] * t[1], c = v->R[6 + r] * t[2];
        v->c[r] = -((a + b) + c);
    }
}

CBA_HD double tsdf_ray_lerp(double a, double b, double t) {
    CBA_NO_CONTRACT
    const double rise = t * (b - a);
    return a + rise;
}

// the row of cell (i, j, k) at (j, k): D and W of voxels i and i + 1
CBA_HD void tsdf_ray_row(const float* vol, const TsdfGrid& g, int i, int j, int k, float* d0, float* w0, float* d1, float* w1) {
    const float* at = vol + tsdf_at(g, i, j, k);
#if defined(__HIP_DEVICE_COMPILE__)
    if ((i & 1) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(at);
        *d0 = q.x; *w0 = q.y; *d1 = q.z; *w1 = q.w;
    } else {
        const float2 a = *reinterpret_cast<const float2*>(at), b = *reinterpret_cast<const float2*>(at + 2);
        *d0 = a.x; *w0 = a.y; *d1 = b.x; *w1 = b.y;
    }
#else
    *d0 = at[0]; *w0 = at[1]; *d1 = at[2]; *w1 = at[3];
#endif
}

// The cell of p (volume frame) and p's place in it ("Sample at z"): false when p is outside the lattice; else cell [3] = (i, j, k), f [3]
CBA_HD bool tsdf_ray_cell(const TsdfGrid& g, double p0, double p1, double p2, int* cell, double* f) {
    CBA_NO_CONTRACT
    const double g0 = (p0 - g.o[0]) / g.vs, g1 = (p1 - g.o[1]) / g.vs, g2 = (p2 - g.o[2]) / g.vs;
    // false for NaN, and decided before any conversion to an integer
    if (!(g0 >= 0.0 && g0 <= static_cast<double>(g.nx - 1) && g1 >= 0.0 && g1 <= static_cast<double>(g.ny - 1) && g2 >= 0.0 &&
          g2 <= static_cast<double>(g.nz - 1)))
        return false;
    int i = static_cast<int>(floor(g0)), j = static_cast<int>(floor(g1)), k = static_cast<int>(floor(g2));
    i = i < g.nx - 2 ? i : g.nx - 2;
    j = j < g.ny - 2 ? j : g.ny - 2;
    k = k < g.nz - 2 ? k : g.nz - 2;
    cell[0] = i; cell[1] = j; cell[2] = k;
    f[0] = g0 - static_cast<double>(i); f[1] = g1 - static_cast<double>(j); f[2] = g2 - static_cast<double>(k);
    return true;
}

// One sample at p (volume frame): false when p is outside the lattice or a voxel of its cell has W < min_weight; else *F
CBA_HD bool tsdf_ray_sample(const float* vol, const TsdfGrid& g, double p0, double p1, double p2, double min_weight, double* F) {
    CBA_NO_CONTRACT
    int cell[3];
    double f[3];
    if (!tsdf_ray_cell(g, p0, p1, p2, cell, f)) return false;
    const int i = cell[0], j = cell[1], k = cell[2];
    const double f0 = f[0], f1 = f[1], f2 = f[2];
    double c[4];
    bool heavy = true;
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // (y, z) = (0,0), (1,0), (0,1), (1,1)
        float d0, w0, d1, w1;
        tsdf_ray_row(vol, g, i, j + (r & 1), k + (r >> 1), &d0, &w0, &d1, &w1);
        heavy = heavy && static_cast<double>(w0) >= min_weight && static_cast<double>(w1) >= min_weight;
        c[r] = tsdf_ray_lerp(static_cast<double>(d0), static_cast<double>(d1), f0);
    }
    if (!heavy) return false;
    *F = tsdf_ray_lerp(tsdf_ray_lerp(c[0], c[1], f1), tsdf_ray_lerp(c[2], c[3], f1), f2);
    return true;
}

CBA_HD double tsdf_ray_min(double a, double b) { return a < b ? a : b; }
CBA_HD double tsdf_ray_max(double a, double b) { return a > b ? a : b; }

// The range [z0, z1] of the ray c + z d inside the lattice's box and [near_depth, far_depth]; false: a miss
CBA_HD bool tsdf_ray_range(const TsdfGrid& g, const double* c, const double* d, const TsdfRayRule& r, double* z0, double* z1) {
    CBA_NO_CONTRACT
    const int n[3] = {g.nx, g.ny, g.nz};
    double a0 = r.near_depth, a1 = r.far_depth;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = g.o[a], hi = tsdf_coord(g.o[a], n[a] - 1, g.vs);
        if (d[a] == 0.0) {
            if (c[a] < lo || c[a] > hi) return false;
            continue;
        }
        const double ta = (lo - c[a]) / d[a], tb = (hi - c[a]) / d[a];
        a0 = tsdf_ray_max(a0, tsdf_ray_min(ta, tb));
        a1 = tsdf_ray_min(a1, tsdf_ray_max(ta, tb));
    }
    *z0 = a0;
    *z1 = a1;
    return a0 <= a1;  // false for NaN
}

// One pixel: the ray (x, y) of the table through the view v.  o->depth and o->nrm are NaN unless the march hits.
CBA_HD void tsdf_ray_pixel(const float* vol, const TsdfGrid& g, const TsdfRayView& v, const TsdfRayRule& r, double x, double y, TsdfRayOut* o) {
    CBA_NO_CONTRACT
    o->depth = NAN;
    o->nrm[0] = o->nrm[1] = o->nrm[2] = NAN;
    o->count = 0;
    o->status = TSDF_RAY_NO_RAY;
    if (!(tsdf_finite(x) && tsdf_finite(y))) return;
    o->status = TSDF_RAY_MISS;
    double d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double s = v.R[a] * x, t = v.R[3 + a] * y;
        d[a] = (s + t) + v.R[6 + a];
    }
    double z, z1;
    if (!tsdf_ray_range(g, v.c, d, r, &z, &z1)) return;
    bool pv = false;
    double Fp = 0.0, zp = 0.0;
    int count = 0;
    int status = TSDF_RAY_MISS;
    double z_hit = 0.0;
#pragma unroll 1
    for (;;) {
        double F = 0.0;
        const double s0 = z * d[0], s1 = z * d[1], s2 = z * d[2];
        const bool ok = tsdf_ray_sample(vol, g, v.c[0] + s0, v.c[1] + s1, v.c[2] + s2, r.min_weight, &F);
        ++count;
        if (ok && F < 0.0) {
            if (pv && Fp >= 0.0) {
                const double w = Fp / (Fp - F);
                const double part = (z - zp) * w;
                z_hit = zp + part;
                status = TSDF_RAY_HIT;
                break;
            }
            if (!pv) {
                status = TSDF_RAY_BEHIND;
                break;
            }
        }
        if (ok && F >= 0.0 && pv && Fp < 0.0) {
            status = TSDF_RAY_BEHIND;
            break;
        }
        double adv = r.step;
        if (ok) {
            const double far = (r.skip * F) * r.trunc;
            adv = far > r.step ? far : r.step;
        }
        const double zn = z + adv;
        // the three guards: past the range, no progress at a large z, the cap.  Each is false-safe for NaN.
        if (!(zn <= z1) || !(zn > z) || count == TSDF_RAY_MAX_SAMPLES) break;
        pv = ok;
        Fp = F;
        zp = z;
        z = zn;
    }
    o->count = count;
    o->status = status;
    if (status != TSDF_RAY_HIT) return;
    o->depth = z_hit;
    double p[3], n[3];
    bool all = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double s = z_hit * d[a];
        p[a] = v.c[a] + s;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double Fa = 0.0, Fb = 0.0;
        const double up = p[a] + g.vs, dn = p[a] - g.vs;
        const bool oka = tsdf_ray_sample(vol, g, a == 0 ? up : p[0], a == 1 ? up : p[1], a == 2 ? up : p[2], r.min_weight, &Fa);
        const bool okb = tsdf_ray_sample(vol, g, a == 0 ? dn : p[0], a == 1 ? dn : p[1], a == 2 ? dn : p[2], r.min_weight, &Fb);
        all = all && oka && okb;
        n[a] = Fa - Fb;
    }
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (!(all && len > 0.0 && tsdf_finite(len))) return;
    const double m0 = n[0] / len, m1 = n[1] / len, m2 = n[2] / len;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        const double s = v.R[3 * rr] * m0, t = v.R[3 * rr + 1] * m1, u = v.R[3 * rr + 2] * m2;
        o->nrm[rr] = (s + t) + u;
    }
}

}  // namespace cba
