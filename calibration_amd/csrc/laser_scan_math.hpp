// laser_scan_math.hpp — laser profile scanning (calibba.h: cba_laser_points, cba_laser_scanner) as __host__ __device__ code: the
// peak of one image line by the rule calibba.h states (maximum, lowest position, saturation plateau, centre of gravity of a window)
// and the intersection of a pixel's ray with the calibrated laser plane.  The kernels (laser_scan.hip) build a line's peak from these
// pieces however they split the line; tests/laser_scan_cpu compiles the same header with g++ and walks every line in one pass.
// The reference has no counterpart: it computes the plane and its homography and never applies them.
//
//   unprojection   ls_unproject (linescan_math.hpp), called where it is
//   plane_xy       ls_plane_homography (linescan_math.hpp), evaluated once per call on the host
//   peak           LaserPeak<V> = (m, p0, p1) of a contiguous run of positions: laser_peak_push adds the next position,
//                  laser_peak_merge joins the run that follows.  Both give the (m, p0, p1) of the joined run exactly, so a line's
//                  peak does not depend on where it was cut.  V: int for uint8 samples, float for float32 samples
//   window sums    uint8: exact integers (any order); float32: fp64, ascending positions, no contraction
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "camera_math.hpp"

namespace cba {

// camera, plane [nx ny nz d] and Hp = ls_plane_homography(plane) (row-major): a kernel argument, wave-uniform
struct LaserGeom {
    LsCamera cam;
    double plane[4];
    double Hp[9];
};
static_assert(sizeof(LaserGeom) == 624, "LaserGeom is a kernel argument: its layout is fixed");

CBA_HD void laser_fill_geom(int model, const double* intr, int n_inv, const double* inv, const double* plane, LaserGeom* g) {
    ls_fill_camera(model, intr, n_inv, inv, &g->cam);
    for (int j = 0; j < 4; ++j) g->plane[j] = plane[j];
    ls_plane_homography(plane, g->Hp);
}

// pose7 -> [R (9, row-major) | t (3)]: the quaternion's matrix without normalisation, as cba_triangulate reads a pose
CBA_HD void laser_pose_rt(const double* pose7, double* Rt) {
    quat_to_rotmat(pose7, Rt);
    for (int j = 0; j < 3; ++j) Rt[9 + j] = pose7[4 + j];
}

// The peak of a run of positions.  p0 < 0: the run holds no sample that is not NaN (m is unspecified then).
template <typename V>
struct LaserPeak {
    V m;
    int p0, p1;
};

template <typename V>
CBA_HD void laser_peak_init(LaserPeak<V>& s) {
    s.m = V(0);
    s.p0 = -1;
    s.p1 = -1;
}

// the sample v at position p joins the run that ends at p - 1.  NaN compares false everywhere: it is never the maximum and it ends a
// plateau
template <typename V>
CBA_HD void laser_peak_push(LaserPeak<V>& s, V v, int p) {
    const bool take = s.p0 < 0 ? v == v : v > s.m;
    const bool grow = !take && v == s.m && s.p1 == p - 1;
    s.m = take ? v : s.m;
    s.p0 = take ? p : s.p0;
    s.p1 = (take || grow) ? p : s.p1;
}

// the run b, which starts at position b0, follows the run a without a gap
template <typename V>
CBA_HD void laser_peak_merge(LaserPeak<V>& a, const LaserPeak<V>& b, int b0) {
    if (b.p0 < 0) return;
    if (a.p0 < 0 || b.m > a.m) {
        a = b;
        return;
    }
    if (b.m == a.m && a.p1 == b0 - 1 && b.p0 == b0) a.p1 = b.p1;  // the plateau crosses the cut
}

// the window [lo, hi] of a peak inside the ROI [pb, pe); hw <= 32768 (clamped by the caller: no side is longer)
CBA_HD void laser_window(int p0, int p1, int hw, int pb, int pe, int* lo, int* hi) {
    *lo = p0 - hw > pb ? p0 - hw : pb;
    *hi = p1 + hw < pe - 1 ? p1 + hw : pe - 1;
}

// uint8: floor_level rounded half to even and clamped to [0, 255] (NaN never reaches here: the entry points refuse it)
inline int laser_floor_u8(double floor_level) {
    const double f = std::nearbyint(floor_level);
    return static_cast<int>(f < 0.0 ? 0.0 : (f > 255.0 ? 255.0 : f));
}

// one sample of the window sums.  uint8: g = max(I - floor, 0), exact; float32: fp64, NaN counts as 0, g p is rounded before it is added
CBA_HD void laser_sum_u8(int v, int p, int floor_u8, uint64_t* sg, uint64_t* sgp) {
    const int g = v > floor_u8 ? v - floor_u8 : 0;
    *sg += static_cast<uint64_t>(g);
    *sgp += static_cast<uint64_t>(g) * static_cast<uint64_t>(p);
}
CBA_HD double laser_g_f32(float v, double floor_level) {
    const double d = static_cast<double>(v) - floor_level;
    return v == v && d > 0.0 ? d : 0.0;
}
CBA_HD void laser_sum_f64(double g, int p, double* sg, double* sgp) {
    CBA_NO_CONTRACT
    const double gp = g * static_cast<double>(p);
    *sg += g;
    *sgp += gp;
}

// centre, amplitude and width_px of one line from its peak and window sums.  any: the ROI holds a sample that is not NaN; level: the
// floor the sums were taken against (the rounded one for uint8).  An invalid line (m < min_peak, or sum g == 0) has centre = width = NaN
CBA_HD void laser_finish(bool any, double m, double sg, double sgp, double level, double min_peak, double* centre, double* amplitude,
                         double* width_px) {
    const double nan = NAN;
    *amplitude = any ? m : nan;
    const bool valid = any && !(m < min_peak) && sg != 0.0;
    *centre = valid ? sgp / sg : nan;
    *width_px = valid ? sg / (m - level) : nan;
}

// The pixel (u, v) on the laser plane: r = (x, y, 1) from ls_unproject, den = n.r, s = -d / den, P = s r; den == 0, s <= 0 or a
// non-finite s give NaN (a NaN pixel too: every comparison fails).  No threshold on den: the plane code this continues
// (ls_backproject, ls_plane_from_scatter) divides without one, and s <= 0 already rejects every ray that meets the plane behind the
// camera.  Rt [12] or null: P <- R P + t, each row summed left to right, then + t.  pxy [2] or null: hnormalized(Hp (x, y, 1)), NaN
// where P is.  Nothing here is contracted into FMAs.
CBA_HD void laser_point(const LaserGeom& g, double u, double v, const double* Rt, double* P, double* pxy) {
    CBA_NO_CONTRACT
    double x, y;
    ls_unproject(g.cam, u, v, &x, &y);
    const double den = g.plane[0] * x + g.plane[1] * y + g.plane[2];
    const double s = -g.plane[3] / den;
    const bool ok = den != 0.0 && s > 0.0 && s <= 1.7976931348623157e308;
    const double nan = NAN;
    double P0 = ok ? s * x : nan, P1 = ok ? s * y : nan, P2 = ok ? s : nan;
    if (Rt) {
        const double Q0 = Rt[0] * P0 + Rt[1] * P1 + Rt[2] * P2 + Rt[9];
        const double Q1 = Rt[3] * P0 + Rt[4] * P1 + Rt[5] * P2 + Rt[10];
        const double Q2 = Rt[6] * P0 + Rt[7] * P1 + Rt[8] * P2 + Rt[11];
        P0 = Q0; P1 = Q1; P2 = Q2;
    }
    P[0] = P0; P[1] = P1; P[2] = P2;
    if (pxy) {
        const double h0 = g.Hp[0] * x + g.Hp[1] * y + g.Hp[2];
        const double h1 = g.Hp[3] * x + g.Hp[4] * y + g.Hp[5];
        const double h2 = g.Hp[6] * x + g.Hp[7] * y + g.Hp[8];
        pxy[0] = ok ? h0 / h2 : nan;
        pxy[1] = ok ? h1 / h2 : nan;
    }
}

// One line in one pass, start to end: what every split of the kernels must reproduce (the host build; the kernels do not call it).
// I(p) = base[p * stride].  out = [centre, amplitude, width_px]
template <typename T>
inline void laser_line(const T* base, int64_t stride, int pb, int pe, int hw, double floor_level, double min_peak, double* out) {
    constexpr bool U8 = sizeof(T) == 1;
    using V = typename std::conditional<U8, int, float>::type;
    LaserPeak<V> s;
    laser_peak_init(s);
    for (int p = pb; p < pe; ++p) laser_peak_push(s, static_cast<V>(base[p * stride]), p);
    const bool any = s.p0 >= 0;
    double sg = 0.0, sgp = 0.0, level = floor_level;
    if (any) {
        int lo, hi;
        laser_window(s.p0, s.p1, hw, pb, pe, &lo, &hi);
        if (U8) {
            const int f8 = laser_floor_u8(floor_level);
            uint64_t ig = 0, igp = 0;
            for (int p = lo; p <= hi; ++p) laser_sum_u8(static_cast<int>(base[p * stride]), p, f8, &ig, &igp);
            sg = static_cast<double>(ig);
            sgp = static_cast<double>(igp);
            level = f8;
        } else {
            for (int p = lo; p <= hi; ++p) laser_sum_f64(laser_g_f32(static_cast<float>(base[p * stride]), floor_level), p, &sg, &sgp);
        }
    } else if (U8) {
        level = laser_floor_u8(floor_level);
    }
    laser_finish(any, static_cast<double>(s.m), sg, sgp, level, min_peak, out, out + 1, out + 2);
}

}  // namespace cba
