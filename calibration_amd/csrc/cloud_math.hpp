// cloud_math.hpp — the one copy of the scan-registration rule (calibba.h: cba_point_normals, cba_cloud_index, cba_cloud_nearest,
// cba_cloud_register, cba_cloud_align), for the device (cloud_register.hip) and the tests' host builds (tests/cloud_cpu, tests/align_cpu):
//   cloud_plan_grid      box, cell counts and extent of a target cloud (host: the handle's create and its argument check)
//   cloud_cell           the cell of a coordinate: one subtraction, one division, floor
//   cloud_nearest_point  the 3 x 3 x 3 neighbourhood as 9 runs of the sorted records; distance and tie rule
//   cloud_normal         the normal of a pixel from its 5-point cross
//   icp_rotation, icp_transform, icp_add_plane, icp_add_point   the rows of a pair, added to the 29 sums
//   icp_add_source_point, icp_add_match   the point rule: what one source point adds to a system against a CloudTarget
//   icp_cholesky6, icp_update, icp_advance                      the solve, the pose update, one step of the iteration
//   align_relative, align_adjoint, align_edge_blocks, align_assemble_entry, align_cholesky, align_begin / align_update / align_advance
//                        cba_cloud_align: an edge's relative pose, Ad(T_b^-1), its blocks M and c, their place in the system of all
//                        scans, the width-n solve, the stop tests and updates
// Every product and sum is rounded on its own: the file is compiled without contraction into FMAs, and an including translation
// unit is too from here on (cloud_register.hip and the tests' drivers include nothing after it that wants them).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/calibba.h"
#include "reproj_math.hpp"  // CBA_HD

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace cba {

constexpr int ICP_SUMS = 29;   // 21 of H (upper triangle by rows), 6 of g, ss, n_pairs
constexpr int ICP_ROW = 32;    // a slab row: the sums padded to wave_transpose_sum's multiple of 16
constexpr int ICP_SS = 27, ICP_NP = 28;

struct CloudGrid {
    double lo[3], hi[3];  // exact minima and maxima of the valid points
    double cell;
    int32_t n[3];         // cells per axis: floor((hi - lo) / cell) + 1
};

// a target point in cell order: two 16-byte loads per candidate
struct alignas(32) CloudRec {
    double x, y, z;
    int64_t idx;  // the point's index in the caller's array
};

// a target of the search and of ICP
struct CloudTarget {
    CloudGrid g;
    const int32_t* start;      // [n_cells + 1]: the first record of each cell
    const CloudRec* rec;       // the valid points in cell order
    const double* rec_normal;  // [][3]: their normals in the same order; NULL: the target has none
};

CBA_HD bool cloud_valid(double x, double y, double z) { return std::isfinite(x) && std::isfinite(y) && std::isfinite(z); }

// floor((p - lo) / cell) as an int; the callers keep the quotient inside [-2, 2^24 + 1]
CBA_HD int32_t cloud_cell(double p, double lo, double cell) { return static_cast<int32_t>(std::floor((p - lo) / cell)); }

// the cell index of a valid target point, x fastest
CBA_HD int32_t cloud_point_cell(const CloudGrid& g, double x, double y, double z) {
    const int32_t cx = std::min(g.n[0] - 1, cloud_cell(x, g.lo[0], g.cell));
    const int32_t cy = std::min(g.n[1] - 1, cloud_cell(y, g.lo[1], g.cell));
    const int32_t cz = std::min(g.n[2] - 1, cloud_cell(z, g.lo[2], g.cell));
    return (cz * g.n[1] + cy) * g.n[0] + cx;
}

// Host: the grid of xyz [n][3].  -> 0, or 1: no valid point, 2: more than CBA_CLOUD_MAX_CELLS cells; *fit is then a cell size that fits
// (the largest box side over 2^8 - 1 cells per axis, which is at most 2^24 cells in all).
inline int cloud_plan_grid(int64_t n, const double* xyz, double cell, CloudGrid* g, double* extent, int64_t* n_cells, double* fit) {
    bool any = false;
    for (int64_t i = 0; i < n; ++i) {
        const double* p = xyz + 3 * i;
        if (!cloud_valid(p[0], p[1], p[2])) continue;
        for (int k = 0; k < 3; ++k) {
            g->lo[k] = any ? std::min(g->lo[k], p[k]) : p[k];
            g->hi[k] = any ? std::max(g->hi[k], p[k]) : p[k];
        }
        any = true;
    }
    if (!any) return 1;
    g->cell = cell;
    double cells = 1.0, side = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double nk = std::floor((g->hi[k] - g->lo[k]) / cell) + 1.0;
        cells *= nk;
        side = std::max(side, g->hi[k] - g->lo[k]);
        g->n[k] = nk <= static_cast<double>(CBA_CLOUD_MAX_CELLS) ? static_cast<int32_t>(nk) : 0;
    }
    if (!(cells <= static_cast<double>(CBA_CLOUD_MAX_CELLS))) {
        *fit = side / 255.0;
        return 2;
    }
    *n_cells = static_cast<int64_t>(g->n[0]) * g->n[1] * g->n[2];
    const double ex = g->hi[0] - g->lo[0], ey = g->hi[1] - g->lo[1], ez = g->hi[2] - g->lo[2];
    *extent = std::sqrt((ex * ex + ey * ey) + ez * ez);
    return 0;
}

// The nearest target point of q within max_distance (md, md2 = md md), by brute force's rule over the 27 cells around q's cell:
// d2 = ((dx dx + dy dy) + dz dz) with dx = q_x - y_x, the smallest d2 <= md2, equal d2 to the lowest original index.  start
// [n_cells + 1]: the first record of each cell.  -> the original index or -1; *pos: the record's place in the sorted arrays; *d2: NaN
// when there is none.
CBA_HD int64_t cloud_nearest_point(const CloudGrid& g, const int32_t* __restrict__ start, const CloudRec* __restrict__ rec, double qx,
                                   double qy, double qz, double md, double md2, int32_t* pos, double* d2) {
    int64_t best = -1;
    double bd = std::numeric_limits<double>::quiet_NaN();
    *pos = -1;
    *d2 = bd;
    if (!cloud_valid(qx, qy, qz)) return -1;
    // further than md outside the box on an axis (by the rounded difference, as brute force would form it): nothing can qualify,
    // and the quotients below stay inside [-1, n_k]
    if (g.lo[0] - qx > md || qx - g.hi[0] > md || g.lo[1] - qy > md || qy - g.hi[1] > md || g.lo[2] - qz > md || qz - g.hi[2] > md) return -1;
    const int32_t cx = cloud_cell(qx, g.lo[0], g.cell), cy = cloud_cell(qy, g.lo[1], g.cell), cz = cloud_cell(qz, g.lo[2], g.cell);
    const int32_t x0 = std::max(cx - 1, 0), x1 = std::min(cx + 1, g.n[0] - 1);
    const int32_t y0 = std::max(cy - 1, 0), y1 = std::min(cy + 1, g.n[1] - 1);
    const int32_t z0 = std::max(cz - 1, 0), z1 = std::min(cz + 1, g.n[2] - 1);
    if (x0 > x1) return -1;
    for (int32_t z = z0; z <= z1; ++z)
        for (int32_t y = y0; y <= y1; ++y) {
            const int32_t row = (z * g.n[1] + y) * g.n[0];
            const int32_t b = start[row + x0], e = start[row + x1 + 1];  // the cells x0..x1 are one run
            for (int32_t k = b; k < e; ++k) {
                const CloudRec r = rec[k];
                const double dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
                const double d = (dx * dx + dy * dy) + dz * dz;
                if (d <= md2 && (best < 0 || d < bd || (d == bd && r.idx < best))) {
                    best = r.idx;
                    bd = d;
                    *pos = k;
                }
            }
        }
    *d2 = bd;
    return best;
}

// ---- normals ----------------------------------------------------------------------------------------------------------------------
// whether the neighbour N of the valid centre P can serve: valid and within max_jump (mj2 = max_jump max_jump)
CBA_HD bool cloud_near(const double* N, const double* P, double mj2) {
    if (!cloud_valid(N[0], N[1], N[2])) return false;
    const double ex = N[0] - P[0], ey = N[1] - P[1], ez = N[2] - P[2];
    return (ex * ex + ey * ey) + ez * ez <= mj2;
}

// the difference along one image axis: A the neighbour after P (right, below), B the one before (left, above); in_a, in_b: inside the map
CBA_HD bool cloud_axis_diff(const double* P, const double* A, bool in_a, const double* B, bool in_b, double mj2, double* d) {
    const bool a = in_a && cloud_near(A, P, mj2), b = in_b && cloud_near(B, P, mj2);
    if (!a && !b) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (a ? A[k] : P[k]) - (b ? B[k] : P[k]);
    return true;
}

// the normal of P from its cross (R right, L left, D the row below, U the row above; in: bit 0 R, 1 L, 2 D, 3 U is inside the map, the
// others are not read); vp: the viewpoint
CBA_HD void cloud_normal(const double* P, const double* R, const double* L, const double* D, const double* U, int in, const double* vp,
                         double mj2, double* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out[0] = nan; out[1] = nan; out[2] = nan;
    if (!cloud_valid(P[0], P[1], P[2])) return;
    double dx[3], dy[3];
    if (!cloud_axis_diff(P, R, (in & 1) != 0, L, (in & 2) != 0, mj2, dx) || !cloud_axis_diff(P, D, (in & 4) != 0, U, (in & 8) != 0, mj2, dy)) return;
    double nx = dx[1] * dy[2] - dx[2] * dy[1];
    double ny = dx[2] * dy[0] - dx[0] * dy[2];
    double nz = dx[0] * dy[1] - dx[1] * dy[0];
    const double len = std::sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.0) || !std::isfinite(len)) return;
    nx /= len; ny /= len; nz /= len;
    const double vx = vp[0] - P[0], vy = vp[1] - P[1], vz = vp[2] - P[2];
    if ((nx * vx + ny * vy) + nz * vz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    out[0] = nx; out[1] = ny; out[2] = nz;
}

// ---- the rows of a pair ---------------------------------------------------------------------------------------------------------
// R [9] (row-major) of the unit quaternion q = [w x y z]
CBA_HD void icp_rotation(const double* q, double* R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);       R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = 1.0 - 2.0 * (xx + yy);
}

// Q = R p + t: each row summed left to right, then + t
CBA_HD void icp_transform(const double* R, const double* t, const double* p, double* Q) {
    Q[0] = ((R[0] * p[0] + R[1] * p[1]) + R[2] * p[2]) + t[0];
    Q[1] = ((R[3] * p[0] + R[4] * p[1]) + R[5] * p[2]) + t[1];
    Q[2] = ((R[6] * p[0] + R[7] * p[1]) + R[8] * p[2]) + t[2];
}

// one row J [6], r into the sums: acc[0..21) H's upper triangle by rows, acc[21..27) g, acc[27] ss
CBA_HD void icp_add_row(const double* J, double r, double* acc) {
    int e = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int l = k; l < 6; ++l) acc[e++] += J[k] * J[l];
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[21 + k] += J[k] * r;
    acc[ICP_SS] += r * r;
}

// point-to-plane: r = n . (Q - y), J = [(Q x n)^T, n^T]
CBA_HD void icp_add_plane(const double* Q, const double* y, const double* n, double* acc) {
    const double e0 = Q[0] - y[0], e1 = Q[1] - y[1], e2 = Q[2] - y[2];
    const double r = (n[0] * e0 + n[1] * e1) + n[2] * e2;
    const double J[6] = {Q[1] * n[2] - Q[2] * n[1], Q[2] * n[0] - Q[0] * n[2], Q[0] * n[1] - Q[1] * n[0], n[0], n[1], n[2]};
    icp_add_row(J, r, acc);
    acc[ICP_NP] += 1.0;
}

// point-to-point: the three rows r = Q - y, J = [-[Q]x, I], x then y then z
CBA_HD void icp_add_point(const double* Q, const double* y, double* acc) {
    const double Jx[6] = {0.0, Q[2], -Q[1], 1.0, 0.0, 0.0};
    const double Jy[6] = {-Q[2], 0.0, Q[0], 0.0, 1.0, 0.0};
    const double Jz[6] = {Q[1], -Q[0], 0.0, 0.0, 0.0, 1.0};
    icp_add_row(Jx, Q[0] - y[0], acc);
    icp_add_row(Jy, Q[1] - y[1], acc);
    icp_add_row(Jz, Q[2] - y[2], acc);
    acc[ICP_NP] += 1.0;
}

// the pair of Q and the target record at pos into the sums; METRIC 0: point-to-plane, nothing without a normal (NaN); 1: point-to-point
template <int METRIC>
CBA_HD void icp_add_match(const double* Q, const CloudRec* __restrict__ rec, const double* __restrict__ rec_normal, int32_t pos, double* acc) {
    const CloudRec r = rec[pos];
    const double y[3] = {r.x, r.y, r.z};
    if (METRIC == 0) {
        const double* np = rec_normal + 3 * static_cast<int64_t>(pos);
        const double n[3] = {np[0], np[1], np[2]};
        if (n[0] != n[0]) return;
        icp_add_plane(Q, y, n, acc);
    } else {
        icp_add_point(Q, y, acc);
    }
}

// The point rule: the source point p [3] at the pose (R, t) against target (md, md2 = md md: max_distance) into the sums.  An invalid
// point, one without a target point within md and, for METRIC 0, one whose match has no normal add nothing.
template <int METRIC>
CBA_HD void icp_add_source_point(const CloudTarget& target, const double* R, const double* t, const double* p, double md, double md2, double* acc) {
    if (!cloud_valid(p[0], p[1], p[2])) return;
    double Q[3], d2;
    int32_t pos;
    icp_transform(R, t, p, Q);
    if (cloud_nearest_point(target.g, target.start, target.rec, Q[0], Q[1], Q[2], md, md2, &pos, &d2) < 0) return;
    icp_add_match<METRIC>(Q, target.rec, target.rec_normal, pos, acc);
}

// ---- the step ---------------------------------------------------------------------------------------------------------------------
// H [36] from the 21 sums
CBA_HD void icp_mirror(const double* acc, double* H) {
    int e = 0;
    for (int k = 0; k < 6; ++k)
        for (int l = k; l < 6; ++l) {
            H[6 * k + l] = acc[e];
            H[6 * l + k] = acc[e++];
        }
}

// H xi = -g by unpivoted Cholesky; false when a squared diagonal entry of L is <= 1e-12 H_kk (or not a number)
CBA_HD bool icp_cholesky6(const double* H, const double* g, double* xi) {
    double L[36];
    for (int k = 0; k < 6; ++k) {
        double d = H[6 * k + k];
        for (int j = 0; j < k; ++j) d -= L[6 * k + j] * L[6 * k + j];
        if (!(d > 1e-12 * H[6 * k + k])) return false;
        const double lkk = std::sqrt(d);
        L[6 * k + k] = lkk;
        for (int i = k + 1; i < 6; ++i) {
            double s = H[6 * i + k];
            for (int j = 0; j < k; ++j) s -= L[6 * i + j] * L[6 * k + j];
            L[6 * i + k] = s / lkk;
        }
    }
    double z[6];
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
        for (int j = 0; j < i; ++j) s -= L[6 * i + j] * z[j];
        z[i] = s / L[6 * i + i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = z[i];
        for (int j = i + 1; j < 6; ++j) s -= L[6 * j + i] * xi[j];
        xi[i] = s / L[6 * i + i];
    }
    return true;
}

// q / |q| with |q| = sqrt(((w w + x x) + y y) + z z); false: zero or non-finite
CBA_HD bool icp_normalise(double* q) {
    const double n = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(n > 0.0) || !std::isfinite(n)) return false;
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
    return true;
}

// pose7 <- the update by xi = (omega, v); *w = |omega|, *vn = |v|
CBA_HD void icp_update(double* pose, const double* xi, double* w, double* vn) {
    const double th = std::sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
    double d[4] = {1.0, 0.0, 0.0, 0.0};
    if (th != 0.0) {
        const double s = std::sin(0.5 * th) / th;
        d[0] = std::cos(0.5 * th);
        d[1] = s * xi[0]; d[2] = s * xi[1]; d[3] = s * xi[2];
    }
    const double* q = pose;
    double p[4];
    p[0] = ((d[0] * q[0] - d[1] * q[1]) - d[2] * q[2]) - d[3] * q[3];
    p[1] = ((d[0] * q[1] + d[1] * q[0]) + d[2] * q[3]) - d[3] * q[2];
    p[2] = ((d[0] * q[2] - d[1] * q[3]) + d[2] * q[0]) + d[3] * q[1];
    p[3] = ((d[0] * q[3] + d[1] * q[2]) - d[2] * q[1]) + d[3] * q[0];
    icp_normalise(p);
    double Rd[9], t[3];
    icp_rotation(d, Rd);
    icp_transform(Rd, xi + 3, pose + 4, t);
    pose[0] = p[0]; pose[1] = p[1]; pose[2] = p[2]; pose[3] = p[3];
    pose[4] = t[0]; pose[5] = t[1]; pose[6] = t[2];
    *w = th;
    *vn = std::sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
}

// what the iteration carries from one evaluation to the next, beside the result's pose, iterations and status
enum : int32_t { ICP_RUN = 0, ICP_LAST = 1, ICP_DONE = 2 };

// One step on the sums of the system at res->pose7 (acc [ICP_SUMS]): the statistics into *res, then by *phase: ICP_LAST: this was
// the evaluation after the last update, the status stands; ICP_RUN: the tests and the update of the rule.  min_pairs: the effective
// bar.
CBA_HD void icp_advance(const double* acc, const cba_icp_options& o, int32_t min_pairs, double extent, cba_icp_result* res, int32_t* phase) {
    icp_mirror(acc, res->H);
    for (int k = 0; k < 6; ++k) res->g[k] = acc[21 + k];
    res->n_pairs = static_cast<int64_t>(acc[ICP_NP]);
    res->rms = res->n_pairs > 0 ? std::sqrt(acc[ICP_SS] / acc[ICP_NP]) : std::numeric_limits<double>::quiet_NaN();
    if (*phase == ICP_LAST) { *phase = ICP_DONE; return; }
    *phase = ICP_DONE;
    if (res->n_pairs < min_pairs) { res->status = CBA_ICP_TOO_FEW; return; }
    if (res->iterations >= o.max_iterations) { res->status = CBA_ICP_NOT_CONVERGED; return; }
    double xi[6];
    if (!icp_cholesky6(res->H, res->g, xi)) { res->status = CBA_ICP_DEGENERATE; return; }
    double w, vn;
    icp_update(res->pose7, xi, &w, &vn);
    res->iterations += 1;
    *phase = ICP_RUN;
    if (w <= o.step_tolerance && vn <= o.step_tolerance * extent) {
        res->status = CBA_ICP_OK;
        *phase = ICP_LAST;
    } else if (res->iterations >= o.max_iterations) {
        res->status = CBA_ICP_NOT_CONVERGED;
        *phase = ICP_LAST;
    }
}

CBA_HD int32_t icp_min_pairs(const cba_icp_options& o) { return std::max(o.min_pairs, o.metric == 0 ? 6 : 3); }

// ---- alignment of many scans (calibba.h: cba_cloud_align) ---------------------------------------------------------------------------
constexpr int ALIGN_EDGE = 42;  // an edge's assembled blocks: M [36] row-major, then c [6]

// The pose of scan a in the frame of scan b, T_b^-1 T_a: Rab [9] and tab [3] from the rotations Ra, Rb [9] and translations ta, tb.
// With T_b the identity they are Ra and ta (up to the sign of a zero).
CBA_HD void align_relative(const double* Ra, const double* ta, const double* Rb, const double* tb, double* Rab, double* tab) {
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) Rab[3 * i + k] = (Rb[i] * Ra[k] + Rb[3 + i] * Ra[3 + k]) + Rb[6 + i] * Ra[6 + k];
    const double d[3] = {ta[0] - tb[0], ta[1] - tb[1], ta[2] - tb[2]};
    for (int i = 0; i < 3; ++i) tab[i] = (Rb[i] * d[0] + Rb[3 + i] * d[1]) + Rb[6 + i] * d[2];
}

// A [36] = Ad(T_b^-1) on (omega, v): [[R^T, 0], [-R^T [t]x, R^T]] of the pose (R [9], t [3]) of scan b
CBA_HD void align_adjoint(const double* R, const double* t, double* A) {
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) {
            A[6 * i + k] = R[3 * k + i];
            A[6 * i + 3 + k] = 0.0;
            A[6 * (3 + i) + 3 + k] = R[3 * k + i];
        }
        A[6 * (3 + i)] = R[6 + i] * t[1] - R[3 + i] * t[2];
        A[6 * (3 + i) + 1] = R[i] * t[2] - R[6 + i] * t[0];
        A[6 * (3 + i) + 2] = R[3 + i] * t[0] - R[i] * t[1];
    }
}

// entry (i, j) of M = A^T (H A): B_kj = sum_l H_kl A_lj, M_ij = sum_k A_ki B_kj, every sum left to right from its first product
CBA_HD double align_block_entry(const double* H, const double* A, int i, int j) {
    double m = 0.0;
    for (int k = 0; k < 6; ++k) {
        double b = H[6 * k] * A[j];
        for (int l = 1; l < 6; ++l) b = b + H[6 * k + l] * A[6 * l + j];
        const double p = A[6 * k + i] * b;
        m = k == 0 ? p : m + p;
    }
    return m;
}

// entry i of c = A^T g
CBA_HD double align_block_gradient(const double* g, const double* A, int i) {
    double c = A[i] * g[0];
    for (int k = 1; k < 6; ++k) c = c + A[6 * k + i] * g[k];
    return c;
}

// out [ALIGN_EDGE]: M and c of an edge's H [36], g [6] under A [36]; A = I gives H and g back
CBA_HD void align_edge_blocks(const double* H, const double* g, const double* A, double* out) {
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) out[6 * i + j] = align_block_entry(H, A, i, j);
        out[36 + i] = align_block_gradient(g, A, i);
    }
}

// What scan p (row block rp of the reduced system; -1: the fixed scan) receives from the used edge (a, b) with blocks mc
// [ALIGN_EDGE], for the entry r of its row: r < 36: entry (i, j) = (r / 6, r % 6) of the blocks of row rp of H [n][n]; r >= 36:
// entry r - 36 of its part of g.  ra, rb: the row blocks of a and b.  Called for the edges in list order, so every entry gets its
// contributions in that order: +M on (a, a) and (b, b), -M on (a, b), -M^T on (b, a), +c on g_a, -c on g_b.
CBA_HD void align_assemble_entry(int n, double* H, double* g, int rp, int r, int ra, int rb, const double* mc) {
    if (rp < 0 || (ra != rp && rb != rp)) return;
    if (r >= 36) {
        const int i = r - 36;
        if (ra == rp) g[6 * rp + i] += mc[36 + i];
        if (rb == rp) g[6 * rp + i] -= mc[36 + i];
        return;
    }
    const int i = r / 6, j = r - 6 * i;
    double* row = H + static_cast<int64_t>(6 * rp + i) * n;
    if (ra == rp) {
        row[6 * rp + j] += mc[r];
        if (rb >= 0) row[6 * rb + j] -= mc[r];
    }
    if (rb == rp) {
        row[6 * rp + j] += mc[r];
        if (ra >= 0) row[6 * ra + j] -= mc[6 * j + i];
    }
}

// The width-n Cholesky in place in the lower triangle of H [n][n], icp_cholesky6's sequence: the entry (i, k), i >= k, before its
// division: H_ik - sum_j<k L_ij L_kj, j from 0 (columns 0 .. k-1 are done)
CBA_HD double align_cholesky_entry(int n, const double* H, int i, int k) {
    const double* ri = H + static_cast<int64_t>(i) * n;
    const double* rk = H + static_cast<int64_t>(k) * n;
    double s = ri[k];
    for (int j = 0; j < k; ++j) s -= ri[j] * rk[j];
    return s;
}

// the test of a squared diagonal entry d against the system's own H_kk
CBA_HD bool align_pivot_ok(double d, double hkk) { return d > 1e-12 * hkk; }

// H xi = -g at width n: H is overwritten by L (lower triangle), z [n] is work.  false: a pivot failed (xi is then not meaningful; the
// loops run to their ends all the same, as the device's do)
CBA_HD bool align_cholesky(int n, double* H, const double* g, double* z, double* xi) {
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        const double d = align_cholesky_entry(n, H, k, k);
        ok = ok && align_pivot_ok(d, H[static_cast<int64_t>(k) * n + k]);
        const double lkk = std::sqrt(d);
        for (int i = k + 1; i < n; ++i) H[static_cast<int64_t>(i) * n + k] = align_cholesky_entry(n, H, i, k) / lkk;
        H[static_cast<int64_t>(k) * n + k] = lkk;
    }
    for (int i = 0; i < n; ++i) {
        double s = -g[i];
        for (int j = 0; j < i; ++j) s -= H[static_cast<int64_t>(i) * n + j] * z[j];
        z[i] = s / H[static_cast<int64_t>(i) * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = z[i];
        for (int j = i + 1; j < n; ++j) s -= H[static_cast<int64_t>(j) * n + i] * xi[j];
        xi[i] = s / H[static_cast<int64_t>(i) * n + i];
    }
    return ok;
}

// what the iteration carries between the rounds, beside the poses
struct AlignState {
    cba_align_result res;
    int32_t phase;  // ICP_RUN, ICP_LAST, ICP_DONE
};

// The tests before the solve, on the totals of the used edges (already in st->res).  -> true: solve and update; false: the call
// has ended (st->phase is ICP_DONE) with its status set, or this was the evaluation after the last update (the status stands).
CBA_HD bool align_begin(const cba_icp_options& o, AlignState* st) {
    const int32_t was = st->phase;
    st->phase = ICP_DONE;
    if (was == ICP_LAST) return false;
    if (st->res.n_used_edges == 0) { st->res.status = CBA_ICP_TOO_FEW; return false; }
    if (st->res.iterations >= o.max_iterations) { st->res.status = CBA_ICP_NOT_CONVERGED; return false; }
    return true;
}

// The update of one scan by its xi [6]; -> whether its step is inside the tolerance
CBA_HD bool align_update(double* pose7, const double* xi, const cba_icp_options& o, double extent) {
    double w, vn;
    icp_update(pose7, xi, &w, &vn);
    return w <= o.step_tolerance && vn <= o.step_tolerance * extent;
}

// After the solve (solved: no pivot failed; on a failure no pose was touched) and the updates (all_small: every scan's step was
// inside the tolerance): iterations, status and phase as icp_advance sets them for one source.
CBA_HD void align_advance(bool solved, bool all_small, const cba_icp_options& o, AlignState* st) {
    if (!solved) { st->res.status = CBA_ICP_DEGENERATE; st->phase = ICP_DONE; return; }
    st->res.iterations += 1;
    st->phase = ICP_RUN;
    if (all_small) {
        st->res.status = CBA_ICP_OK;
        st->phase = ICP_LAST;
    } else if (st->res.iterations >= o.max_iterations) {
        st->res.status = CBA_ICP_NOT_CONVERGED;
        st->phase = ICP_LAST;
    }
}

}  // namespace cba
