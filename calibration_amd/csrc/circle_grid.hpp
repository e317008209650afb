// circle_grid.hpp — grid order of a symmetric or asymmetric circle grid's blobs (calibba.h: cba_circle_grid_order).  Host only, fp64.
//
//   metric      from blob c, q_c(v) = v^T M_c^-1 v with M_c the blob's ellipse (the board's metric to first order, so foreshortening
//               does not mix neighbours with diagonals); no shapes: the identity
//   links       a blob's candidates are its up to four nearest blobs within 1.2 x the nearest (1.44 x in q); only mutual ones stay
//   labels      breadth-first growth carries a local basis (e1, e2) of actual link vectors; a blob refreshes each axis from its own
//               links, then every link is +-e1 or +-e2 by the larger |cos|, which must exceed cos 30 degrees
//   acceptance  exactly rows cols blobs, no label conflict, and under one of the lattice's eight symmetries the occupied cells equal
//               the pattern's (asymmetric: (p, q) -> (p - q, p + q) first) with cross(mean i-step, mean j-step) > 0; one such
//               labelling: unique; several: the chessboard's rule (mean i-step most to +x, then +y)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <queue>
#include <vector>

namespace cba {

constexpr int CIRCLES_SYMMETRIC = 0, CIRCLES_ASYMMETRIC = 1;
constexpr double CIRCLE_REACH2 = 1.44;                   // (1.2)^2: candidates lie within 1.2 x the nearest blob
constexpr double CIRCLE_COS = 0.86602540378443864676;    // cos 30 degrees

// xy [n][2], shape [n][3] or null -> index [rows cols], row-major over (j, i), and *unique.  Returns 1 when the grid was found, else 0
// (index untouched).  rows, cols >= 2; shapes positive definite.
inline int circle_grid_order(int n, const double* xy, const double* shape, int pattern, int rows, int cols, int32_t* index, int* unique) {
    const int need = rows * cols;
    *unique = 0;
    if (n < need) return 0;
    // inverse metric per blob: (a, b, c) with q(v) = a vx^2 + 2 b vx vy + c vy^2
    std::vector<double> im(3 * static_cast<size_t>(n));
    for (int c = 0; c < n; ++c) {
        double mxx = 1.0, mxy = 0.0, myy = 1.0;
        if (shape) { mxx = shape[3 * c]; mxy = shape[3 * c + 1]; myy = shape[3 * c + 2]; }
        const double det = mxx * myy - mxy * mxy;
        im[3 * c] = myy / det;
        im[3 * c + 1] = -mxy / det;
        im[3 * c + 2] = mxx / det;
    }
    auto dot = [&](int c, double vx, double vy, double wx, double wy) {
        return im[3 * c] * vx * wx + im[3 * c + 1] * (vx * wy + vy * wx) + im[3 * c + 2] * vy * wy;
    };
    auto cosine = [&](int c, double vx, double vy, double wx, double wy) {
        return dot(c, vx, vy, wx, wy) / std::sqrt(dot(c, vx, vy, vx, vy) * dot(c, wx, wy, wx, wy));
    };
    std::vector<int> cand(4 * static_cast<size_t>(n), -1), link(4 * static_cast<size_t>(n), -1), ord(n);
    std::vector<double> q(n);
    for (int c = 0; c < n; ++c) {
        int m = 0;
        for (int j = 0; j < n; ++j) {
            if (j == c) continue;
            const double vx = xy[2 * j] - xy[2 * c], vy = xy[2 * j + 1] - xy[2 * c + 1];
            q[j] = dot(c, vx, vy, vx, vy);
            ord[m++] = j;
        }
        std::stable_sort(ord.begin(), ord.begin() + m, [&](int s, int t) { return q[s] < q[t]; });
        if (m == 0 || !(q[ord[0]] > 0.0)) continue;
        for (int k = 0; k < 4 && k < m; ++k)
            if (q[ord[k]] <= CIRCLE_REACH2 * q[ord[0]]) cand[4 * c + k] = ord[k];
    }
    for (int c = 0; c < n; ++c) {
        int m = 0;
        for (int k = 0; k < 4; ++k) {
            const int j = cand[4 * c + k];
            if (j < 0) continue;
            for (int kk = 0; kk < 4; ++kk)
                if (cand[4 * j + kk] == c) { link[4 * c + m++] = j; break; }
        }
    }
    double mx = 0.0, my = 0.0;
    for (int c = 0; c < n; ++c) { mx += xy[2 * c]; my += xy[2 * c + 1]; }
    mx /= n; my /= n;
    std::vector<int> order(n);
    for (int c = 0; c < n; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int s, int t) {
        return std::hypot(xy[2 * s] - mx, xy[2 * s + 1] - my) < std::hypot(xy[2 * t] - mx, xy[2 * t + 1] - my);
    });
    std::vector<char> seen(n, 0);
    std::vector<int> lp(n), lq(n), comp;
    std::vector<double> basis(4 * static_cast<size_t>(n));  // e1x e1y e2x e2y
    for (int start : order) {
        if (seen[start]) continue;
        comp.clear();
        bool ok = true;
        std::queue<int> todo;
        seen[start] = 1; lp[start] = 0; lq[start] = 0;
        {
            double* e = &basis[4 * start];
            e[0] = e[1] = e[2] = e[3] = 0.0;
            const int j0 = link[4 * start];
            if (j0 >= 0) {
                e[0] = xy[2 * j0] - xy[2 * start]; e[1] = xy[2 * j0 + 1] - xy[2 * start + 1];
                double best = 2.0;
                for (int k = 1; k < 4; ++k) {
                    const int j = link[4 * start + k];
                    if (j < 0) continue;
                    const double wx = xy[2 * j] - xy[2 * start], wy = xy[2 * j + 1] - xy[2 * start + 1];
                    const double cs = std::fabs(cosine(start, e[0], e[1], wx, wy));
                    if (cs < best) { best = cs; e[2] = wx; e[3] = wy; }
                }
                if (!(best < 2.0)) ok = false;
            }
        }
        todo.push(start);
        while (!todo.empty()) {
            const int c = todo.front();
            todo.pop();
            comp.push_back(c);
            if (!ok) continue;  // still mark the whole component as seen
            double* e = &basis[4 * c];
            const double carried[4] = {e[0], e[1], e[2], e[3]};
            for (int ax = 0; ax < 2; ++ax) {  // refresh each axis from the blob's own links
                double best = CIRCLE_COS;
                for (int k = 0; k < 4; ++k) {
                    const int j = link[4 * c + k];
                    if (j < 0) continue;
                    const double wx = xy[2 * j] - xy[2 * c], wy = xy[2 * j + 1] - xy[2 * c + 1];
                    const double cs = cosine(c, carried[2 * ax], carried[2 * ax + 1], wx, wy);
                    if (std::fabs(cs) > best) {
                        best = std::fabs(cs);
                        e[2 * ax] = cs > 0.0 ? wx : -wx;
                        e[2 * ax + 1] = cs > 0.0 ? wy : -wy;
                    }
                }
            }
            for (int k = 0; k < 4; ++k) {
                const int j = link[4 * c + k];
                if (j < 0) continue;
                const double wx = xy[2 * j] - xy[2 * c], wy = xy[2 * j + 1] - xy[2 * c + 1];
                const double c1 = cosine(c, e[0], e[1], wx, wy), c2 = cosine(c, e[2], e[3], wx, wy);
                const bool first = std::fabs(c1) >= std::fabs(c2);
                const double cs = first ? c1 : c2;
                if (!(std::fabs(cs) > CIRCLE_COS)) { ok = false; continue; }
                const int sgn = cs > 0.0 ? 1 : -1;
                const int np = lp[c] + (first ? sgn : 0), nq = lq[c] + (first ? 0 : sgn);
                if (seen[j]) {
                    // a blob of another, earlier component cannot be linked to this one: links are symmetric, so it is of this one
                    if (lp[j] != np || lq[j] != nq) ok = false;
                    continue;
                }
                seen[j] = 1; lp[j] = np; lq[j] = nq;
                std::copy(e, e + 4, &basis[4 * j]);
                todo.push(j);
            }
        }
        if (!ok || static_cast<int>(comp.size()) != need) continue;
        int fits = 0;
        bool have = false;
        double bx = 0.0, by = 0.0;
        std::vector<int32_t> G(need), best(need);
        std::vector<int> u(need), v(need);
        for (int t = 0; t < 8; ++t) {
            const bool tr = t & 1, fp = t & 2, fq = t & 4;
            int u0 = 0, v0 = 0;
            for (int m = 0; m < need; ++m) {
                int p = lp[comp[m]], qq = lq[comp[m]];
                if (tr) std::swap(p, qq);
                if (fp) p = -p;
                if (fq) qq = -qq;
                u[m] = pattern == CIRCLES_ASYMMETRIC ? p - qq : p;
                v[m] = pattern == CIRCLES_ASYMMETRIC ? p + qq : qq;
                u0 = m ? std::min(u0, u[m]) : u[m];
                v0 = m ? std::min(v0, v[m]) : v[m];
            }
            std::fill(G.begin(), G.end(), -1);
            bool fit = true;
            for (int m = 0; m < need && fit; ++m) {
                const int uu = u[m] - u0, j = v[m] - v0;
                int i = uu;
                if (pattern == CIRCLES_ASYMMETRIC) {
                    if ((uu - (j & 1)) & 1) { fit = false; break; }
                    i = (uu - (j & 1)) / 2;
                }
                if (i < 0 || i >= cols || j < 0 || j >= rows || G[j * cols + i] >= 0) { fit = false; break; }
                G[j * cols + i] = comp[m];
            }
            if (!fit) continue;  // need blobs in need distinct cells: every cell is filled
            double ix = 0.0, iy = 0.0, jx = 0.0, jy = 0.0;
            for (int b = 0; b < rows; ++b)
                for (int a = 0; a + 1 < cols; ++a) {
                    ix += xy[2 * G[b * cols + a + 1]] - xy[2 * G[b * cols + a]];
                    iy += xy[2 * G[b * cols + a + 1] + 1] - xy[2 * G[b * cols + a] + 1];
                }
            for (int b = 0; b + 1 < rows; ++b)
                for (int a = 0; a < cols; ++a) {
                    jx += xy[2 * G[(b + 1) * cols + a]] - xy[2 * G[b * cols + a]];
                    jy += xy[2 * G[(b + 1) * cols + a] + 1] - xy[2 * G[b * cols + a] + 1];
                }
            ix /= rows * (cols - 1); iy /= rows * (cols - 1);
            jx /= (rows - 1) * cols; jy /= (rows - 1) * cols;
            if (!(ix * jy - iy * jx > 0.0)) continue;
            ++fits;
            if (!have || ix > bx || (ix == bx && iy > by)) {
                have = true; bx = ix; by = iy;
                best = G;
            }
        }
        if (!have) continue;
        std::copy(best.begin(), best.end(), index);
        *unique = fits == 1 ? 1 : 0;
        return 1;
    }
    return 0;
}

}  // namespace cba
