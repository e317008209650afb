// corner_grid.hpp — grid order of a plain chessboard's corners (calibba.h: cba_chessboard_order).  Host only, fp64.
//
//   neighbours  per corner, the corners of opposite polarity (|wrap_pi(angle difference)| > pi/4) within 1.7 x the distance of the
//               nearest such corner are candidates; slot k = 0..3 takes the nearest candidate whose displacement lies within 35
//               degrees of angle + pi/4 + k pi/2; only mutual links stay
//   labels      breadth-first growth assigns integer (i, j); a corner's frame is a quarter-turn count o: slot k steps by
//               rot^(k + o) (1, 0) with rot (a, b) = (-b, a), and the slot of a neighbour that points back fixes the neighbour's o
//   acceptance  a component of exactly rows cols corners without a label conflict, every cell filled once, extents cols x rows
//               after an optional transpose.  Components are tried from the corner nearest the centroid outwards
//   canonical   of the eight labellings of the lattice (transpose, flip i, flip j) those with extents cols x rows and
//               cross(mean i-step, mean j-step) > 0 (x right, y down) remain; the largest x of the mean i-step wins, then the largest y
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <queue>
#include <vector>

namespace cba {

constexpr double GRID_PI = 3.14159265358979323846;
constexpr double GRID_REACH = 1.7;                       // candidates: within this x the nearest opposite corner
constexpr double GRID_CONE = 35.0 * GRID_PI / 180.0;     // a slot's half-angle

inline double grid_wrap_pi(double d) {  // into (-pi/2, pi/2]
    d = std::fmod(d, GRID_PI);
    if (d > GRID_PI / 2) d -= GRID_PI;
    if (d <= -GRID_PI / 2) d += GRID_PI;
    return d;
}
inline double grid_wrap_2pi(double d) {  // into (-pi, pi]
    d = std::fmod(d, 2 * GRID_PI);
    if (d > GRID_PI) d -= 2 * GRID_PI;
    if (d <= -GRID_PI) d += 2 * GRID_PI;
    return d;
}

// xy [n][2], angle [n] (finite) -> index [rows cols], row-major over (j, i).  Returns 1 when the board was found, else 0 (index
// untouched).  rows, cols >= 2.
inline int chessboard_order(int n, const double* xy, const double* angle, int rows, int cols, int32_t* index) {
    const int need = rows * cols;
    if (n < need) return 0;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<int> nb(4 * static_cast<size_t>(n), -1), link(4 * static_cast<size_t>(n), -1);
    std::vector<double> dist(n);
    for (int c = 0; c < n; ++c) {
        double dmin = inf;
        for (int j = 0; j < n; ++j) {
            dist[j] = inf;
            if (j == c || !(std::fabs(grid_wrap_pi(angle[j] - angle[c])) > GRID_PI / 4)) continue;
            dist[j] = std::hypot(xy[2 * j] - xy[2 * c], xy[2 * j + 1] - xy[2 * c + 1]);
            dmin = std::min(dmin, dist[j]);
        }
        if (!(dmin < inf) || !(dmin > 0.0)) continue;
        for (int k = 0; k < 4; ++k) {
            const double phi = angle[c] + GRID_PI / 4 + k * (GRID_PI / 2);
            double bd = inf;
            for (int j = 0; j < n; ++j) {
                if (!(dist[j] <= GRID_REACH * dmin) || !(dist[j] < bd)) continue;
                const double psi = std::atan2(xy[2 * j + 1] - xy[2 * c + 1], xy[2 * j] - xy[2 * c]);
                if (std::fabs(grid_wrap_2pi(psi - phi)) <= GRID_CONE) {
                    bd = dist[j];
                    nb[4 * c + k] = j;
                }
            }
        }
    }
    for (int c = 0; c < n; ++c)
        for (int k = 0; k < 4; ++k) {
            const int j = nb[4 * c + k];
            if (j < 0) continue;
            for (int kk = 0; kk < 4; ++kk)
                if (nb[4 * j + kk] == c) link[4 * c + k] = j;
        }
    double mx = 0.0, my = 0.0;
    for (int c = 0; c < n; ++c) { mx += xy[2 * c]; my += xy[2 * c + 1]; }
    mx /= n; my /= n;
    std::vector<int> order(n);
    for (int c = 0; c < n; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int p, int q) {
        return std::hypot(xy[2 * p] - mx, xy[2 * p + 1] - my) < std::hypot(xy[2 * q] - mx, xy[2 * q + 1] - my);
    });
    std::vector<char> seen(n, 0);
    std::vector<int> li(n), lj(n), lo(n), comp;
    static const int SI[4] = {1, 0, -1, 0}, SJ[4] = {0, 1, 0, -1};
    for (int start : order) {
        if (seen[start]) continue;
        comp.clear();
        bool ok = true;
        std::queue<int> q;
        seen[start] = 1; li[start] = 0; lj[start] = 0; lo[start] = 0;
        q.push(start);
        while (!q.empty()) {
            const int c = q.front();
            q.pop();
            comp.push_back(c);
            for (int k = 0; k < 4; ++k) {
                const int j = link[4 * c + k];
                if (j < 0) continue;
                int back = -1;
                for (int kk = 0; kk < 4 && back < 0; ++kk)
                    if (link[4 * j + kk] == c) back = kk;
                if (back < 0) { ok = false; continue; }
                const int s = (k + lo[c]) & 3, ni = li[c] + SI[s], nj = lj[c] + SJ[s], no = (k + lo[c] + 2 - back) & 3;
                if (seen[j]) {
                    if (li[j] != ni || lj[j] != nj || lo[j] != no) ok = false;
                    continue;
                }
                seen[j] = 1; li[j] = ni; lj[j] = nj; lo[j] = no;
                q.push(j);
            }
        }
        if (!ok || static_cast<int>(comp.size()) != need) continue;
        int i0 = li[comp[0]], i1 = i0, j0 = lj[comp[0]], j1 = j0;
        for (int c : comp) { i0 = std::min(i0, li[c]); i1 = std::max(i1, li[c]); j0 = std::min(j0, lj[c]); j1 = std::max(j1, lj[c]); }
        const int ni = i1 - i0 + 1, nj = j1 - j0 + 1;
        if (!((ni == cols && nj == rows) || (ni == rows && nj == cols))) continue;
        std::vector<int> cell(need, -1);  // [nj][ni]
        bool once = true;
        for (int c : comp) {
            int& slot = cell[(lj[c] - j0) * ni + li[c] - i0];
            if (slot >= 0) once = false;
            slot = c;
        }
        if (!once) continue;
        bool have = false;
        double bx = 0.0, by = 0.0;
        std::vector<int32_t> G(need), best(need);
        for (int t = 0; t < 8; ++t) {
            const bool tr = t & 1, fi = t & 2, fj = t & 4;
            if ((tr ? nj : ni) != cols || (tr ? ni : nj) != rows) continue;
            for (int j = 0; j < nj; ++j)
                for (int i = 0; i < ni; ++i) {
                    int a = tr ? j : i, b = tr ? i : j;
                    if (fi) a = cols - 1 - a;
                    if (fj) b = rows - 1 - b;
                    G[b * cols + a] = cell[j * ni + i];
                }
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
            if (!have || ix > bx || (ix == bx && iy > by)) {
                have = true; bx = ix; by = iy;
                best = G;
            }
        }
        if (!have) continue;
        std::copy(best.begin(), best.end(), index);
        return 1;
    }
    return 0;
}

}  // namespace cba
