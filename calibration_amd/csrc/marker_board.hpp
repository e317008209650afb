// marker_board.hpp — the host stages of ChArUco detection (calibba.h: cba_marker_dictionary_generate, cba_chessboard_lattice,
// cba_charuco_match).  Host only, fp64.
//
//   dictionary  greedy over splitmix64 candidates: a code is kept when it is min_distance from its own rotations and from every
//               rotation of every kept code
//   lattice     the links of corner_grid.hpp (polarity, reach, cone, mutual), breadth-first labels with the quarter-turn count; a link
//               that contradicts a label is dropped, both claimants of a doubly claimed cell are dropped and the labels made once more,
//               corners left with fewer than two links are dropped; every component is made right-handed in the image
//   cells       the lattice cells whose four corners are labelled, as the quads the marker read takes
//   match       per component the accepted readings vote for (quarter-turn, shift); the winner gives the corners their board indices
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <queue>
#include <utility>
#include <vector>

#include "corner_grid.hpp"
#include "marker_math.hpp"

namespace cba {

constexpr int64_t DICT_BUDGET = 200000;  // candidates drawn at most

inline uint64_t splitmix64(uint64_t* state) {
    uint64_t z = (*state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// -> the number of codes found (<= count) within DICT_BUDGET candidates
inline int marker_dictionary_generate(int bits, int count, int min_distance, uint64_t seed, uint64_t* codes) {
    uint64_t state = seed;
    std::vector<uint64_t> rot;  // the four rotations of every kept code
    int found = 0;
    for (int64_t t = 0; t < DICT_BUDGET && found < count; ++t) {
        const uint64_t c = splitmix64(&state) >> (64 - bits * bits);
        uint64_t r[4] = {c, 0, 0, 0};
        for (int k = 1; k < 4; ++k) r[k] = marker_rotate(r[k - 1], bits);
        bool ok = true;
        for (int k = 1; k < 4 && ok; ++k) ok = marker_popcount(c ^ r[k]) >= min_distance;
        for (size_t e = 0; e < rot.size() && ok; ++e) ok = marker_popcount(c ^ rot[e]) >= min_distance;
        if (!ok) continue;
        codes[found++] = c;
        rot.insert(rot.end(), r, r + 4);
    }
    return found;
}

// ---- the lattice of a partial view ------------------------------------------------------------------------------------------------
// the mutual links of corner_grid.hpp's neighbour rule: link [n][4], -1 where there is none
inline void lattice_links(int n, const double* xy, const double* angle, std::vector<int>& link) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<int> nb(4 * static_cast<size_t>(n), -1);
    link.assign(4 * static_cast<size_t>(n), -1);
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
}

inline int lattice_back(const std::vector<int>& link, int j, int c) {
    for (int kk = 0; kk < 4; ++kk)
        if (link[4 * j + kk] == c) return kk;
    return -1;
}
inline void lattice_unlink(std::vector<int>& link, int c) {
    for (int k = 0; k < 4; ++k) {
        const int j = link[4 * c + k];
        if (j < 0) continue;
        const int b = lattice_back(link, j, c);
        if (b >= 0) link[4 * j + b] = -1;
        link[4 * c + k] = -1;
    }
}

// one labelling pass over the corners that are alive: comp (by first corner, -1: none), li, lj.  Links that contradict are dropped.
inline int lattice_label(int n, std::vector<int>& link, const std::vector<char>& alive, std::vector<int>& comp, std::vector<int>& li,
                         std::vector<int>& lj) {
    static const int SI[4] = {1, 0, -1, 0}, SJ[4] = {0, 1, 0, -1};
    std::vector<int> lo(n, 0);
    comp.assign(n, -1);
    li.assign(n, 0);
    lj.assign(n, 0);
    int n_comp = 0;
    for (int start = 0; start < n; ++start) {
        if (!alive[start] || comp[start] >= 0) continue;
        std::queue<int> q;
        comp[start] = n_comp;
        q.push(start);
        while (!q.empty()) {
            const int c = q.front();
            q.pop();
            for (int k = 0; k < 4; ++k) {
                const int j = link[4 * c + k];
                if (j < 0) continue;
                const int back = lattice_back(link, j, c);
                const int s = (k + lo[c]) & 3, ni = li[c] + SI[s], nj = lj[c] + SJ[s], no = (k + lo[c] + 2 - back) & 3;
                if (comp[j] >= 0) {
                    if (li[j] != ni || lj[j] != nj || lo[j] != no) {
                        link[4 * c + k] = -1;
                        link[4 * j + back] = -1;
                    }
                    continue;
                }
                comp[j] = n_comp; li[j] = ni; lj[j] = nj; lo[j] = no;
                q.push(j);
            }
        }
        ++n_comp;
    }
    return n_comp;
}

// the corners whose (component, i, j) another corner claims too
inline std::vector<int> lattice_twice(int n, const std::vector<int>& comp, const std::vector<int>& li, const std::vector<int>& lj) {
    std::map<std::pair<int, std::pair<int, int>>, std::vector<int>> cell;
    for (int c = 0; c < n; ++c)
        if (comp[c] >= 0) cell[{comp[c], {li[c], lj[c]}}].push_back(c);
    std::vector<int> out;
    for (const auto& kv : cell)
        if (kv.second.size() > 1) out.insert(out.end(), kv.second.begin(), kv.second.end());
    return out;
}

// xy [n][2], angle [n] -> comp [n] (-1: in no component), ij [n][2].  Returns the number of components.
inline int chessboard_lattice(int n, const double* xy, const double* angle, int min_component, int32_t* out_comp, int32_t* out_ij) {
    std::vector<int> link, comp, li, lj;
    std::vector<char> alive(n, 1);
    lattice_links(n, xy, angle, link);
    lattice_label(n, link, alive, comp, li, lj);
    const std::vector<int> twice = lattice_twice(n, comp, li, lj);
    if (!twice.empty()) {
        for (int c : twice) {
            alive[c] = 0;
            lattice_unlink(link, c);
        }
        lattice_label(n, link, alive, comp, li, lj);
        for (int c : lattice_twice(n, comp, li, lj)) {
            alive[c] = 0;
            comp[c] = -1;
            lattice_unlink(link, c);
        }
    }
    // corners left with fewer than two links (counted before any of them is dropped)
    std::vector<int> weak;
    for (int c = 0; c < n; ++c) {
        if (comp[c] < 0) continue;
        int links = 0;
        for (int k = 0; k < 4; ++k) links += link[4 * c + k] >= 0;
        if (links < 2) weak.push_back(c);
    }
    for (int c : weak) comp[c] = -1;
    // per component: size, handedness, origin
    int n_comp = 0;
    for (int c = 0; c < n; ++c) n_comp = std::max(n_comp, comp[c] + 1);
    std::vector<std::vector<int>> members(n_comp);
    for (int c = 0; c < n; ++c)
        if (comp[c] >= 0) members[comp[c]].push_back(c);
    std::vector<int> keep;
    for (int m = 0; m < n_comp; ++m) {
        std::vector<int>& mem = members[m];
        bool ok = static_cast<int>(mem.size()) >= min_component && !mem.empty();
        if (ok) {
            std::map<std::pair<int, int>, int> at;
            for (int c : mem) at[{li[c], lj[c]}] = c;
            double ix = 0.0, iy = 0.0, jx = 0.0, jy = 0.0;
            int ci = 0, cj = 0;
            for (int c : mem) {
                auto a = at.find({li[c] + 1, lj[c]});
                if (a != at.end()) { ix += xy[2 * a->second] - xy[2 * c]; iy += xy[2 * a->second + 1] - xy[2 * c + 1]; ++ci; }
                auto b = at.find({li[c], lj[c] + 1});
                if (b != at.end()) { jx += xy[2 * b->second] - xy[2 * c]; jy += xy[2 * b->second + 1] - xy[2 * c + 1]; ++cj; }
            }
            ok = ci > 0 && cj > 0;
            if (ok) {
                const double cross = (ix / ci) * (jy / cj) - (iy / ci) * (jx / cj);
                if (cross < 0.0)
                    for (int c : mem) li[c] = -li[c];
                ok = cross != 0.0;
            }
        }
        if (!ok) {
            for (int c : mem) comp[c] = -1;
            continue;
        }
        int i0 = li[mem[0]], j0 = lj[mem[0]];
        for (int c : mem) { i0 = std::min(i0, li[c]); j0 = std::min(j0, lj[c]); }
        for (int c : mem) { li[c] -= i0; lj[c] -= j0; }
        keep.push_back(m);
    }
    // numbered by size, ties by the lowest corner index (members are ascending)
    std::stable_sort(keep.begin(), keep.end(), [&](int a, int b) {
        if (members[a].size() != members[b].size()) return members[a].size() > members[b].size();
        return members[a][0] < members[b][0];
    });
    for (int c = 0; c < n; ++c) {
        out_comp[c] = -1;
        out_ij[2 * c] = out_ij[2 * c + 1] = 0;
    }
    for (size_t r = 0; r < keep.size(); ++r)
        for (int c : members[keep[r]]) {
            out_comp[c] = static_cast<int32_t>(r);
            out_ij[2 * c] = li[c];
            out_ij[2 * c + 1] = lj[c];
        }
    return static_cast<int>(keep.size());
}

// The cells of one image's lattice, by component, then j, then i: cell [m][3] = (component, i, j) and the quads [m][8] of the corners
// (i, j) (i+1, j) (i+1, j+1) (i, j+1).  At most `room` are written; returns the true number.
inline int lattice_cells(int n, const double* xy, const int32_t* comp, const int32_t* ij, int room, int32_t* cell, double* quad) {
    std::map<std::pair<int, std::pair<int, int>>, int> at;  // (component, (j, i)) -> corner
    for (int c = 0; c < n; ++c)
        if (comp[c] >= 0) at[{comp[c], {ij[2 * c + 1], ij[2 * c]}}] = c;
    int m = 0;
    for (const auto& kv : at) {
        const int k = kv.first.first, j = kv.first.second.first, i = kv.first.second.second;
        const auto b = at.find({k, {j, i + 1}}), c = at.find({k, {j + 1, i + 1}}), d = at.find({k, {j + 1, i}});
        if (b == at.end() || c == at.end() || d == at.end()) continue;
        if (m < room) {
            cell[3 * m] = k; cell[3 * m + 1] = i; cell[3 * m + 2] = j;
            const int idx[4] = {kv.second, b->second, c->second, d->second};
            for (int t = 0; t < 4; ++t) { quad[8 * m + 2 * t] = xy[2 * idx[t]]; quad[8 * m + 2 * t + 1] = xy[2 * idx[t] + 1]; }
        }
        ++m;
    }
    return m;
}

// ---- board indices -----------------------------------------------------------------------------------------------------------------
struct CharucoBoard {
    int squares_x, squares_y;
};
// marker id -> its square: the bright squares ((sx + sy) odd) row-major.  false when the board has no such marker
inline bool charuco_marker_square(const CharucoBoard& b, int id, int* sx, int* sy) {
    int k = 0;
    for (int y = 0; y < b.squares_y; ++y)
        for (int x = 0; x < b.squares_x; ++x) {
            if (((x + y) & 1) == 0) continue;
            if (k++ == id) { *sx = x; *sy = y; return true; }
        }
    return false;
}
inline void charuco_turn(int r, int a, int b, int* oa, int* ob) {  // T^r, T (a, b) = (b, -a)
    for (int t = 0; t < r; ++t) { const int na = b, nb = -a; a = na; b = nb; }
    *oa = a; *ob = b;
}

// One image.  Corners: comp [n], ij [n][2], xy [n][2].  Readings: cell [m][3] = (component, i, j), flags / id / rotation [m].
// Outputs: ids ascending and xy, at most (squares_x - 1)(squares_y - 1); returns the count; *n_markers: the readings that voted
// for a winning labelling.
inline int charuco_match(const CharucoBoard& b, int min_markers, int n, const int32_t* comp, const int32_t* ij, const double* xy, int m,
                         const int32_t* cell, const int32_t* flags, const int32_t* id, const int32_t* rotation, int32_t* out_ids,
                         double* out_xy, int32_t* n_markers) {
    const int nx = b.squares_x - 1, ny = b.squares_y - 1;
    int n_comp = 0;
    for (int c = 0; c < n; ++c) n_comp = std::max(n_comp, comp[c] + 1);
    struct Win { int votes, r, sx, sy, comp; };
    std::vector<Win> wins;
    for (int k = 0; k < n_comp; ++k) {
        std::map<std::pair<int, std::pair<int, int>>, int> votes;
        for (int t = 0; t < m; ++t) {
            int qx, qy, tx, ty;
            if (cell[3 * t] != k || flags[t] != 0 || !charuco_marker_square(b, id[t], &qx, &qy)) continue;
            charuco_turn(rotation[t] & 3, 2 * cell[3 * t + 1] + 1, 2 * cell[3 * t + 2] + 1, &tx, &ty);
            ++votes[{rotation[t] & 3, {(2 * qx - 1 - tx) / 2, (2 * qy - 1 - ty) / 2}}];
        }
        Win w{0, 0, 0, 0, k};
        int second = 0;
        for (const auto& kv : votes) {
            if (kv.second > w.votes) {
                second = w.votes;
                w = Win{kv.second, kv.first.first, kv.first.second.first, kv.first.second.second, k};
            } else if (kv.second > second) {
                second = kv.second;
            }
        }
        if (w.votes >= min_markers && w.votes > second) wins.push_back(w);
    }
    std::stable_sort(wins.begin(), wins.end(), [](const Win& a, const Win& c) { return a.votes > c.votes; });
    std::vector<int> owner(static_cast<size_t>(nx) * ny, -1);
    *n_markers = 0;
    for (const Win& w : wins) {
        std::vector<std::pair<int, int>> mine;  // (board index, corner)
        bool clash = false;
        for (int c = 0; c < n && !clash; ++c) {
            if (comp[c] != w.comp) continue;
            int bi, bj;
            charuco_turn(w.r, ij[2 * c], ij[2 * c + 1], &bi, &bj);
            bi += w.sx; bj += w.sy;
            if (bi < 0 || bj < 0 || bi >= nx || bj >= ny) continue;
            clash = owner[bj * nx + bi] >= 0;
            mine.push_back({bj * nx + bi, c});
        }
        if (clash) continue;
        for (const auto& p : mine) owner[p.first] = p.second;
        *n_markers += w.votes;
    }
    int count = 0;
    for (int k = 0; k < nx * ny; ++k) {
        if (owner[k] < 0) continue;
        out_ids[count] = k;
        out_xy[2 * count] = xy[2 * owner[k]];
        out_xy[2 * count + 1] = xy[2 * owner[k] + 1];
        ++count;
    }
    for (int k = count; k < nx * ny; ++k) {
        out_ids[k] = -1;
        out_xy[2 * k] = out_xy[2 * k + 1] = NAN;
    }
    return count;
}

}  // namespace cba
