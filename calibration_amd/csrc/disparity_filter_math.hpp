// disparity_filter_math.hpp — the median and speckle filters of a disparity map (calibba.h: cba_disparity_filter) as __host__ __device__
// code.  The kernels of disparity_filter.hip call these pieces per pixel; tests/dispfilter_cpu compiles the same header with g++ and
// runs the same tile-local, border-merge and flatten sequence over the tiles one after the other.  The reference has no counterpart.
//
//   reading    df_read: a non-finite value is NaN, -0.0 is +0.0
//   median     df_median<M>: the lower median of the valid values of the (2M+1)^2 window by rank counting.  A NaN compares false with
//              everything, so an invalid or outside pixel takes part in no count; equal values have equal bits after df_read, so
//              whichever of them is selected the output bits are the same
//   join       df_joined: both valid and |double(a) - double(b)| <= diff
//   components df_find / df_union on a label array through an Ops policy (plain memory on the host, atomicMin on the device).  A label
//              array L is a forest with L[i] <= i; a root has L[i] == i; a union only ever lowers a label.  Hence the lowest index
//              of a component is its root when the unions are done, whatever the order they ran in.
//   tile       df_tile_link: the joins of a pixel with its left and upper neighbour inside a DF_TW x DF_TH tile (indices local to the
//              tile); df_border_link: the joins across the left and upper edge of a tile (indices global over the batch).
#pragma once
#include <cmath>
#include <cstdint>

#include "reproj_math.hpp"  // CBA_HD

namespace cba {

constexpr int DF_TW = 32, DF_TH = 8;  // the component tile: one workgroup of DF_TW * DF_TH lanes, one pixel per lane
constexpr int DF_TILE = DF_TW * DF_TH;
constexpr int DF_MAX_HALF = 2;        // the largest median_half

CBA_HD float df_nan() { return __builtin_nanf(""); }

CBA_HD float df_read(float v) {
    if (!(v - v == 0.0f)) return df_nan();  // NaN and +-inf: v - v is NaN
    return v == 0.0f ? 0.0f : v;            // -0.0 -> +0.0
}

// The lower median of the valid values among at(i, j), |i|, |j| <= M (NaN: invalid or outside the image); NaN when the centre is
// invalid.  at is called once per window position with compile-time constant loop bounds, so the window lives in registers.
template <int M, class At>
CBA_HD float df_median(At&& at) {
    constexpr int N = (2 * M + 1) * (2 * M + 1);
    float v[N];
    int k = 0;
#pragma unroll
    for (int j = -M; j <= M; ++j)
#pragma unroll
        for (int i = -M; i <= M; ++i) {
            const float t = at(i, j);
            v[(j + M) * (2 * M + 1) + (i + M)] = t;
            k += t == t ? 1 : 0;
        }
    const float centre = v[M * (2 * M + 1) + M];
    if (!(centre == centre)) return df_nan();
    const int t = (k - 1) / 2;  // the index of the lower median among the k sorted valid values
    float out = centre;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        int lt = 0, le = 0;  // valid values below v[a] / not above it
#pragma unroll
        for (int b = 0; b < N; ++b) {
            lt += v[b] < v[a] ? 1 : 0;
            le += v[b] <= v[a] ? 1 : 0;
        }
        if (lt <= t && t < le) out = v[a];  // the sorted positions [lt, le) hold v[a]; never true for a NaN (le == 0)
    }
    return out;
}

CBA_HD bool df_joined(float a, float b, double diff) {
    return a == a && b == b && std::fabs(static_cast<double>(a) - static_cast<double>(b)) <= diff;
}

// Ops: int load(int i) - the label of i; int min(int i, int v) - L[i] = min(L[i], v), returns the label before.
//
// Termination: L[i] <= i holds at the start (L[i] = i) and is kept by every min (v < i below).  So a step p = L[a] != a has p < a:
// the indices visited decrease strictly and are bounded below by 0.  Labels that other lanes lower meanwhile keep the invariant.
template <class Ops>
CBA_HD int df_find(Ops& L, int a) {
    for (;;) {
        const int p = L.load(a);
        if (p == a) return a;
        a = p;
    }
}

// Joins the trees of a and b.  Termination: inside the loop a > b.  min(a, b) returns old <= a.  old == a: a was a root and now
// points to b - done.  Otherwise old < a (the label had decreased, by an earlier step of any lane) and the loop goes on with the
// pair (old, b): a + b has decreased strictly and is bounded below by 0, so a retry happens only after a label has decreased and
// only finitely often.  No lane waits for another one.  Correctness: L[a] was old; it is now min(old, b); a stays connected to old
// because the loop goes on to join old and b.
template <class Ops>
CBA_HD void df_union(Ops& L, int a, int b) {
    a = df_find(L, a);
    b = df_find(L, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = L.min(a, b);
        if (old == a) break;
        a = old;
    }
}

// the joins of the tile pixel (tx, ty) with its left and upper neighbour in the tile; val [DF_TILE]: the tile's values, NaN outside
// the image; L: labels local to the tile
template <class Ops>
CBA_HD void df_tile_link(Ops& L, const float* val, int tx, int ty, double diff) {
    const int t = ty * DF_TW + tx;
    const float v = val[t];
    if (tx > 0 && df_joined(v, val[t - 1], diff)) df_union(L, t, t - 1);
    if (ty > 0 && df_joined(v, val[t - DF_TW], diff)) df_union(L, t, t - DF_TW);
}

// the joins of pixel (x, y) of the image that starts at element `base` of img across the left and the upper edge of its tile; L:
// labels global over the batch (n W H <= 2^31 - 1, so an index fits an int)
//
// A join across an edge is left out when the previous pixel pair along the same edge of the same tile, (p, q), makes it redundant: p
// and q are joined, L[p] == L[i] and L[q] == L[j].  Every value a label ever holds is a pixel of its owner's final component (a union
// only links trees that end up joined), so equal labels prove i ~ p and j ~ q at the end of the pass; p ~ q holds because the lane of
// p either joins them or leaves that out by the same argument one pixel earlier, and the first pixel of a tile's edge never leaves
// its join out.  Labels read while other lanes lower them can only make the test fail, which costs one redundant union.
template <class Ops>
CBA_HD bool df_pair_covered(Ops& L, const float* img, int64_t i, int64_t j, int64_t p, int64_t q, double diff) {
    return df_joined(img[p], img[q], diff) && L.load(static_cast<int>(p)) == L.load(static_cast<int>(i)) &&
           L.load(static_cast<int>(q)) == L.load(static_cast<int>(j));
}
template <class Ops>
CBA_HD void df_border_link(Ops& L, const float* img, int64_t base, int W, int x, int y, double diff) {
    const int64_t i = base + static_cast<int64_t>(y) * W + x;
    const float v = img[i];
    if (!(v == v)) return;
    if (x > 0 && x % DF_TW == 0 && df_joined(v, img[i - 1], diff) &&
        !(y % DF_TH != 0 && df_pair_covered(L, img, i, i - 1, i - W, i - W - 1, diff)))  // the pair one row up, in the same two tiles
        df_union(L, static_cast<int>(i), static_cast<int>(i - 1));
    if (y > 0 && y % DF_TH == 0 && df_joined(v, img[i - W], diff) &&
        !(x % DF_TW != 0 && df_pair_covered(L, img, i, i - W, i - 1, i - W - 1, diff)))  // the pair one column left, in the same two tiles
        df_union(L, static_cast<int>(i), static_cast<int>(i - W));
}

}  // namespace cba
