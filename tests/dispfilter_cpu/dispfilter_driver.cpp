// dispfilter_driver.cpp — TEST-ONLY: extern "C" wrapper of disparity_filter_math.hpp for ctypes (tests/dispfilter_ref.py) and, built
// with -DCBA_HOST_DRIVER_MAIN, a stand-alone program whose main checks itself (for the sanitizers).  dispfilter_run walks the sequence
// of disparity_filter.hip with the tiles one after the other: median, tile-local union-find on labels local to the tile, merges along
// the tile borders on the batch-wide labels, flatten, sizes, apply.  The self-check compares it with a sort for the median and a
// flood fill over whole images for the components.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../calibration_amd/csrc/disparity_filter_math.hpp"

using namespace cba;

namespace {

struct HostOps {  // one lane at a time: a plain minimum
    int* L;
    int load(int i) { return L[i]; }
    int min(int i, int v) {
        const int old = L[i];
        if (v < old) L[i] = v;
        return old;
    }
};

template <int M>
void median_pass(int W, int H, const float* in, float* med) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            med[static_cast<size_t>(y) * W + x] = df_median<M>([&](int i, int j) {
                const int xx = x + i, yy = y + j;
                return xx >= 0 && xx < W && yy >= 0 && yy < H ? df_read(in[static_cast<size_t>(yy) * W + xx]) : df_nan();
            });
}

}  // namespace

extern "C" {

// cba_disparity_filter_create + _process in one call; stats [n][3] or null; out == in allowed
void dispfilter_run(int W, int H, int n, int median_half, int max_size, double diff, const float* in, float* out, int64_t* stats) {
    const int64_t frame = static_cast<int64_t>(W) * H, n_px = frame * n;
    std::vector<float> med(static_cast<size_t>(n_px));
    std::vector<int> label(static_cast<size_t>(n_px), -1), size(static_cast<size_t>(n_px), 0);
    for (int img = 0; img < n; ++img) {
        const float* src = in + img * frame;
        float* dst = med.data() + img * frame;
        if (median_half == 0) median_pass<0>(W, H, src, dst);
        else if (median_half == 1) median_pass<1>(W, H, src, dst);
        else median_pass<2>(W, H, src, dst);
        if (stats) {
            int64_t valid = 0;
            for (int64_t i = 0; i < frame; ++i) valid += df_read(src[i]) == df_read(src[i]) ? 1 : 0;
            stats[3 * img] = valid;
            stats[3 * img + 1] = stats[3 * img + 2] = 0;
        }
    }
    if (max_size > 0) {
        // tile-local labels
        for (int img = 0; img < n; ++img)
            for (int y0 = 0; y0 < H; y0 += DF_TH)
                for (int x0 = 0; x0 < W; x0 += DF_TW) {
                    const int64_t base = img * frame;
                    float val[DF_TILE];
                    int lab[DF_TILE];
                    for (int t = 0; t < DF_TILE; ++t) {
                        const int x = x0 + t % DF_TW, y = y0 + t / DF_TW;
                        val[t] = x < W && y < H ? med[static_cast<size_t>(base + static_cast<int64_t>(y) * W + x)] : df_nan();
                        lab[t] = t;
                    }
                    HostOps ops = {lab};
                    for (int t = 0; t < DF_TILE; ++t)
                        if (val[t] == val[t]) df_tile_link(ops, val, t % DF_TW, t / DF_TW, diff);
                    for (int t = 0; t < DF_TILE; ++t) {
                        const int x = x0 + t % DF_TW, y = y0 + t / DF_TW;
                        if (x >= W || y >= H || !(val[t] == val[t])) continue;
                        const int r = df_find(ops, t);
                        label[static_cast<size_t>(base + static_cast<int64_t>(y) * W + x)] =
                            static_cast<int>(base + static_cast<int64_t>(y0 + r / DF_TW) * W + x0 + r % DF_TW);
                    }
                }
        // merges along the tile borders, then flatten and sizes
        HostOps ops = {label.data()};
        for (int img = 0; img < n; ++img)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (x % DF_TW == 0 || y % DF_TH == 0) df_border_link(ops, med.data(), img * frame, W, x, y, diff);
        for (int64_t i = 0; i < n_px; ++i)
            if (label[static_cast<size_t>(i)] >= 0) label[static_cast<size_t>(i)] = df_find(ops, static_cast<int>(i));
        for (int64_t i = 0; i < n_px; ++i)
            if (label[static_cast<size_t>(i)] >= 0) ++size[static_cast<size_t>(label[static_cast<size_t>(i)])];
    }
    for (int64_t i = 0; i < n_px; ++i) {
        float v = med[static_cast<size_t>(i)];
        const int r = label[static_cast<size_t>(i)];
        if (max_size > 0 && r >= 0 && size[static_cast<size_t>(r)] <= max_size) {
            v = df_nan();
            if (stats) {
                stats[3 * (i / frame) + 2] += 1;
                if (r == i) stats[3 * (i / frame) + 1] += 1;
            }
        }
        out[i] = v;
    }
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
// ---- the self-check's own statement of the rule: a sort and a flood fill -------------------------------------------------------------
static void plain_filter(int W, int H, int n, int m, int max_size, double diff, const float* in, float* out) {
    const size_t frame = static_cast<size_t>(W) * H;
    for (int img = 0; img < n; ++img) {
        std::vector<float> a(frame), b(frame);
        for (size_t i = 0; i < frame; ++i) a[i] = df_read(in[img * frame + i]);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float c = a[static_cast<size_t>(y) * W + x];
                if (!(c == c)) { b[static_cast<size_t>(y) * W + x] = c; continue; }
                std::vector<float> w;
                for (int yy = std::max(0, y - m); yy <= std::min(H - 1, y + m); ++yy)
                    for (int xx = std::max(0, x - m); xx <= std::min(W - 1, x + m); ++xx)
                        if (a[static_cast<size_t>(yy) * W + xx] == a[static_cast<size_t>(yy) * W + xx]) w.push_back(a[static_cast<size_t>(yy) * W + xx]);
                std::sort(w.begin(), w.end());
                b[static_cast<size_t>(y) * W + x] = w[(w.size() - 1) / 2];
            }
        std::vector<char> seen(frame, 0);
        for (size_t s = 0; s < frame && max_size > 0; ++s) {
            if (seen[s] || !(b[s] == b[s])) continue;
            std::vector<size_t> comp = {s};
            seen[s] = 1;
            for (size_t k = 0; k < comp.size(); ++k) {
                const size_t p = comp[k];
                const int x = static_cast<int>(p % W), y = static_cast<int>(p / W);
                const size_t nb[4] = {p - 1, p + 1, p - W, p + W};
                const bool ok[4] = {x > 0, x < W - 1, y > 0, y < H - 1};
                for (int d = 0; d < 4; ++d)
                    if (ok[d] && !seen[nb[d]] && b[nb[d]] == b[nb[d]] && std::fabs(static_cast<double>(b[p]) - static_cast<double>(b[nb[d]])) <= diff) {
                        seen[nb[d]] = 1;
                        comp.push_back(nb[d]);
                    }
            }
            if (comp.size() <= static_cast<size_t>(max_size))
                for (size_t p : comp) out[img * frame + p] = df_nan();
            else
                for (size_t p : comp) out[img * frame + p] = b[p];
        }
        for (size_t i = 0; i < frame; ++i)
            if (max_size <= 0 || !(b[i] == b[i])) out[img * frame + i] = b[i];
    }
}

int main() {
    int bad = 0;
    uint32_t s = 2468u;
    const int sizes[][2] = {{1, 1}, {9, 1}, {1, 7}, {DF_TW - 1, DF_TH - 1}, {DF_TW, DF_TH}, {DF_TW + 1, DF_TH + 1}, {2 * DF_TW + 3, 2 * DF_TH + 3}};
    for (const auto& wh : sizes)
        for (int m = 0; m <= 2; ++m)
            for (int max_size : {0, 1, 5, 0x7fffffff})
                for (double diff : {0.0, 0.5, 1.0}) {
                    const int W = wh[0], H = wh[1], n = 2;
                    std::vector<float> in(static_cast<size_t>(W) * H * n), got(in.size()), want(in.size());
                    for (auto& v : in) {
                        s = s * 1664525u + 1013904223u;
                        const uint32_t r = s >> 24;
                        v = r < 77 ? df_nan() : r == 77 ? -0.0f : r == 78 ? INFINITY : 0.5f * static_cast<float>(r % 8);
                    }
                    std::vector<int64_t> stats(3 * n);
                    dispfilter_run(W, H, n, m, max_size, diff, in.data(), got.data(), stats.data());
                    plain_filter(W, H, n, m, max_size, diff, in.data(), want.data());
                    int64_t removed = 0;
                    for (size_t i = 0; i < in.size(); ++i) {
                        const bool gn = !(got[i] == got[i]), wn = !(want[i] == want[i]);
                        uint32_t gb, wb;
                        __builtin_memcpy(&gb, &got[i], 4);
                        __builtin_memcpy(&wb, &want[i], 4);
                        if (gn != wn || (!gn && gb != wb)) ++bad;
                    }
                    for (int img = 0; img < n; ++img) removed += stats[3 * img + 2];
                    if (max_size == 0 && removed != 0) ++bad;
                    std::vector<float> inplace(in);  // out == in
                    dispfilter_run(W, H, n, m, max_size, diff, inplace.data(), inplace.data(), nullptr);
                    for (size_t i = 0; i < in.size(); ++i)
                        if ((inplace[i] == inplace[i]) != (got[i] == got[i]) || (got[i] == got[i] && inplace[i] != got[i])) ++bad;
                }
    std::printf("disparity filter self-check: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
