// charuco_driver.cpp — TEST-ONLY: extern "C" wrapper of marker_math.hpp and marker_board.hpp for ctypes (tests/test_charuco_cpu.py)
// and, built with -DCBA_HOST_DRIVER_MAIN, a stand-alone program whose main checks itself (for the sanitizers) over planted lattices,
// votes and a marker.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../calibration_amd/csrc/marker_board.hpp"
#include "../../calibration_amd/csrc/marker_math.hpp"

using namespace cba;

extern "C" {

// k_corner_arms on the host: scores [n][max_corners], NaN past the kept corners
void ch_arms(int W, int H, int n_images, int max_corners, const uint8_t* images, const int32_t* count, const double* xy, const double* dirs,
             double len0, double len1, double off, double* score) {
    const double len[2] = {len0, len1};
    for (int im = 0; im < n_images; ++im)
        for (int c = 0; c < max_corners; ++c) {
            const size_t i = static_cast<size_t>(im) * max_corners + c;
            score[i] = c < std::min(count[im], max_corners)
                           ? corner_arms_one(images + static_cast<size_t>(im) * W * H, W, H, xy[2 * i], xy[2 * i + 1], dirs + 24 * i, len, off)
                           : static_cast<double>(NAN);
        }
}

// k_marker_read on the host
void ch_read(int W, int H, const uint8_t* images, int bits, double ratio, int n_markers, const uint64_t* codes, int samples, double min_contrast,
             int max_border_errors, int max_correction, int n_cells, const int32_t* cell_image, const double* quad, MarkerReading* out) {
    std::vector<uint64_t> table(4 * static_cast<size_t>(n_markers));
    marker_rotated_table(bits, n_markers, codes, table.data());
    const MarkerParams p{W, H, bits, samples, 4 * n_markers, max_border_errors, max_correction, ratio, min_contrast};
    for (int t = 0; t < n_cells; ++t)
        marker_read_one(p, images + static_cast<size_t>(cell_image[t]) * W * H, quad + 8 * static_cast<size_t>(t), table.data(), out + t);
}

int ch_dictionary(int bits, int count, int min_distance, uint64_t seed, uint64_t* codes) {
    return marker_dictionary_generate(bits, count, min_distance, seed, codes);
}

int ch_lattice(int n, const double* xy, const double* angle, int min_component, int32_t* comp, int32_t* ij) {
    return chessboard_lattice(n, xy, angle, min_component, comp, ij);
}

int ch_cells(int n, const double* xy, const int32_t* comp, const int32_t* ij, int room, int32_t* cell, double* quad) {
    return lattice_cells(n, xy, comp, ij, room, cell, quad);
}

int ch_match(int squares_x, int squares_y, int min_markers, int n, const int32_t* comp, const int32_t* ij, const double* xy, int m,
             const int32_t* cell, const int32_t* flags, const int32_t* id, const int32_t* rotation, int32_t* out_ids, double* out_xy,
             int32_t* n_markers) {
    return charuco_match(CharucoBoard{squares_x, squares_y}, min_markers, n, comp, ij, xy, m, cell, flags, id, rotation, out_ids, out_xy,
                         n_markers);
}

}  // extern "C"

#ifdef CBA_HOST_DRIVER_MAIN
#define FAIL() (std::printf("charuco self-check: line %d\n", __LINE__), ++bad)

// an axis-aligned lattice of nx x ny corners, `step` px apart, from (x0, y0): the angle alternates between +pi/4 and -pi/4
static void plant(int nx, int ny, double x0, double y0, double step, std::vector<double>& xy, std::vector<double>& angle) {
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            xy.push_back(x0 + step * i);
            xy.push_back(y0 + step * j);
            angle.push_back(((i + j) & 1) ? -GRID_PI / 4 : GRID_PI / 4);
        }
}

// Self-check: a full lattice is one component with every label; a false corner planted inside a square costs at most itself and its
// cell-mates; two far lattices are two components; the readings of a 7 x 6 board vote every corner onto its index, a 1 : 1 vote is
// rejected; a dictionary respects its distance; a drawn marker reads back in each quarter-turn, a constant image is LOW_CONTRAST, a
// quad over the border is WINDOW and a collapsed one DEGENERATE.
int main() {
    int bad = 0;
    const int nx = 6, ny = 5;  // inner corners of a 7 x 6 board
    std::vector<double> xy, angle;
    plant(nx, ny, 40.0, 30.0, 30.0, xy, angle);
    std::vector<int32_t> comp(64), ij(128);
    if (ch_lattice(nx * ny, xy.data(), angle.data(), 4, comp.data(), ij.data()) != 1) FAIL();
    for (int c = 0; c < nx * ny; ++c)
        if (comp[c] != 0) FAIL();
    std::vector<int32_t> cell(3 * 64);
    std::vector<double> quad(8 * 64);
    const int m = ch_cells(nx * ny, xy.data(), comp.data(), ij.data(), 64, cell.data(), quad.data());
    if (m != (nx - 1) * (ny - 1)) FAIL();
    // every bright interior square votes; the rotation follows from the labelling: the board step of the lattice's i-step is T^r (1, 0)
    const CharucoBoard board{nx + 1, ny + 1};
    std::vector<int32_t> flags(m, MARKER_FLAG_NO_MATCH), id(m, 0), rot(m, 0), out_ids(nx * ny);
    std::vector<double> out_xy(2 * nx * ny);
    for (int t = 0; t < m; ++t) {
        const double* q = &quad[8 * t];
        const int di = static_cast<int>(std::lround((q[2] - q[0]) / 30.0)), dj = static_cast<int>(std::lround((q[3] - q[1]) / 30.0));
        rot[t] = di == 1 ? 0 : dj == -1 ? 1 : di == -1 ? 2 : 3;
        const int sx = static_cast<int>(std::floor(((q[0] + q[4]) / 2 - 40.0) / 30.0)) + 1, sy = static_cast<int>(std::floor(((q[1] + q[5]) / 2 - 30.0) / 30.0)) + 1;
        for (int k = 0, qx, qy; charuco_marker_square(board, k, &qx, &qy); ++k)
            if (qx == sx && qy == sy) { flags[t] = 0; id[t] = k; }
    }
    int32_t nm = 0;
    int count = ch_match(board.squares_x, board.squares_y, 2, nx * ny, comp.data(), ij.data(), xy.data(), m, cell.data(), flags.data(),
                         id.data(), rot.data(), out_ids.data(), out_xy.data(), &nm);
    if (count != nx * ny || nm != 10) FAIL();
    for (int c = 0; c < count; ++c)
        if (out_ids[c] != c || out_xy[2 * c] != xy[2 * c] || out_xy[2 * c + 1] != xy[2 * c + 1]) FAIL();
    // two votes that disagree, one each: rejected
    {
        std::vector<int32_t> f2(flags), i2(id);
        int seen = 0;
        for (int t = 0; t < m; ++t) {
            if (f2[t] != 0) continue;
            if (seen == 1) i2[t] = i2[t] + 1;
            if (seen >= 2) f2[t] = MARKER_FLAG_NO_MATCH;
            ++seen;
        }
        if (ch_match(board.squares_x, board.squares_y, 1, nx * ny, comp.data(), ij.data(), xy.data(), m, cell.data(), f2.data(), i2.data(),
                     rot.data(), out_ids.data(), out_xy.data(), &nm) != 0) FAIL();
    }
    // a false corner inside a square, a second lattice far away
    {
        std::vector<double> xy2(xy), a2(angle);
        xy2.push_back(40.0 + 30.0 * 2 + 11.0); xy2.push_back(30.0 + 30.0 * 2 + 9.0); a2.push_back(-GRID_PI / 4);
        plant(3, 3, 400.0, 300.0, 20.0, xy2, a2);
        const int n2 = static_cast<int>(a2.size());
        std::vector<int32_t> c2(n2), l2(2 * n2);
        if (ch_lattice(n2, xy2.data(), a2.data(), 4, c2.data(), l2.data()) != 2) FAIL();
        int lost = 0;
        for (int c = 0; c < nx * ny; ++c) lost += c2[c] != 0;
        if (lost > 4 || c2[nx * ny] >= 0) FAIL();
        for (int c = nx * ny + 1; c < n2; ++c)
            if (c2[c] != 1) FAIL();
    }
    // dictionary
    uint64_t codes[32];
    const int found = ch_dictionary(4, 32, 4, 5, codes);
    if (found != 32) FAIL();
    std::vector<uint64_t> table(4 * 32);
    marker_rotated_table(4, 32, codes, table.data());
    for (int a = 0; a < 32; ++a)
        for (int e = 0; e < 4 * 32; ++e)
            if (e != 4 * a && marker_popcount(codes[a] ^ table[e]) < 4) FAIL();
    uint64_t few[64];
    if (ch_dictionary(3, 64, 4, 1, few) >= 64) FAIL();
    // a drawn marker: 6 x 6 cells of 10 px at (20, 20), the square's quad at ratio 0.6
    const int W = 100, H = 100, side = 60;
    MarkerReading r;
    for (int id0 = 0; id0 < 3; ++id0)
        for (int turn = 0; turn < 4; ++turn) {
            std::vector<uint8_t> img(static_cast<size_t>(W) * H, 210);
            const uint64_t code = table[4 * id0 + turn];
            for (int y = 0; y < side; ++y)
                for (int x = 0; x < side; ++x) {
                    const int cx = x / 10, cy = y / 10;
                    const bool inner = cx >= 1 && cx <= 4 && cy >= 1 && cy <= 4;
                    const bool on = inner && ((code >> (15 - ((cy - 1) * 4 + cx - 1))) & 1u);
                    img[(20 + y) * W + 20 + x] = on ? 210 : 40;
                }
            const double c0 = 19.5 + side / 2.0, hf = side / 0.6 / 2.0;
            const double q[8] = {c0 - hf, c0 - hf, c0 + hf, c0 - hf, c0 + hf, c0 + hf, c0 - hf, c0 + hf};
            const int32_t zero = 0;
            ch_read(W, H, img.data(), 4, 0.6, 32, codes, 3, 40.0, 0, 0, 1, &zero, q, &r);
            if (r.flags != 0 || r.id != id0 || r.rotation != turn || r.distance != 0 || r.code != code) FAIL();
            const double over[8] = {-30.0, 1.0, 70.0, 1.0, 70.0, 99.0, -30.0, 99.0};
            ch_read(W, H, img.data(), 4, 0.6, 32, codes, 3, 40.0, 0, 0, 1, &zero, over, &r);
            if (r.flags != MARKER_FLAG_WINDOW || r.id != -1) FAIL();
            const double flat[8] = {10.0, 10.0, 50.0, 50.0, 90.0, 90.0, 30.0, 30.0};
            ch_read(W, H, img.data(), 4, 0.6, 32, codes, 3, 40.0, 0, 0, 1, &zero, flat, &r);
            if (r.flags != MARKER_FLAG_DEGENERATE) FAIL();
            std::fill(img.begin(), img.end(), 77);
            ch_read(W, H, img.data(), 4, 0.6, 32, codes, 3, 40.0, 0, 0, 1, &zero, q, &r);
            if (!(r.flags & MARKER_FLAG_LOW_CONTRAST) || r.code != 0 || r.level_min != 77.0 || r.level_max != 77.0) FAIL();
        }
    std::printf("charuco self-check: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
#endif
