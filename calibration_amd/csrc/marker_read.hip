// marker_read.hip — ChArUco boards on the GPU (marker_math.hpp, marker_board.hpp, calibba.h: cba_charuco_detector).  The handle owns a
// corner detector (corner_detect.hip) and works on its resident images.  A process call is the corner stage (one upload of the images,
// one synchronise) and two small device stages, each one upload, one launch, one download and one synchronise:
//   k_corner_arms   one lane per slot (image, corner), grid-stride: the arm test from the 12 direction vectors the host made
//                   (corner_arms_one); slots past the kept corners get NaN.  No cross-lane step, loops not unrolled.
//   k_marker_read   one wavefront per lattice cell, four per workgroup.  The quad and the image index come from the cell table; every
//                   lane forms the same homography.  A lane owns marker cells lane and lane + 64 and sums their sub-samples in the
//                   stated order.  Minimum and maximum of the means are DPP reductions (wave_reduce.hpp), ballots give the mask of
//                   bright cells, the border count is a popcount against a constant mask, lanes stride over the rotated-code table
//                   and two more wave minimums pick the match.  Lane 0 writes the record.  No atomics, no LDS, no scratch.
// Each device stage is one stream-ordered sequence; stage_ms (experiment builds) times them with device events, the host stages with
// the steady clock.  Between them the host labels the partial lattices and, at the end, assigns the board indices (marker_board.hpp).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "pipelines.hpp"
#include "marker_board.hpp"
#include "image_tile.hpp"
#include "wave_reduce.hpp"

namespace cba {

constexpr int MRK_BLOCK = 256;
constexpr int MRK_WAVE = 64;
constexpr int MRK_WAVES = MRK_BLOCK / MRK_WAVE;  // wavefronts, and so cells, per workgroup
constexpr int MRK_GRID = 4096;                   // grid-stride cap of k_corner_arms

struct ArmArgs {
    const uint8_t* img;
    int W, H, n_slots, max_corners;
    const int32_t* count;
    const int32_t* peak_px;
    const double* xy;    // [n_slots][2]
    const double* dirs;  // [n_slots][12][2]
    double len[2], off;
    double* score;       // [n_slots]
};

__global__ __launch_bounds__(MRK_BLOCK) void k_corner_arms(ArmArgs a) {
    for (int i = blockIdx.x * MRK_BLOCK + threadIdx.x; i < a.n_slots; i += gridDim.x * MRK_BLOCK) {
        const SlotAt s = slot_at(i, a.max_corners, a.count, a.peak_px, a.W, a.H);
        double score = NAN;
        if (s.kept) score = corner_arms_one(a.img + s.fbase, a.W, a.H, a.xy[2 * i], a.xy[2 * i + 1], a.dirs + 24 * static_cast<size_t>(i), a.len, a.off);
        a.score[i] = score;
    }
}

struct ReadArgs {
    const uint8_t* img;           // [n_images][H][W]
    MarkerParams p;
    int n_cells;
    const int32_t* cell_image;    // [n_cells]
    const double* quad;           // [n_cells][8]
    const uint64_t* table;        // [p.n_codes]
    uint64_t border_lo, border_hi;
    MarkerReading* out;           // [n_cells]
};

__global__ __launch_bounds__(MRK_BLOCK) void k_marker_read(ReadArgs a) {
    const int lane = static_cast<int>(threadIdx.x) & (MRK_WAVE - 1);
    const int cell = static_cast<int>(blockIdx.x) * MRK_WAVES + (static_cast<int>(threadIdx.x) >> 6);
    if (cell >= a.n_cells) return;  // the whole wavefront; nothing below crosses wavefronts
    const MarkerParams& p = a.p;
    MarkerReading r;
    double q[8], hc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = a.quad[8 * static_cast<size_t>(cell) + k];
    if (!marker_homography(q, hc)) {
        marker_unread(MARKER_FLAG_DEGENERATE, &r);
        if (lane == 0) a.out[cell] = r;
        return;
    }
    const uint8_t* img = a.img + static_cast<int64_t>(a.cell_image[cell]) * p.W * p.H;
    const int cells = (p.bits + 2) * (p.bits + 2);
    const bool own0 = lane < cells, own1 = lane + MRK_WAVE < cells;
    double m0 = 0.0, m1 = 0.0;
    bool ok = true;
    if (own0) ok = marker_cell_mean(img, p.W, p.H, hc, p.ratio, p.bits, p.samples, lane, &m0);
    if (own1) ok = marker_cell_mean(img, p.W, p.H, hc, p.ratio, p.bits, p.samples, lane + MRK_WAVE, &m1) && ok;
    if (__ballot(!ok) != 0) {
        marker_unread(MARKER_FLAG_WINDOW, &r);
        if (lane == 0) a.out[cell] = r;
        return;
    }
    const double inf = __builtin_huge_val();
    const double lo_level = wave_from63(wave_min63(fmin(own0 ? m0 : inf, own1 ? m1 : inf)));
    const double hi_level = wave_from63(wave_max63(fmax(own0 ? m0 : 0.0, own1 ? m1 : 0.0)));  // the means are >= 0
    double t;
    {
        CBA_NO_CONTRACT
        t = (lo_level + hi_level) / 2.0;
    }
    const uint64_t lo = __ballot(own0 && m0 > t), hi = __ballot(own1 && m1 > t);
    const int border_errors = __popcll(lo & a.border_lo) + __popcll(hi & a.border_hi);
    const uint64_t code = marker_code_of(lo, hi, p.bits);
    int best = MARKER_NO_KEY;
#pragma unroll 1
    for (int e = lane; e < p.n_codes; e += MRK_WAVE) best = min(best, (__popcll(code ^ a.table[e]) << 16) | e);
    best = wave_from63(wave_min63(best));
    const int winner = (best & 0xffff) >> 2;
    int second = MARKER_NO_KEY;
#pragma unroll 1
    for (int e = lane; e < p.n_codes; e += MRK_WAVE)
        if ((e >> 2) != winner) second = min(second, __popcll(code ^ a.table[e]));
    second = wave_from63(wave_min63(second));
    marker_finish(p, lo_level, hi_level, border_errors, code, best, second == MARKER_NO_KEY ? -1 : second, &r);
    if (lane == 0) a.out[cell] = r;
}

// ---- host glue ---------------------------------------------------------------------------------------------------------------------
// The handle: a corner detector, the tables made at create and every device and host buffer of a call, sized there.  Each device
// stage ends with the handle's stream synchronised.
struct CharucoDetector : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    struct Closer { void operator()(CornerDetector* d) const noexcept { corner_detector_destroy(d); } };
    std::unique_ptr<CornerDetector, Closer> corners;
    cba_charuco_options opts;
    cba_charuco_board board;
    int W = 0, H = 0, max_images = 0, max_corners = 0, max_cells = 0, n_images = 0;  // n_images: of the last process
    MarkerParams mp;
    uint64_t border_lo = 0, border_hi = 0;
    DevBuf<uint64_t> table;
    DevBuf<double> dirs, score, quad;
    DevBuf<int32_t> cell_image;
    DevBuf<MarkerReading> readings;
    // host staging of a call
    std::vector<int32_t> h_count, h_status, h_flags, h_cell_image, h_cell, h_comp, h_ij, h_good;
    std::vector<double> h_xy, h_angle, h_dirs, h_score, h_quad, h_gxy, h_gangle;
    std::vector<MarkerReading> h_readings;
};
static_assert(!std::is_copy_constructible_v<CharucoDetector>, "a handle owns its stream and buffers");

CharucoDetector* charuco_detector_create(int W, int H, int max_images, int max_corners, int max_cells, const cba_corner_options& co,
                                         const cba_charuco_options& o, const cba_charuco_board& b, const uint64_t* codes, int device) {
    auto h = std::make_unique<CharucoDetector>(device);
    h->corners.reset(corner_detector_create(W, H, max_images, max_corners, co, device));
    h->opts = o;
    h->board = b;
    h->W = W; h->H = H; h->max_images = max_images; h->max_corners = max_corners; h->max_cells = max_cells;
    h->mp = MarkerParams{W, H, b.marker_bits, o.cell_samples, 4 * b.n_markers, o.max_border_errors, o.max_correction, b.marker_ratio,
                         o.min_marker_contrast};
    marker_border_mask(b.marker_bits, &h->border_lo, &h->border_hi);
    std::vector<uint64_t> table(4 * static_cast<size_t>(b.n_markers));
    marker_rotated_table(b.marker_bits, b.n_markers, codes, table.data());
    const hipStream_t s = h->begin();
    h->table.assign(table.data(), table.size(), s);
    const size_t slots = static_cast<size_t>(max_images) * max_corners;
    h->dirs.alloc(24 * slots);
    h->score.alloc(slots);
    h->quad.alloc(8 * static_cast<size_t>(max_cells));
    h->cell_image.alloc(max_cells);
    h->readings.alloc(max_cells);
    h->h_count.resize(max_images); h->h_status.resize(max_images); h->h_flags.resize(slots);
    h->h_xy.resize(2 * slots); h->h_angle.resize(slots); h->h_dirs.resize(24 * slots); h->h_score.resize(slots);
    h->h_cell_image.resize(max_cells); h->h_cell.resize(3 * static_cast<size_t>(max_cells)); h->h_quad.resize(8 * static_cast<size_t>(max_cells));
    h->h_readings.resize(max_cells);
    h->h_comp.resize(max_corners); h->h_ij.resize(2 * static_cast<size_t>(max_corners)); h->h_good.resize(max_corners);
    h->h_gxy.resize(2 * static_cast<size_t>(max_corners)); h->h_gangle.resize(max_corners);
    CBA_HIP(hipStreamSynchronize(s));
    return h.release();
}

int charuco_detector_max_images(const CharucoDetector* h) { return h->max_images; }
int charuco_detector_max_corners(const CharucoDetector* h) { return h->max_corners; }
int charuco_detector_max_cells(const CharucoDetector* h) { return h->max_cells; }
int charuco_detector_last_images(const CharucoDetector* h) { return h->n_images; }
int charuco_detector_board_corners(const CharucoDetector* h) { return (h->board.squares_x - 1) * (h->board.squares_y - 1); }

// directions in -> scores, on the images, positions and counts of the last process
void charuco_detector_arms(CharucoDetector* h, int n_images, const double* dirs, double* out_score, double* ms) {
    const hipStream_t s = h->begin();
    StageTimer<2> tm(s, ms != nullptr);
    tm.mark(0);
    const size_t slots = static_cast<size_t>(n_images) * h->max_corners;
    const CornerDeviceView v = corner_detector_view(h->corners.get());
    h->dirs.upload(dirs, 24 * slots, s);
    ArmArgs a{v.img, h->W, h->H, static_cast<int>(slots), h->max_corners, v.count, v.peak_px, v.xy, h->dirs.p,
              {h->opts.arm_lengths[0], h->opts.arm_lengths[1]}, h->opts.arm_offset, h->score.p};
    hipLaunchKernelGGL(k_corner_arms, dim3(launch_grid(static_cast<int64_t>(slots), MRK_BLOCK, MRK_GRID)), dim3(MRK_BLOCK), 0, s, a);
    CBA_HIP(hipGetLastError());
    h->score.download(out_score, slots, s);
    tm.mark(1);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(ms);
}

// cells in -> readings, on the images of the last process
void charuco_detector_read(CharucoDetector* h, int n_cells, const int32_t* cell_image, const double* quad, cba_marker_reading* out, double* ms) {
    static_assert(sizeof(cba_marker_reading) == sizeof(MarkerReading), "one record layout");
    if (ms) *ms = 0.0;
    if (n_cells == 0) return;
    const hipStream_t s = h->begin();
    StageTimer<2> tm(s, ms != nullptr);
    tm.mark(0);
    const CornerDeviceView v = corner_detector_view(h->corners.get());
    h->cell_image.upload(cell_image, n_cells, s);
    h->quad.upload(quad, 8 * static_cast<size_t>(n_cells), s);
    ReadArgs a{v.img, h->mp, n_cells, h->cell_image.p, h->quad.p, h->table.p, h->border_lo, h->border_hi, h->readings.p};
    hipLaunchKernelGGL(k_marker_read, dim3((n_cells + MRK_WAVES - 1) / MRK_WAVES), dim3(MRK_BLOCK), 0, s, a);
    CBA_HIP(hipGetLastError());
    h->readings.download(reinterpret_cast<MarkerReading*>(out), n_cells, s);
    tm.mark(1);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(ms);
}

// the 12 direction vectors of a corner of angle `angle`: direction 3 k + f at angle + pi/4 + k pi/2 + (f - 1) fan
void charuco_directions(double angle, double fan_deg, double* dirs) {
    const double fan = fan_deg * (GRID_PI / 180.0);
    for (int k = 0; k < 4; ++k)
        for (int f = 0; f < 3; ++f) {
            const double phi = angle + GRID_PI / 4 + k * (GRID_PI / 2) + (f - 1) * fan;
            dirs[2 * (3 * k + f)] = std::cos(phi);
            dirs[2 * (3 * k + f) + 1] = std::sin(phi);
        }
}

void charuco_detector_process(CharucoDetector* h, int n_images, const uint8_t* images, int32_t* out_count, int32_t* out_status,
                              int32_t* out_ids, double* out_xy, int32_t* out_n_markers, int32_t* out_n_corners, int32_t* out_n_cells,
                              int32_t* out_cells, cba_marker_reading* out_readings, double* stage_ms) {
    using clk = std::chrono::steady_clock;
    const auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    double cms[5] = {}, arms_ms = 0.0, read_ms = 0.0;
    const int mc = h->max_corners, nb = charuco_detector_board_corners(h);
    h->n_images = n_images;
    corner_detector_process(h->corners.get(), n_images, images, h->h_count.data(), h->h_status.data(), h->h_xy.data(), h->h_angle.data(),
                            nullptr, h->h_flags.data(), stage_ms ? cms : nullptr);
    const size_t slots = static_cast<size_t>(n_images) * mc;
    for (size_t i = 0; i < slots; ++i) {
        const bool kept = static_cast<int>(i % mc) < std::min(h->h_count[i / mc], mc);
        if (kept) charuco_directions(h->h_angle[i], h->opts.arm_fan_deg, &h->h_dirs[24 * i]);
        else std::fill(h->h_dirs.begin() + 24 * i, h->h_dirs.begin() + 24 * (i + 1), 0.0);
    }
    charuco_detector_arms(h, n_images, h->h_dirs.data(), h->h_score.data(), stage_ms ? &arms_ms : nullptr);
    const clk::time_point t_lattice = clk::now();
    // lattices and cells.  The good corners of image im are compacted for the host stages; the labels are kept per image slot
    std::vector<int32_t> comp(slots, -1), ij(2 * slots, 0), first_cell(n_images + 1, 0);
    int total = 0;  // true number of cells
    for (int im = 0; im < n_images; ++im) {
        const int kept = std::min(h->h_count[im], mc);
        int g = 0;
        for (int c = 0; c < kept; ++c) {
            const size_t i = static_cast<size_t>(im) * mc + c;
            if (h->h_flags[i] != 0 || !(h->h_score[i] >= h->opts.min_arm_contrast)) continue;
            h->h_good[g] = c;
            h->h_gxy[2 * g] = h->h_xy[2 * i]; h->h_gxy[2 * g + 1] = h->h_xy[2 * i + 1];
            h->h_gangle[g] = h->h_angle[i];
            ++g;
        }
        chessboard_lattice(g, h->h_gxy.data(), h->h_gangle.data(), h->opts.min_component, h->h_comp.data(), h->h_ij.data());
        for (int k = 0; k < g; ++k) {
            const size_t i = static_cast<size_t>(im) * mc + h->h_good[k];
            comp[i] = h->h_comp[k]; ij[2 * i] = h->h_ij[2 * k]; ij[2 * i + 1] = h->h_ij[2 * k + 1];
        }
        const int used = std::min(total, h->max_cells);
        const int m = lattice_cells(g, h->h_gxy.data(), h->h_comp.data(), h->h_ij.data(), h->max_cells - used, &h->h_cell[3 * static_cast<size_t>(used)],
                                    &h->h_quad[8 * static_cast<size_t>(used)]);
        first_cell[im] = used;
        total += m;
        const int now = std::min(total, h->max_cells);
        std::fill(h->h_cell_image.begin() + used, h->h_cell_image.begin() + now, im);
        if (out_status) out_status[im] = (h->h_status[im] ? CBA_CHARUCO_STATUS_CORNER_OVERFLOW : 0) | (total > h->max_cells && m > 0 ? CBA_CHARUCO_STATUS_CELL_OVERFLOW : 0);
        if (out_n_corners) out_n_corners[im] = h->h_count[im];
    }
    const int n_cells = std::min(total, h->max_cells);
    first_cell[n_images] = n_cells;
    const double lattice_ms = since(t_lattice);
    charuco_detector_read(h, n_cells, h->h_cell_image.data(), h->h_quad.data(), reinterpret_cast<cba_marker_reading*>(h->h_readings.data()),
                          stage_ms ? &read_ms : nullptr);
    const clk::time_point t_match = clk::now();
    // board indices
    const CharucoBoard cb{h->board.squares_x, h->board.squares_y};
    std::vector<int32_t> fl, id, rot, ids(nb);
    std::vector<double> oxy(2 * static_cast<size_t>(nb));
    for (int im = 0; im < n_images; ++im) {
        const int c0 = first_cell[im], m = first_cell[im + 1] - c0;
        fl.resize(m); id.resize(m); rot.resize(m);
        for (int t = 0; t < m; ++t) { fl[t] = h->h_readings[c0 + t].flags; id[t] = h->h_readings[c0 + t].id; rot[t] = h->h_readings[c0 + t].rotation; }
        int32_t nm = 0;
        const size_t base = static_cast<size_t>(im) * mc;
        const int count = charuco_match(cb, h->opts.min_markers, mc, &comp[base], &ij[2 * base], &h->h_xy[2 * base], m, &h->h_cell[3 * static_cast<size_t>(c0)],
                                        fl.data(), id.data(), rot.data(), ids.data(), oxy.data(), &nm);
        if (out_count) out_count[im] = count;
        if (out_n_markers) out_n_markers[im] = nm;
        if (out_ids) std::copy(ids.begin(), ids.end(), out_ids + static_cast<size_t>(im) * nb);
        if (out_xy) std::copy(oxy.begin(), oxy.end(), out_xy + 2 * static_cast<size_t>(im) * nb);
    }
    if (out_n_cells) *out_n_cells = total;
    if (stage_ms) {  // upload, response, peaks, refine, arms, host lattice, read, host match, download
        const double t[9] = {cms[0], cms[1], cms[2], cms[3], arms_ms, lattice_ms, read_ms, since(t_match), cms[4]};
        std::copy(t, t + 9, stage_ms);
    }
    for (int t = 0; t < n_cells; ++t) {
        if (out_cells) {
            out_cells[4 * t] = h->h_cell_image[t];
            for (int k = 0; k < 3; ++k) out_cells[4 * t + 1 + k] = h->h_cell[3 * static_cast<size_t>(t) + k];
        }
        if (out_readings) std::memcpy(&out_readings[t], &h->h_readings[t], sizeof(MarkerReading));
    }
}

void charuco_detector_destroy(CharucoDetector* h) noexcept { destroy_handle(h); }

}  // namespace cba
