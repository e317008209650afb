// laser_scan_driver.cpp — TEST-ONLY: extern "C" wrapper of laser_scan_math.hpp for ctypes (tests/test_laser_scan_cpu.py).  It fills
// the camera and plane as laser_scan.hip's host glue does, walks every line start to end with laser_line (the one-pass form that every
// split of the kernels must reproduce) and puts the pixels on the plane with laser_point, the function every lane runs.
#include <cstdint>
#include <vector>

#include "../../calibration_amd/csrc/laser_scan_math.hpp"

using namespace cba;

extern "C" {

// the arguments of cba_laser_points
void ls_points(int model, const double* intr, int n_inv, const double* inv, const double* plane, int64_t n, const double* uv, int n_frames,
               const int64_t* frame_offset, const double* frame_pose7, double* xyz, double* plane_xy) {
    LaserGeom g;
    laser_fill_geom(model, intr, n_inv, inv, plane, &g);
    for (int64_t i = 0; i < n; ++i) {
        double Rt[12];
        const double* rt = nullptr;
        if (frame_pose7) {
            int f = 0;
            if (frame_offset)
                while (f + 1 < n_frames && !(frame_offset[f] <= i && i < frame_offset[f + 1])) ++f;
            laser_pose_rt(frame_pose7 + 7 * f, Rt);
            rt = Rt;
        }
        laser_point(g, uv[2 * i], uv[2 * i + 1], rt, xyz + 3 * i, plane_xy ? plane_xy + 2 * i : nullptr);
    }
}

// cba_laser_scanner_create + _process in one call: images [n_frames][H][W] of uint8 (dtype 0) or float32 (1); ROI [pb, pe) resolved
void ls_scan(int model, const double* intr, int n_inv, const double* inv, const double* plane, int W, int H, int axis, int pb, int pe,
             int half_window, double floor_level, double min_peak, int n_frames, int dtype, const void* images, const double* frame_pose7,
             double* centre, double* amplitude, double* width_px, double* xyz) {
    LaserGeom g;
    laser_fill_geom(model, intr, n_inv, inv, plane, &g);
    const int n_lines = axis == 0 ? W : H;
    const int64_t stride = axis == 0 ? W : 1;
    const int hw = half_window < 32768 ? half_window : 32768;
    for (int f = 0; f < n_frames; ++f) {
        double Rt[12];
        if (frame_pose7) laser_pose_rt(frame_pose7 + 7 * f, Rt);
        for (int l = 0; l < n_lines; ++l) {
            const int64_t first = static_cast<int64_t>(f) * W * H + (axis == 0 ? l : static_cast<int64_t>(l) * W);
            double out[3];
            if (dtype == 0) laser_line(static_cast<const uint8_t*>(images) + first, stride, pb, pe, hw, floor_level, min_peak, out);
            else laser_line(static_cast<const float*>(images) + first, stride, pb, pe, hw, floor_level, min_peak, out);
            const int64_t line = static_cast<int64_t>(f) * n_lines + l;
            centre[line] = out[0];
            amplitude[line] = out[1];
            width_px[line] = out[2];
            const double u = axis == 0 ? l : out[0], v = axis == 0 ? out[0] : l;
            laser_point(g, u, v, frame_pose7 ? Rt : nullptr, xyz + 3 * line, nullptr);
        }
    }
}

}  // extern "C"
