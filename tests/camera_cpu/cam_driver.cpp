// cam_driver.cpp — TEST-ONLY: extern "C" wrappers of camera_math.hpp for ctypes (tests/test_camera_cpu.py).  Each wrapper runs the
// per-point / per-pixel function the kernels of camera.hip run, in a plain loop.
#include <cstdint>
#include <cstring>

#include "../../calibration_amd/csrc/camera_math.hpp"

using namespace cba;

extern "C" {

void cam_project(int model, const double* intr, int64_t n, const double* xyz, double* uv) {
    double in[12], sd[SD_SIZE];
    ls_fill_intr(model, intr, in, sd);
    for (int64_t i = 0; i < n; ++i) {
        const double* p = xyz + 3 * i;
        if (model == CAM_SCHEIMPFLUG) cam_project<CAM_SCHEIMPFLUG>(in, sd, p[0], p[1], p[2], uv + 2 * i, uv + 2 * i + 1);
        else cam_project<CAM_PINHOLE_BC>(in, sd, p[0], p[1], p[2], uv + 2 * i, uv + 2 * i + 1);
    }
}

void cam_unproject(int model, const double* intr, int n_inv, const double* inv, int64_t n, const double* uv, double* xy) {
    LsCamera c;
    ls_fill_camera(model, intr, n_inv, inv, &c);
    for (int64_t i = 0; i < n; ++i) ls_unproject(c, uv[2 * i], uv[2 * i + 1], xy + 2 * i, xy + 2 * i + 1);
}

// ls_fill_camera on an LsCamera whose every byte was 0xff before (a NaN in each double), member by member; sd_ref: scheimpflug_consts
// of the 12 numbers the camera ends up with
void cam_fill_camera(int model, const double* intr, int n_inv, const double* inv, int* model_out, int* n_inv_out, double* intr12,
                     double* inv16, double* sd, double* sd_ref) {
    LsCamera c;
    std::memset(&c, 0xff, sizeof(c));
    ls_fill_camera(model, intr, n_inv, inv, &c);
    *model_out = c.model;
    *n_inv_out = c.n_inv;
    std::memcpy(intr12, c.intr, sizeof(c.intr));
    std::memcpy(inv16, c.inv, sizeof(c.inv));
    std::memcpy(sd, c.sd, sizeof(c.sd));
    scheimpflug_consts(c.intr, sd_ref);
}

// maps [n_cams][H][W] of cameras intr [n_cams][10 | 12], R [n_cams][9] or NULL, new_k5 [n_cams][5] or NULL
void cam_map(int model, int n_cams, const double* intr, const double* R, const double* kp, int W, int H, float* mx, float* my) {
    const int ni = cam_intr_size(model);
    for (int c = 0; c < n_cams; ++c) {
        CamMapCam k{};
        ls_fill_intr(model, intr + c * ni, k.intr, k.sd);
        for (int j = 0; j < 9; ++j) k.R[j] = R ? R[9 * c + j] : (j % 4 == 0 ? 1.0 : 0.0);
        for (int j = 0; j < 5; ++j) k.kp[j] = kp ? kp[5 * c + j] : k.intr[j];
        for (int v = 0; v < H; ++v)
            for (int u = 0; u < W; ++u) {
                const int64_t o = (static_cast<int64_t>(c) * H + v) * W + u;
                if (model == CAM_SCHEIMPFLUG) cam_map_pixel<CAM_SCHEIMPFLUG>(k, u, v, mx + o, my + o);
                else cam_map_pixel<CAM_PINHOLE_BC>(k, u, v, mx + o, my + o);
            }
    }
}

// one image through one map (W x H), dtype 0: uint8, 1: float32
void cam_apply(int dtype, const void* src, int sw, int sh, int ch, const float* mx, const float* my, int W, int H, double border,
               void* dst) {
    for (int64_t p = 0; p < static_cast<int64_t>(W) * H; ++p) {
        if (dtype == 0) {
            const double b = std::nearbyint(border);
            const uint8_t b8 = std::isnan(border) ? 0 : static_cast<uint8_t>(b < 0.0 ? 0.0 : (b > 255.0 ? 255.0 : b));
            cam_remap_u8(static_cast<const uint8_t*>(src), sw, sh, ch, mx[p], my[p], b8, static_cast<uint8_t*>(dst) + p * ch);
        } else {
            cam_remap_f32(static_cast<const float*>(src), sw, sh, ch, mx[p], my[p], static_cast<float>(border),
                          static_cast<float*>(dst) + p * ch);
        }
    }
}

}  // extern "C"
