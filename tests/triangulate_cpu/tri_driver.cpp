// tri_driver.cpp — TEST-ONLY: extern "C" wrapper of tri_math.hpp for ctypes (tests/test_triangulate_cpu.py).  It builds the camera
// table as triangulate.hip's host glue does and runs tri_point, the function every lane of k_triangulate runs, in a plain loop.
#include <cstdint>
#include <vector>

#include "../../calibration_amd/csrc/tri_math.hpp"

using namespace cba;

extern "C" {

// the arguments of cba_triangulate (all outputs required) + linearisations [n]
void tri_points(int model, int n_cams, const double* intr, int n_inv, const double* inv, const double* c_T_r, int64_t n, const double* uv,
                const cba_triangulate_options* o, double* xyz, double* rms, uint32_t* mask, int32_t* status, double* cov6,
                int32_t* linearisations) {
    const int ni = model == CAM_SCHEIMPFLUG ? 12 : 10;
    std::vector<TriCamera> cams(n_cams);
    for (int c = 0; c < n_cams; ++c)
        tri_fill_camera(model, intr + c * ni, n_inv, inv ? inv + c * n_inv : nullptr, c_T_r + 7 * c, &cams[c]);
    for (int64_t i = 0; i < n; ++i) {
        TriResult r;
        if (model == CAM_SCHEIMPFLUG) tri_point<CAM_SCHEIMPFLUG, true>(cams.data(), n_cams, uv + 2 * i, 2 * n, *o, &r);
        else tri_point<CAM_PINHOLE_BC, true>(cams.data(), n_cams, uv + 2 * i, 2 * n, *o, &r);
        for (int j = 0; j < 3; ++j) xyz[3 * i + j] = r.X[j];
        for (int j = 0; j < 6; ++j) cov6[6 * i + j] = r.cov[j];
        rms[i] = r.rms;
        mask[i] = r.mask;
        status[i] = r.status;
        linearisations[i] = r.linearisations;
    }
}

}  // extern "C"
