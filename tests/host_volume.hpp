// host_volume.hpp — TEST-ONLY: the one host copy of a TSDF volume for the drivers of tests/fusion_cpu, tests/mesh_cpu and
// tests/raycast_cpu.  The volume is kept as the device keeps it ({D, W} pairs in rows of an even pitch); the padding voxel of an odd
// row is poisoned with NaN, so that a rule that read it would show in what the tests compare.
#pragma once
#include <cstdint>
#include <limits>
#include <vector>

#include "../calibration_amd/csrc/tsdf_math.hpp"

namespace cba {

struct HostVolume {
    TsdfGrid g;
    std::vector<float> vol;  // exactly the stored volume: a read past it is the sanitizer's to find
    // D, W [nz][ny][nx]: the dense planes; NULL: the empty volume's D = 1, W = 0
    HostVolume(int nx, int ny, int nz, const double* origin, double vs, const float* D, const float* W) {
        g.nx = nx; g.ny = ny; g.nz = nz; g.pitch = (nx + 1) & ~1;
        for (int c = 0; c < 3; ++c) g.o[c] = origin[c];
        g.vs = vs;
        vol.assign(2 * static_cast<size_t>(g.pitch) * ny * nz, std::numeric_limits<float>::quiet_NaN());
        for (int64_t l = 0; l < static_cast<int64_t>(nx) * ny * nz; ++l) {
            int i, j, k;
            tsdf_voxel_of(g, l, &i, &j, &k);
            vol[tsdf_at(g, i, j, k)] = D ? D[l] : 1.0f;
            vol[tsdf_at(g, i, j, k) + 1] = W ? W[l] : 0.0f;
        }
    }
    void planes(float* D, float* W) const {
        for (int64_t l = 0; l < static_cast<int64_t>(g.nx) * g.ny * g.nz; ++l) {
            int i, j, k;
            tsdf_voxel_of(g, l, &i, &j, &k);
            D[l] = vol[tsdf_at(g, i, j, k)];
            W[l] = vol[tsdf_at(g, i, j, k) + 1];
        }
    }
};

}  // namespace cba
