// host_cloud.hpp — TEST-ONLY: the one host target of the drivers of tests/cloud_cpu and tests/align_cpu: the grid of a cloud, built by a
// counting sort with cloud_math.hpp's cell arithmetic (the points of a cell in index order), as the device's count, scan and scatter
// build it up to the order inside a cell.
#pragma once
#include <cstdint>
#include <vector>

#include "../calibration_amd/csrc/cloud_math.hpp"

namespace cba {

struct HostCloud {
    CloudGrid g;
    double extent = 0.0;
    int64_t n_cells = 0;
    std::vector<int32_t> start;
    std::vector<CloudRec> rec;
    std::vector<double> nrm;
    CloudTarget target() const { return CloudTarget{g, start.data(), rec.data(), nrm.empty() ? nullptr : nrm.data()}; }
};

// -> the grid plan's answer (0: built)
inline int host_build(int64_t n, const double* xyz, const double* normals, double cell, HostCloud* ix) {
    double fit;
    const int plan = cloud_plan_grid(n, xyz, cell, &ix->g, &ix->extent, &ix->n_cells, &fit);
    if (plan != 0) return plan;
    ix->start.assign(static_cast<size_t>(ix->n_cells) + 1, 0);
    std::vector<int32_t> cell_of(static_cast<size_t>(n), -1);
    int64_t n_valid = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double* p = xyz + 3 * i;
        if (!cloud_valid(p[0], p[1], p[2])) continue;
        cell_of[i] = cloud_point_cell(ix->g, p[0], p[1], p[2]);
        ++ix->start[static_cast<size_t>(cell_of[i]) + 1];
        ++n_valid;
    }
    for (int64_t c = 0; c < ix->n_cells; ++c) ix->start[c + 1] += ix->start[c];
    std::vector<int32_t> at(ix->start.begin(), ix->start.end() - 1);
    ix->rec.resize(static_cast<size_t>(n_valid));
    if (normals) ix->nrm.resize(3 * static_cast<size_t>(n_valid));
    for (int64_t i = 0; i < n; ++i) {
        if (cell_of[i] < 0) continue;
        const int32_t k = at[cell_of[i]]++;
        CloudRec r;
        r.x = xyz[3 * i]; r.y = xyz[3 * i + 1]; r.z = xyz[3 * i + 2]; r.idx = i;
        ix->rec[k] = r;
        if (normals)
            for (int j = 0; j < 3; ++j) ix->nrm[3 * static_cast<size_t>(k) + j] = normals[3 * i + j];
    }
    return 0;
}

}  // namespace cba
