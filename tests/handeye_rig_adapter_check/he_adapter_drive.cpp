// he_adapter_drive.cpp — TEST-ONLY driver of include/calibba_handeye_rig.hpp (tests/test_handeye_rig_adapter.py).  Reads a rig
// (n_cams, per camera fx fy cx cy skew, n_obs, then per observation: camera, b_T_g as 12 numbers (R row-major, t), a point count and
// that many "X Y u v" rows), runs estimate_bundle_seed through the adapter and prints every pose at full precision ("G c" / "T" + 12
// numbers: R row-major, t), the statuses ("S c status pairs") and the target source.  Also checks the given / config paths and the
// argument error.
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>

#include "calib/models/pinhole.h"
#include "calibba_handeye_rig.hpp"

using Cam = calib::PinholeCamera<calib::DualDistortion>;

static void print_pose(const char* tag, const Eigen::Isometry3d& T) {
    std::printf("%s", tag);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) std::printf(" %.17g", T.linear()(r, c));
    for (int k = 0; k < 3; ++k) std::printf(" %.17g", T.translation()[k]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    size_t n_cams = 0, n_obs = 0;
    in >> n_cams;
    std::vector<Cam> cams(n_cams);
    for (auto& c : cams) in >> c.kmtx.fx >> c.kmtx.fy >> c.kmtx.cx >> c.kmtx.cy >> c.kmtx.skew;
    in >> n_obs;
    std::vector<calib::BundleObservation> obs(n_obs);
    for (auto& o : obs) {
        in >> o.camera_index;
        o.b_se3_g = Eigen::Isometry3d::Identity();
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) in >> o.b_se3_g.linear()(r, c);
        for (int k = 0; k < 3; ++k) in >> o.b_se3_g.translation()[k];
        size_t n = 0;
        in >> n;
        o.view.resize(n);
        for (auto& p : o.view) in >> p.object_xy.x() >> p.object_xy.y() >> p.image_uv.x() >> p.image_uv.y();
    }
    if (!in) return 3;
    const auto s = calibba_adapter::estimate_bundle_seed(obs, cams, 1.0);
    for (size_t c = 0; c < n_cams; ++c) {
        print_pose(("G " + std::to_string(c)).c_str(), s.g_se3_c[c]);
        std::printf("S %zu %d %d\n", c, s.status[c], s.pairs[c]);
    }
    print_pose("T", s.b_se3_t);
    std::printf("SRC %s FAILED %d\n", s.target_source.c_str(), s.failed ? 1 : 0);
    // the given and config paths: camera 0's hand-eye and the target are copied
    std::vector<std::optional<Eigen::Isometry3d>> he(n_cams);
    he[0] = s.g_se3_c[0];
    const auto g = calibba_adapter::estimate_bundle_seed(obs, cams, 1.0, he, s.b_se3_t);
    bool ok = g.status[0] == CBA_HANDEYE_GIVEN && g.target_source == "config";
    for (int k = 0; k < 3; ++k) ok = ok && std::abs(g.g_se3_c[0].translation()[k] - s.g_se3_c[0].translation()[k]) <= 1e-15;
    bool threw = false;
    try {
        calibba_adapter::estimate_bundle_seed(obs, cams, 1.0, std::vector<std::optional<Eigen::Isometry3d>>(n_cams + 1));
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    bool threw_angle = false;
    try {
        calibba_adapter::estimate_bundle_seed(obs, cams, -1.0);
    } catch (const std::invalid_argument&) {
        threw_angle = true;
    }
    if (!ok || !threw || !threw_angle) {
        std::printf("he_adapter_drive: FAILED given/config %d, size error %d, angle error %d\n", ok, threw, threw_angle);
        return 1;
    }
    std::printf("he_adapter_drive: all ok\n");
    return 0;
}
