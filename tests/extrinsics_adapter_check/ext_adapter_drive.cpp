// ext_adapter_drive.cpp — TEST-ONLY driver of include/calibba_extrinsics.hpp (tests/test_extrinsics_adapter.py).  Reads a rig scene
// (n_views n_cams, then per camera fx fy cx cy skew, then per view and camera a point count and that many "X Y u v" rows), runs
// estimate_extrinsic_dlt through the adapter with pinhole cameras and again with the same cameras wrapped as Scheimpflug cameras,
// and prints every pose at full precision ("CR c" / "RT v" + 12 numbers: R row-major, t).  Also checks the reference's two errors.
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>

#include "calib/models/pinhole.h"
#include "calib/models/scheimpflug.h"
#include "calibba_extrinsics.hpp"

using Cam = calib::PinholeCamera<calib::DualDistortion>;

static void print_pose(const char* tag, size_t i, const Eigen::Isometry3d& T) {
    std::printf("%s %zu", tag, i);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) std::printf(" %.17g", T.linear()(r, c));
    for (int k = 0; k < 3; ++k) std::printf(" %.17g", T.translation()[k]);
    std::printf("\n");
}

static bool same(const calib::ExtrinsicPoses& a, const calib::ExtrinsicPoses& b) {
    auto eq = [](const Eigen::Isometry3d& x, const Eigen::Isometry3d& y) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                if (x.linear()(r, c) != y.linear()(r, c)) return false;
        for (int k = 0; k < 3; ++k)
            if (x.translation()[k] != y.translation()[k]) return false;
        return true;
    };
    if (a.c_se3_r.size() != b.c_se3_r.size() || a.r_se3_t.size() != b.r_se3_t.size()) return false;
    for (size_t i = 0; i < a.c_se3_r.size(); ++i)
        if (!eq(a.c_se3_r[i], b.c_se3_r[i])) return false;
    for (size_t i = 0; i < a.r_se3_t.size(); ++i)
        if (!eq(a.r_se3_t[i], b.r_se3_t[i])) return false;
    return true;
}

template <class F>
static bool throws_runtime(F&& f, const std::string& msg) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return false;
    } catch (const std::runtime_error& e) {
        return msg == e.what();
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: ext_adapter_drive scene.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    size_t nv = 0, nc = 0;
    in >> nv >> nc;
    std::vector<Cam> cams(nc);
    for (auto& c : cams) in >> c.kmtx.fx >> c.kmtx.fy >> c.kmtx.cx >> c.kmtx.cy >> c.kmtx.skew;
    std::vector<calib::MulticamPlanarView> views(nv, calib::MulticamPlanarView(nc));
    for (auto& mv : views)
        for (auto& pv : mv) {
            size_t n = 0;
            in >> n;
            pv.resize(n);
            for (auto& o : pv) in >> o.object_xy.x() >> o.object_xy.y() >> o.image_uv.x() >> o.image_uv.y();
        }
    if (!in) { std::fprintf(stderr, "bad scene file\n"); return 2; }

    const calib::ExtrinsicPoses p = calibba_adapter::estimate_extrinsic_dlt(views, cams);
    for (size_t c = 0; c < p.c_se3_r.size(); ++c) print_pose("CR", c, p.c_se3_r[c]);
    for (size_t v = 0; v < p.r_se3_t.size(); ++v) print_pose("RT", v, p.r_se3_t[v]);

    std::vector<calib::ScheimpflugCamera<Cam>> sch;
    for (const auto& c : cams) sch.emplace_back(c, 0.02, -0.01);
    if (!same(p, calibba_adapter::estimate_extrinsic_dlt(views, sch))) { std::printf("ext_FAIL scheimpflug K differs\n"); return 1; }

    if (!throws_runtime([&] { calibba_adapter::estimate_extrinsic_dlt(std::vector<calib::MulticamPlanarView>{}, cams); },
                        "Empty views or cameras provided")) { std::printf("ext_FAIL empty views\n"); return 1; }
    if (!throws_runtime([&] { calibba_adapter::estimate_extrinsic_dlt(views, std::vector<Cam>{}); }, "Empty views or cameras provided")) {
        std::printf("ext_FAIL empty cameras\n");
        return 1;
    }
    auto bad = views;
    bad.back().pop_back();
    const std::string msg = "View " + std::to_string(nv - 1) + " has wrong number of cameras: expected " + std::to_string(nc) + ", got " +
                            std::to_string(nc - 1);
    if (!throws_runtime([&] { calibba_adapter::estimate_extrinsic_dlt(bad, cams); }, msg)) { std::printf("ext_FAIL camera count\n"); return 1; }
    std::printf("ext_adapter_drive: all ok\n");
    return 0;
}
