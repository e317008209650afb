// ls_adapter_drive.cpp — TEST-ONLY driver of include/calibba_linescan.hpp (tests/test_linescan_adapter.py), compiled against the
// stand-ins under stand_ins/.  Reads a scene (text: 12 camera parameters, then n_views, then per view k m, k rows X Y u v and
// m rows u v) and prints the planes of calibrate_laser_plane for the three camera types, of the facade and of the RANSAC form.
#include <cstdio>
#include <fstream>
#include <iostream>

#include "calibba_linescan.hpp"

using namespace calib;

static void print(const char* tag, const Eigen::Vector4d& p, double rms) {
    std::printf("%s %.17g %.17g %.17g %.17g %.17g\n", tag, p[0], p[1], p[2], p[3], rms);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    double intr[12];
    for (double& x : intr) in >> x;
    int n_views = 0;
    in >> n_views;
    std::vector<LineScanView> views(static_cast<size_t>(n_views));
    for (auto& v : views) {
        int k = 0, m = 0;
        in >> k >> m;
        v.target_view.resize(static_cast<size_t>(k));
        for (auto& o : v.target_view) in >> o.object_xy[0] >> o.object_xy[1] >> o.image_uv[0] >> o.image_uv[1];
        v.laser_uv.resize(static_cast<size_t>(m));
        for (auto& p : v.laser_uv) in >> p[0] >> p[1];
    }
    if (!in) return 3;
    const CameraMatrix K{intr[0], intr[1], intr[2], intr[3], intr[4]};
    BrownConradyd bc;
    bc.coeffs = Eigen::VectorXd(5);
    for (int i = 0; i < 5; ++i) bc.coeffs[i] = intr[5 + i];
    const PinholeCamera<BrownConradyd> pin(K, bc);
    DualDistortion dual;
    dual.forward = bc.coeffs;
    dual.inverse = calibba_adapter::invert_brown_conrady(bc.coeffs);
    const PinholeCamera<DualDistortion> pin_dual(K, dual);
    const ScheimpflugCamera<PinholeCamera<BrownConradyd>> sch(pin, intr[10], intr[11]);

    const auto a = calibba_adapter::calibrate_laser_plane(views, pin);
    print("pinhole", a.plane, a.rms_error);
    const auto b = calibba_adapter::calibrate_laser_plane(views, pin_dual);
    print("dual", b.plane, b.rms_error);
    const auto c = calibba_adapter::calibrate_laser_plane(views, sch);
    print("scheimpflug", c.plane, c.rms_error);
    const auto run = calibba_adapter::LinescanCalibrationFacade().calibrate(pin, views);
    if (!run.success || run.used_views != views.size()) return 4;
    print("facade", run.result.plane, run.result.rms_error);
    LineScanPlaneFitOptions ro;
    ro.use_ransac = true;
    ro.ransac_options.thresh = 2e-3;
    ro.ransac_options.max_iters = 200;
    const auto r = calibba_adapter::calibrate_laser_plane(views, pin, ro);
    if (r.summary != "ransac") return 5;
    print("ransac", r.plane, r.rms_error);
    const auto pts = calibba_adapter::points_from_view(views[0], pin);
    if (pts.size() != views[0].laser_uv.size()) return 6;
    const Eigen::Vector4d p = calibba_adapter::fit_plane_svd(pts);
    print("view0_svd", p, 0.0);
    bool threw = false;
    try {
        (void)calibba_adapter::calibrate_laser_plane(std::vector<LineScanView>{views[0]}, pin);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) return 7;
    std::printf("ls_adapter_drive: all ok\n");
    return 0;
}
