// cam_adapter_drive.cpp — TEST-ONLY driver of include/calibba_camera.hpp (tests/test_camera_adapter.py).  Builds three cameras of
// fixed parameters, calls every entry point of the header on fixed points and prints tagged rows with %.17g, which the test compares
// with the Python API bit for bit.
#include <cstdio>
#include <stdexcept>

#include "calibba_camera.hpp"

namespace ca = calibba_adapter;

static void rows(const char* tag, const std::vector<Eigen::Vector2d>& v) {
    std::printf("%s", tag);
    for (const auto& p : v) std::printf(" %.17g %.17g", p.x(), p.y());
    std::printf("\n");
}

static Eigen::VectorXd vec(std::initializer_list<double> l) {
    Eigen::VectorXd v(static_cast<Eigen::Index>(l.size()));
    Eigen::Index i = 0;
    for (double x : l) v[i++] = x;
    return v;
}

int main() {
    calib::PinholeCamera<calib::BrownConradyd> bc;
    bc.kmtx = {800.0, 780.0, 640.0, 480.0, 0.4};
    bc.distortion.coeffs = vec({-0.21, 0.08, -0.012, 0.0011, -0.0007});
    calib::PinholeCamera<calib::DualDistortion> dual;
    dual.kmtx = {800.0, 780.0, 640.0, 480.0, 0.0};
    dual.distortion.forward = vec({-0.2, 0.05, 0.001, -0.0005});
    dual.distortion.inverse = vec({0.2, 0.07, -0.001, 0.0005});
    calib::ScheimpflugCamera<calib::PinholeCamera<calib::BrownConradyd>> sc;
    sc.camera = bc;
    sc.tau_x = 0.2;
    sc.tau_y = -0.2;

    const std::vector<Eigen::Vector3d> xyz = {{0.1, -0.2, 1.0}, {-0.3, 0.25, 2.0}, {0.0, 0.0, 1.5}};
    const std::vector<Eigen::Vector2d> nxy = {{0.1, -0.2}, {-0.15, 0.125}};
    rows("PB", ca::project(bc, xyz));
    rows("PD", ca::project(dual, xyz));
    rows("PS", ca::project(sc, xyz));
    rows("PN", ca::project(bc, nxy));
    const auto uv = ca::project(bc, xyz);
    rows("UB", ca::unproject(bc, uv));
    rows("UD", ca::unproject(dual, ca::project(dual, xyz)));
    rows("US", ca::unproject(sc, ca::project(sc, xyz)));
    rows("DB", ca::distort(bc, nxy));
    rows("XB", ca::undistort(bc, ca::distort(bc, nxy)));
    rows("XD", ca::undistort(dual, ca::distort(dual, nxy)));
    {
        ca::UndistortMap m(std::vector<calib::PinholeCamera<calib::BrownConradyd>>{bc, bc}, 64, 48, {}, {500.0, 500.0, 32.0, 24.0, 0.0,
                                                                                                    600.0, 600.0, 31.5, 23.5, 0.0});
        std::vector<float> mx, my;
        m.maps(mx, my);
        std::printf("MAP %.9g %.9g %.9g %.9g\n", mx[0], my[0], mx[64 * 48 + 100], my[64 * 48 + 100]);
        std::vector<uint8_t> img(2 * 48 * 64 * 3);
        for (size_t i = 0; i < img.size(); ++i) img[i] = static_cast<uint8_t>((i * 37) % 251);
        const auto out = m.apply(img, {0, 1}, 64, 48, 3, 9.0);
        unsigned long sum = 0;
        for (uint8_t b : out) sum += b;
        std::printf("APPLY %zu %lu\n", out.size(), sum);
    }
    bool threw = false;
    try {
        calib::PinholeCamera<calib::BrownConradyd> bad = bc;
        bad.distortion.coeffs = vec({0.1, 0.2, 0.3});
        (void)ca::project(bad, xyz);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) return 9;
    std::printf("cam_adapter_drive: all ok\n");
    return 0;
}
