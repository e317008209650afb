// df_adapter_drive.cpp — TEST-ONLY driver of include/calibba_distortion.hpp (tests/test_distortion_adapter.py).  Reads a scene
// file (line 1: fx fy cx cy skew, line 2: N, then N lines x y u v), calls every entry point of the header and prints tagged rows
// with %.17g, which the test compares with the Python API bit for bit.
#include <cstdio>
#include <fstream>
#include <stdexcept>

#include "calibba_distortion.hpp"

namespace cd = calibba_adapter;

static void row(const char* tag, const double* a, long n) {
    std::printf("%s", tag);
    for (long i = 0; i < n; ++i) std::printf(" %.17g", a[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    calib::CameraMatrix K;
    long n = 0;
    in >> K.fx >> K.fy >> K.cx >> K.cy >> K.skew >> n;
    std::vector<calib::Observation<double>> obs(static_cast<size_t>(n));
    for (auto& o : obs) in >> o.x >> o.y >> o.u >> o.v;

    auto f = cd::fit_distortion_full(obs, K, 2);
    if (!f) return 3;
    row("F", f->distortion.data(), f->distortion.size());
    row("FR", f->residuals.data(), f->residuals.size());
    const std::vector<int> idx = {0, 3};
    const std::vector<double> val = {-0.2};  // the second value is missing: 0
    auto fx = cd::fit_distortion(obs, K, 2, std::span<const int>(idx), std::span<const double>(val));
    if (!fx) return 4;
    row("FX", fx->distortion.data(), fx->distortion.size());
    auto d = cd::fit_distortion_dual(obs, K, 3);
    if (!d) return 5;
    row("DF", d->distortion.forward.data(), d->distortion.forward.size());
    row("DI", d->distortion.inverse.data(), d->distortion.inverse.size());
    auto k = cd::estimate_intrinsics_linear(obs);
    if (!k) return 6;
    const double k5[5] = {k->fx, k->fy, k->cx, k->cy, k->skew};
    row("L", k5, 5);
    auto it = cd::estimate_intrinsics_linear_iterative(obs, 2, 50, true);
    if (!it) return 7;
    const double i5[5] = {it->kmtx.fx, it->kmtx.fy, it->kmtx.cx, it->kmtx.cy, it->kmtx.skew};
    row("IK", i5, 5);
    row("IC", it->distortion.coeffs.data(), it->distortion.coeffs.size());
    const std::vector<calib::Observation<double>> few(obs.begin(), obs.begin() + 7);
    if (cd::fit_distortion_full(few, K, 2) || cd::fit_distortion_dual(few, K, 2) || cd::estimate_intrinsics_linear_iterative(few, 2))
        return 8;
    bool threw = false;
    try {
        const std::vector<int> bad = {7};
        (void)cd::fit_distortion_full(obs, K, 2, std::span<const int>(bad), std::span<const double>());
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) return 9;
    std::printf("df_adapter_drive: all ok\n");
    return 0;
}
