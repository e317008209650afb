// tests/golden/gen_distortion_scenes.cpp — generator of tests/golden/distortion_scenes.json (TEST INFRASTRUCTURE).
//
// The scenes of the reference's DistortionTest (tests/unit/distortion_test.cpp:17-164), drawn from the SAME random stream the
// reference binary draws them from: generate_synthetic_data (:17-47) seeds std::mt19937(42), draws `Eigen::Vector2d xy{dist(rng),
// dist(rng)}` from uniform_real_distribution(-0.6, 0.6) (a braced list: left to right), then two normal_distribution(0, noise)
// draws (u first), which are made even at noise 0.  apply_distortion (distortion.h:91-116) and denormalize (camera_matrix.h:41-46)
// are restated in their operation order.
//
//   scene        reference test                               camera                   points  noise
//   exact_fit    ExactFit (:60-82)                            800, 800, 400, 300, 0    500     0
//   noisy_fit    NoisyFit (:84-107)                           800, 820, 400, 300, 0    1000    0.5
//   dual_model   DualModel (:109-127)                         800, 800, 400, 300, 0    200     0
//   fixed        RespectsFixedCoefficientConstraints (:129-151)  800, 800, 400, 300, 0  400     0
//   bad_index    ThrowsOnOutOfRangeFixedIndex (:153-164)      800, 800, 400, 300, 0    50      0   (p1 = p2 = 0)
// All use k = (-0.2, 0.05), p = (0.001, -0.0005) unless noted.  Rows are [x, y, u, v].
//
// Build + run:  g++ -O0 -std=c++20 -ffp-contract=off gen_distortion_scenes.cpp -o /tmp/gen_distortion_scenes && /tmp/gen_distortion_scenes > distortion_scenes.json
#include <cstdio>
#include <random>
#include <vector>

struct Obs {
    double x, y, u, v;
};

static std::vector<Obs> generate(const std::vector<double>& k, double p1, double p2, const double* K, int n, double noise_level) {
    std::mt19937 rng(42);
    std::uniform_real_distribution<double> dist(-0.6, 0.6);
    std::normal_distribution<double> noise(0.0, noise_level);
    std::vector<double> c(k);
    c.push_back(p1);
    c.push_back(p2);
    const int nr = static_cast<int>(k.size());
    std::vector<Obs> out;
    for (int i = 0; i < n; ++i) {
        const double xy[2]{dist(rng), dist(rng)};
        const double x = xy[0], y = xy[1];
        // apply_distortion
        const double r2 = x * x + y * y;
        double radial = 1.0, rpow = r2;
        for (int j = 0; j < nr; ++j) {
            radial += c[j] * rpow;
            rpow *= r2;
        }
        const double t1 = c[nr], t2 = c[nr + 1];
        const double xd = x * radial + 2.0 * t1 * x * y + t2 * (r2 + 2.0 * x * x);
        const double yd = y * radial + t1 * (r2 + 2.0 * y * y) + 2.0 * t2 * x * y;
        // denormalize: fx x + skew y + cx, fy y + cy
        double u = K[0] * xd + K[4] * yd + K[2];
        double v = K[1] * yd + K[3];
        u += noise(rng);
        v += noise(rng);
        out.push_back({x, y, u, v});
    }
    return out;
}

static void scene(const char* name, const double* K, const std::vector<Obs>& obs, bool last) {
    std::printf("\"%s\": {\"camera\": [%.17g, %.17g, %.17g, %.17g, %.17g], \"obs\": [", name, K[0], K[1], K[2], K[3], K[4]);
    for (size_t i = 0; i < obs.size(); ++i)
        std::printf("%s[%.17g, %.17g, %.17g, %.17g]", i ? ", " : "", obs[i].x, obs[i].y, obs[i].u, obs[i].v);
    std::printf("]}%s\n", last ? "" : ",");
}

int main() {
    const double K800[5] = {800.0, 800.0, 400.0, 300.0, 0.0};
    const double K820[5] = {800.0, 820.0, 400.0, 300.0, 0.0};
    const std::vector<double> k = {-0.2, 0.05};
    std::printf("{\n");
    scene("exact_fit", K800, generate(k, 0.001, -0.0005, K800, 500, 0.0), false);
    scene("noisy_fit", K820, generate(k, 0.001, -0.0005, K820, 1000, 0.5), false);
    scene("dual_model", K800, generate(k, 0.001, -0.0005, K800, 200, 0.0), false);
    scene("fixed", K800, generate(k, 0.001, -0.0005, K800, 400, 0.0), false);
    scene("bad_index", K800, generate(k, 0.0, 0.0, K800, 50, 0.0), true);
    std::printf("}\n");
    return 0;
}
