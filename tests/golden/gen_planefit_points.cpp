// gen_planefit_points.cpp — writes the 140 points of the reference's PlaneFit.RansacRejectsOutliers
// (tests/unit/planefit_test.cpp:24-46) as drawn by libstdc++'s std::mt19937(1337) and std::uniform_real_distribution: 100 points
// on the plane through (0, 0, 1) with normal (0.2, -0.3, 1), then 40 outliers in [5, 10)^3.  Output: tests/golden/planefit_points.txt
// (one "x y z" row per point, %.17g), the fixture tests/test_linescan_gpu.py reads.
//   g++ -std=c++17 -O2 tests/golden/gen_planefit_points.cpp -o /tmp/gen && /tmp/gen > tests/golden/planefit_points.txt
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

struct P {  // Eigen::Vector3d(x, y, z) stand-in: the three draws below are evaluated as the reference's are, by g++
    double x, y, z;
    P(double a, double b, double c) : x(a), y(b), z(c) {}
};

int main() {
    std::mt19937 rng(1337);
    std::uniform_real_distribution<double> dist_xy(-1.0, 1.0);
    // make_plane_from_point_normal({0, 0, 1}, (0.2, -0.3, 1)): unit normal, d = -n.p
    const double nn = std::sqrt(0.2 * 0.2 + 0.3 * 0.3 + 1.0);
    const double g[4] = {0.2 / nn, -0.3 / nn, 1.0 / nn, -(1.0 / nn)};
    for (int i = 0; i < 100; ++i) {
        const double x = dist_xy(rng);
        const double y = dist_xy(rng);
        const double z = (-g[3] - g[0] * x - g[1] * y) / g[2];
        std::printf("%.17g %.17g %.17g\n", x, y, z);
    }
    std::uniform_real_distribution<double> dist_out(5.0, 10.0);
    std::vector<P> out;
    for (int i = 0; i < 40; ++i) out.emplace_back(dist_out(rng), dist_out(rng), dist_out(rng));  // the reference's expression
    for (const P& p : out) std::printf("%.17g %.17g %.17g\n", p.x, p.y, p.z);
    return 0;
}
