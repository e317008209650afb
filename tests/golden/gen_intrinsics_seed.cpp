// tests/golden/gen_intrinsics_seed.cpp — generator of tests/golden/intrinsics_seed_scenes.json (TEST INFRASTRUCTURE).
//
// The scenes of the reference's linear-seed tests, drawn from the SAME random streams the reference binary draws them from
// (libstdc++'s std::mt19937 and distributions, compiled with g++ like the reference's CI):
//
//   scene                    reference test                                                   stream
//   recovers_camera_matrix   tests/unit/intrinsics_estimate_test.cpp:11-55 (RecoversCameraMatrix)   RNG(10), SimulatedHandEye
//   too_few_views            tests/unit/intrinsics_estimate_test.cpp:57-82 (FailsWithTooFewViews)   RNG(5), SimulatedHandEye
//   exact_homography         tests/unit/homography_test.cpp:49-71 (ExactHomography)                 none
//   noisy_homography         tests/unit/homography_test.cpp:73-93 (NoisyHomography)                 mt19937(42), 50 points, noise 0.1
//   ransac_outliers          tests/unit/homography_test.cpp:103-133 (RansacRecoversHomography...)   mt19937(42) 100 exact + mt19937(7) 30
//   ransac_too_few_inliers   tests/unit/homography_test.cpp:136-160 (RansacFailsWithTooFewInliers)  mt19937(42) 4 exact + mt19937(3) 50
//
// SimulatedHandEye (utils.h) is restated as in gen_ref_scenes.cpp.  generate_synthetic_data (homography_test.cpp:20-46) draws
// `Vec2 point(dist(rng), dist(rng))` and `Vec2(noise(rng), noise(rng))`, whose argument evaluation order is unspecified; the same
// two-argument constructor calls are used here, so g++ makes the same choice for both.  H x is Eigen's (H * p.homogeneous())
// .hnormalized(), restated in its operation order.
//
// Build + run:  g++ -O0 -std=c++20 -ffp-contract=off -I../../oracle gen_intrinsics_seed.cpp -o /tmp/gen_intrinsics_seed && /tmp/gen_intrinsics_seed > intrinsics_seed_scenes.json
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numbers>
#include <random>
#include <string>
#include <vector>

#include "models.hpp"  // oracle/: project()

struct V3 {
    double x, y, z;
    V3(const double& a, const double& b, const double& c) : x(a), y(b), z(c) {}
};
struct Iso {  // R row-major, t
    double R[9], t[3];
};
static Iso identity() { return Iso{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}}; }
static Iso mul(const Iso& A, const Iso& B) {  // Eigen Isometry product: (A.R B.R, A.R B.t + A.t)
    Iso C;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) C.R[3 * i + j] = A.R[3 * i] * B.R[j] + A.R[3 * i + 1] * B.R[3 + j] + A.R[3 * i + 2] * B.R[6 + j];
        C.t[i] = A.R[3 * i] * B.t[0] + A.R[3 * i + 1] * B.t[1] + A.R[3 * i + 2] * B.t[2] + A.t[i];
    }
    return C;
}
static Iso inv(const Iso& A) {  // Transform<Isometry>::inverse(): (R^T, -R^T t)
    Iso C;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C.R[3 * i + j] = A.R[3 * j + i];
    for (int i = 0; i < 3; ++i) C.t[i] = -(C.R[3 * i] * A.t[0] + C.R[3 * i + 1] * A.t[1] + C.R[3 * i + 2] * A.t[2]);
    return C;
}
// axis_angle_to_R (utils.h:53-56): identity below 1e-16, else Eigen::AngleAxisd(angle, axis.normalized()).toRotationMatrix()
static void axis_angle_to_R(const V3& axis, double angle, double* R) {
    if (angle < 1e-16) { const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; for (int i = 0; i < 9; ++i) R[i] = I[i]; return; }
    const double n = std::sqrt(axis.x * axis.x + axis.y * axis.y + axis.z * axis.z);
    const double a[3] = {axis.x / n, axis.y / n, axis.z / n};
    // Eigen/src/Geometry/AngleAxis.h toRotationMatrix (third-party, restated)
    const double s = std::sin(angle), c = std::cos(angle);
    const double sa[3] = {s * a[0], s * a[1], s * a[2]}, ca[3] = {(1 - c) * a[0], (1 - c) * a[1], (1 - c) * a[2]};
    double tmp;
    tmp = ca[0] * a[1]; R[1] = tmp - sa[2]; R[3] = tmp + sa[2];
    tmp = ca[0] * a[2]; R[2] = tmp + sa[1]; R[6] = tmp - sa[1];
    tmp = ca[1] * a[2]; R[5] = tmp - sa[0]; R[7] = tmp + sa[0];
    R[0] = ca[0] * a[0] + c; R[4] = ca[1] * a[1] + c; R[8] = ca[2] * a[2] + c;
}
static Iso make_pose(const V3& t, const V3& axis, double angle) {  // utils.h:58-64
    Iso T = identity();
    axis_angle_to_R(axis, angle, T.R);
    T.t[0] = t.x; T.t[1] = t.y; T.t[2] = t.z;
    return T;
}
static double deg2rad(double d) { return d * std::numbers::pi / 180.0; }

struct RNG {  // utils.h:163-181: a fresh distribution object per draw
    std::mt19937 gen;
    explicit RNG(uint32_t seed) : gen(seed) {}
    double uni(double a, double b) {
        std::uniform_real_distribution<double> d(a, b);
        return d(gen);
    }
    V3 rand_unit_axis() {
        double z = uni(-1.0, 1.0);
        double t = uni(0.0, 2.0 * std::numbers::pi);
        double r = std::sqrt(1.0 - z * z);
        return V3(r * std::cos(t), r * std::sin(t), z);
    }
};

// SimulatedHandEye (utils.h:183-251)
struct Sim {
    Iso g_T_c, b_T_t;
    std::vector<double> cam;  // 10
    std::vector<Iso> b_T_g, c_T_t;
    std::vector<std::pair<double, double>> grid;
    std::vector<std::vector<double>> views;  // rows of X, Y, u, v
    void make_sequence(size_t n, RNG& rng) {
        Iso T = identity();
        for (size_t k = 0; k < n; ++k) {
            b_T_g.push_back(T);
            c_T_t.push_back(mul(mul(inv(g_T_c), inv(T)), b_T_t));
            if (k + 1 < n) {
                const double ang = deg2rad(rng.uni(5.0, 25.0));
                const V3 ax = rng.rand_unit_axis();
                const V3 dt(rng.uni(-0.10, 0.10), rng.uni(-0.10, 0.10), rng.uni(-0.10, 0.10));
                T = mul(T, make_pose(dt, ax, ang));
            }
        }
    }
    void make_target_grid(int rows, int cols, double spacing) {
        const double x0 = -0.5 * (cols - 1) * spacing, y0 = -0.5 * (rows - 1) * spacing;
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) grid.emplace_back(x0 + c * spacing, y0 + r * spacing);
    }
    void render_pixels() {
        for (const Iso& T : c_T_t) {
            std::vector<double> v;
            for (const auto& p : grid) {
                const double Pc[3] = {T.R[0] * p.first + T.R[1] * p.second + T.R[2] * 0.0 + T.t[0],
                                      T.R[3] * p.first + T.R[4] * p.second + T.R[5] * 0.0 + T.t[1],
                                      T.R[6] * p.first + T.R[7] * p.second + T.R[8] * 0.0 + T.t[2]};
                if (Pc[2] <= 1e-6) continue;
                double uv[2];
                orc::project(orc::PINHOLE_BC, cam.data(), Pc, uv);
                v.insert(v.end(), {p.first, p.second, uv[0], uv[1]});
            }
            views.push_back(v);
        }
    }
};

// ---- JSON ----------------------------------------------------------------------------------------------------------
static std::string num(double v) { char b[40]; std::snprintf(b, sizeof b, "%.17g", v); return b; }
static std::string arr(const std::vector<double>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + num(v[i]);
    return s + "]";
}
static std::string mat4(const Iso& T) {
    std::string s = "[";
    for (int i = 0; i < 3; ++i) s += "[" + num(T.R[3 * i]) + "," + num(T.R[3 * i + 1]) + "," + num(T.R[3 * i + 2]) + "," + num(T.t[i]) + "],";
    return s + "[0,0,0,1]]";
}
static std::string view_json(const std::vector<double>& v) {
    std::string s = "[";
    for (size_t i = 0; i + 3 < v.size(); i += 4) s += (i ? "," : "") + arr({v[i], v[i + 1], v[i + 2], v[i + 3]});
    return s + "]";
}
static std::vector<double> cam10(double fx, double fy, double cx, double cy, double skew, std::vector<double> dist = {0, 0, 0, 0, 0}) {
    std::vector<double> c = {fx, fy, cx, cy, skew};
    c.insert(c.end(), dist.begin(), dist.end());
    return c;
}


struct V2 {
    double x, y;
    V2(const double& a, const double& b) : x(a), y(b) {}
};
static V2 apply_h(const double* H, const V2& p) {  // (H * p.homogeneous()).hnormalized()
    const double q0 = H[0] * p.x + H[1] * p.y + H[2] * 1.0, q1 = H[3] * p.x + H[4] * p.y + H[5] * 1.0, q2 = H[6] * p.x + H[7] * p.y + H[8] * 1.0;
    return V2(q0 / q2, q1 / q2);
}
// generate_synthetic_data (homography_test.cpp:20-46): rows X, Y, u, v
static std::vector<double> synthetic(double* H, int n, double noise_level) {
    const double angle = 0.1, c = std::cos(angle), s = std::sin(angle), tx = 10.0, ty = -5.0;
    const double Ht[9] = {c, -s, tx, s, c, ty, 0.001, -0.002, 1.0};
    for (int i = 0; i < 9; ++i) H[i] = Ht[i];
    std::mt19937 rng(42);
    std::uniform_real_distribution<double> dist(-100.0, 100.0);
    std::normal_distribution<double> noise(0.0, noise_level > 0 ? noise_level : 1.0);  // only drawn from when noise_level > 0
    std::vector<double> v;
    for (int i = 0; i < n; ++i) {
        const V2 point(dist(rng), dist(rng));
        V2 pixel = apply_h(H, point);
        if (noise_level > 0) {
            const V2 d(noise(rng), noise(rng));
            pixel.x += d.x;
            pixel.y += d.y;
        }
        v.insert(v.end(), {point.x, point.y, pixel.x, pixel.y});
    }
    return v;
}
static void add_outliers(std::vector<double>& v, uint32_t seed, int n) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> dist(-100.0, 100.0);
    for (int i = 0; i < n; ++i) {
        const V2 src(dist(rng), dist(rng));
        const V2 dst(dist(rng), dist(rng));
        v.insert(v.end(), {src.x, src.y, dst.x, dst.y});
    }
}
static std::string h_json(const double* H) {
    return "[" + arr({H[0], H[1], H[2]}) + "," + arr({H[3], H[4], H[5]}) + "," + arr({H[6], H[7], H[8]}) + "]";
}

static std::string scene_sim(uint32_t seed, size_t n, int rows, int cols, double spacing, std::vector<double> cam, const char* ref) {
    RNG rng(seed);
    Sim sim{identity(), make_pose(V3(0.0, 0.0, 2.0), V3(0, 0, 1), 0.0), cam};
    sim.make_sequence(n, rng);
    sim.make_target_grid(rows, cols, spacing);
    sim.render_pixels();
    std::string s = "{\"views\":[";
    for (size_t i = 0; i < sim.views.size(); ++i) s += (i ? "," : "") + view_json(sim.views[i]);
    s += "],\"c_T_t\":[";
    for (size_t i = 0; i < sim.c_T_t.size(); ++i) s += (i ? "," : "") + mat4(sim.c_T_t[i]);
    s += "],\"cam_gt\":" + arr(sim.cam) + ",\"seed\":" + std::to_string(seed) + ",\"ref\":\"" + ref + "\"}";
    return s;
}

static std::string scene_h(const std::vector<double>& v, const double* H, const std::string& opts, const char* ref) {
    return "{\"view\":" + view_json(v) + ",\"H_true\":" + h_json(H) + (opts.empty() ? "" : ",\"ransac\":" + opts) + ",\"ref\":\"" + ref + "\"}";
}

int main() {
    std::printf("{\"recovers_camera_matrix\":%s,\n",
                scene_sim(10, 8, 6, 9, 0.03, cam10(900, 920, 640, 360, 0.0), "tests/unit/intrinsics_estimate_test.cpp:11-55").c_str());
    std::printf("\"too_few_views\":%s,\n",
                scene_sim(5, 3, 5, 7, 0.04, cam10(800, 805, 320, 240, 0.0), "tests/unit/intrinsics_estimate_test.cpp:57-82").c_str());
    {
        const double H[9] = {1, 0, 10.0, 0, 1, -5.0, 0, 0, 1};
        std::vector<double> v;
        for (const V2& p : {V2(0.0, 0.0), V2(1.0, 0.0), V2(0.0, 1.0), V2(1.0, 1.0)}) {
            const V2 q = apply_h(H, p);
            v.insert(v.end(), {p.x, p.y, q.x, q.y});
        }
        std::printf("\"exact_homography\":%s,\n", scene_h(v, H, "", "tests/unit/homography_test.cpp:49-71").c_str());
    }
    double H[9];
    std::vector<double> v = synthetic(H, 50, 0.1);
    std::printf("\"noisy_homography\":%s,\n", scene_h(v, H, "", "tests/unit/homography_test.cpp:73-93").c_str());
    v = synthetic(H, 100, 0.0);
    add_outliers(v, 7, 30);
    std::printf("\"ransac_outliers\":%s,\n",
                scene_h(v, H, "{\"max_iters\":1000,\"thresh\":1.0,\"min_inliers\":90,\"seed\":123,\"refit_on_inliers\":true}",
                        "tests/unit/homography_test.cpp:103-133").c_str());
    v = synthetic(H, 4, 0.0);
    add_outliers(v, 3, 50);
    std::printf("\"ransac_too_few_inliers\":%s}\n",
                scene_h(v, H, "{\"max_iters\":1000,\"thresh\":0.5,\"min_inliers\":10,\"seed\":42,\"refit_on_inliers\":true}",
                        "tests/unit/homography_test.cpp:136-160").c_str());
    return 0;
}
