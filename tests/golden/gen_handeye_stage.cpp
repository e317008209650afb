// tests/golden/gen_handeye_stage.cpp — generator of tests/golden/handeye_stage_scenes.json (TEST INFRASTRUCTURE).
//
// The synthetic rig of the reference's pipeline-stage tests, make_synthetic_handeye_data (tests/unit/pipeline_stages_test.cpp:44-81),
// drawn from the reference binary's own random stream: std::mt19937 + a fresh std::uniform_real_distribution<double> per draw
// (tests/unit/utils.h:163-181), libstdc++, RNG(17).  Camera fx 750, fy 760, cx 640, cy 360, no distortion; g_se3_c = pose
// ((0.05, -0.02, 0.1), y axis, 5 deg); b_se3_t = pose((0.4, 0.1, 0.8), z axis, -8 deg) — utils.h's axis_angle_to_R returns the
// identity for a negative angle, so b_se3_t has no rotation, as in the reference; 12 robot poses (SimulatedHandEye::make_sequence);
// a 6 x 8 grid at 0.03 m; no pixel noise; views with >= 16 points kept.  Used by HandEyeCalibrationStageTest.CalibratesSyntheticHandEye
// and BundleAdjustmentStageTest.CalibratesSyntheticBundle (pipeline_stages_test.cpp:265-372).  The pose helpers, the RNG and the
// simulator are the same restatements as gen_ref_scenes.cpp's (no reference source is copied).
//
// Build + run:  g++ -O0 -std=c++20 -ffp-contract=off -I../../oracle gen_handeye_stage.cpp -o /tmp/gen_handeye_stage && /tmp/gen_handeye_stage > handeye_stage_scenes.json
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
static std::string scene_handeye_stage() {
    RNG rng(17);
    Sim sim{make_pose(V3(0.05, -0.02, 0.1), V3(0.0, 1.0, 0.0), deg2rad(5.0)), make_pose(V3(0.4, 0.1, 0.8), V3(0.0, 0.0, 1.0), deg2rad(-8.0)),
            {750.0, 760.0, 640.0, 360.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    sim.make_sequence(12, rng);
    sim.make_target_grid(6, 8, 0.03);
    sim.render_pixels();
    std::string obs = "[";
    bool first = true;
    for (size_t i = 0; i < sim.views.size(); ++i) {
        if (sim.views[i].size() / 4 < 16) continue;  // copy_if view.size() >= 16
        obs += std::string(first ? "" : ",") + "{\"view\":" + view_json(sim.views[i]) + ",\"b_T_g\":" + mat4(sim.b_T_g[i]) + ",\"cam\":0}";
        first = false;
    }
    obs += "]";
    return "{\"kind\":\"handeye_stage\",\"obs\":" + obs + ",\"camera\":" + arr(sim.cam) + ",\"g_T_c_gt\":" + mat4(sim.g_T_c) +
           ",\"b_T_t_gt\":" + mat4(sim.b_T_t) + ",\"min_angle_deg\":1.0,\"handeye_max_iterations\":50,\"bundle_max_iterations\":60" +
           ",\"seed\":17,\"ref\":\"tests/unit/pipeline_stages_test.cpp:44-81, 265-372\"}";
}

int main() {
    std::printf("{\"synthetic_handeye\":%s}\n", scene_handeye_stage().c_str());
    return 0;
}
