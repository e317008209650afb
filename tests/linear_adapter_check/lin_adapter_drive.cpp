// lin_adapter_drive.cpp — TEST-ONLY driver of include/calibba_linear.hpp (tests/test_linear_adapter.py), compiled against the
// stand-ins under stand_ins/.  Reads a scene (text: n_views, then per view k and k rows X Y u v) and prints what the adapter's
// four entry points return for it.
#include <cstdio>
#include <fstream>

#include "calibba_linear.hpp"

using namespace calib;

static void print_h(const Eigen::Matrix3d& H) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) std::printf(" %.17g", H(r, c));
}
static void print_pose(const Eigen::Isometry3d& T) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) std::printf(" %.17g", T.linear()(r, c));
    for (int r = 0; r < 3; ++r) std::printf(" %.17g", T.translation()[r]);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int n_views = 0;
    in >> n_views;
    std::vector<PlanarView> views(static_cast<size_t>(n_views));
    for (auto& v : views) {
        int k = 0;
        in >> k;
        v.resize(static_cast<size_t>(k));
        for (auto& o : v) in >> o.object_xy[0] >> o.object_xy[1] >> o.image_uv[0] >> o.image_uv[1];
    }
    int bad = 0;
    // estimate_intrinsics, DLT homographies
    const IntrinsicsEstimateResult r = calibba_adapter::estimate_intrinsics(views);
    std::printf("K %d %.17g %.17g %.17g %.17g %.17g\n", r.success ? 1 : 0, r.kmtx.fx, r.kmtx.fy, r.kmtx.cx, r.kmtx.cy, r.kmtx.skew);
    std::vector<HomographyResult> hs;
    for (const auto& ve : r.views) {
        std::printf("V %zu %zu %.17g", ve.view_index, ve.homography.inliers.size(), ve.forward_rms_px);
        print_h(ve.homography.hmtx);
        print_pose(ve.c_se3_t);
        std::printf("\n");
        hs.push_back(ve.homography);
    }
    // estimate_intrinsics, RANSAC homographies and bounds
    IntrinsicsEstimOptions o;
    RansacOptions ro;
    ro.max_iters = 200;
    o.homography_ransac = ro;
    o.bounds = CalibrationBounds{};
    const IntrinsicsEstimateResult rr = calibba_adapter::estimate_intrinsics(views, o);
    std::printf("KR %d %.17g %.17g %.17g %.17g %.17g\n", rr.success ? 1 : 0, rr.kmtx.fx, rr.kmtx.fy, rr.kmtx.cx, rr.kmtx.cy, rr.kmtx.skew);
    std::printf("KR_log %s\n", rr.log.empty() ? "-" : "sanitized");
    for (const auto& ve : rr.views) std::printf("VR %zu %zu %.17g\n", ve.view_index, ve.homography.inliers.size(), ve.forward_rms_px);
    // estimate_homography of view 0, both forms
    for (int use : {0, 1}) {
        const HomographyResult h = calibba_adapter::estimate_homography(views[0], use ? std::optional<RansacOptions>(ro) : std::nullopt);
        std::printf("H%d %d %zu %.17g", use, h.success ? 1 : 0, h.inliers.size(), h.symmetric_rms_px);
        print_h(h.hmtx);
        std::printf("\n");
    }
    // zhang_intrinsics_from_hs over the DLT homographies; fewer than 4 fails
    const auto z = calibba_adapter::zhang_intrinsics_from_hs(hs);
    std::printf("Z %d %.17g %.17g %.17g %.17g %.17g\n", z ? 1 : 0, z ? z->fx : 0.0, z ? z->fy : 0.0, z ? z->cx : 0.0, z ? z->cy : 0.0,
                z ? z->skew : 0.0);
    if (calibba_adapter::zhang_intrinsics_from_hs(std::vector<HomographyResult>(hs.begin(), hs.begin() + 3))) ++bad;
    // pose_from_homography with the linear K; a K with cx <= 0 fails with the reference's message
    const PoseFromHResult p = calibba_adapter::pose_from_homography(r.kmtx, hs[0].hmtx);
    std::printf("P %d %.17g %.17g", p.success ? 1 : 0, p.scale, p.cond_check);
    print_pose(p.c_se3_t);
    std::printf("\n");
    CameraMatrix k0 = r.kmtx;
    k0.cx = 0.0;
    const PoseFromHResult pb = calibba_adapter::pose_from_homography(k0, hs[0].hmtx);
    if (pb.success || pb.message != "Invalid camera matrix K") ++bad;
    // no views: an unsuccessful result, not an error
    if (calibba_adapter::estimate_intrinsics({}).success) ++bad;
    // a negative max_iters: std::invalid_argument, as the C ABI returns CBA_ERR_INVALID_ARGUMENT
    RansacOptions neg;
    neg.max_iters = -1;
    try {
        (void)calibba_adapter::estimate_homography(views[0], neg);
        ++bad;
    } catch (const std::invalid_argument&) {
    }
    std::printf(bad ? "lin_adapter_drive: %d checks failed\n" : "lin_adapter_drive: all ok\n", bad);
    return bad ? 1 : 0;
}
