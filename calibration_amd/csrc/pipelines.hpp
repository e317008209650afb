// pipelines.hpp — the entry points of the one-shot solvers and the batched pipelines, as capi.cpp and capi_pipelines.cpp call them.
// Each is defined in the .hip file its comment names.
#pragma once
#include <memory>

#include "../../include/calibba.h"
#include "hip_glue.hpp"

namespace cba {

void planar_pose_batch(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                       const double* kmtx5, int num_radial, double* pose7, const cba_options* o, cba_summary* summaries,
                       double* distortion, double* rms, double* cov, int device);
void homography_batch(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                      double* h9, const cba_options* o, cba_summary* summaries, double* cov64, int device);
void semidlt_solve(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                   double* kappa5, double* poses7, int num_radial, const double* bounds_lo, const double* bounds_hi,
                   const int32_t* fixed_idx, const double* fixed_val, int n_fixed, const cba_options* o, cba_summary* summary,
                   double* distortion, double* view_errors, double* cov, int device);
void semidlt_solve_sharded(int n_local, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                           int n_views_total, int first_view, double* kappa5, double* poses7, int num_radial, const double* bounds_lo,
                           const double* bounds_hi, const int32_t* fixed_idx, const double* fixed_val, int n_fixed, const cba_options* o,
                           cba_summary* summary, double* distortion, double* view_errors, double* cov, int device, cba_allreduce_fn fn,
                           void* user, void* rccl_comm);
void dlt_homography_batch(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                          double* H9, int32_t* ok, int device);
void planar_seed_batch(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                       const double* kmtx5, double* pose7, int device);
// linescan.hip: calibrate_laser_plane (camera: model, intr, optional inverse coefficients; stage_ms [5] optional timing) and
// fit_plane_svd / fit_plane_ransac on caller points
void laser_plane_calibrate(int model, const double* intr, int n_inv, const double* inv, int n_views, const int64_t* toff, const double* X,
                           const double* Y, const double* u, const double* v, const int64_t* loff, const double* lu, const double* lv,
                           const cba_plane_fit_options& o, cba_laser_plane_result* res, double* points_xyz, uint8_t* inlier_mask,
                           double* stage_ms, int device);
void plane_fit(int64_t n, const double* xyz, const cba_plane_fit_options& o, double* plane, double* rms, int64_t* count, uint8_t* mask,
               int device);
// hom_ransac.hip: estimate_homography (RANSAC when o != nullptr, else DLT) of a batch of views, and estimate_intrinsics as one device
// pipeline (o: RANSAC options or nullptr; bounds optional; inlier_mask, stage_ms [5] optional)
void homography_ransac_batch(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                             const cba_ransac_options* o, double* h9, int32_t* success, int32_t* inlier_count, double* symmetric_rms,
                             uint8_t* inlier_mask, int device);
void estimate_intrinsics_gpu(int n_views, const int64_t* view_offset, const double* X, const double* Y, const double* u, const double* v,
                             const cba_ransac_options* o, const double* bounds_lo5, const double* bounds_hi5, int32_t* success,
                             double* kmtx5, int32_t* sanitized, int32_t* view_ok, double* h9, double* forward_rms_px, double* rt12,
                             int32_t* pose_ok, uint8_t* inlier_mask, double* stage_ms, int device);
// extrinsic_dlt.hip: estimate_extrinsic_dlt on the blocked layout of cba_optimize_extrinsics; table [n_views][n_cams] = block index or
// -1 (built and checked by the caller); blk_pose, blk_ok, stage_ms [4] optional
void extrinsic_dlt_gpu(int n_cams, int n_views, int n_blocks, const int64_t* blk_offset, const int32_t* blk_cam, const int32_t* table,
                       const double* X, const double* Y, const double* u, const double* v, const double* kmtx5, double* c_T_r,
                       double* r_T_t, double* blk_pose, int32_t* blk_ok, double* stage_ms, int device);
// bundle_seed.hip: the hand-eye / bundle seed on the blocked layout of cba_optimize_bundle.  cam_start / cam_blk: each camera's list
// (built and checked by the caller); g_T_c / cam_status in: the given or identity rows and GIVEN / TOO_FEW_VIEWS / DLT (the cameras
// to estimate), out: the DLT cameras' results; b_T_t written only when b_T_t_given is NULL and some block is listed; blk_pose,
// blk_ok, stage_ms [6] optional
void bundle_seed_gpu(int n_cams, int n_blocks, const int64_t* blk_offset, const int32_t* blk_cam, const double* blk_b_T_g, const double* X,
                     const double* Y, const double* u, const double* v, const double* kmtx5, double min_angle_deg, const int32_t* cam_start,
                     const int32_t* cam_blk, double* g_T_c, int32_t* cam_status, int32_t* cam_pairs, const double* b_T_t_given,
                     double* b_T_t, double* blk_pose, int32_t* blk_ok, double* stage_ms, int device);
// distortion_fit.hip: fit_distortion_full / _dual and estimate_intrinsics_linear(_iterative) over a batch of problems (offset
// [P+1], checked by the caller).  fixed_mask / fixed_val5: the resolved fixed coefficients; residuals, stage_ms [6] optional
void distortion_fit_gpu(int n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v,
                        const double* kmtx5, int num_radial, int fixed_mask, const double* fixed_val5, bool dual, double* coeffs,
                        double* inverse, int32_t* ok, double* residuals, double* stage_ms, int device);
void intrinsics_linear_gpu(int n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v,
                           const double* bounds_lo5, const double* bounds_hi5, int use_skew, double* kmtx5, int32_t* status,
                           int32_t* fallback, int device);
void intrinsics_linear_iterative_gpu(int n_problems, const int64_t* offset, const double* x, const double* y, const double* u, const double* v,
                                     int num_radial, int max_iterations, int use_skew, double* kmtx5, double* coeffs, int32_t* status,
                                     int32_t* iterations, int32_t* fallback, double* stage_ms, int device);
// camera.hip: project / unproject of caller points (intr: 10 | 12 entries; inv: n_inv inverse coefficients or NULL) and the
// undistortion / rectification map handle (checked by the caller; stage_ms [3] optional: upload, kernel, download)
void camera_project_gpu(int model, const double* intr, int64_t n, const double* xyz, double* uv, double* stage_ms, int device);
void camera_unproject_gpu(int model, const double* intr, int n_inv, const double* inv, int64_t n, const double* uv, double* xy,
                          double* stage_ms, int device);
struct UndistortMap;
UndistortMap* undistort_map_create(int model, int n_cams, const double* intr, const double* R9, const double* new_k5, int W, int H,
                                   double* stage_ms, int device);
void undistort_map_fetch(UndistortMap* m, float* map_x, float* map_y);
void undistort_map_apply(UndistortMap* m, int n_images, const int32_t* cam, int sw, int sh, int ch, int dtype, double border,
                         const void* src, void* dst, double* stage_ms);
void undistort_map_destroy(UndistortMap* m) noexcept;
int undistort_map_cams(const UndistortMap* m);
// triangulate.hip: cba_triangulate (checked by the caller; rms_px, used_mask, cov6 optional; linearisations [n] and stage_ms [3] =
// upload, kernel, download optional: the experiment builds' per-point pass counts and timing)
void triangulate_gpu(int model, int n_cams, const double* intr, int n_inv, const double* inv, const double* c_T_r, int64_t n,
                     const double* uv, const cba_triangulate_options& o, double* xyz, double* rms_px, uint32_t* used_mask, int32_t* status,
                     double* cov6, int32_t* linearisations, double* stage_ms, int device);
// laser_scan.hip: cba_laser_points and the cba_laser_scanner handle (checked by the caller).  frame_offset [n_frames + 1] and
// frame_pose7 [n_frames][7]: both or neither; plane_xy optional; stage_ms [3] optional: upload, kernel, download
void laser_points_gpu(int model, const double* intr, int n_inv, const double* inv, const double* plane, int64_t n, const double* uv,
                      int n_frames, const int64_t* frame_offset, const double* frame_pose7, double* xyz, double* plane_xy, int device);
struct LaserScanner;
LaserScanner* laser_scanner_create(int model, const double* intr, int n_inv, const double* inv, const double* plane, int W, int H,
                                   int max_frames, const cba_laser_scan_options& o, int device);
int laser_scanner_max_frames(const LaserScanner* h);
void laser_scanner_process(LaserScanner* h, int n_frames, int dtype, const void* images, const double* frame_pose7, double* centre,
                           double* amplitude, double* width_px, double* xyz, double* stage_ms);
void laser_scanner_destroy(LaserScanner* h) noexcept;
// structured_light.hip: the host pattern generator and the cba_sl_decoder handle (checked by the caller).  set_rig: two cameras of
// one model, the camera then the projector; every output of process optional; stage_ms [4] optional: upload, decode, points, download
void sl_patterns_host(const cba_sl_options& o, uint8_t* out);
int sl_options_image_count(const cba_sl_options& o);
struct SlDecoder;
SlDecoder* sl_decoder_create(const cba_sl_options& o, int W, int H, int max_sequences, int device);
int sl_decoder_max_sequences(const SlDecoder* h);
bool sl_decoder_can_point(const SlDecoder* h);  // a rig is set and both axes are decoded
void sl_decoder_set_rig(SlDecoder* h, int model, const double* intr, int n_inv, const double* inv, const double* c_T_r,
                        const cba_triangulate_options& o);
void sl_decoder_process(SlDecoder* h, int n_seq, const uint8_t* images, double* coord, double* modulation, uint8_t* status, double* xyz,
                        double* rms_px, int32_t* tri_status, double* stage_ms);
void sl_decoder_destroy(SlDecoder* h) noexcept;
// cloud_register.hip: cba_point_normals and the cba_cloud_index handle (checked by the caller).  cloud_plan: the host's grid plan of a
// target (0, or 1: no valid point, 2: too many cells, *fit then a cell size that fits).  register: results holds the normalised
// initial poses on entry (iterations 0, the rest zero); stage_ms [3] optional: upload, rounds, download
void point_normals_gpu(int n_maps, int H, int W, const double* xyz, const double* viewpoint, double max_jump, double* normals, int device);
int cloud_plan(int64_t n, const double* xyz, double cell_size, double* fit);
struct CloudIndex;
CloudIndex* cloud_index_create(int64_t n, const double* xyz, const double* normals, double cell_size, int device);
double cloud_index_cell_size(const CloudIndex* h);
bool cloud_index_has_normals(const CloudIndex* h);
void cloud_index_nearest(CloudIndex* h, int64_t m, const double* query, double max_distance, int64_t* index, double* dist2);
void cloud_index_register(CloudIndex* h, int n_sources, const int64_t* source_offset, const double* source_xyz, const cba_icp_options& o,
                          cba_icp_result* results, double* stage_ms);
void cloud_index_destroy(CloudIndex* h) noexcept;
// cloud_register.hip: the cba_cloud_set handle (checked by the caller).  cloud_set_plan: cloud_plan of every scan, *scan the first one
// that has no grid.  align: pose7 holds the normalised initial poses on entry; stage_ms [3] optional: upload, rounds, download
int cloud_set_plan(int n_scans, const int64_t* offset, const double* xyz, double cell_size, int* scan, double* fit);
struct CloudSet;
CloudSet* cloud_set_create(int n_scans, const int64_t* offset, const double* xyz, const double* normals, double cell_size, int device);
int cloud_set_scans(const CloudSet* h);
double cloud_set_cell_size(const CloudSet* h);
bool cloud_set_has_normals(const CloudSet* h);
void cloud_set_align(CloudSet* h, int n_edges, const int32_t* edges, const cba_icp_options& o, int fixed, double* pose7, cba_align_edge* edge_out,
                     cba_align_result* result, double* stage_ms);
void cloud_set_destroy(CloudSet* h) noexcept;
// tsdf_fusion.hip: the cba_tsdf_volume handle (checked by the caller).  integrate: stage_ms [2] optional: upload, kernel; extract:
// stage_ms [2] optional: count and scan, place; mesh: stage_ms [4] optional: the extract's two, the triangles' count and scan, their
// place.  points: the count of the last extract, -1 before the first; triangles: of the handle's mesh, -1 when there is none
struct TsdfVolume;
TsdfVolume* tsdf_volume_create(int nx, int ny, int nz, const double* origin, const cba_tsdf_options& o, int device);
int64_t tsdf_volume_points(const TsdfVolume* h);
double tsdf_volume_voxel_size(const TsdfVolume* h);
void tsdf_volume_reset(TsdfVolume* h);
// rgba: uint8 [n_maps][H][W][4] (cba_tsdf_integrate_colour) or NULL (cba_tsdf_integrate); eager: the experiment builds' colour kernel
void tsdf_volume_integrate(TsdfVolume* h, int model, const double* intr, int n_maps, int H, int W, const double* depth, const uint8_t* rgba,
                           const double* c_T_v, bool eager, double* stage_ms);
void tsdf_volume_fetch(TsdfVolume* h, float* tsdf, float* weight);
void tsdf_volume_upload(TsdfVolume* h, const float* tsdf, const float* weight);
void tsdf_volume_extract(TsdfVolume* h, double min_weight, int64_t* n_points, double* stage_ms);
void tsdf_volume_extract_fetch(TsdfVolume* h, double* xyz, double* normals);
int64_t tsdf_volume_triangles(const TsdfVolume* h);
void tsdf_volume_mesh(TsdfVolume* h, double min_weight, int64_t* n_points, int64_t* n_triangles, double* stage_ms);
void tsdf_volume_mesh_fetch(TsdfVolume* h, int32_t* triangles);
// the ray cast: the views of the last one (-1: none yet); stage_ms [2] optional: upload and the rays table, the cast
int64_t tsdf_volume_ray_views(const TsdfVolume* h);
void tsdf_volume_raycast(TsdfVolume* h, int model, const double* intr, int n_views, int H, int W, const double* c_T_v,
                         const cba_tsdf_raycast_options& o, int wave_w, double* stage_ms, double* colour_ms);
void tsdf_volume_raycast_fetch(TsdfVolume* h, double* depth, double* xyz, double* normals, uint8_t* status, double* rays);
// colour: whether the handle has a colour volume, and whether the last extract (or mesh) and the last ray cast ran with one
bool tsdf_volume_has_colour(const TsdfVolume* h);
bool tsdf_volume_points_coloured(const TsdfVolume* h);
bool tsdf_volume_rays_coloured(const TsdfVolume* h);
void tsdf_volume_colour_fetch(TsdfVolume* h, float* colour);
void tsdf_volume_colour_upload(TsdfVolume* h, const float* colour);
void tsdf_volume_extract_fetch_colour(TsdfVolume* h, uint8_t* rgba);
void tsdf_volume_raycast_fetch_colour(TsdfVolume* h, uint8_t* rgba);
void tsdf_volume_destroy(TsdfVolume* h) noexcept;
// stereo_match.hip: cba_stereo_points and the cba_stereo_matcher handle (checked by the caller).  geom and pose7 optional at create;
// disparity, cost, xyz optional; stage_ms [3] optional: upload, kernels, download
void stereo_points_gpu(const cba_stereo_geometry& geom, const double* pose7, int64_t n, const double* uvd, double* xyz, int device);
struct StereoMatcher;
StereoMatcher* stereo_matcher_create(int W, int H, int max_pairs, const cba_stereo_match_options& o, const cba_stereo_geometry* geom,
                                     const double* pose7, int device);
int stereo_matcher_max_pairs(const StereoMatcher* h);
bool stereo_matcher_has_geometry(const StereoMatcher* h);
void stereo_matcher_process(StereoMatcher* h, int n_pairs, const uint8_t* left, const uint8_t* right, float* disparity, int32_t* cost,
                            float* xyz, double* stage_ms);
void stereo_matcher_destroy(StereoMatcher* h) noexcept;
// the finish step both matchers share (k_stereo_finish of stereo_match.hip), queued on s: the left-right check (lr_max_diff >= 0, dr
// then required) and the points (xyz optional)
struct StereoGeom;
void stereo_finish_launch(hipStream_t s, int64_t n_px, int W, int H, int lr_max_diff, const int16_t* dl, const int16_t* dr, float* disparity,
                          float* xyz, const StereoGeom& g);
// disparity_filter.hip: the median and speckle filters.  DispFilter is the device-side object behind the cba_disparity_filter handle
// and behind a matcher with a filter set: options and every buffer fixed by disp_filter_init (on the current device), the one launch
// sequence queued on the caller's stream by disp_filter_run (in, out: device maps [n][H][W], in == out allowed; stats stays in
// f.stats, [n][3]).  stage_ms [DISP_FILTER_STAGES] optional: median, local labels, merge, flatten, sizes, apply
constexpr int DISP_FILTER_STAGES = 6;
struct __attribute__((visibility("hidden"))) DispFilter {
    cba_disparity_filter_options opts;
    int W = 0, H = 0, max_images = 0;
    DevBuf<float> med;             // the maps after the median step
    DevBuf<int32_t> label, size;   // per pixel; only with speckle_max_size > 0
    DevBuf<int64_t> stats;
};
void disp_filter_init(DispFilter& f, int W, int H, int max_images, const cba_disparity_filter_options& o);
void disp_filter_run(DispFilter& f, hipStream_t s, int n, const float* in, float* out, double* stage_ms);
struct DisparityFilter;
DisparityFilter* disparity_filter_create(int W, int H, int max_images, const cba_disparity_filter_options& o, int device);
int disparity_filter_max_images(const DisparityFilter* h);
void disparity_filter_process(DisparityFilter* h, int n, const float* in, float* out, int64_t* stats, double* stage_ms);
void disparity_filter_destroy(DisparityFilter* h) noexcept;
// a matcher's filter: o == nullptr removes it; the workspace is allocated here.  Both matchers keep it as std::unique_ptr<DispFilter>
// filter beside W, H and max_pairs, and with it set they run their finish step without xyz, then matcher_filter_finish.
void stereo_matcher_set_filter(StereoMatcher* h, const cba_disparity_filter_options* o);
template <class Matcher>
__attribute__((visibility("hidden"))) void matcher_set_filter(Matcher* h, const cba_disparity_filter_options* o) {
    h->begin();
    h->filter.reset();  // every call has ended with its stream synchronised
    if (!o) return;
    auto f = std::make_unique<DispFilter>();
    disp_filter_init(*f, h->W, h->H, h->max_pairs, *o);
    h->filter = std::move(f);
}
// the resident disparity filtered in place, then the points from the filtered map (the finish step with the left-right check off)
__attribute__((visibility("hidden"))) inline void matcher_filter_finish(DispFilter& f, hipStream_t s, int n_pairs, float* disparity, float* xyz,
                                                                        const StereoGeom& g) {
    disp_filter_run(f, s, n_pairs, disparity, disparity, nullptr);
    if (xyz) stereo_finish_launch(s, static_cast<int64_t>(n_pairs) * f.W * f.H, f.W, f.H, -1, nullptr, nullptr, disparity, xyz, g);
}
// stereo_sgm.hip: the cba_sgm_matcher handle (checked by the caller).  geom and pose7 optional at create; disparity, cost, xyz optional;
// stage_ms [SGM_STAGES] optional: upload, census, cost, the 8 path launches, selection, download
constexpr int SGM_STAGES = 13;
struct SgmMatcher;
SgmMatcher* sgm_matcher_create(int W, int H, int max_pairs, const cba_sgm_options& o, const cba_stereo_geometry* geom, const double* pose7,
                               int device);
int sgm_matcher_max_pairs(const SgmMatcher* h);
bool sgm_matcher_has_geometry(const SgmMatcher* h);
void sgm_matcher_process(SgmMatcher* h, int n_pairs, const uint8_t* left, const uint8_t* right, float* disparity, int32_t* cost, float* xyz,
                         double* stage_ms);
void sgm_matcher_set_filter(SgmMatcher* h, const cba_disparity_filter_options* o);
void sgm_matcher_destroy(SgmMatcher* h) noexcept;
// corner_detect.hip: the cba_corner_detector handle (checked by the caller).  Every output optional; stage_ms [5] optional: upload,
// response, peaks, refine, download
struct CornerDetector;
CornerDetector* corner_detector_create(int W, int H, int max_images, int max_corners, const cba_corner_options& o, int device);
int corner_detector_max_images(const CornerDetector* h);
void corner_detector_process(CornerDetector* h, int n_images, const uint8_t* images, int32_t* out_count, int32_t* out_status, double* out_xy,
                             double* out_angle, int32_t* out_response, int32_t* out_flags, double* stage_ms);
void corner_detector_destroy(CornerDetector* h) noexcept;
// what marker_read.hip reaches of a corner detector: its resident images and the peak list, positions and counts of its last process
struct CornerDeviceView {
    const uint8_t* img;
    const double* xy;
    const int32_t* count;
    const int32_t* peak_px;
};
CornerDeviceView corner_detector_view(const CornerDetector* h);
// blob_detect.hip: the cba_blob_detector handle (checked by the caller).  Every output optional; stage_ms [5] optional: upload, response,
// peaks, refine, download
struct BlobDetector;
BlobDetector* blob_detector_create(int W, int H, int max_images, int max_blobs, const cba_blob_options& o, int device);
int blob_detector_max_images(const BlobDetector* h);
void blob_detector_process(BlobDetector* h, int n_images, const uint8_t* images, int32_t* out_count, int32_t* out_status, double* out_xy,
                           double* out_shape, double* out_fit_error, int32_t* out_response, int32_t* out_flags, double* stage_ms);
void blob_detector_destroy(BlobDetector* h) noexcept;
// fn / user / n_ranks / rank: multi-GPU form — this rank's share of the pairs, sums all-reduced through the host callback
// (rccl_comm: an ncclComm_t over the ranks' devices - the sums are all-reduced on the device instead of through fn)
void handeye_dlt(int n_poses, const double* bTg, const double* cTt, double min_angle_deg, double* pose7, int device,
                 cba_allreduce_fn fn = nullptr, void* user = nullptr, int n_ranks = 1, int rank = 0, void* rccl_comm = nullptr);
void handeye_solve(int n_poses, const double* bTg, const double* cTt, double* pose7, const cba_options* o, cba_summary* s,
                   double* cov, int device, cba_allreduce_fn fn = nullptr, void* user = nullptr, int n_ranks = 1, int rank = 0,
                   void* rccl_comm = nullptr);
void* rccl_comm_create(const uint8_t* id, int n_ranks, int rank);  // collectives.cpp: ncclCommInitRank on the current device
void rccl_comm_destroy(void* comm, bool abort);

// marker_read.hip: the cba_charuco_detector handle (checked by the caller).  Every output optional.  arms and read act on the images
// of the last process.  stage_ms [9] optional: upload, response, peaks, refine, arms, host lattice, read, host match, download; ms [1]
// optional: the device time of the stage.
struct CharucoDetector;
CharucoDetector* charuco_detector_create(int W, int H, int max_images, int max_corners, int max_cells, const cba_corner_options& co,
                                         const cba_charuco_options& o, const cba_charuco_board& b, const uint64_t* codes, int device);
int charuco_detector_max_images(const CharucoDetector* h);
int charuco_detector_max_corners(const CharucoDetector* h);
int charuco_detector_max_cells(const CharucoDetector* h);
int charuco_detector_last_images(const CharucoDetector* h);
void charuco_detector_process(CharucoDetector* h, int n_images, const uint8_t* images, int32_t* out_count, int32_t* out_status,
                              int32_t* out_ids, double* out_xy, int32_t* out_n_markers, int32_t* out_n_corners, int32_t* out_n_cells,
                              int32_t* out_cells, cba_marker_reading* out_readings, double* stage_ms);
void charuco_detector_arms(CharucoDetector* h, int n_images, const double* dirs, double* out_score, double* ms = nullptr);
void charuco_detector_read(CharucoDetector* h, int n_cells, const int32_t* cell_image, const double* quad, cba_marker_reading* out,
                           double* ms = nullptr);
void charuco_detector_destroy(CharucoDetector* h) noexcept;

}  // namespace cba
