// camera.hip — the camera models on the GPU (camera_math.hpp): project and unproject of caller points, and the undistortion /
// rectification map handle (create, fetch, apply).  One stream, one synchronise per call:
//   k_cam_project<MODEL>   one lane per PAIR of points, grid-stride: the pair's xyz are three 16-byte loads, its uv two stores
//   k_cam_unproject        one lane per point, grid-stride: one 16-byte load, one 16-byte store; ls_unproject as it is
//   k_cam_map<MODEL, VEC>  one lane per CAM_MAP_PX consecutive pixels of one row; each camera's lanes are padded to whole
//                          wavefronts, so the camera (and its constants) is wave-uniform and read with scalar loads; VEC: the
//                          row width is a multiple of CAM_MAP_PX and the pixels go out as one float4 per map, else one store each
//   k_cam_apply<T, CH, L>  one lane per output pixel of one image (images padded to whole wavefronts: image and camera are
//                          wave-uniform); the lane reads its map entry and gathers the four taps x CH channels.  L (uint8, 3
//                          channels only): three aligned dword loads per tap row (1, the default) or byte loads (0)
#include <algorithm>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "pipelines.hpp"
#include "camera_math.hpp"

namespace cba {

constexpr int CAM_BLOCK = 256;
constexpr int CAM_GRID = 8192;  // grid-stride cap: 32 workgroups of 4 wavefronts per CU
constexpr int CAM_MAP_PX = 4;

namespace {

struct CamProj {  // one camera of project: intrinsics and Scheimpflug constants (a kernel argument)
    double intr[12];
    double sd[SD_SIZE];
};

int64_t whole_waves(int64_t lanes) { return (lanes + 63) / 64 * 64; }

// device events of the experiment builds' timing: 0 start, 1 uploaded, 2 kernel done, 3 downloaded; stage_ms [3]: upload, kernel, download
using CamTimer = StageTimer<4>;

}  // namespace

template <int MODEL>
__global__ __launch_bounds__(CAM_BLOCK) void k_cam_project(int64_t n, const double* __restrict__ xyz, double* __restrict__ uv, CamProj c) {
    const int64_t pairs = (n + 1) / 2;
    for (int64_t q = blockIdx.x * static_cast<int64_t>(CAM_BLOCK) + threadIdx.x; q < pairs; q += static_cast<int64_t>(gridDim.x) * CAM_BLOCK) {
        if (2 * q + 1 < n) {
            const double2* src = reinterpret_cast<const double2*>(xyz + 6 * q);
            const double2 a = src[0], b = src[1], d = src[2];
            double2 o0, o1;
            cam_project<MODEL>(c.intr, c.sd, a.x, a.y, b.x, &o0.x, &o0.y);
            cam_project<MODEL>(c.intr, c.sd, b.y, d.x, d.y, &o1.x, &o1.y);
            double2* dst = reinterpret_cast<double2*>(uv + 4 * q);
            dst[0] = o0;
            dst[1] = o1;
        } else {  // the odd last point
            const double* p = xyz + 6 * q;
            double2 o;
            cam_project<MODEL>(c.intr, c.sd, p[0], p[1], p[2], &o.x, &o.y);
            reinterpret_cast<double2*>(uv + 4 * q)[0] = o;
        }
    }
}

__global__ __launch_bounds__(CAM_BLOCK) void k_cam_unproject(int64_t n, const double* __restrict__ uv, double* __restrict__ xy, LsCamera c) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(CAM_BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * CAM_BLOCK) {
        const double2 p = reinterpret_cast<const double2*>(uv)[i];
        double2 o;
        ls_unproject(c, p.x, p.y, &o.x, &o.y);
        reinterpret_cast<double2*>(xy)[i] = o;
    }
}

// lanes_per_cam = whole_waves(H * cw), cw = ceil(W / CAM_MAP_PX)
template <int MODEL, bool VEC>
__global__ __launch_bounds__(CAM_BLOCK) void k_cam_map(int n_cams, int W, int H, int cw, int64_t lanes_per_cam, const CamMapCam* __restrict__ cams,
                                                       float* __restrict__ map_x, float* __restrict__ map_y) {
    const int64_t total = lanes_per_cam * n_cams, row_lanes = static_cast<int64_t>(H) * cw;
    for (int64_t g = blockIdx.x * static_cast<int64_t>(CAM_BLOCK) + threadIdx.x; g < total; g += static_cast<int64_t>(gridDim.x) * CAM_BLOCK) {
        const int cam = __builtin_amdgcn_readfirstlane(static_cast<int>(g / lanes_per_cam));  // whole wavefronts per camera
        const int64_t r = g - cam * lanes_per_cam;
        if (r >= row_lanes) continue;
        const CamMapCam& c = cams[cam];
        const int row = static_cast<int>(r / cw);
        const int u0 = static_cast<int>(r - static_cast<int64_t>(row) * cw) * CAM_MAP_PX;
        float ox[CAM_MAP_PX], oy[CAM_MAP_PX];
#pragma unroll
        for (int k = 0; k < CAM_MAP_PX; ++k) cam_map_pixel<MODEL>(c, static_cast<double>(u0 + k), static_cast<double>(row), ox + k, oy + k);
        const int64_t o = (static_cast<int64_t>(cam) * H + row) * W + u0;
        if (VEC) {
            *reinterpret_cast<float4*>(map_x + o) = make_float4(ox[0], ox[1], ox[2], ox[3]);
            *reinterpret_cast<float4*>(map_y + o) = make_float4(oy[0], oy[1], oy[2], oy[3]);
        } else {
#pragma unroll
            for (int k = 0; k < CAM_MAP_PX; ++k)
                if (u0 + k < W) {  // the row tail
                    map_x[o + k] = ox[k];
                    map_y[o + k] = oy[k];
                }
        }
    }
}

// the 6 bytes [o, o + 6) of a 4-byte-aligned buffer as the low bytes of a 64-bit word: three aligned dword loads (the buffer is
// padded by CAM_SRC_PAD bytes, so the third never leaves it)
constexpr int CAM_SRC_PAD = 16;
__device__ __forceinline__ uint64_t cam_load6(const uint8_t* __restrict__ base, int64_t o) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(base + (o & ~int64_t(3)));
    const int s = static_cast<int>(o & 3) * 8;
    const uint64_t lo = static_cast<uint64_t>(w[0]) | static_cast<uint64_t>(w[1]) << 32;
    const uint64_t hi = w[2];
    return s == 0 ? lo : (lo >> s) | (hi << (64 - s));
}

// lanes_per_img = whole_waves(W * H); src images [n_images][sh][sw][CH], dst [n_images][H][W][CH]
template <typename T, int CH, int LOAD>
__global__ __launch_bounds__(CAM_BLOCK) void k_cam_apply(int n_images, const int32_t* __restrict__ img_cam, int W, int H, int64_t lanes_per_img,
                                                         int sw, int sh, const T* __restrict__ src, T* __restrict__ dst,
                                                         const float* __restrict__ map_x, const float* __restrict__ map_y, T border) {
    const int64_t total = lanes_per_img * n_images, npx = static_cast<int64_t>(W) * H, nsrc = static_cast<int64_t>(sw) * sh * CH;
    for (int64_t g = blockIdx.x * static_cast<int64_t>(CAM_BLOCK) + threadIdx.x; g < total; g += static_cast<int64_t>(gridDim.x) * CAM_BLOCK) {
        const int img = __builtin_amdgcn_readfirstlane(static_cast<int>(g / lanes_per_img));  // whole wavefronts per image
        const int64_t p = g - img * lanes_per_img;
        if (p >= npx) continue;
        const int cam = img_cam[img];
        const float mx = map_x[cam * npx + p], my = map_y[cam * npx + p];
        const T* s = src + img * nsrc;
        T* d = dst + (img * npx + p) * CH;
        if constexpr (sizeof(T) == 1) {
            int x0, y0, w[4];
            if (!cam_taps_u8(mx, my, &x0, &y0, w)) {
#pragma unroll
                for (int k = 0; k < CH; ++k) d[k] = border;
                continue;
            }
            const bool i00 = cam_in_source(x0, y0, sw, sh), i01 = cam_in_source(x0 + 1, y0, sw, sh);
            const bool i10 = cam_in_source(x0, y0 + 1, sw, sh), i11 = cam_in_source(x0 + 1, y0 + 1, sw, sh);
            const int64_t o = (static_cast<int64_t>(y0) * sw + x0) * CH, row = static_cast<int64_t>(sw) * CH;
            int p00[CH], p01[CH], p10[CH], p11[CH];
            if (LOAD == 1 && CH == 3 && i00 && i01 && i10 && i11) {
                const uint64_t t = cam_load6(src, img * nsrc + o), b = cam_load6(src, img * nsrc + o + row);
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    p00[k] = static_cast<int>(t >> (8 * k) & 0xff);
                    p01[k] = static_cast<int>(t >> (8 * (k + 3)) & 0xff);
                    p10[k] = static_cast<int>(b >> (8 * k) & 0xff);
                    p11[k] = static_cast<int>(b >> (8 * (k + 3)) & 0xff);
                }
            } else {
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    p00[k] = i00 ? s[o + k] : border;
                    p01[k] = i01 ? s[o + CH + k] : border;
                    p10[k] = i10 ? s[o + row + k] : border;
                    p11[k] = i11 ? s[o + row + CH + k] : border;
                }
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) d[k] = cam_blend_u8(w, p00[k], p01[k], p10[k], p11[k]);
        } else {
            int x0, y0;
            float fx, fy;
            if (!cam_taps_f32(mx, my, &x0, &y0, &fx, &fy)) {
#pragma unroll
                for (int k = 0; k < CH; ++k) d[k] = border;
                continue;
            }
            const bool i00 = cam_in_source(x0, y0, sw, sh), i01 = cam_in_source(x0 + 1, y0, sw, sh);
            const bool i10 = cam_in_source(x0, y0 + 1, sw, sh), i11 = cam_in_source(x0 + 1, y0 + 1, sw, sh);
            const int64_t o = (static_cast<int64_t>(y0) * sw + x0) * CH, row = static_cast<int64_t>(sw) * CH;
            float p00[CH], p01[CH], p10[CH], p11[CH];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                p00[k] = i00 ? s[o + k] : border;
                p01[k] = i01 ? s[o + CH + k] : border;
                p10[k] = i10 ? s[o + row + k] : border;
                p11[k] = i11 ? s[o + row + CH + k] : border;
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) d[k] = cam_blend_f32(fx, fy, p00[k], p01[k], p10[k], p11[k]);
        }
    }
}

// ---- host glue -----------------------------------------------------------------------------------------------------------
void camera_project_gpu(int model, const double* intr, int64_t n, const double* xyz, double* uv, double* stage_ms, int device) {
    CamProj c;
    ls_fill_intr(model, intr, c.intr, c.sd);
    StreamLease lease(device);
    const hipStream_t s = lease;
    CamTimer tm(s, stage_ms != nullptr);
    DevBuf<double> dxyz, duv;
    dxyz.alloc(3 * static_cast<size_t>(n));
    duv.alloc(2 * static_cast<size_t>(n));
    tm.mark(0);
    dxyz.upload(xyz, 3 * static_cast<size_t>(n), s);
    tm.mark(1);
    const int g = launch_grid((n + 1) / 2, CAM_BLOCK, CAM_GRID);
    if (model == CAM_SCHEIMPFLUG)
        hipLaunchKernelGGL(k_cam_project<CAM_SCHEIMPFLUG>, dim3(g), dim3(CAM_BLOCK), 0, s, n, dxyz.p, duv.p, c);
    else
        hipLaunchKernelGGL(k_cam_project<CAM_PINHOLE_BC>, dim3(g), dim3(CAM_BLOCK), 0, s, n, dxyz.p, duv.p, c);
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    duv.download(uv, 2 * static_cast<size_t>(n), s);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(stage_ms);
}

void camera_unproject_gpu(int model, const double* intr, int n_inv, const double* inv, int64_t n, const double* uv, double* xy,
                          double* stage_ms, int device) {
    LsCamera c;
    ls_fill_camera(model, intr, n_inv, inv, &c);
    StreamLease lease(device);
    const hipStream_t s = lease;
    CamTimer tm(s, stage_ms != nullptr);
    DevBuf<double> duv, dxy;
    duv.alloc(2 * static_cast<size_t>(n));
    dxy.alloc(2 * static_cast<size_t>(n));
    tm.mark(0);
    duv.upload(uv, 2 * static_cast<size_t>(n), s);
    tm.mark(1);
    hipLaunchKernelGGL(k_cam_unproject, dim3(launch_grid(n, CAM_BLOCK, CAM_GRID)), dim3(CAM_BLOCK), 0, s, n, duv.p, dxy.p, c);
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    dxy.download(xy, 2 * static_cast<size_t>(n), s);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(stage_ms);
}

// The map handle: the maps stay on the device from create to destroy.  Every call ends with its stream synchronised, so nothing is
// in flight when a buffer grows or goes.
struct UndistortMap : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    int n_cams = 0, W = 0, H = 0;
    DevBuf<float> map_x, map_y;
    DevBuf<uint8_t> src, dst;  // apply's images, kept for the next call of the same size
    DevBuf<int32_t> img_cam;
};
static_assert(!std::is_copy_constructible_v<UndistortMap> && !std::is_copy_assignable_v<UndistortMap>, "a handle owns its stream and buffers");

UndistortMap* undistort_map_create(int model, int n_cams, const double* intr, const double* R9, const double* new_k5, int W, int H,
                                   double* stage_ms, int device) {
    auto m = std::make_unique<UndistortMap>(device);
    m->n_cams = n_cams; m->W = W; m->H = H;
    const int ni = cam_intr_size(model);
    std::vector<CamMapCam> hc(n_cams);
    for (int c = 0; c < n_cams; ++c) {
        CamMapCam& k = hc[c];
        ls_fill_intr(model, intr + static_cast<size_t>(c) * ni, k.intr, k.sd);
        for (int j = 0; j < 9; ++j) k.R[j] = R9 ? R9[9 * static_cast<size_t>(c) + j] : (j % 4 == 0 ? 1.0 : 0.0);
        for (int j = 0; j < 5; ++j) k.kp[j] = new_k5 ? new_k5[5 * static_cast<size_t>(c) + j] : k.intr[j];
    }
    const hipStream_t s = m->lease;
    CamTimer tm(s, stage_ms != nullptr);
    DevBuf<CamMapCam> dcams;
    dcams.alloc(n_cams);
    const size_t npx = static_cast<size_t>(W) * H * n_cams;
    m->map_x.alloc(npx);
    m->map_y.alloc(npx);
    tm.mark(0);
    dcams.upload(hc.data(), n_cams, s);
    tm.mark(1);
    const int cw = (W + CAM_MAP_PX - 1) / CAM_MAP_PX;
    const int64_t lpc = whole_waves(static_cast<int64_t>(H) * cw);
    const int g = launch_grid(lpc * n_cams, CAM_BLOCK, CAM_GRID);
    const bool vec = W % CAM_MAP_PX == 0;
#define CAM_MAP_LAUNCH(MODEL, VEC)                                                                                              \
    hipLaunchKernelGGL((k_cam_map<MODEL, VEC>), dim3(g), dim3(CAM_BLOCK), 0, s, n_cams, W, H, cw, lpc, dcams.p, m->map_x.p, m->map_y.p)
    if (model == CAM_SCHEIMPFLUG) {
        if (vec) CAM_MAP_LAUNCH(CAM_SCHEIMPFLUG, true); else CAM_MAP_LAUNCH(CAM_SCHEIMPFLUG, false);
    } else {
        if (vec) CAM_MAP_LAUNCH(CAM_PINHOLE_BC, true); else CAM_MAP_LAUNCH(CAM_PINHOLE_BC, false);
    }
#undef CAM_MAP_LAUNCH
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));  // dcams goes out of scope
    tm.report(stage_ms);
    return m.release();
}

void undistort_map_fetch(UndistortMap* m, float* map_x, float* map_y) {
    const hipStream_t s = m->begin();
    const size_t npx = static_cast<size_t>(m->W) * m->H * m->n_cams;
    m->map_x.download(map_x, npx, s);
    m->map_y.download(map_y, npx, s);
    CBA_HIP(hipStreamSynchronize(s));
}

template <typename T, int CH, int LOAD>
static void apply_launch(UndistortMap* m, int n_images, int sw, int sh, T border, hipStream_t s) {
    const int64_t lpi = whole_waves(static_cast<int64_t>(m->W) * m->H);
    hipLaunchKernelGGL((k_cam_apply<T, CH, LOAD>), dim3(launch_grid(lpi * n_images, CAM_BLOCK, CAM_GRID)), dim3(CAM_BLOCK), 0, s, n_images, m->img_cam.p, m->W, m->H,
                       lpi, sw, sh, reinterpret_cast<const T*>(m->src.p), reinterpret_cast<T*>(m->dst.p), m->map_x.p, m->map_y.p, border);
}

template <typename T>
static void apply_dispatch(UndistortMap* m, int n_images, int sw, int sh, int ch, T border, int load, hipStream_t s) {
    switch (ch) {
        case 1: apply_launch<T, 1, 0>(m, n_images, sw, sh, border, s); break;
        case 2: apply_launch<T, 2, 0>(m, n_images, sw, sh, border, s); break;
        case 3:
            if (load == 1) apply_launch<T, 3, 1>(m, n_images, sw, sh, border, s);
            else apply_launch<T, 3, 0>(m, n_images, sw, sh, border, s);
            break;
        default: apply_launch<T, 4, 0>(m, n_images, sw, sh, border, s); break;
    }
}

// the uint8 RGB load shape: three aligned dword loads per tap row (1; 0.50 ms against 0.85 ms for byte loads at 8 x 4096 x 3000,
// DESIGN.md section 7g) unless an experiment build selects the byte loads (0)
static int u8_load_shape() {
    const char* e = cba_exp_env("CBA_EXP_CAMERA_U8_LOAD");
    return e && std::strcmp(e, "byte") == 0 ? 0 : 1;
}

void undistort_map_apply(UndistortMap* m, int n_images, const int32_t* cam, int sw, int sh, int ch, int dtype, double border,
                         const void* src, void* dst, double* stage_ms) {
    const hipStream_t s = m->begin();
    const size_t esz = dtype == CBA_DTYPE_F32 ? 4 : 1;
    const size_t src_bytes = static_cast<size_t>(n_images) * sw * sh * ch * esz;
    const size_t dst_bytes = static_cast<size_t>(n_images) * m->W * m->H * ch * esz;
    // the buffers grow before anything is queued on the stream in this call, and the previous call synchronised it
    m->src.ensure(src_bytes + CAM_SRC_PAD);
    m->dst.ensure(dst_bytes);
    m->img_cam.ensure(n_images);
    CamTimer tm(s, stage_ms != nullptr);
    tm.mark(0);
    m->img_cam.upload(cam, n_images, s);
    m->src.upload(static_cast<const uint8_t*>(src), src_bytes, s);
    tm.mark(1);
    if (dtype == CBA_DTYPE_F32) {
        apply_dispatch<float>(m, n_images, sw, sh, ch, static_cast<float>(border), 0, s);
    } else {
        const double b = std::nearbyint(border);  // saturate_cast<uchar>: round half to even, then clamp
        const uint8_t b8 = std::isnan(border) ? 0 : static_cast<uint8_t>(b < 0.0 ? 0.0 : (b > 255.0 ? 255.0 : b));
        apply_dispatch<uint8_t>(m, n_images, sw, sh, ch, b8, u8_load_shape(), s);
    }
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    m->dst.download(static_cast<uint8_t*>(dst), dst_bytes, s);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(stage_ms);
}

int undistort_map_cams(const UndistortMap* m) { return m->n_cams; }

void undistort_map_destroy(UndistortMap* m) noexcept { destroy_handle(m); }

}  // namespace cba
