// laser_scan.hip — laser profile scanning on the GPU (laser_scan_math.hpp, calibba.h: cba_laser_points, cba_laser_scanner).  One
// stream, one launch and one synchronise per call:
//   k_laser_points            one lane per caller pixel, grid-stride: one 16-byte load, laser_point, the stores.  Camera, plane and
//                             homography are a kernel argument (wave-uniform); with poses the lane finds its frame in the offset table
//                             by bisection and reads that frame's [R | t] row.  It follows k_cam_unproject (camera.hip).
//   k_laser_scan_cols<T, NC>  one peak per COLUMN (axis 0).  A workgroup of LSC_WAVES wavefronts owns 64 NC adjacent columns of one frame; a
//                             lane owns NC adjacent columns (one 16-byte load per row: NC = 16 uint8 / 4 float32 when the width is a
//                             multiple of NC; otherwise one dword per lane: NC = 4 uint8 columns cut out of the two aligned dwords
//                             that hold them, or 1 float32 column) and walks the rows of its wavefront's quarter of the ROI with
//                             laser_peak_push.  The four (m, p0, p1) per column meet in LDS and are joined in row order by
//                             laser_peak_merge.  For the window pass the workgroup's columns are dealt out again, consecutive columns
//                             to consecutive threads, and each thread re-reads only the window rows of its columns, sums them in
//                             ascending order and goes on to laser_finish and laser_point: peaks never pass through memory.
//   k_laser_scan_rows<T>      one peak per ROW (axis 1), one wavefront per row (grid-stride).  The lanes read the aligned 16-byte vectors that
//                             cover the ROI (samples outside it are masked), each keeps (m, p0) of its own samples, and the wave
//                             maximum of the key (m, -p0) by wave_max63 is the line's maximum at its lowest position.  The plateau
//                             end is found by comparing the 64 samples after p0 at a time (ballot); the window is read once, 64
//                             consecutive samples per step.  uint8 sums are exact integers and are added by wave_sum63; float32
//                             terms are added in ascending position through readlane, one fp64 sum for the whole wavefront.
// No atomics, no scratch, no dynamically indexed private array.  Image loads never leave the scanner's image buffer: it is
// allocated LSC_IMG_PAD bytes longer than the frames, and a sample past a row or past the last frame is never used.
#include <algorithm>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "pipelines.hpp"
#include "laser_scan_math.hpp"
#include "wave_reduce.hpp"

namespace cba {

constexpr int LSC_BLOCK = 256;
constexpr int LSC_WAVES = LSC_BLOCK / 64;
constexpr int LSC_GRID = 8192;     // grid-stride cap of the per-row and per-pixel kernels
constexpr int LSC_IMG_PAD = 32;    // bytes after the last frame that a 16-byte or funnel load may touch

struct LaserScanArgs {
    const uint8_t* img;  // frames [n_frames][H][W] of T
    int W, H, n_frames;
    int pb, pe, hw;      // ROI [pb, pe) along the search direction, half window (<= 32768)
    int floor_u8;        // the floor for uint8 samples
    double floor_level, min_peak;
    const double* Rt;    // [n_frames][12] or null
    double *centre, *amplitude, *width_px, *xyz;
};

template <typename T>
using LscV = typename std::conditional<sizeof(T) == 1, int, float>::type;

// NC adjacent samples from element index e of the buffer.  uint8 x 16 and float32 x 4: one aligned 16-byte load; uint8 x 4: the dword
// at e cut out of the two aligned dwords around it (one when e is aligned); float32 x 1: one dword
template <typename T, int NC>
__device__ __forceinline__ void lsc_load(const uint8_t* __restrict__ img, int64_t e, LscV<T>* v) {
    if constexpr (sizeof(T) == 1 && NC == 16) {
        const uint4 q = *reinterpret_cast<const uint4*>(img + e);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = static_cast<int>(w[k >> 2] >> (8 * (k & 3)) & 0xffu);
    } else if constexpr (sizeof(T) == 1) {
        static_assert(sizeof(T) != 1 || NC == 4 || NC == 16, "uint8: 4 or 16 samples");
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(img + (e & ~int64_t(3)));
        const int s = static_cast<int>(e & 3) * 8;
        uint32_t w = wp[0];
        if (s) w = (w >> s) | (wp[1] << (32 - s));
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = static_cast<int>(w >> (8 * k) & 0xffu);
    } else if constexpr (NC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(img) + e);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        static_assert(sizeof(T) == 1 || NC == 1 || NC == 4, "float32: 1 or 4 samples");
        v[0] = reinterpret_cast<const float*>(img)[e];
    }
}

// the sample at element index e: one dword per lane (uint8: the aligned dword that holds it)
template <typename T>
__device__ __forceinline__ LscV<T> lsc_load_one(const uint8_t* __restrict__ img, int64_t e) {
    if constexpr (sizeof(T) == 1) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(img)[e >> 2];
        return static_cast<int>(w >> (8 * static_cast<int>(e & 3)) & 0xffu);
    } else {
        return reinterpret_cast<const float*>(img)[e];
    }
}

__device__ __forceinline__ double lsc_readlane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// centre, amplitude, width and the 3D point of line `line` (frame `frame`), whose pixel is (other, centre) by the axis
template <int AXIS>
__device__ __forceinline__ void lsc_emit(const LaserScanArgs& a, const LaserGeom& g, int frame, int64_t line, int other, bool any, double m,
                                         double sg, double sgp, double level) {
    double c, amp, wd, P[3];
    laser_finish(any, m, sg, sgp, level, a.min_peak, &c, &amp, &wd);
    const double u = AXIS == 0 ? static_cast<double>(other) : c, v = AXIS == 0 ? c : static_cast<double>(other);
    laser_point(g, u, v, a.Rt ? a.Rt + 12 * static_cast<int64_t>(frame) : nullptr, P, nullptr);
    a.centre[line] = c;
    a.amplitude[line] = amp;
    a.width_px[line] = wd;
    a.xyz[3 * line] = P[0];
    a.xyz[3 * line + 1] = P[1];
    a.xyz[3 * line + 2] = P[2];
}

// ---- axis 0: one peak per column -------------------------------------------------------------------------------------------------
// grid = n_frames * bpf workgroups, bpf = ceil(W / (64 NC))
template <typename T, int NC>
__global__ __launch_bounds__(LSC_BLOCK) void k_laser_scan_cols(LaserScanArgs a, LaserGeom g, int bpf) {
    using V = LscV<T>;
    constexpr int BC = 64 * NC;               // columns of a workgroup
    constexpr int WC = NC >= 4 ? NC / 4 : 1;  // window pass: adjacent columns of a thread
    __shared__ V sm_m[LSC_WAVES * BC];
    __shared__ short sm_p0[LSC_WAVES * BC], sm_p1[LSC_WAVES * BC];  // positions are below 32768 (CBA_IMAGE_MAX_SIDE)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int frame = blockIdx.x / bpf, cb = (blockIdx.x - frame * bpf) * BC;
    const int64_t fbase = static_cast<int64_t>(frame) * a.W * a.H;
    const int chunk = (a.pe - a.pb + LSC_WAVES - 1) / LSC_WAVES;  // rows of a wavefront
    {
        const int c0 = cb + lane * NC;
        const int r0 = min(a.pb + wave * chunk, a.pe), r1 = min(r0 + chunk, a.pe);
        LaserPeak<V> s[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) laser_peak_init(s[k]);
        if (c0 < a.W) {  // a lane whose group crosses the row end (NC = 4) reads on into the next row: those columns are never emitted
#pragma unroll 2
            for (int r = r0; r < r1; ++r) {
                V vals[NC];
                lsc_load<T, NC>(a.img, fbase + static_cast<int64_t>(r) * a.W + c0, vals);
#pragma unroll
                for (int k = 0; k < NC; ++k) laser_peak_push(s[k], vals[k], r);
            }
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int i = (wave * NC + k) * 64 + lane;
            sm_m[i] = s[k].m;
            sm_p0[i] = static_cast<short>(s[k].p0);
            sm_p1[i] = static_cast<short>(s[k].p1);
        }
    }
    __syncthreads();
    // the window pass: thread t takes the workgroup's columns [t WC, t WC + WC)
    const int cl0 = static_cast<int>(threadIdx.x) * WC;
    const int c0 = cb + cl0;
    if (cl0 >= BC || c0 >= a.W) return;
    LaserPeak<V> pk[WC];
    int lo[WC], hi[WC], rlo = a.pe, rhi = a.pb - 1;
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        const int src = (cl0 + j) / NC, k = (cl0 + j) % NC;
        laser_peak_init(pk[j]);
#pragma unroll
        for (int w = 0; w < LSC_WAVES; ++w) {
            const int i = (w * NC + k) * 64 + src;
            LaserPeak<V> b;
            b.m = sm_m[i];
            b.p0 = sm_p0[i];
            b.p1 = sm_p1[i];
            laser_peak_merge(pk[j], b, min(a.pb + w * chunk, a.pe));
        }
        lo[j] = 1;
        hi[j] = 0;
        if (pk[j].p0 >= 0) {
            laser_window(pk[j].p0, pk[j].p1, a.hw, a.pb, a.pe, &lo[j], &hi[j]);
            rlo = min(rlo, lo[j]);
            rhi = max(rhi, hi[j]);
        }
    }
    uint64_t ig[WC], igp[WC];
    double sg[WC], sgp[WC];
#pragma unroll
    for (int j = 0; j < WC; ++j) { ig[j] = 0; igp[j] = 0; sg[j] = 0.0; sgp[j] = 0.0; }
    for (int r = rlo; r <= rhi; ++r) {
        const int64_t e = fbase + static_cast<int64_t>(r) * a.W + c0;
        V vals[WC];
        if constexpr (WC == 1) vals[0] = lsc_load_one<T>(a.img, e);
        else lsc_load<T, WC>(a.img, e, vals);
#pragma unroll
        for (int j = 0; j < WC; ++j) {
            if (r < lo[j] || r > hi[j]) continue;
            if constexpr (sizeof(T) == 1) laser_sum_u8(vals[j], r, a.floor_u8, &ig[j], &igp[j]);
            else laser_sum_f64(laser_g_f32(vals[j], a.floor_level), r, &sg[j], &sgp[j]);
        }
    }
    const int64_t line0 = static_cast<int64_t>(frame) * a.W + c0;
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        if (c0 + j >= a.W) continue;
        if constexpr (sizeof(T) == 1)
            lsc_emit<0>(a, g, frame, line0 + j, c0 + j, pk[j].p0 >= 0, static_cast<double>(pk[j].m), static_cast<double>(ig[j]),
                        static_cast<double>(igp[j]), static_cast<double>(a.floor_u8));
        else
            lsc_emit<0>(a, g, frame, line0 + j, c0 + j, pk[j].p0 >= 0, static_cast<double>(pk[j].m), sg[j], sgp[j], a.floor_level);
    }
}

// ---- axis 1: one peak per row ----------------------------------------------------------------------------------------------------
// float32 <-> a uint32 that orders as the floats do (NaN never gets here; -0 was made +0)
__device__ __forceinline__ uint32_t lsc_ord(float v) {
    const uint32_t b = __float_as_uint(v);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float lsc_unord(uint32_t o) { return __uint_as_float(o & 0x80000000u ? o ^ 0x80000000u : ~o); }

template <typename T>
__global__ __launch_bounds__(LSC_BLOCK) void k_laser_scan_rows(LaserScanArgs a, LaserGeom g) {
    using V = LscV<T>;
    constexpr int EPV = 16 / static_cast<int>(sizeof(T));  // samples of a 16-byte vector
    const int lane = threadIdx.x & 63;
    const int64_t rows = static_cast<int64_t>(a.n_frames) * a.H;
    for (int64_t row = blockIdx.x * static_cast<int64_t>(LSC_WAVES) + (threadIdx.x >> 6); row < rows;
         row += static_cast<int64_t>(gridDim.x) * LSC_WAVES) {
        const int64_t e0 = row * a.W;  // element index of the row's first sample
        const int64_t v0 = (e0 + a.pb) / EPV, v1 = (e0 + a.pe - 1) / EPV;  // the aligned vectors that cover the ROI
        V m = V(0);
        int p0 = -1;
        for (int64_t vi = v0 + lane; vi <= v1; vi += 64) {
            V vals[EPV];
            lsc_load<T, EPV>(a.img, vi * EPV, vals);
            const int pbase = static_cast<int>(vi * EPV - e0);
#pragma unroll
            for (int k = 0; k < EPV; ++k) {
                const int p = pbase + k;
                V v = vals[k];
                if constexpr (sizeof(T) != 1) v += 0.0f;  // -0 -> +0: one key for both
                const bool take = p >= a.pb && p < a.pe && (p0 < 0 ? v == v : v > m);  // ascending p: the lowest position stays
                m = take ? v : m;
                p0 = take ? p : p0;
            }
        }
        // key = (m, 65535 - p0) as an exact non-negative double, 0 for "no sample": the largest is the maximum at its lowest position
        uint64_t key = 0;
        if (p0 >= 0) {
            if constexpr (sizeof(T) == 1) key = static_cast<uint64_t>(m + 1) << 16 | static_cast<uint64_t>(65535 - p0);
            else key = static_cast<uint64_t>(lsc_ord(m)) << 16 | static_cast<uint64_t>(65535 - p0);
        }
        key = static_cast<uint64_t>(lsc_readlane(wave_max63(static_cast<double>(key)), 63));
        const bool any = key != 0;
        p0 = 65535 - static_cast<int>(key & 0xffffu);
        if constexpr (sizeof(T) == 1) m = static_cast<int>(key >> 16) - 1;
        else m = lsc_unord(static_cast<uint32_t>(key >> 16));
        double sg = 0.0, sgp = 0.0;
        if (any) {  // wave-uniform
            int p1 = p0;
            for (;;) {  // the plateau: the run of samples equal to m after p0, 64 at a time
                const int q = p1 + 1 + lane;
                bool eq = false;
                if (q < a.pe) eq = lsc_load_one<T>(a.img, e0 + q) == m;
                const unsigned long long b = __ballot(eq);
                const int n = ~b == 0ull ? 64 : __builtin_ctzll(~b);
                p1 += n;
                if (n < 64) break;
            }
            int lo, hi;
            laser_window(p0, p1, a.hw, a.pb, a.pe, &lo, &hi);
            if constexpr (sizeof(T) == 1) {
                uint64_t ig = 0, igp = 0;
                for (int p = lo + lane; p <= hi; p += 64) laser_sum_u8(lsc_load_one<T>(a.img, e0 + p), p, a.floor_u8, &ig, &igp);
                sg = lsc_readlane(wave_sum63(static_cast<double>(ig)), 63);   // integers below 2^53: exact in any order
                sgp = lsc_readlane(wave_sum63(static_cast<double>(igp)), 63);
            } else {
                for (int base = lo; base <= hi; base += 64) {
                    const int p = base + lane;
                    double gl = 0.0, gp = 0.0;
                    if (p <= hi) laser_sum_f64(laser_g_f32(lsc_load_one<T>(a.img, e0 + p), a.floor_level), p, &gl, &gp);  // gl = g, gp = g p
                    const int cnt = min(64, hi - base + 1);
                    for (int j = 0; j < cnt; ++j) {  // ascending positions, one sum for the wavefront
                        sg += lsc_readlane(gl, j);
                        sgp += lsc_readlane(gp, j);
                    }
                }
            }
        }
        if (lane == 0) {
            const int frame = static_cast<int>(row / a.H);
            const int r = static_cast<int>(row - static_cast<int64_t>(frame) * a.H);
            lsc_emit<1>(a, g, frame, row, r, any, static_cast<double>(m), sg, sgp,
                        sizeof(T) == 1 ? static_cast<double>(a.floor_u8) : a.floor_level);
        }
    }
}

// ---- caller pixels -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LSC_BLOCK) void k_laser_points(int64_t n, const double* __restrict__ uv, int n_frames,
                                                            const int64_t* __restrict__ frame_offset, const double* __restrict__ Rt,
                                                            double* __restrict__ xyz, double* __restrict__ pxy, LaserGeom g) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(LSC_BLOCK) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * LSC_BLOCK) {
        const double2 p = reinterpret_cast<const double2*>(uv)[i];
        const double* rt = nullptr;
        if (Rt) {  // the frame f with frame_offset[f] <= i < frame_offset[f + 1] (empty frames are stepped over)
            int lo = 0, hi = n_frames;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (frame_offset[mid] <= i) lo = mid; else hi = mid;
            }
            rt = Rt + 12 * static_cast<int64_t>(lo);
        }
        double P[3], q[2];
        if (pxy) laser_point(g, p.x, p.y, rt, P, q);
        else laser_point(g, p.x, p.y, rt, P, nullptr);
        xyz[3 * i] = P[0];
        xyz[3 * i + 1] = P[1];
        xyz[3 * i + 2] = P[2];
        if (pxy) reinterpret_cast<double2*>(pxy)[i] = make_double2(q[0], q[1]);
    }
}

// ---- host glue ---------------------------------------------------------------------------------------------------------------------
// frame_offset / frame_pose7: both or neither (the caller supplies [0, n] for a single posed frame)
void laser_points_gpu(int model, const double* intr, int n_inv, const double* inv, const double* plane, int64_t n, const double* uv,
                      int n_frames, const int64_t* frame_offset, const double* frame_pose7, double* xyz, double* plane_xy, int device) {
    LaserGeom g;
    laser_fill_geom(model, intr, n_inv, inv, plane, &g);
    std::vector<double> hrt;
    if (frame_pose7) {
        hrt.resize(12 * static_cast<size_t>(n_frames));
        for (int f = 0; f < n_frames; ++f) laser_pose_rt(frame_pose7 + 7 * static_cast<size_t>(f), hrt.data() + 12 * static_cast<size_t>(f));
    }
    StreamLease lease(device);
    const hipStream_t s = lease;
    const size_t np = static_cast<size_t>(n);
    DevBuf<double> duv, dxyz, dpxy, drt;
    DevBuf<int64_t> doff;
    duv.alloc(2 * np);
    dxyz.alloc(3 * np);
    if (plane_xy) dpxy.alloc(2 * np);
    duv.upload(uv, 2 * np, s);
    if (frame_pose7) {
        drt.assign(hrt.data(), hrt.size(), s);
        doff.assign(frame_offset, static_cast<size_t>(n_frames) + 1, s);
    }
    hipLaunchKernelGGL(k_laser_points, dim3(launch_grid(n, LSC_BLOCK, LSC_GRID)), dim3(LSC_BLOCK), 0, s, n, duv.p, n_frames, doff.p, drt.p, dxyz.p, dpxy.p, g);
    CBA_HIP(hipGetLastError());
    dxyz.download(xyz, 3 * np, s);
    if (plane_xy) dpxy.download(plane_xy, 2 * np, s);
    CBA_HIP(hipStreamSynchronize(s));  // hrt and the device buffers go out of scope
}

// The scanner: camera, plane and options fixed at create, every buffer sized for max_frames there.  Every call ends with its stream
// synchronised.
struct LaserScanner : DeviceHandle {
    using DeviceHandle::DeviceHandle;
    LaserGeom geom;
    int axis = 0, W = 0, H = 0, max_frames = 0, pb = 0, pe = 0, hw = 0;
    double floor_level = 0.0, min_peak = 0.0;
    DevBuf<uint8_t> img;   // max_frames float32 frames + LSC_IMG_PAD
    DevBuf<double> out;    // [centre | amplitude | width_px | xyz (3)] x max_frames n_lines
    DevBuf<double> rt;     // [max_frames][12]
    std::vector<double> h_rt;
    int n_lines() const { return axis == 0 ? W : H; }
};
static_assert(!std::is_copy_constructible_v<LaserScanner> && !std::is_copy_assignable_v<LaserScanner>, "a handle owns its stream and buffers");

LaserScanner* laser_scanner_create(int model, const double* intr, int n_inv, const double* inv, const double* plane, int W, int H,
                                   int max_frames, const cba_laser_scan_options& o, int device) {
    auto h = std::make_unique<LaserScanner>(device);
    laser_fill_geom(model, intr, n_inv, inv, plane, &h->geom);
    h->axis = o.axis; h->W = W; h->H = H; h->max_frames = max_frames;
    const int side = o.axis == 0 ? H : W;
    const bool whole = o.roi_begin == 0 && o.roi_end == 0;
    h->pb = whole ? 0 : o.roi_begin;
    h->pe = whole ? side : o.roi_end;
    h->hw = std::min(o.half_window, CBA_IMAGE_MAX_SIDE);  // no side is longer: the window is the same and p0 - hw cannot overflow
    h->floor_level = o.floor_level;
    h->min_peak = o.min_peak;
    const size_t frames = static_cast<size_t>(std::max(max_frames, 1));
    h->img.alloc(frames * W * H * sizeof(float) + LSC_IMG_PAD);
    h->out.alloc(6 * frames * h->n_lines());
    h->rt.alloc(12 * frames);
    h->h_rt.resize(12 * frames);
    return h.release();
}

int laser_scanner_max_frames(const LaserScanner* h) { return h->max_frames; }

template <typename T>
static void lsc_launch(const LaserScanner& h, const LaserScanArgs& a, hipStream_t s) {
    constexpr int WIDE = 16 / static_cast<int>(sizeof(T)), NARROW = sizeof(T) == 1 ? 4 : 1;
    if (h.axis == 1) {
        hipLaunchKernelGGL(k_laser_scan_rows<T>, dim3(launch_grid(static_cast<int64_t>(a.n_frames) * a.H, LSC_WAVES, LSC_GRID)), dim3(LSC_BLOCK), 0, s, a,
                           h.geom);
    } else if (a.W % WIDE == 0) {  // every row starts on a 16-byte boundary
        const int bpf = (a.W + 64 * WIDE - 1) / (64 * WIDE);
        hipLaunchKernelGGL((k_laser_scan_cols<T, WIDE>), dim3(a.n_frames * bpf), dim3(LSC_BLOCK), 0, s, a, h.geom, bpf);
    } else {
        const int bpf = (a.W + 64 * NARROW - 1) / (64 * NARROW);
        hipLaunchKernelGGL((k_laser_scan_cols<T, NARROW>), dim3(a.n_frames * bpf), dim3(LSC_BLOCK), 0, s, a, h.geom, bpf);
    }
}

// stage_ms [3] (experiment builds): upload, kernel, download
void laser_scanner_process(LaserScanner* h, int n_frames, int dtype, const void* images, const double* frame_pose7, double* centre,
                           double* amplitude, double* width_px, double* xyz, double* stage_ms) {
    const hipStream_t s = h->begin();
    const size_t esz = dtype == CBA_DTYPE_F32 ? 4 : 1;
    const size_t L = static_cast<size_t>(n_frames) * h->n_lines(), Lmax = static_cast<size_t>(std::max(h->max_frames, 1)) * h->n_lines();
    StageTimer<4> tm(s, stage_ms != nullptr);
    tm.mark(0);
    h->img.upload(static_cast<const uint8_t*>(images), static_cast<size_t>(n_frames) * h->W * h->H * esz, s);
    if (frame_pose7) {
        for (int f = 0; f < n_frames; ++f) laser_pose_rt(frame_pose7 + 7 * static_cast<size_t>(f), h->h_rt.data() + 12 * static_cast<size_t>(f));
        h->rt.upload(h->h_rt.data(), 12 * static_cast<size_t>(n_frames), s);
    }
    tm.mark(1);
    LaserScanArgs a;
    a.img = h->img.p;
    a.W = h->W; a.H = h->H; a.n_frames = n_frames;
    a.pb = h->pb; a.pe = h->pe; a.hw = h->hw;
    a.floor_u8 = laser_floor_u8(h->floor_level);
    a.floor_level = h->floor_level;
    a.min_peak = h->min_peak;
    a.Rt = frame_pose7 ? h->rt.p : nullptr;
    a.centre = h->out.p;
    a.amplitude = h->out.p + Lmax;
    a.width_px = h->out.p + 2 * Lmax;
    a.xyz = h->out.p + 3 * Lmax;
    if (dtype == CBA_DTYPE_F32) lsc_launch<float>(*h, a, s);
    else lsc_launch<uint8_t>(*h, a, s);
    CBA_HIP(hipGetLastError());
    tm.mark(2);
    if (centre) h->out.download(centre, L, s, 0);
    if (amplitude) h->out.download(amplitude, L, s, Lmax);
    if (width_px) h->out.download(width_px, L, s, 2 * Lmax);
    if (xyz) h->out.download(xyz, 3 * L, s, 3 * Lmax);
    tm.mark(3);
    CBA_HIP(hipStreamSynchronize(s));
    tm.report(stage_ms);
}

void laser_scanner_destroy(LaserScanner* h) noexcept { destroy_handle(h); }

}  // namespace cba
