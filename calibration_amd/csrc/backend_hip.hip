// backend_hip.hip — the HIP implementation of cba::Backend (lm_core.hpp) on an Engine: struct HipBackend, the launch sequences of
// one LM step over the kernels of lm_kernels.hpp, and the engine's LM entry points (init_lm_state, warm_lm, solve_lm, covariance).
// The decision of a step is the controller kernel's (lm_ctl.hip), queued behind the exchange by the ctl_* functions of HipBackend;
// the collective itself is a host callback or RCCL over xGMI (collectives.cpp).
#include <rccl/rccl.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <thread>
#include <set>

#include "engine.hpp"
#include "pipelines.hpp"
#include "lm_core.hpp"
#include "lm_state.hpp"
#include "lm_kernels.hpp"

namespace cba {


static inline unsigned nblk(int64_t n, int per) { return static_cast<unsigned>(std::max<int64_t>(1, (n + per - 1) / per)); }

// runs f when the scope is left, by return or by exception: a launch sequence that borrows a piece of Engine state gives it back
template <class F>
struct ScopeExit {
    F f;
    ~ScopeExit() { f(); }
};
template <class F>
ScopeExit(F) -> ScopeExit<F>;

// ---- Backend on an Engine (state: lm_state.hpp) -------------------------------------------------------
struct HipBackend final : Backend {
    Engine& e;
    HipLMState& st;
    const double* lmp_src;  // [radius, init_scale] as the elimination kernels read it: page-locked host memory written by the host-side
                            // form of the iteration, or the controller's device copy
    explicit HipBackend(Engine& eng, HipLMState& s) : e(eng), st(s), lmp_src(s.pin_lmp.p) { st.current_is_on_device = false; }

    // the shared blocks as one packed run [intr | cam | target] (Engine::pk_cam, pk_target), and back
    void stage_shared(double* pk, const double* intr, const double* cam, const double* target) const {
        std::memcpy(pk, intr, sizeof(double) * e.h_intr.size());
        if (e.chain != CBA_CHAIN_INTRINSIC) std::memcpy(pk + e.pk_cam, cam, sizeof(double) * e.h_cam.size());
        if (e.chain == CBA_CHAIN_BUNDLE) std::memcpy(pk + e.pk_target, target, sizeof(double) * 7);
    }
    void unstage_shared(const double* pk, double* intr, double* cam, double* target) const {
        std::memcpy(intr, pk, sizeof(double) * e.h_intr.size());
        if (e.chain != CBA_CHAIN_INTRINSIC) std::memcpy(cam, pk + e.pk_cam, sizeof(double) * e.h_cam.size());
        if (e.chain == CBA_CHAIN_BUNDLE) std::memcpy(target, pk + e.pk_target, sizeof(double) * 7);
    }
    void set_lmp(double radius, bool init_scale) {  // [radius, init_scale] of the next elimination (the host-side form's copy)
        st.pin_lmp.p[0] = radius;
        st.pin_lmp.p[1] = init_scale ? 1.0 : 0.0;
    }
    // The second set of block sums / weights: a linearisation at a trial point goes there, so that the current set stays valid for
    // a rejected step.  with_alt_blocks(f): f's launches see the second set as THE set.
    void ensure_alt_blocks() {
        if (e.blk_acc_alt.n < e.blk_acc.n) { e.blk_acc_alt.alloc(e.blk_acc.n); e.blk_w_alt.alloc(e.blk_w.n); }
    }
    void swap_block_sets() {
        std::swap(e.blk_acc.p, e.blk_acc_alt.p);
        std::swap(e.blk_w.p, e.blk_w_alt.p);
    }
    template <class F>
    void with_alt_blocks(F&& f) {
        swap_block_sets();
        ScopeExit back{[this] { swap_block_sets(); }};
        f();
    }

    void set_view_fixed(const std::vector<int32_t>& f) override {
        if (!f.empty()) e.view_fixed.upload(f.data(), f.size(), e.stream);
        CBA_HIP(hipStreamSynchronize(e.stream));
    }
    // Copy 0 goes up at once as ONE copy of the packed blocks (page-locked staging: queued, not blocking).  Copy 1 is only
    // staged here: trial() uploads it together with the shared step.  Right after accept() the device already holds the
    // accepted point in copy 0 (k_accept), so the driver's upload of the same values is skipped.
    void upload_shared(int which, const double* intr, const double* cam, const double* target) override {
        if (which == 0 && st.current_is_on_device) { st.current_is_on_device = false; return; }
        double* pk = st.pin_pack[which].p;
        stage_shared(pk, intr, cam, target);
        if (which == 0) {
            // the staging area may still be the source of the previous upload: wait for the stream first (rare path:
            // start of a solve, covariance)
            e.shared_pack[0].upload(pk, e.pk_delta, e.stream);
            CBA_HIP(hipStreamSynchronize(e.stream));
        }
    }
    // ---- stage plumbing: host preparation (every call) / device enqueue (captured once) / result collection ----------
    template <class F>
    void run_stage(HipLMState::GraphSlot& slot, double huber, bool constrained, F&& enqueue) {
        if (!st.graphs_ok) { enqueue(); return; }
        if (slot.huber != huber || slot.constrained != static_cast<int>(constrained) || slot.scalar != e.scalar) {
            if (slot.exec) (void)hipGraphExecDestroy(slot.exec);
            slot.exec = nullptr;
            slot.uses = 0;
            slot.huber = huber; slot.constrained = static_cast<int>(constrained); slot.scalar = e.scalar;
        }
        if (!slot.exec && slot.uses < st.graph_after) {
            ++slot.uses;
            enqueue();
            return;
        }
        if (!slot.exec) {
            if (hipStreamBeginCapture(e.stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
                (void)hipGetLastError();
                st.graphs_ok = false;
                enqueue();
                return;
            }
            hipGraph_t graph = nullptr;
            try {
                enqueue();
            } catch (...) {
                (void)hipStreamEndCapture(e.stream, &graph);
                if (graph) (void)hipGraphDestroy(graph);
                throw;
            }
            const hipError_t ec = hipStreamEndCapture(e.stream, &graph);
            const hipError_t ei = (ec == hipSuccess && graph) ? hipGraphInstantiate(&slot.exec, graph, nullptr, nullptr, 0) : hipErrorUnknown;
            if (graph) (void)hipGraphDestroy(graph);
            if (ei != hipSuccess) {  // no graph support for this sequence: plain launches from now on
                (void)hipGetLastError();
                slot.exec = nullptr;
                st.graphs_ok = false;
                enqueue();
                return;
            }
        }
        CBA_HIP(hipGraphLaunch(slot.exec, e.stream));
    }

    bool prep_normal_eq(std::vector<double>& cam_acc, double cost2[2]) {
        const Structure& s = st.s;
        cam_acc.assign(static_cast<size_t>(s.n_cams) * s.NACC, 0.0);
        cost2[0] = cost2[1] = 0.0;
        return s.n_blocks != 0;
    }
    // which: parameter copy to linearise at; cam_out [n_cams][NACC] and cost_out {cost, sum s} may be device or page-locked host memory
    void enqueue_normal_eq(double huber, int which = 0, double* cam_out = nullptr, double* cost_out = nullptr) {
        enqueue_normal_eq_head(which, huber);
        enqueue_normal_eq_tail(huber, cam_out, cost_out);
    }
    // block constants at copy `which` (unless the caller has built them: k_step_head), Mode B: the per-block [H | g | s]; huber >= 0:
    // the kernel that finishes a block's row also leaves its robust weight where it can (Engine::head_weights says whether it did)
    void enqueue_normal_eq_head(int which, double huber = -1.0, bool consts_done = false) {
        if (!consts_done) launch_block_consts(e, which);
        e.head_huber = st.fuse_small ? huber : -1.0;
        ScopeExit reset{[this] { e.head_huber = -1.0; }};
        launch_normal_eq(e);
    }
    void enqueue_normal_eq_tail(double huber, double* cam_out = nullptr, double* cost_out = nullptr) {  // weights, cost, per-camera sums
        const Structure& s = st.s;
        const size_t nca = static_cast<size_t>(s.n_cams) * s.NACC;
        if (!cam_out) cam_out = st.pin_ne.p;
        if (!cost_out) cost_out = st.pin_ne.p + nca;
        const bool fused_cost = s.n_blocks <= 4096 && !e.head_weights;
        if (e.head_weights)
            ;  // the weights came with the block rows; the cost follows below
        else if (fused_cost)
            hipLaunchKernelGGL(k_weights_cost, dim3(1), dim3(256), 0, e.stream, s.n_blocks, s.NACC, s.NH + s.PL, e.blk_acc.p, huber,
                               e.blk_w.p, e.blk_s.p, cost_out);
        else
            hipLaunchKernelGGL(k_weights, dim3(nblk(s.n_blocks, 256)), dim3(256), 0, e.stream, s.n_blocks, s.NACC, s.NH + s.PL,
                               e.blk_acc.p, huber, e.blk_w.p, e.blk_s.p);
        hipLaunchKernelGGL(k_cam_partial, dim3(std::max(1, st.n_cchunks)), dim3(256), 0, e.stream, s.NACC, st.cchunk_off.p,
                           st.cam_blk.p, e.blk_w.p, e.blk_acc.p, st.cam_partial.p);
        // the stage's results are written straight into page-locked host memory (device-visible): no copy command on the stream
        hipLaunchKernelGGL(k_seg_sum, dim3(nblk(s.NACC, RS_COLS), s.n_cams), dim3(RS_COLS * RS_GROUPS), 0, e.stream, s.n_cams,
                           s.NACC, st.cam_seg.p, st.cam_partial.p, cam_out);
        if (!fused_cost) launch_cost(e, huber, cost_out);
        CBA_HIP(hipGetLastError());
    }
    // ---- one linear solve's small stages in three launches (k_sys_stage2 / 3 / k_sys_pack, lm_kernels.hpp) ---------------------------
    bool vstats_pending = false;  // k_step_head has left the views' step statistics unreduced: stage 3 takes them along
    double ctl_huber = 0.0;       // the Huber parameter of the running solve (the head of a step is queued without one at hand)
    bool can_fuse() const { return st.fuse_small && st.schur_wave && st.s.n_views != 0 && !e.scalar; }
    // Everything between Mode B and the exchange: [weights, cost, camera sums] (tail), the elimination of the views at private copy
    // `which`, the contraction and the pack.  has_blocks / has_stats / has_cost: PackArgs.
    void enqueue_system(double huber, bool tail, bool has_blocks, bool constrained, int which, const PackLayout& L, int has_stats, int has_cost = -1) {
        const Structure& s = st.s;
        const bool q2 = s.n_views != 0;
        if (!can_fuse()) {
            if (tail) enqueue_normal_eq_tail(huber, pack_target() + L.cam, st.stat_dev.p + 4);
            if (q2) enqueue_schur(constrained, which, st.sys_tiles.p);
            enqueue_pack(L, has_blocks, q2, has_stats, has_cost);
            return;
        }
        const int n = s.nsh;
        const int64_t sw = static_cast<int64_t>(st.n_pairs) * 4096;
        if (tail && !e.head_weights)
            hipLaunchKernelGGL(k_weights, dim3(nblk(s.n_blocks, 256)), dim3(256), 0, e.stream, s.n_blocks, s.NACC, s.NH + s.PL, e.blk_acc.p,
                               huber, e.blk_w.p, e.blk_s.p);
        SysArgs a{};
        a.d = st.dims; a.n_views = s.n_views; a.n_blocks = s.n_blocks; a.nsh = n; a.n_tiles = st.n_tiles; a.n_pairs = st.n_pairs;
        a.n_vchunks = st.n_vchunks; a.n_cams = s.n_cams; a.NACC = s.NACC; a.constrained = constrained ? 1 : 0;
        a.n_cc = tail ? std::max(1, st.n_cchunks) : 0;
        a.n_vb = static_cast<int>(nblk(s.n_views, 4));
        a.n_costp = tail ? (s.n_blocks <= 4096 ? 1 : (s.n_blocks + 2047) / 2048) : 0;
        a.n_seg_x = static_cast<int>(nblk(s.NACC, RS_COLS));
        a.n_seg = tail ? a.n_seg_x * s.n_cams : 0;
        a.n_syrk = st.n_vchunks * st.n_pairs;
        a.has_vstats = vstats_pending ? 1 : 0;
        a.huber = huber;
        a.link_off = st.link_off.p; a.cchunk_off = st.cchunk_off.p; a.cam_seg = st.cam_seg.p;
        a.link_blk = st.link_blk.p; a.cam_blk = st.cam_blk.p; a.view_fixed = e.view_fixed.p; a.view_cam_blk = st.view_cam_blk.p;
        a.blk_acc = e.blk_acc.p; a.blk_w = e.blk_w.p; a.blk_s = e.blk_s.p; a.lmp = lmp_src; a.view = e.view[which].p;
        a.view_scale2 = e.view_scale2.p; a.view_L = e.view_L.p; a.view_y = e.view_y.p; a.view_D = e.view_D.p; a.view_gp = e.view_gp.p;
        a.blk_Z = e.blk_Z.p; a.view_gmax = st.view_gmax.p; a.cam_partial = st.cam_partial.p; a.cam_out = pack_target() + L.cam;
        if (a.n_costp > 1) e.cost_part.ensure(static_cast<size_t>(2 * a.n_costp));
        a.cost_part = e.cost_part.p; a.cost_out = st.stat_dev.p + 4;
        a.syrk_partial = st.syrk_partial.p; a.tiles_tail = st.sys_tiles.p + sw + n; a.view_stats = st.view_stats.p; a.stat_out = st.stat_dev.p;
        hipLaunchKernelGGL(k_sys_stage2, dim3(a.n_cc + a.n_vb + a.n_costp), dim3(256), 0, e.stream, a);
        const unsigned g3 = static_cast<unsigned>(a.n_seg + a.n_syrk + 1 + a.has_vstats + (a.n_costp > 1 ? 1 : 0));
        if (n >= 64 && st.syrk_mfma) hipLaunchKernelGGL(k_sys_stage3<true>, dim3(g3), dim3(256), 0, e.stream, a);
        else hipLaunchKernelGGL(k_sys_stage3<false>, dim3(g3), dim3(256), 0, e.stream, a);
        vstats_pending = false;
        hipLaunchKernelGGL(k_sys_pack, dim3(nblk(sw + n, RS_COLS)), dim3(RS_COLS * RS_GROUPS), 0, e.stream,
                           pack_args(L, has_blocks, true, has_stats, has_cost), static_cast<int64_t>(st.n_vchunks), st.syrk_partial.p,
                           st.sys_tiles.p + sw + n, st.stat_dev.p, pack_target());
        CBA_HIP(hipGetLastError());
    }
    void collect_normal_eq(std::vector<double>& cam_acc, double cost2[2]) {
        std::memcpy(cam_acc.data(), st.pin_ne.p, sizeof(double) * cam_acc.size());
        cost2[0] = st.pin_ne.p[cam_acc.size()];
        cost2[1] = st.pin_ne.p[cam_acc.size() + 1];
        e.active = 0;
    }
    bool prep_schur(double radius, bool init_scale, std::vector<double>& S, std::vector<double>& g, double* gmax_priv, int* nfail) {
        const Structure& s = st.s;
        const int n = s.nsh;
        S.assign(static_cast<size_t>(n) * n, 0.0);
        g.assign(n, 0.0);
        *gmax_priv = 0.0;
        *nfail = 0;
        if (s.n_views == 0) return false;
        set_lmp(radius, init_scale);
        return true;
    }
    // which: private pose copy the elimination is made at; tiles_out [syrk tiles | g_schur | gmax, #failed] device or page-locked
    void enqueue_schur(bool constrained, int which = 0, double* tiles_out = nullptr) {
        const Structure& s = st.s;
        const int n = s.nsh;
        const int vpw = st.schur_wave ? 4 : 64;  // views per workgroup: one wavefront, or one thread, per view
        hipLaunchKernelGGL(st.schur_wave ? k_schur_view_wave : k_schur_view, dim3(nblk(s.n_views, vpw)), dim3(st.schur_wave ? 256 : 64), 0,
                           e.stream, st.dims, s.n_views, st.link_off.p, st.link_blk.p, e.blk_acc.p, e.blk_w.p, e.view_fixed.p, lmp_src,
                           constrained ? 1 : 0, e.view[which].p, e.view_scale2.p, e.view_L.p, e.view_y.p, e.view_D.p, e.view_gp.p, e.blk_Z.p,
                           st.view_gmax.p);
        const int64_t sw = static_cast<int64_t>(st.n_pairs) * 4096;
        hipLaunchKernelGGL(n >= 64 && st.syrk_mfma ? k_schur_syrk_mfma : k_schur_syrk, dim3(st.n_vchunks, st.n_pairs), dim3(256), 0, e.stream,
                           st.dims, s.n_views, n, st.n_tiles, st.view_cam_blk.p, e.blk_Z.p, e.view_y.p, st.syrk_partial.p);
        double* pack = tiles_out ? tiles_out : st.pin.p;  // [syrk tiles | g_schur | gmax, #failed views]; default: page-locked host memory
        hipLaunchKernelGGL(k_row_sum, dim3(nblk(sw + n, RS_COLS)), dim3(RS_COLS * RS_GROUPS), 0, e.stream, static_cast<int64_t>(st.n_vchunks),
                           sw + n, st.syrk_partial.p, pack);
        hipLaunchKernelGGL(k_col_reduce, dim3(1), dim3(256), 0, e.stream, s.n_views, 0, st.view_gmax.p, st.view_gmax.p, pack + sw + n);
        CBA_HIP(hipGetLastError());
    }
    void collect_schur(std::vector<double>& S, std::vector<double>& g, double* gmax_priv, int* nfail) {
        const Structure& s = st.s;
        const int n = s.nsh;
        const int64_t sw = static_cast<int64_t>(st.n_pairs) * 4096;
        const double* tiles = st.pin.p;
        const int32_t nf = static_cast<int32_t>(tiles[static_cast<size_t>(sw) + n + 1] + 0.5);
        for (int i = 0; i < n; ++i) g[i] = tiles[static_cast<size_t>(sw) + i];
        *gmax_priv = tiles[static_cast<size_t>(sw) + n];
        *nfail = nf;
        int pair = 0;
        for (int ti = 0; ti < st.n_tiles; ++ti)
            for (int tj = ti; tj < st.n_tiles; ++tj, ++pair) {
                const double* T = &tiles[static_cast<size_t>(pair) * 4096];
                for (int a = 0; a < 64; ++a) {
                    const int i = ti * 64 + a;
                    if (i >= n) break;
                    for (int b = 0; b < 64; ++b) {
                        const int j = tj * 64 + b;
                        if (j >= n) break;
                        S[static_cast<size_t>(i) * n + j] = T[a * 64 + b];
                        S[static_cast<size_t>(j) * n + i] = T[a * 64 + b];
                    }
                }
            }
    }

    void normal_eq(double huber, std::vector<double>& cam_acc, double cost2[2]) override {  // covariance / cost paths: plain launches
        if (!prep_normal_eq(cam_acc, cost2)) return;
        enqueue_normal_eq(huber);
        CBA_HIP(hipStreamSynchronize(e.stream));
        collect_normal_eq(cam_acc, cost2);
    }
    void schur(double radius, bool init_scale, bool constrained, std::vector<double>& S, std::vector<double>& g, double* gmax_priv,
               int* nfail) override {
        if (!prep_schur(radius, init_scale, S, g, gmax_priv, nfail)) return;
        run_stage(st.g_schur, 0.0, constrained, [&] { enqueue_schur(constrained); });
        CBA_HIP(hipStreamSynchronize(e.stream));
        collect_schur(S, g, gmax_priv, nfail);
    }
    // a new linearisation: every kernel of both stages and both result copies in one graph, ONE stream synchronisation
    void normal_eq_schur(double huber, std::vector<double>& cam_acc, double cost2[2], double radius, bool init_scale, bool constrained,
                         std::vector<double>& S, std::vector<double>& g, double* gmax_priv, int* nfail) override {
        const bool q1 = prep_normal_eq(cam_acc, cost2);
        const bool q2 = prep_schur(radius, init_scale, S, g, gmax_priv, nfail);
        if (!q1 && !q2) return;
        run_stage(st.g_new, huber, constrained, [&] {
            if (q1) enqueue_normal_eq(huber);
            if (q2) enqueue_schur(constrained);
        });
        CBA_HIP(hipStreamSynchronize(e.stream));
        if (q1) collect_normal_eq(cam_acc, cost2);
        if (q2) collect_schur(S, g, gmax_priv, nfail);
    }
    // ---- packed systems (lm_core.hpp): assembled on the device, ONE all-reduce in place on the engine's stream (RCCL), one
    // device-to-host copy of the reduced buffer, one synchronisation ---------------------------------------------------------------
    PackArgs pack_args(const PackLayout& L, bool has_blocks, bool has_schur, int has_stats, int has_cost) const {
        const Structure& s = st.s;
        PackArgs a;
        a.off_stats = L.stats; a.off_cam = L.cam; a.off_cost = L.cost; a.off_nfail = L.nfail; a.off_S = L.S; a.off_g = L.g; a.off_gmax = L.gmax;
        a.n = s.nsh; a.n_tiles = st.n_tiles; a.n_ranks = L.n_ranks; a.rank = e.rank; a.n_cam_doubles = s.n_cams * s.NACC;
        a.has_blocks = has_blocks; a.has_schur = has_schur; a.has_stats = has_stats; a.has_cost = has_cost < 0 ? has_blocks : has_cost;
        return a;
    }
    void ensure_pack(const PackLayout& L) {
        if (st.pack_dev.n < static_cast<size_t>(L.size)) {
            st.pack_dev.alloc(static_cast<size_t>(L.size));
            st.pack_dev.zero(e.stream);
            st.sys_tiles.alloc(static_cast<size_t>(st.n_pairs) * 4096 + st.s.nsh + 8);
            st.stat_dev.alloc(8);
            st.stat_dev.zero(e.stream);
        }
        st.pin_packed.reserve(static_cast<size_t>(L.size));
    }
    // Where the pack is assembled: in device memory, where RCCL reduces it in place and the controller (lm_ctl.hip) reads it;
    // with a host-callback transport (gloo / MPI) the kernels write it straight into page-locked host memory instead.
    bool host_transport() const { return !e.rccl_comm && e.allreduce != nullptr; }
    double* pack_target() { return host_transport() ? st.pin_packed.p : st.pack_dev.p; }
    void enqueue_pack(const PackLayout& L, bool has_blocks, bool has_schur, int has_stats, int has_cost = -1) {
        const int64_t work = std::max<int64_t>({static_cast<int64_t>(st.s.nsh) * st.s.nsh, static_cast<int64_t>(st.s.n_cams) * st.s.NACC, L.n_ranks, 1});
        hipLaunchKernelGGL(k_pack, dim3(nblk(work, 256)), dim3(256), 0, e.stream, pack_args(L, has_blocks, has_schur, has_stats, has_cost),
                           st.stat_dev.p, st.sys_tiles.p, pack_target());
        CBA_HIP(hipGetLastError());
    }
    void wait_step() {
        if (!st.sync_spin) { CBA_HIP(hipStreamSynchronize(e.stream)); return; }
        if (!st.step_done) CBA_HIP(hipEventCreateWithFlags(&st.step_done, hipEventDisableTiming));
        CBA_HIP(hipEventRecord(st.step_done, e.stream));
        const auto t0 = std::chrono::steady_clock::now();
        for (int spins = 0;; ++spins) {
            const hipError_t q = hipEventQuery(st.step_done);
            if (q == hipSuccess) return;
            if (q != hipErrorNotReady) CBA_HIP(q);
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            // a long stage (Mode B over 1e7+ observations) gains nothing from polling: sleep after 300 us
            if ((spins & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300)) break;
        }
        CBA_HIP(hipStreamSynchronize(e.stream));
    }
    // Sum [off, off + count) of the packed buffer over the ranks.  host_out != nullptr: the reduced range is also brought to the
    // host (the host-side form of the iteration, line-search samples); to_device: with a host transport the reduced range goes
    // back up for the controller.
    void exchange(int64_t off, int64_t count, const AllReduce& ar, double* host_out, bool to_device = false) {
        if (e.rccl_comm) {  // RCCL over xGMI, in place on the device buffer, on the engine's stream: no host staging
            const ncclResult_t r = ncclAllReduce(st.pack_dev.p + off, st.pack_dev.p + off, static_cast<size_t>(count), ncclDouble, ncclSum,
                                                 reinterpret_cast<ncclComm_t>(e.rccl_comm), e.stream);
            if (r != ncclSuccess) throw HipError(std::string("ncclAllReduce: ") + ncclGetErrorString(r));
            ++device_allreduce_calls;
            device_allreduce_doubles += count;
        } else if (host_transport()) {  // gloo / MPI callback on the page-locked pack
            wait_step();
            ar(st.pin_packed.p + off, count);
            if (to_device) st.pack_dev.upload(st.pin_packed.p + off, static_cast<size_t>(count), e.stream, static_cast<size_t>(off));
            if (host_out) std::memcpy(host_out + off, st.pin_packed.p + off, sizeof(double) * static_cast<size_t>(count));
            return;
        } else {  // a single rank: the exchange is the identity (counted like one: the protocol does not depend on the rank count)
            ++device_allreduce_calls;
            device_allreduce_doubles += count;
        }
        if (host_out) {
            st.pack_dev.download(st.pin_packed.p + off, static_cast<size_t>(count), e.stream, static_cast<size_t>(off));
            wait_step();
            std::memcpy(host_out + off, st.pin_packed.p + off, sizeof(double) * static_cast<size_t>(count));
        }
    }
    void sys_new(double huber, double radius, bool init_scale, bool constrained, const PackLayout& L, const AllReduce& ar, int rank,
                 double* pack) override {
        (void)rank;
        const Structure& s = st.s;
        ensure_pack(L);
        const bool q1 = s.n_blocks != 0;
        set_lmp(radius, init_scale);
        ctl_huber = huber;
        if (q1) enqueue_normal_eq_head(0, huber);
        enqueue_system(huber, q1, q1, constrained, 0, L, 0);
        exchange(L.cam, L.size - L.cam, ar, pack);
        e.active = 0;
    }
    void sys_resolve(double radius, bool constrained, const PackLayout& L, const AllReduce& ar, int rank, double* pack) override {
        (void)rank;
        const Structure& s = st.s;
        ensure_pack(L);
        set_lmp(radius, false);
        enqueue_system(0.0, false, s.n_blocks != 0, constrained, 0, L, 0, 0);  // only [nfail .. g] travels (the cost slot, outside that range, is not a cost after this)
        exchange(L.nfail, L.gmax - L.nfail, ar, pack);
    }
    bool sys_step(const double* delta_sh, double huber, double radius_next, bool constrained, const PackLayout& L, const AllReduce& ar,
                  int rank, double* pack) override {
        (void)rank;
        const Structure& s = st.s;
        if (e.scalar) return false;  // fp32 study mode keeps the plain sequence
        ensure_pack(L);
        ensure_alt_blocks();
        std::memcpy(st.pin_pack[1].p + e.pk_delta, delta_sh, sizeof(double) * s.nsh);
        e.shared_pack[1].upload(st.pin_pack[1].p, e.pk_delta + static_cast<size_t>(s.nsh), e.stream);  // trial blocks + step
        // statistics of the step from the CURRENT factors, trial poses into copy 1; then the linearisation at the trial point into the
        // second set of block sums / weights (the current set stays valid for a rejected step)
        set_lmp(radius_next, false);
        ctl_huber = huber;
        step_head_speculative();
        step_tail_enqueue(huber, constrained, L);
        exchange(0, L.size, ar, pack);
        e.active = 1;
        return true;
    }
    void line_eval(double a, double huber, bool want_slope, const PackLayout& L, const AllReduce& ar, int rank, double* pack) override {
        (void)rank;
        const Structure& s = st.s;
        ensure_pack(L);
        if (want_slope) ensure_alt_blocks();
        const bool q1 = s.n_blocks != 0, q2 = s.n_views != 0;
        e.shared_pack[1].upload(st.pin_pack[1].p, e.pk_delta, e.stream);  // the shared blocks at this step size (staged by upload_shared(1))
        if (q2)
            hipLaunchKernelGGL(k_scale_step, dim3(nblk(s.n_views, 64)), dim3(64), 0, e.stream, s.n_views, a, e.view_fixed.p, e.view[0].p,
                               st.view_delta.p, e.view[1].p, st.view_stats.p);
        if (q1 && want_slope) {  // linearise at the sample into the second set of block sums (the current set stays valid)
            with_alt_blocks([&] {
                enqueue_normal_eq(huber, 1, pack_target() + L.cam, st.stat_dev.p + 4);
                if (q2)
                    hipLaunchKernelGGL(k_view_slope, dim3(nblk(s.n_views, 64)), dim3(64), 0, e.stream, st.dims, s.n_views, st.link_off.p,
                                       st.link_blk.p, e.blk_acc.p, e.blk_w.p, e.view_fixed.p, st.view_delta.p, st.view_stats.p);
            });
        } else if (q1) {  // the cost alone (Mode R)
            launch_block_consts(e, 1);
            launch_resid(e);
            launch_cost(e, huber, st.stat_dev.p + 4);
        }
        if (q2)
            hipLaunchKernelGGL(k_col_reduce, dim3(1), dim3(256), 0, e.stream, s.n_views, 4, st.view_stats.p, static_cast<const double*>(nullptr),
                               st.stat_dev.p);
        else
            CBA_HIP(hipMemsetAsync(st.stat_dev.p, 0, 4 * sizeof(double), e.stream));
        CBA_HIP(hipGetLastError());
        enqueue_pack(L, q1 && want_slope, false, 2, q1 ? 1 : 0);
        exchange(0, L.size, ar, pack);
        e.active = 1;
    }
    void launch_accept() {  // trial copies -> current copies: the shared pack and the private poses
        const int64_t n_shared = static_cast<int64_t>(e.pk_delta), n_view = static_cast<int64_t>(e.h_view.size());
        hipLaunchKernelGGL(k_accept, dim3(nblk(std::max(n_shared, n_view), 256)), dim3(256), 0, e.stream, n_shared, e.shared_pack[1].p,
                           e.shared_pack[0].p, n_view, e.view[1].p, e.view[0].p);
    }
    void accept_step() override {
        launch_accept();
        const int64_t n_acc = static_cast<int64_t>(st.s.n_blocks) * st.s.NACC, n_w = st.s.n_blocks;
        if (n_acc > 0)
            hipLaunchKernelGGL(k_accept_blocks, dim3(nblk(n_acc, 256)), dim3(256), 0, e.stream, n_acc, e.blk_acc_alt.p, e.blk_acc.p, n_w,
                               e.blk_w_alt.p, e.blk_w.p);
        CBA_HIP(hipGetLastError());
        e.active = 1;  // bc / sd were built from copy 1 = the values copy 0 now holds
    }

    // ---- the controller form of the iteration (lm_core.hpp Backend::ctl_*, lm_ctl.hip) ---------------------------------------------
    // Nothing below waits except ctl_wait(): the launch sequences are queued on the engine's stream, the controller kernel behind
    // the exchange decides, and what the host needs to know arrives in the control record.
    bool ctl_constrained = false;
    int64_t ctl_invocations = 0;
    void ensure_ctl(const PackLayout& L) {
        const Structure& s = st.s;
        const int n = s.nsh;
        const int lda = ctl_lda(n), M8 = ctl_padded(n);
        const bool lds = lm_ctl_fits_lds(n);
        const size_t o_scal = 0, o_lmp = CS_COUNT, o_camc = o_lmp + 8, o_gc = o_camc + static_cast<size_t>(s.n_cams) * s.NACC, o_scale2 = o_gc + n,
                     o_hdiag = o_scale2 + n, o_xs = o_hdiag + n, o_rdiag = o_xs + M8, o_xtmp = o_rdiag + M8, o_Ld = o_xtmp + e.pk_size,
                     o_A = o_Ld + static_cast<size_t>(M8) * CTL_NB, total = o_A + (lds ? 8 : static_cast<size_t>(M8 + 1) * lda);
        if (st.ctl_n != n || st.ctl_buf.n < total) {
            st.ctl_buf.alloc(total);
            st.ctl_buf.zero(e.stream);
            st.ctl_idx.alloc(static_cast<size_t>(3 * std::max(1, n)));  // [effective columns | column -> camera | column -> local column]
            st.ctl_eff.alloc(static_cast<size_t>(std::max(1, n)));
            {   // the column tables (structure.hpp shared_col, inverted), once per problem
                std::vector<int32_t> tab(static_cast<size_t>(3 * std::max(1, n)), 0);
                CtlView T{};
                T.chain = s.chain; T.PC = s.PC;
                for (int i = 0; i < n; ++i) ctl_decode(T, i, &tab[static_cast<size_t>(n) + i], &tab[static_cast<size_t>(2 * n) + i]);
                st.ctl_idx.upload(tab.data(), tab.size(), e.stream);
                CBA_HIP(hipStreamSynchronize(e.stream));
            }
            st.ctl_rec.reserve(CTL_REC_FETCH + e.pk_size + static_cast<size_t>(n) + 8);
            st.ctl_n = n;
        }
        CtlView& V = st.ctl_view;
        V.n = n; V.n_cams = s.n_cams; V.PI = s.PI; V.PL = s.PL; V.NH = s.NH; V.NACC = s.NACC; V.PC = s.PC; V.sh_base = s.sh_base;
        V.chain = s.chain; V.n_ranks = L.n_ranks;
        V.off_stats = L.stats; V.off_cam = L.cam; V.off_cost = L.cost; V.off_nfail = L.nfail; V.off_S = L.S; V.off_g = L.g; V.off_gmax = L.gmax;
        V.pk_cam = static_cast<int64_t>(e.pk_cam); V.pk_target = static_cast<int64_t>(e.pk_target); V.pk_delta = static_cast<int64_t>(e.pk_delta);
        double* b = st.ctl_buf.p;
        V.x_cur = e.shared_pack[0].p; V.x_trial = e.shared_pack[1].p; V.x_tmp = b + o_xtmp;
        V.scal = b + o_scal; V.lmp = b + o_lmp; V.camc = b + o_camc; V.gc = b + o_gc; V.scale2 = b + o_scale2; V.hdiag = b + o_hdiag; V.xs = b + o_xs;
        V.rdiag = b + o_rdiag; V.A = b + o_A; V.Ld = b + o_Ld; V.lda = lda; V.okflag = nullptr;  // (okflag: LDS, set by the kernel)
        V.pack = st.pack_dev.p;
        V.eff = st.ctl_eff.p; V.idx = st.ctl_idx.p; V.colcam = st.ctl_idx.p + n; V.collc = st.ctl_idx.p + 2 * n;
        V.active = st.res_active.p; V.cam_var = st.res_cam_var.p;
        V.rec = st.ctl_rec.p;
    }
    void run_ctl(int mode, int flag) {
        launch_lm_ctl(st.ctl_view, mode, flag, e.stream);
        ++ctl_invocations;
        if (st.ctl_event) {  // (experiment builds: ctl_wait sleeping on an event behind THIS launch; see there why not)
            if (!st.ctl_done) CBA_HIP(hipEventCreateWithFlags(&st.ctl_done, hipEventDisableTiming));
            CBA_HIP(hipEventRecord(st.ctl_done, e.stream));
        }
    }
    bool ctl_begin(const CtlSetup& cs, const PackLayout& L) override {
        if (!st.lm_ctl_mode) return false;
        const Structure& s = st.s;
        ensure_pack(L);
        ensure_ctl(L);
        ensure_alt_blocks();
        CtlView& V = st.ctl_view;
        V.eps = cs.eps; V.max_iterations = cs.max_iterations; V.constrained = cs.constrained; V.line_search = cs.line_search;
        V.speculate = (cs.speculate && !e.scalar) ? 1 : 0;  // the fp32 study mode keeps the plain sequence
        V.intr_var = cs.intr_var; V.target_var = cs.target_var;
        ctl_constrained = cs.constrained;
        // masks, control scalars, [radius, init_scale] and the start point: page-locked staging, queued copies
        st.pin_mask.reserve(static_cast<size_t>(s.nsh + s.n_cams));
        for (int i = 0; i < s.nsh; ++i) st.pin_mask.p[i] = (*cs.active)[i];
        for (int c = 0; c < s.n_cams; ++c) st.pin_mask.p[s.nsh + c] = (*cs.cam_var)[c];
        st.res_active.upload(st.pin_mask.p, s.nsh, e.stream);
        st.res_cam_var.upload(st.pin_mask.p + s.nsh, s.n_cams, e.stream);
        double* stage = st.ctl_rec.p + CS_COUNT;  // [scal | lmp] then the start point
        ctl_reset(stage);
        stage[CS_COUNT] = 1e4; stage[CS_COUNT + 1] = 1.0;
        st.ctl_buf.upload(stage, CS_COUNT + 2, e.stream);
        for (int k = 0; k < CS_COUNT; ++k) st.ctl_rec.p[k] = 0.0;
        double* pk = st.pin_pack[0].p;
        stage_shared(pk, cs.intr, cs.cam, cs.target);
        e.shared_pack[0].upload(pk, e.pk_delta, e.stream);
        e.shared_pack[1].upload(pk, e.pk_delta, e.stream);
        lmp_src = V.lmp;
        ctl_invocations = 0;
        st.current_is_on_device = false;
        return true;
    }
    void ctl_new(double huber, bool first, const PackLayout& L, const AllReduce& ar, int rank) override {
        (void)rank;
        const Structure& s = st.s;
        const bool q1 = s.n_blocks != 0;
        ctl_huber = huber;
        if (q1) enqueue_normal_eq_head(0, huber);
        enqueue_system(huber, q1, q1, ctl_constrained, 0, L, 0);
        exchange(L.cam, L.size - L.cam, ar, nullptr, true);
        run_ctl(CTL_NEW, first ? 1 : 0);
        e.active = 0;
    }
    void ctl_resolve(const PackLayout& L, const AllReduce& ar, int rank) override {
        (void)rank;
        const Structure& s = st.s;
        enqueue_system(0.0, false, s.n_blocks != 0, ctl_constrained, 0, L, 0, 0);  // only [nfail .. g] travels
        exchange(L.nfail, L.gmax - L.nfail, ar, nullptr, true);
        run_ctl(CTL_RESOLVED, 0);
    }
    // delta_p, trial poses (copy 1) and the views' share of the step statistics, from the CURRENT factors; stat_out[0..4) device or
    // page-locked host memory
    void launch_backsub(const double* gate, double* stat_out) {
        const Structure& s = st.s;
        hipLaunchKernelGGL(st.schur_wave ? k_backsub_wave : k_backsub, st.schur_wave ? dim3(nblk(s.n_views, 4)) : dim3(nblk(s.n_views, 64)),
                           st.schur_wave ? dim3(256) : dim3(64), 0, e.stream, st.dims, s.n_views, st.link_off.p, st.link_blk.p, e.d_blk_cam.p,
                           e.blk_Z.p, e.delta_sh.p, e.view_fixed.p, e.view_L.p, e.view_y.p, e.view_D.p, e.view_gp.p, e.view[0].p,
                           st.view_delta.p, e.view[1].p, st.view_stats.p, gate);
        hipLaunchKernelGGL(k_col_reduce, dim3(1), dim3(256), 0, e.stream, s.n_views, 4, st.view_stats.p, static_cast<const double*>(nullptr),
                           stat_out, gate);
    }
    void enqueue_backsub() { launch_backsub(e.gate, st.stat_dev.p); }
    // The head of a speculative step: back-substitution, then block constants and Mode B at the trial point into the SECOND set of
    // block sums (the current set stays valid for a rejected step).  Nothing in it needs the host.
    void step_head_speculative() {
        const Structure& s = st.s;
        const bool q1 = s.n_blocks != 0, q2 = s.n_views != 0;
        // one launch for the back-substitution and the block constants where a block's constants hang on its own view's pose
        const bool fused_head = q1 && q2 && can_fuse() && e.chain != CBA_CHAIN_BUNDLE;
        if (fused_head) {
#define CBA_STEP_HEAD(CH)                                                                                                                  \
    hipLaunchKernelGGL(k_step_head<CH>, dim3(nblk(s.n_views, 4)), dim3(256), 0, e.stream, e.gate, st.dims, s.n_views, st.link_off.p,         \
                       st.link_blk.p, e.d_blk_cam.p, e.blk_Z.p, e.delta_sh.p, e.view_fixed.p, e.view_L.p, e.view_y.p, e.view_D.p,          \
                       e.view_gp.p, e.view[0].p, st.view_delta.p, e.view[1].p, st.view_stats.p, e.cam[1].p, e.bc.p)
            if (e.chain == CBA_CHAIN_INTRINSIC) CBA_STEP_HEAD(CH_INTRINSIC); else CBA_STEP_HEAD(CH_EXTRINSIC);
#undef CBA_STEP_HEAD
            launch_camera_consts(e, 1);
            vstats_pending = true;
        } else if (q2) {
            enqueue_backsub();
        } else {
            CBA_HIP(hipMemsetAsync(st.stat_dev.p, 0, 4 * sizeof(double), e.stream));
        }
        if (q1) with_alt_blocks([&] { enqueue_normal_eq_head(1, ctl_huber, fused_head); });
    }
    // ... and what follows Mode B, up to the assembled pack (the second set of block sums / weights, the trial poses)
    void step_tail_enqueue(double huber, bool constrained, const PackLayout& L) {
        const Structure& s = st.s;
        const bool q1 = s.n_blocks != 0;
        // (the elimination with the radius the controller / the driver predicted)
        with_alt_blocks([&] { enqueue_system(huber, q1, q1, constrained, 1, L, 1); });
    }
    void step_tail_speculative(double huber, const PackLayout& L, const AllReduce& ar) {
        step_tail_enqueue(huber, ctl_constrained, L);
        exchange(0, L.size, ar, nullptr, true);
        run_ctl(CTL_STEP, 1);
        e.active = 1;
    }
    void ctl_step(double huber, bool speculative, const PackLayout& L, const AllReduce& ar, int rank) override {
        (void)rank;
        const Structure& s = st.s;
        const bool q1 = s.n_blocks != 0, q2 = s.n_views != 0;
        // the shared trial blocks and the shared step are where the controller left them (copy 1)
        ctl_huber = huber;
        if (speculative) {
            step_head_speculative();
            step_tail_speculative(huber, L, ar);
            return;
        }
        if (q2) enqueue_backsub();
        else CBA_HIP(hipMemsetAsync(st.stat_dev.p, 0, 4 * sizeof(double), e.stream));
        if (q1) {  // the cost alone (Mode R); the block sums / weights of the current point stay
            launch_block_consts(e, 1);
            launch_resid(e);
            launch_cost(e, huber, st.stat_dev.p + 4);
        } else {
            CBA_HIP(hipMemsetAsync(st.stat_dev.p + 4, 0, sizeof(double), e.stream));
        }
        enqueue_pack(L, false, false, 1, 1);
        exchange(L.stats, 6, ar, nullptr, true);
        run_ctl(CTL_STEP, 0);
        e.active = 1;
    }
    // Queue the head of the NEXT speculative step behind the controller invocation that was just queued, before its decision is
    // known: every launch of the head checks the controller's CS_GO flag on the device and does nothing unless the controller
    // accepted the step it decided on with the predicted radius and asks for another speculative step - the usual case, in which
    // the chip goes from the controller straight into the next step (the host's read of the record and its ~15 launches of 3-5 us
    // are off the critical path).  The head assumes the accept has happened: the buffer exchange is made here and undone by
    // ctl_prelaunch_cancel() if the record says otherwise.
    // Queuing the head also sets host-side flags for what follows it (vstats_pending: stage 3 reduces the views' step statistics;
    // e.head_weights: Mode B left the robust weights): a cancel restores them with the buffers, so that the next system does not
    // take along the output of launches that did nothing.
    bool pre_vstats_pending = false, pre_head_weights = false;
    bool ctl_prelaunch() override {
        if (!st.ctl_prelaunch || e.scalar || !e.modeb_shared || (e.chain != CBA_CHAIN_INTRINSIC && !e.modeb_moments)) return false;
        pre_vstats_pending = vstats_pending;
        pre_head_weights = e.head_weights;
        ctl_accept(true);
        e.gate = st.ctl_view.scal + CS_GO;
        bool queued = false;
        ScopeExit reset{[&] {
            e.gate = nullptr;
            if (!queued) ctl_prelaunch_cancel();
        }};
        step_head_speculative();
        queued = true;
        return true;
    }
    void ctl_prelaunch_cancel() override {  // (the gated launches did nothing)
        ctl_accept(true);
        vstats_pending = pre_vstats_pending;
        e.head_weights = pre_head_weights;
    }
    void ctl_step_tail(double huber, const PackLayout& L, const AllReduce& ar, int rank) override {
        (void)rank;
        step_tail_speculative(huber, L, ar);
    }
    // trial -> current without a copy: the two sets of private poses (and, after a speculative step, of block sums and weights)
    // trade places.  A stage graph captured with the old pointers would be stale: the captured stages belong to the host-side
    // form of the iteration, which is not running; they are dropped and re-captured if it ever runs again.
    void ctl_accept(bool blocks) override {
        std::swap(e.view[0].p, e.view[1].p);
        if (blocks) swap_block_sets();
        for (HipLMState::GraphSlot* g : {&st.g_new, &st.g_schur, &st.g_trial})
            if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; g->uses = 0; }
    }
    const double* ctl_wait() override {
        // the controller publishes the record's sequence number last (system-scope release): poll it, fall back to the stream
        volatile const double* seq = st.ctl_rec.p + CS_SEQ;
        const double want = static_cast<double>(ctl_invocations);
        if (st.sync_spin) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int spins = 0; *seq < want; ++spins) {
#if defined(__x86_64__)
                __builtin_ia32_pause();
#endif
                if ((spins & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(st.ctl_poll_us)) break;
            }
        }
        if (*seq < want) {
            // Still not there (a Mode B pass over 1e7+ observations is in front of the controller): nap and look again.  No event is
            // recorded behind the controller for this - an event record is a barrier packet between the controller and the head of
            // the next step that is already queued behind it (~6 us of idle chip per step) - and the stream itself cannot be waited
            // on: it holds that next step.  Every millisecond or so: has the stream died or drained without a record, has a peer's
            // collective failed (a rank that threw out of its solve aborts its communicator; this rank must not wait for ever), is
            // the deadline over?
            const auto t0 = std::chrono::steady_clock::now();
            for (int naps = 0; *seq < want; ++naps) {
                std::this_thread::sleep_for(std::chrono::microseconds(st.ctl_event ? 0 : 30));
                if (st.ctl_event) {  // (experiment builds: the event-based wait of the first version)
                    CBA_HIP(hipEventSynchronize(st.ctl_done));
                    break;
                }
                if ((naps & 31) != 31) continue;
                const hipError_t q = hipStreamQuery(e.stream);
                if (q == hipSuccess) break;  // the stream is empty: the record is there, or never will be
                if (q != hipErrorNotReady) CBA_HIP(q);
                if (!e.rccl_comm) continue;
                ncclResult_t async = ncclSuccess;
                (void)ncclCommGetAsyncError(reinterpret_cast<ncclComm_t>(e.rccl_comm), &async);
                const bool late = std::chrono::steady_clock::now() - t0 > std::chrono::seconds(st.rccl_timeout_s);
                if (async != ncclSuccess || late) {
                    rccl_abort(e);
                    throw HipError(late ? "RCCL exchange: no progress within the deadline (a peer rank failed or hung); communicator aborted"
                                        : std::string("RCCL exchange failed on a peer: ") + ncclGetErrorString(async) + "; communicator aborted");
                }
            }
            if (*seq < want) throw HipError("LM controller: the control record did not arrive");
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return st.ctl_rec.p;
    }
    void ctl_fetch(double* intr, double* cam, double* target, double* delta) override {
        double* stage = st.ctl_rec.p + CTL_REC_FETCH;
        e.shared_pack[0].download(stage, e.pk_delta, e.stream);
        e.shared_pack[1].download(stage + e.pk_delta, static_cast<size_t>(st.s.nsh), e.stream, e.pk_delta);
        CBA_HIP(hipStreamSynchronize(e.stream));
        unstage_shared(stage, intr, cam, target);
        std::memcpy(delta, stage + e.pk_delta, sizeof(double) * static_cast<size_t>(st.s.nsh));
    }
    void ctl_line_search_done(const double* scal) override {
        double* stage = st.ctl_rec.p + CS_COUNT;
        std::memcpy(stage, scal, sizeof(double) * CS_COUNT);
        st.ctl_buf.upload(stage, CS_COUNT, e.stream);
        run_ctl(CTL_LS_DONE, 0);
    }

    void trial(const double* delta_sh, double huber, TrialStats* out) override {
        const Structure& s = st.s;
        *out = TrialStats();
        if (s.n_blocks == 0) return;
        std::memcpy(st.pin_pack[1].p + e.pk_delta, delta_sh, sizeof(double) * s.nsh);
        run_stage(st.g_trial, huber, false, [&] {
            e.shared_pack[1].upload(st.pin_pack[1].p, e.pk_delta + static_cast<size_t>(s.nsh), e.stream);  // trial blocks + step
            if (s.n_views > 0) launch_backsub(nullptr, st.pin_tr.p + 8);
            // cost at the trial point (Mode R); blk_s / blk_w of the ACCEPTED point stay in blk_acc / blk_w
            launch_block_consts(e, 1);
            launch_resid(e);  // Mode R writes blk_s; blk_acc / blk_w keep the accepted point's values
            launch_cost(e, huber, st.pin_tr.p + 24);
            CBA_HIP(hipGetLastError());
        });
        CBA_HIP(hipStreamSynchronize(e.stream));
        e.active = 1;
        const double* h = st.pin_tr.p;
        const double* c2 = st.pin_tr.p + 24;
        out->step2 = s.n_views > 0 ? h[8] : 0.0;
        out->xnorm2 = s.n_views > 0 ? h[9] : 0.0;
        out->gd = s.n_views > 0 ? h[10] : 0.0;
        out->dHd = s.n_views > 0 ? h[11] : 0.0;
        out->cost = c2[0];
    }
    void accept() override {
        launch_accept();
        CBA_HIP(hipGetLastError());
        st.current_is_on_device = true;
    }
    void download_private(double* view_pose) override {
        if (e.h_view.empty()) return;
        e.view[0].download(view_pose, e.h_view.size(), e.stream);
        CBA_HIP(hipStreamSynchronize(e.stream));
    }
    void download_blocks(std::vector<double>& acc, std::vector<double>& w) override {
        acc.resize(static_cast<size_t>(e.n_blocks) * e.NACC);
        w.resize(e.n_blocks);
        e.blk_acc.download(acc.data(), acc.size(), e.stream);
        e.blk_w.download(w.data(), w.size(), e.stream);
        CBA_HIP(hipStreamSynchronize(e.stream));
    }
};

// ---- engine glue -----------------------------------------------------------------------------------
void destroy_lm_state(Engine& e) {
    delete lm_state(e);
    e.lm_state = nullptr;
}

void init_lm_state(Engine& e, const cba_reproj_problem& d, bool have_records) {
    auto* st = new HipLMState();
    e.lm_state = st;
    build_structure(d, st->s, have_records);
    const Structure& s = st->s;
    st->dims = SchurDims{s.PL, s.NH, s.NACC, s.PSH, s.PC, s.n_cams, s.chain};
    st->n_vchunks = std::max(1, (s.n_views + VCHUNK - 1) / VCHUNK);
    st->n_tiles = (s.nsh + 63) / 64;
    st->n_pairs = st->n_tiles * (st->n_tiles + 1) / 2;
    // camera chunks
    std::vector<int64_t> coff{0}, cseg(s.n_cams + 1, 0);
    for (int c = 0; c < s.n_cams; ++c) {
        for (int64_t p = s.cam_off[c]; p < s.cam_off[c + 1]; p += CCHUNK) coff.push_back(std::min<int64_t>(p + CCHUNK, s.cam_off[c + 1]));
        cseg[c + 1] = static_cast<int64_t>(coff.size()) - 1;
    }
    st->n_cchunks = static_cast<int>(coff.size()) - 1;
    auto up64 = [&](DevBuf<int64_t>& b, const std::vector<int64_t>& v) { b.alloc(v.size()); b.upload(v.data(), v.size(), e.stream); };
    auto up32 = [&](DevBuf<int32_t>& b, const std::vector<int32_t>& v) { b.alloc(v.size()); b.upload(v.data(), v.size(), e.stream); };
    up64(st->cchunk_off, coff);
    up64(st->cam_seg, cseg);
    up32(st->cam_blk, s.cam_blk);
    up64(st->link_off, s.link_off);
    up32(st->link_blk, s.link_blk);
    up32(st->view_cam_blk, s.view_cam_blk);
    st->cam_partial.alloc(static_cast<size_t>(std::max(1, st->n_cchunks)) * s.NACC);
    const size_t nv = std::max(1, s.n_views);
    st->view_gmax.alloc(nv);
    st->view_delta.alloc(nv * 6);
    st->view_delta.zero(e.stream);
    st->view_stats.alloc(nv * 4);
    st->syrk_partial.alloc(static_cast<size_t>(st->n_vchunks) * (static_cast<size_t>(st->n_pairs) * 4096 + s.nsh));  // + g_schur
    // pinned staging of everything a captured stage copies (sizes are fixed per problem: nothing is allocated in a capture)
    st->pin.reserve(static_cast<size_t>(st->n_pairs) * 4096 + s.nsh + 8);
    st->pin_ne.reserve(static_cast<size_t>(s.n_cams) * s.NACC + 2);
    st->pin_tr.reserve(32);
    st->pin_lmp.reserve(2);
    st->pin_pack[0].reserve(e.pk_size);
    st->pin_pack[1].reserve(e.pk_size);
    {   // ROCm loads a translation unit's code object on the first use of one of its kernels (milliseconds for the
        // template-heavy ones): touch both units here so that the first solve does not pay for it
        hipFuncAttributes fa;
        (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_schur_view));
        warm_reproj_kernels();
    }
    if (const char* env = std::getenv("CBA_SYRK_MFMA")) st->syrk_mfma = std::atoi(env);
    if (const char* env = cba_exp_env("CBA_SCHUR_WAVE")) st->schur_wave = std::atoi(env);
    if (const char* env = cba_exp_env("CBA_LM_FUSE")) st->fuse_small = std::atoi(env);
    if (const char* env = cba_exp_env("CBA_LM_CTL_EVENT")) st->ctl_event = std::atoi(env);
    if (const char* env = cba_exp_env("CBA_SYNC_SPIN")) st->sync_spin = std::atoi(env);
    if (const char* env = std::getenv("CBA_LM_GRAPH")) {
        const int v = std::atoi(env);
        st->graphs_ok = v != 0;
        st->graph_after = v > 1 ? v : (v == 1 ? 0 : st->graph_after);
    }
    e.blk_w.alloc(std::max(1, s.n_blocks));
    e.cam_acc.alloc(static_cast<size_t>(s.n_cams) * s.NACC);
    e.view_L.alloc(nv * 36);
    e.view_y.alloc(nv * 6);
    e.view_D.alloc(nv * 6);
    e.view_gp.alloc(nv * 6);
    e.view_scale2.alloc(nv * 6);
    e.view_fixed.alloc(nv);
    e.view_fixed.zero(e.stream);
    e.blk_Z.alloc(static_cast<size_t>(std::max(1, s.n_blocks)) * 6 * s.PSH);
    e.blk_Z.zero(e.stream);
    // resident LM (resident_lm.hip)
    up64(st->cam_off, s.cam_off);
    st->res_active.alloc(std::max(1, s.nsh));
    st->res_cam_var.alloc(std::max(1, s.n_cams));
    st->res_Hcc.alloc(static_cast<size_t>(s.nsh) * s.nsh);
    st->res_Ssch.alloc(static_cast<size_t>(s.nsh) * s.nsh);
    st->res_out.alloc(32);
    if (const char* env = cba_exp_env("CBA_LM_CTL")) st->lm_ctl_mode = std::atoi(env) != 0;
    if (const char* env = cba_exp_env("CBA_LM_CTL_POLL_US")) st->ctl_poll_us = std::atoi(env);
    if (const char* env = cba_exp_env("CBA_LM_PRELAUNCH")) st->ctl_prelaunch = std::atoi(env);
    if (const char* env = std::getenv("CBA_RCCL_TIMEOUT_S")) st->rccl_timeout_s = std::max(1, std::atoi(env));
    warm_lm_ctl();
    if (const char* env = std::getenv("CBA_LM_RESIDENT")) st->resident_mode = std::atoi(env);
    if (const char* env = std::getenv("CBA_LM_RESIDENT_MAX_OBS")) st->resident_max_obs = std::atoll(env);
    CBA_HIP(hipStreamSynchronize(e.stream));
}

void solve_stats(const Engine& e, int64_t stats8[8]) {
    const HipLMState* st = reinterpret_cast<const HipLMState*>(e.lm_state);
    for (int k = 0; k < 8; ++k) stats8[k] = st ? st->xs[k] : 0;
}

void set_lm_mode(Engine& e, int mode) {
    if (mode < 0 || mode > 3)
        throw std::invalid_argument("lm mode: 0 chip-wide kernels, 1 automatic, 2 resident kernel whenever possible, 3 chip-wide kernels with the host-side iteration (diagnosis)");
    lm_state(e)->resident_mode = mode == 3 ? 0 : mode;
    lm_state(e)->lm_ctl_mode = mode == 3 ? 0 : 1;
}


static LMDriver make_driver(Engine& e, HipBackend& be) {
    AllReduce ar = [&e](double* buf, int64_t n) { engine_allreduce(e, buf, n); };
    return LMDriver(lm_state(e)->s, be, e.h_intr, e.h_cam, e.h_view, e.h_target, ar, e.n_ranks, e.rank);
}

// One throw-away pass through the three LM stages at handle creation: the first launch of every kernel carries a
// one-time cost on ROCm (code-object load, ~0.1-0.3 ms of per-kernel set-up) that added ~8 ms to the first solve of
// a small problem.  Paid once per process, device and kernel family; results are discarded (every solve re-evaluates from
// the parameters).
void warm_lm(Engine& e) {
    cba_options o{};
    o.max_iterations = 1;
    const bool resident = resident_lm_eligible(e, o);  // default options decide which form this handle will use first
    {   // the cost is per process and device (code objects, kernel set-up), not per handle: pay it once per kernel family
        static std::mutex mu;
        static std::set<uint32_t> warmed;
        const uint32_t key = (static_cast<uint32_t>(e.device) << 8) | (resident ? 0x80u : 0u) | (e.scalar ? 0x40u : 0u) |
                             (static_cast<uint32_t>(e.chain) << 2) | static_cast<uint32_t>(e.model);
        std::lock_guard<std::mutex> lock(mu);
        if (!warmed.insert(key).second) return;
    }
    if (resident) { resident_lm_warm(e); return; }
    HipBackend be(e, *lm_state(e));
    const Structure& s = lm_state(e)->s;
    if (s.n_blocks == 0) return;
    std::vector<double> cam_acc, S, g, d(std::max(1, s.nsh), 0.0);
    double c2[2], gm = 0.0;
    int nf = 0;
    std::vector<int32_t> fixed(s.n_views, 0);
    be.set_view_fixed(fixed);
    be.upload_shared(0, e.h_intr.data(), e.h_cam.data(), e.h_target.data());
    be.normal_eq_schur(1.0, cam_acc, c2, 1e4, true, false, S, g, &gm, &nf);
    std::vector<double> S2, g2;
    be.schur(1e4, false, false, S2, g2, &gm, &nf);
    be.upload_shared(1, e.h_intr.data(), e.h_cam.data(), e.h_target.data());
    TrialStats ts;
    be.trial(d.data(), 1.0, &ts);
    {   // the packed forms of the same stages (k_pack, k_accept_blocks) — without a collective: warm-up is per process, not per group
        const PackLayout L(s, 1);
        std::vector<double> pack(static_cast<size_t>(L.size), 0.0);
        const AllReduce none = [](double*, int64_t) {};
        void* comm = e.rccl_comm;
        e.rccl_comm = nullptr;
        be.sys_new(1.0, 1e4, true, false, L, none, 0, pack.data());
        be.sys_resolve(1e4, false, L, none, 0, pack.data());
        be.upload_shared(1, e.h_intr.data(), e.h_cam.data(), e.h_target.data());
        (void)be.sys_step(d.data(), 1.0, 1e4, false, L, none, 0, pack.data());
        // (the step is NOT accepted: even with a zero shared step the trial poses differ from the current ones; the kernel of
        // accept_step is set up by an empty launch)
        hipLaunchKernelGGL(k_accept_blocks, dim3(1), dim3(64), 0, e.stream, static_cast<int64_t>(0), e.blk_acc_alt.p, e.blk_acc.p,
                           static_cast<int64_t>(0), e.blk_w_alt.p, e.blk_w.p);
        // the controller kernel: one invocation out of turn (the control scalars say the solve has ended: it changes nothing)
        be.ensure_ctl(L);
        double* stage = lm_state(e)->ctl_rec.p + CS_COUNT;
        ctl_reset(stage);
        stage[CS_TERM] = 0.0;
        lm_state(e)->ctl_buf.upload(stage, CS_COUNT, e.stream);
        be.run_ctl(CTL_NEW, 0);
        e.rccl_comm = comm;
    }
    lm_state(e)->g_new.uses = lm_state(e)->g_schur.uses = lm_state(e)->g_trial.uses = 0;
    CBA_HIP(hipStreamSynchronize(e.stream));
}

void solve_lm(Engine& e, const cba_options& o, cba_summary* out) {
    if (resident_lm_eligible(e, o)) {  // small problem: the whole iteration in one kernel launch
        for (int k = 0; k < 8; ++k) lm_state(e)->xs[k] = 0;
        if (resident_lm_solve(e, o, out)) return;
    }
    HipBackend be(e, *lm_state(e));
    LMDriver drv = make_driver(e, be);
    try {
        drv.solve(o, out);
    } catch (...) {
        // this rank leaves the solve: its peers may be inside (or about to enter) the collective of the same step - abort the
        // communicator so that they fail too instead of waiting for a contribution that will never come
        e.gate = nullptr;
        rccl_abort(e);
        throw;
    }
    {
        const ExchangeStats& x = drv.exchange_stats();
        int64_t* xs = lm_state(e)->xs;
        xs[0] = x.allreduce_calls; xs[1] = x.allreduce_doubles; xs[2] = x.speculative_steps; xs[3] = x.speculation_hits;
        xs[4] = x.speculation_misses; xs[5] = x.rejected_steps; xs[6] = x.line_searches; xs[7] = x.line_search_evaluations;
    }
    // leave copy 0 on the device equal to the host state
    e.intr[0].upload(e.h_intr.data(), e.h_intr.size(), e.stream);
    CBA_HIP(hipStreamSynchronize(e.stream));
}

int64_t covariance_dim(const Engine& e) {
    int64_t n = static_cast<int64_t>(e.n_cams) * e.PI;
    if (e.chain != CBA_CHAIN_INTRINSIC) n += 7LL * e.n_cams;
    if (e.chain != CBA_CHAIN_BUNDLE) n += 7LL * e.n_views;
    else n += 7;
    return n;
}

int64_t shared_covariance_dim(const Engine& e) {
    if (e.chain == CBA_CHAIN_BUNDLE) return covariance_dim(e);
    int64_t n = static_cast<int64_t>(e.n_cams) * e.PI;
    if (e.chain != CBA_CHAIN_INTRINSIC) n += 7LL * e.n_cams;
    return n;
}

void compute_covariance(Engine& e, const cba_options& o, double* cov, bool shared_only) {
    HipBackend be(e, *lm_state(e));
    LMDriver drv = make_driver(e, be);
    drv.covariance(o, cov, shared_only);
}
void compute_covariance_views(Engine& e, const cba_options& o, const int32_t* views, int n_sel, double* view_cov) {
    HipBackend be(e, *lm_state(e));
    LMDriver drv = make_driver(e, be);
    drv.covariance(o, nullptr, true, views, n_sel, view_cov);
}

}  // namespace cba
