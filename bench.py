#!/usr/bin/env python3
"""bench.py — residual+Jacobian evals/sec of the reprojection hot path on MI355X.

Workload (BASELINE.json configs[1]): pinhole + Brown-Conrady intrinsics refinement, 1000 views x
10000 points (100x100 planar grid), fp64, per GPU.  A "step" is one Mode A pass (k_eval): the
2-vector residual and the 2x16 tangent-space Jacobian of every observation of this rank's views are
produced and written to HBM, inputs already resident.  With N > 1 ranks each rank owns 1000 views of
an N*1000-view problem (weak scaling, views sharded, no data-path collective inside the pass); the
one real exchange of the path — the sum-all-reduce of the packed reduced normal equations, one per LM
step — is exercised by the LM solves reported under "lm" (this workload, weak) and "lm_strong"
(BASELINE configs[2], the 8-camera extrinsic bundle of 1.6e8 observations split over the N ranks: the
north-star's obs-sharded strong-scaling case; wall clock, collective count and bytes), RCCL over xGMI.

Prints ONE JSON line on rank 0 (contract in the task statement) with "roofline" and "cpu_baseline".
"""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
DUMP_BUDGET_BYTES = 60_000_000  # --dump-outputs stays under 64 MB


def dump_outputs(h, flat, out_dir):
    """--dump-outputs: the residuals (2n,) and the Jacobian (2n, P) of the last Mode A pass, in the layout a caller of
    cba_reproj_eval_fetch receives (observation order, u row then v row).  Whole views are taken in a fixed order (seed 0) while
    they fit the budget and are written in ascending view order, so with the same arguments every run writes the same rows; a
    single view over the budget is cut to a fixed sample of its observations (seed 1)."""
    P = h.local_columns
    counts = np.diff(flat.blk_offset).astype(np.int64)
    obs_bytes = 8 * 2 * (1 + P)
    pick, total = [], 0
    for b in np.random.default_rng(0).permutation(len(counts)):
        if pick and (total + counts[b]) * obs_bytes > DUMP_BUDGET_BYTES:
            break
        pick.append(int(b))
        total += int(counts[b])
    parts = [h.eval_fetch_blocks(b, b + 1) for b in sorted(pick)]
    r = np.concatenate([p[0] for p in parts])
    J = np.concatenate([p[1] for p in parts])
    if total * obs_bytes > DUMP_BUDGET_BYTES:
        keep = np.sort(np.random.default_rng(1).choice(total, DUMP_BUDGET_BYTES // obs_bytes, replace=False))
        rows = np.stack([2 * keep, 2 * keep + 1], axis=1).reshape(-1)
        r, J = r[rows], J[rows]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "residuals.npy"), np.ascontiguousarray(r, dtype=np.float64))
    np.save(os.path.join(out_dir, "jacobian.npy"), np.ascontiguousarray(J, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=100, help="points per view = grid^2")
    ap.add_argument("--pitch", type=float, default=0.002, help="target pitch in metres (SURVEY.md section 8d: 0.002 m for the 100 x 100 board of C2 / C5)")
    ap.add_argument("--no-lm", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--lm-timeout", type=float, default=240.0, help="watchdog for the LM section, seconds")
    ap.add_argument("--c3-views", type=int, default=4000, help="views of the strong-scaling problem (BASELINE configs[2]: 4000), split over the ranks; 0 = skip")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write rank 0's residuals and Jacobian of the last step as DIR/<name>.npy (fp64; a fixed, "
                         "seeded sample of views when the whole output exceeds 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N > 1")
        args.gpus = world

    import torch

    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # rehearsal on a box with fewer GPUs than ranks (CBA_BENCH_BACKEND=gloo): ranks share devices and talk over gloo
        backend = os.environ.get("CBA_BENCH_BACKEND", "nccl")
        local_rank = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    from calibration_amd import capi, optim
    from tests import synth

    lib = capi.load_library()
    if lib.cba_device_count() <= 0:
        raise SystemExit("bench.py needs a GPU: libcalibba has no CPU fallback")

    # ---- synthetic scene: this rank's shard of the (world * views)-view problem ----------------------
    t_gen = time.time()
    scene = synth.scene_intrinsics(args.views, rows=args.grid, cols=args.grid, spacing=args.pitch, seed=7 + rank,
                                   noise_px=0.2, first_view_global=rank * args.views)
    flat = scene.flat
    init_intr, init_view = flat.intr.copy(), flat.view_pose.copy()
    n_obs = flat.n_obs
    t_gen = time.time() - t_gen
    h = optim.ReprojHandle(flat, device=local_rank)
    P = h.local_columns

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- timed region: W warmup + K steps of Mode A ---------------------------------------------------
    h.eval_timed(0, max(1, args.warmup))
    barrier()
    t0 = time.perf_counter()
    ms_kernel = h.eval_timed(0, args.steps)  # K back-to-back k_eval launches, HIP events on the engine's stream
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    value = world * n_obs * args.steps / elapsed
    if args.dump_outputs and rank == 0:  # before anything else runs on the handle's buffers
        dump_outputs(h, flat, args.dump_outputs)

    bytes_per_obs = 8 * (4 + 2 + 2 * P)  # 4 loads + 2 residual + 2P Jacobian stores, fp64
    achieved = bytes_per_obs * n_obs / (ms_kernel * 1e-3) / 1e9
    # HBM traffic of one k_eval launch from the committed PMC passes (FETCH_SIZE / WRITE_SIZE, separate
    # rocprofv3 --pmc runs of this same command; gfx950 FETCH_SIZE correction applied), same unit as `achieved`
    traffic, traffic_src, traffic_bytes = None, None, None
    pmc_path = os.path.join(ROOT, "profiles", "pmc_k_eval.json")
    if os.path.exists(pmc_path) and args.views == 1000 and args.grid == 100:
        pmc = json.load(open(pmc_path))
        traffic_bytes = pmc["hbm_bytes_per_launch"]
        traffic = traffic_bytes / (ms_kernel * 1e-3) / 1e9
        traffic_src = "profiles/pmc_k_eval.json"
    roofline = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                "traffic_bytes_per_launch": traffic_bytes, "algorithmic_bytes_per_launch": bytes_per_obs * n_obs,
                "kernel": "k_eval<INTRINSIC,PINHOLE_BC>", "kernel_ms": ms_kernel, "bytes_per_eval": bytes_per_obs}

    # ---- Mode B (per-block normal equations, the kernel that sets the LM wall clock): fp64-issue bound ----------------
    # FLOPs counted from the ISA of the shipped kernel's hot loop (tools/isa_mix.py, FMA = 2, mul / add = 1;
    # profiles/r02_modeb_isa_mix.txt): one workgroup of two wavefronts per tile, each accumulating its half of the 225 FMAs of
    # [H | g | s] for every observation and evaluating the residual / Jacobian rows of every second 64-observation chunk (the other
    # chunk's rows arrive through LDS): 257 FMA + 94 mul/add per wavefront and pair of chunks = 608 FLOP per observation, all of
    # it useful work (round 1 evaluated the rows once per launch: 786 FLOP issued for the same 608).
    # The chip's clock follows the load: right after the memory-bound Mode A section a pass takes ~0.18 ms, after ~35 ms of
    # sustained fp64 work it settles at ~0.16 ms (tools/exp.py modeb_warm).  Both are reported; `ms_per_pass` is the settled one.
    ms_b_first = h.normal_eq_timed(2, 10)
    ms_b = h.normal_eq_timed(200, 50)
    flop_per_obs, valu_per_obs = 605, 374  # tools/isa_mix.py on the shipped kernel (profiles/r03_modeb_isa_mix.txt)
    mode_b = {"kernel": "k_ne_shared<DirectForm<INTRINSIC,PINHOLE_BC,2 parts>> (one tile per view at this size: no k_tile_sum)", "ms_per_pass": ms_b,
              "ms_per_pass_right_after_mode_a": ms_b_first, "timing": "200 warm-up passes, 50 timed (HIP events); the other figure: 2 + 10",
              "bound": "fp64 vector issue",
              "flop_per_obs": flop_per_obs, "valu_instructions_per_obs": valu_per_obs, "achieved_TFLOPs": flop_per_obs * n_obs / (ms_b * 1e-3) / 1e12,
              "peak_TFLOPs": 78.6, "frac": flop_per_obs * n_obs / (ms_b * 1e-3) / 78.6e12,
              "issue_slots_frac_at_2p4GHz": valu_per_obs * 4 * (n_obs / 64 / 1024) / (ms_b * 1e-3 * 2.4e9), "hbm_GBs": 16 * n_obs / (ms_b * 1e-3) / 1e9}

    # ---- LM wall-clock to tolerance on the same data (all ranks; RCCL all-reduce when world > 1) -----
    # Runs on a worker thread under a watchdog: a collective that never completes (the multi-rank RCCL path
    # cannot be rehearsed on a 1-GPU box) must not swallow the evals/s line measured above.
    lm_box = {}

    def setup_transport(handle):
        if world > 1 and dist.get_backend() != "nccl":  # rehearsal: host-callback transport over the CPU backend
            def _allreduce(arr):
                dist.all_reduce(torch.from_numpy(arr))
            handle.set_allreduce(_allreduce, world, rank)
            return f"host callback over torch.distributed {dist.get_backend()} (rehearsal)"
        if world > 1:
            # RCCL-native: ncclAllReduce of the device-resident packed system on the engine's stream.  A failure here is a failure of
            # the run (no host-staged fall-back: the figure would describe another transport than the one it is labelled with).
            uid = torch.zeros(capi.RCCL_UNIQUE_ID_BYTES, dtype=torch.uint8, device="cuda")
            if rank == 0:
                uid = torch.tensor(list(optim.rccl_unique_id()), dtype=torch.uint8, device="cuda")
            dist.broadcast(uid, 0)
            handle.init_rccl(bytes(uid.cpu().numpy().tolist()), world, rank)
            return "rccl (libcalibba ncclAllReduce, device-resident pack)"
        return "none (1 rank)"

    def timed_solve(handle):
        o = capi.default_options()
        o.compute_covariance = 0
        barrier()
        t1 = time.perf_counter()
        s = handle.solve(o)
        barrier()
        wall = time.perf_counter() - t1
        if dist is not None:  # the slowest rank's clock
            t = torch.tensor([wall], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            wall = float(t.item())
        return s, wall

    def run_lm():
        try:
            torch.cuda.set_device(local_rank)
            transport = setup_transport(h)
            h.set_params(intr=init_intr, view_pose=init_view)
            s, lm_s = timed_solve(h)
            xs = h.solve_stats()
            flat_result = flat.intr.copy()
            ab = None
            if world == 1:  # A/B (one rank only): the same iteration with the reduced solve and the step decision on the HOST
                h.set_lm_mode(3)  # (cba_reproj_set_lm_mode 3: diagnostic form; the default keeps them on the device, lm_ctl.hip)
                h.set_params(intr=init_intr, view_pose=init_view)
                s_ab, ab = timed_solve(h)
                h.set_lm_mode(1)
                ab = {"wall_s": ab, "iterations": int(s_ab.iterations)}
            lm_box["lm"] = {"wall_s": lm_s, "host_side_form": ab, "iterations": int(s.iterations), "success": bool(s.success),
                            "final_cost": float(s.final_cost),
                            "intr_err_max": float(np.abs(flat_result - scene.gt_intr).max()), "views_total": world * args.views,
                            "obs_total": world * n_obs, "allreduce": transport, "allreduce_calls": xs["allreduce_calls"],
                            "allreduce_bytes": 8 * xs["allreduce_doubles"], "accepted_steps": int(s.successful_steps),
                            "speculation": {k: xs[k] for k in ("speculative_steps", "speculation_hits", "speculation_misses", "rejected_steps")}}
        except Exception as ex:  # the evals/s line must still be printed
            lm_box["lm"] = {"error": f"{type(ex).__name__}: {ex}"}
            return
        # ---- STRONG scaling of the LM (the north-star's obs-sharded case): BASELINE configs[2], 8-camera extrinsic bundle,
        # c3_views x 8 x 5000 observations in total, views split over the ranks, one packed all-reduce per LM step ----------------
        if args.c3_views <= 0:
            return
        try:
            v0, v1 = rank * args.c3_views // world, (rank + 1) * args.c3_views // world
            t2 = time.time()
            sc3 = synth.scene_extrinsics_shard(args.c3_views, v0, v1)
            gen3 = time.time() - t2
            with optim.ReprojHandle(sc3.flat, device=local_rank) as h3:
                transport3 = setup_transport(h3)
                start = (sc3.flat.intr.copy(), sc3.flat.cam_pose.copy(), sc3.flat.view_pose.copy())
                s3, wall3 = timed_solve(h3)  # first solve on the handle
                h3.set_params(intr=start[0], cam_pose=start[1], view_pose=start[2])
                s3, wall3b = timed_solve(h3)
                xs3 = h3.solve_stats()
                ab3 = None
                if world == 1:  # A/B as above
                    h3.set_lm_mode(3)
                    h3.set_params(intr=start[0], cam_pose=start[1], view_pose=start[2])
                    s_ab3, ab3 = timed_solve(h3)
                    h3.set_lm_mode(1)
                    ab3 = {"wall_s": ab3, "iterations": int(s_ab3.iterations)}
                ms_b3 = h3.normal_eq_timed(1, 3)
            obs_total = args.c3_views * 8 * 5000
            lm_box["lm_strong"] = {"workload": f"8-camera extrinsic bundle, {args.c3_views} views x 8 cameras x 5000 pts = {obs_total:.3g} observations "
                                               f"in total, views split over {world} rank(s) (BASELINE configs[2])",
                                   "scaling": "strong", "wall_s": min(wall3, wall3b), "wall_first_s": wall3, "host_side_form": ab3, "iterations": int(s3.iterations),
                                   "accepted_steps": int(s3.successful_steps), "success": bool(s3.success), "final_cost": float(s3.final_cost),
                                   "intr_err_max": float(np.abs(sc3.flat.intr - sc3.gt_intr)[:, :4].max()), "allreduce": transport3,
                                   "allreduce_calls": xs3["allreduce_calls"], "allreduce_bytes": 8 * xs3["allreduce_doubles"],
                                   "speculation": {k: xs3[k] for k in ("speculative_steps", "speculation_hits", "speculation_misses", "rejected_steps")},
                                   "mode_b_ms_per_pass_this_rank": ms_b3, "obs_this_rank": int(sc3.flat.n_obs), "scene_gen_s": gen3,
                                   # k_ne_shared<MomentForm<PINHOLE_BC, 4 parts>>: 616 FLOP in 410 vector instructions per observation
                                   # (tools/isa_mix.py, profiles/r03_modeb_isa_mix.txt), against the 78.6 TFLOP/s fp64 vector peak
                                   "mode_b": {"kernel": "k_ne_shared<MomentForm<PINHOLE_BC,4 parts>> + k_mom_expand (one tile per block at this size)", "flop_per_obs": 616,
                                              "valu_instructions_per_obs": 410, "bound": "fp64 vector issue",
                                              "achieved_TFLOPs": 616 * int(sc3.flat.n_obs) / (ms_b3 * 1e-3) / 1e12, "peak_TFLOPs": 78.6,
                                              "frac": 616 * int(sc3.flat.n_obs) / (ms_b3 * 1e-3) / 78.6e12}}
        except Exception as ex:
            lm_box["lm_strong"] = {"error": f"{type(ex).__name__}: {ex}"}

    lm, lm_strong, lm_hung = None, None, False
    if not args.no_lm:
        import threading

        th = threading.Thread(target=run_lm, daemon=True)
        th.start()
        th.join(args.lm_timeout)
        lm_hung = th.is_alive()
        lm = lm_box.get("lm") or ({"error": f"LM solve did not finish within {args.lm_timeout:.0f} s (watchdog)"} if lm_hung else None)
        lm_strong = lm_box.get("lm_strong") or ({"error": f"did not finish within {args.lm_timeout:.0f} s (watchdog)"} if lm_hung else None)

    # ---- BASELINE.json configs[0] (20 views x 88 points, the reference's own test size), rank 0 only: the complete call the
    # reference's pipeline makes (handle + LM + covariance + release), in the form the automatic mode picks for this size
    # (the report says which: the staged iteration since round 3, the resident single-launch kernel below ~10 views x 88 points)
    lm_c1 = None
    if rank == 0 and not args.no_lm and not lm_hung:
        try:
            from calibration_amd.geometry import pose_to_matrix

            sc1 = synth.scene_intrinsics(20, noise_px=0.2)
            f1 = sc1.flat
            views1 = [np.c_[f1.X[a:b], f1.Y[a:b], f1.u[a:b], f1.v[a:b]] for a, b in zip(f1.blk_offset[:-1], f1.blk_offset[1:])]
            poses1 = [pose_to_matrix(p) for p in f1.view_pose]
            best = None
            for _ in range(4):
                t1 = time.perf_counter()
                r1 = optim.optimize_intrinsics(views1, f1.intr.reshape(-1).copy(), poses1)
                dt = time.perf_counter() - t1
                if best is None or dt < best[0]:
                    best = (dt, r1)
            lm_c1 = {"workload": "pinhole intrinsics, 20 views x 88 pts (configs[0])", "call_s": best[0],
                     "solve_s": float(best[1].core.solve_seconds), "iterations": int(best[1].core.iterations),
                     "success": bool(best[1].core.success), "call": "handle + LM + 150x150 covariance + release, best of 4",
                     "report": best[1].core.report}
        except Exception as ex:
            lm_c1 = {"error": f"{type(ex).__name__}: {ex}"}

    # ---- CPU baseline: the oracle's autodiff evaluation on a bounded sample, rank 0 only --------------
    cpu = None
    if rank == 0 and not args.no_cpu:
        from tests import helpers

        if not os.path.exists(helpers.ORACLE_SO):
            import subprocess

            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
        orc = helpers.load_oracle()
        # the GPU box gives a 1-GPU job a 16-core CPU share whatever os.cpu_count() says
        cores = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
        sample_views = min(args.views, max(cores, 32))
        d = flat.struct()
        t_probe = orc.orc_reproj_bench_eval(C.byref(d), 0, sample_views, cores, 1)
        reps = int(max(1, min(50, 12.0 / max(t_probe, 1e-3))))
        secs = orc.orc_reproj_bench_eval(C.byref(d), 0, sample_views, cores, reps)
        sample_obs = int(flat.blk_offset[sample_views])
        cpu = {"value": sample_obs * reps / secs, "unit": "evals/s", "cores": cores, "kind": "port",
               "sample": f"{sample_views} views x {args.grid * args.grid} pts x {reps} passes of the oracle's Jet<17> "
                         f"autodiff residual+Jacobian, one residual block per view, {cores} threads over views"}
        # The second half of the metric, "LM wall-clock to tolerance", on the same host: the oracle's LM (the restated Ceres path:
        # Jet autodiff per residual block, dense normal equations, the same trust-region rules and epsilon; ceresutils.h:27-43) at 1
        # thread and at all threads, on the exact configs[0] problem and on a bounded sample of this workload (the dense oracle
        # cannot hold all 1000 views: 64 views x 10000 points, the same scene generator, pitch and noise).
        def oracle_lm(flat_cpu, threads):
            f2 = copy.deepcopy(flat_cpu)
            o2 = capi.default_options()
            o2.compute_covariance = 0
            t1 = time.perf_counter()
            s2 = helpers.oracle_solve(orc, f2, o2, threads=threads)
            return {"wall_s": time.perf_counter() - t1, "iterations": int(s2.iterations), "success": bool(s2.success), "final_cost": float(s2.final_cost)}
        try:
            sc1c = synth.scene_intrinsics(20, noise_px=0.2)
            sc2c = synth.scene_intrinsics(64, rows=args.grid, cols=args.grid, spacing=args.pitch, seed=7, noise_px=0.2)
            cpu["lm"] = {"kind": "port (oracle/lm.hpp: restated Ceres trust-region LM, dense, Jet autodiff)", "epsilon": float(capi.default_options().epsilon),
                         "c1": {"workload": "pinhole intrinsics, 20 views x 88 pts (configs[0]), the problem of lm_c1",
                                "threads_1": oracle_lm(sc1c.flat, 1), f"threads_{cores}": oracle_lm(sc1c.flat, cores)},
                         "c2_sample": {"workload": f"64 of the {args.views} views x {args.grid * args.grid} pts of this workload (pitch {args.pitch} m)",
                                       "observations": int(sc2c.flat.n_obs), "threads_1": oracle_lm(sc2c.flat, 1),
                                       f"threads_{cores}": oracle_lm(sc2c.flat, cores)}}
        except Exception as ex:
            cpu["lm"] = {"error": f"{type(ex).__name__}: {ex}"}

    if rank == 0:
        out = {
            "metric": "residual+Jacobian evals/sec",
            "value": value,
            "unit": "evals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "scaling_metric": "lm_strong.wall_s",  # the strong-scaling figure of the north-star (configs[2] split over the ranks);
                                                   # `value` is the weak scaling of a kernel with no collective
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"pinhole+Brown-Conrady intrinsics, {args.views} views x {args.grid * args.grid} pts per GPU "
                                   f"({args.grid} x {args.grid} board, pitch {args.pitch} m), fp64",
                       "views_per_gpu": args.views, "points_per_view": args.grid * args.grid, "tangent_columns": P,
                       "parallelism": f"views sharded over {world} GPU(s)"},
            "roofline": roofline,
            "cpu_baseline": cpu,
            "mode_b": mode_b,
            "lm": lm,
            "lm_strong": lm_strong,
            "lm_c1": lm_c1,
            "scene_gen_s": t_gen,
        }
        print(json.dumps(out), flush=True)
    if lm_hung:  # a stuck collective cannot be cancelled: the metric line is out; leave without touching the GPU again, and
        os._exit(3)  # not as a success
    lm_failed = any(isinstance(x, dict) and "error" in x for x in (lm, lm_strong))
    h.close()
    if dist is not None:
        dist.destroy_process_group()
    if lm_failed:  # (e.g. the RCCL transport could not be set up): the metric line is out, the run is not a success
        sys.exit(4)


if __name__ == "__main__":
    main()
