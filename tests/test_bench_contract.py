"""bench.py's one-JSON-line contract, on one GPU and as a 2-rank rehearsal (both ranks on GPU 0, gloo transport): the multi-rank control
flow the driver's `--gpus N` runs go through — process group, barriers, weak-scaled evaluation, the LM with its exchange statistics
and the strong-scaling LM section — at sizes that take seconds."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--steps", "3", "--warmup", "1", "--views", "40", "--grid", "20", "--c3-views", "16"]
FIELDS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
          "data", "config", "roofline", "cpu_baseline")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out  # exactly ONE JSON line on stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_on_one_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *COMMON], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert all(k in d for k in FIELDS), sorted(d)
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["metric"] == "residual+Jacobian evals/sec" and d["dtype"] == "f64" and d["scaling"] == "weak" and "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert abs(d["value"] - 40 * 400 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    assert d["lm"]["success"] and d["lm"]["allreduce"] == "none (1 rank)" and d["lm_strong"]["success"] and d["lm_strong"]["scaling"] == "strong"


@pytest.mark.gpu
def test_bench_two_rank_rehearsal_on_one_gpu():
    env = dict(os.environ, CBA_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", *COMMON, "--no-cpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)  # rank 0 alone prints
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    lm, ls = d["lm"], d["lm_strong"]
    assert lm["success"] and lm["views_total"] == 80 and "gloo" in lm["allreduce"]
    # one exchange point per LM step: the initial system, one per trial point, one more per miss / rejected step / plain-trial acceptance
    sp = lm["speculation"]
    assert lm["allreduce_calls"] >= 1 + lm["iterations"] and sp["speculative_steps"] >= 1
    assert ls["success"] and ls["scaling"] == "strong" and "split over 2 rank(s)" in ls["workload"] and ls["allreduce_calls"] >= 1 + ls["iterations"]


class _FakeHandle:
    """Stands in for optim.ReprojHandle in dump_outputs: every value encodes (observation, row, column)."""

    def __init__(self, blk_offset, P):
        self.blk_offset, self.local_columns = blk_offset, P

    def eval_fetch_blocks(self, b0, b1):
        i = np.arange(2 * self.blk_offset[b0], 2 * self.blk_offset[b1], dtype=np.float64)
        return i, i[:, None] * 100 + np.arange(self.local_columns)


class _FakeFlat:
    def __init__(self, counts):
        self.blk_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("counts,budget", [([5, 7, 0, 9], 10 ** 6), ([50] * 40, 20000), ([4000], 20000)])
def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch, counts, budget):
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    P = 4
    flat = _FakeFlat(counts)
    outs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(_FakeHandle(flat.blk_offset, P), flat, str(d))
        outs.append((np.load(d / "residuals.npy"), np.load(d / "jacobian.npy")))
    (r, J), (r2, J2) = outs
    assert np.array_equal(r, r2) and np.array_equal(J, J2)  # same arguments, same rows
    assert r.dtype == J.dtype == np.float64 and J.shape == (r.size, P) and r.size % 2 == 0
    assert r.nbytes + J.nbytes <= budget
    assert np.array_equal(J, r[:, None] * 100 + np.arange(P))  # row i of J belongs to residual i
    assert np.all(r[0::2] % 2 == 0) and np.array_equal(r[1::2], r[0::2] + 1)  # u and v rows of an observation stay together
    assert np.all(np.diff(r) > 0)  # observation order
    if 2 * sum(counts) * (1 + P) * 8 <= budget:
        assert np.array_equal(r, np.arange(2 * sum(counts)))  # the whole output when it fits
    else:
        assert r.nbytes + J.nbytes > budget // 2  # a sample, but not a needlessly small one


@pytest.mark.gpu
def test_bench_dump_outputs_hold_the_timed_pass(tmp_path, oracle):
    from tests import helpers, synth

    lines = []
    for k, steps in enumerate(("3", "2")):  # --steps differs between the two runs, nothing else
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", steps, *COMMON[2:], "--no-lm", "--no-cpu", "--dump-outputs", str(tmp_path / str(k))],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(_line(r.stdout))
    assert lines[0]["steps"] == 3 and lines[1]["steps"] == 2
    r0, J0 = np.load(tmp_path / "0" / "residuals.npy"), np.load(tmp_path / "0" / "jacobian.npy")
    r1, J1 = np.load(tmp_path / "1" / "residuals.npy"), np.load(tmp_path / "1" / "jacobian.npy")
    assert np.array_equal(r0, r1) and np.array_equal(J0, J1)
    # 40 views x 400 points fit the budget whole: the dump is the full output of Mode A at bench.py's (unsolved) starting point
    sc = synth.scene_intrinsics(40, rows=20, cols=20, spacing=0.002, seed=7, noise_px=0.2)
    ro, Jo = helpers.oracle_eval(oracle, sc.flat)
    assert r0.shape == ro.shape and J0.shape == Jo.shape
    assert np.abs(r0 - ro).max() <= 1e-9
    assert (np.abs(J0 - Jo) / np.maximum(1.0, np.abs(Jo))).max() <= 1e-9
