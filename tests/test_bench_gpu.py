"""bench.py itself in the GPU suite: the N > 1 path (the parent starts the ranks, one process group, the barrier / all_reduce
/ padded all_gather of every region, the component -> rank deal of the configs[3] region) on two gloo ranks that share the
one GPU of the box, with the plumbing workload -- what the driver's scaling run executes with RCCL on a real node
(there the CLI ranks of regions D and F gather through gpemu_rccl_allgather; here, sharing a device, through files);
and --dump-outputs, the results of the last timed step written for comparing two builds; a plain run (no --full) with its
headline fields alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_two_gloo_ranks_sharing_the_gpu():
    env = dict(os.environ, BENCH_BACKEND="gloo", GPEMU_GATHER="file")     # (two RCCL ranks cannot share a device)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "tiny", "--steps", "3",
                          "--warmup", "1", "--full", "--no-cpu-baseline", "--train-runs", "6", "--pca8-steps", "1"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]                 # rank 0 prints ONE JSON line
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["dtype"] == "f64" and j["value"] > 0
    assert j["process_group"] == "gloo" and j["rccl_ranks"] == 0
    assert j["roofline"]["bound"] == "mfma" and "cpu_baseline" in j and j["cpu_baseline"] is None
    assert j["predictions"]["value"] > 0 and j["value_grad"]["value"] > 0
    p = j["pca8"]
    assert p["components"] == 8 and p["components_this_rank"] == 4 and len(p["best_neg_loglik_per_component"]) == 8
    assert all(v == v for v in p["best_neg_loglik_per_component"])          # every component's result arrived in the gather
    # regions D and F: the C product as one CLI process per bench rank (csrc/host/ranks.c), the run list / the 8 PCA components
    # dealt to the two processes, one gather at the end, rank 0's snapshot hashed
    t = j["estimate_thetas_c_layer"]
    assert "error" not in t and t["processes"] == 2 and t["runs"] == 6 and len(t["snapshot_sha256"]) == 64
    f = j["pca8_trained_by_cli_ranks"]
    assert "error" not in f and f["processes"] == 2 and not f["ranks_failed"] and f["components_trained_here"] == 4
    assert len(f["snapshot_sha256"]) == 64


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_timed_step_and_repeat_bit_for_bit(tmp_path):
    """--dump-outputs: what the last of the --steps timed steps handed back (one lock-step batch of likelihood evaluations),
    as float64 .npy files; two runs with the same arguments write the same bits"""
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "5",
                              "--warmup", "1", "--no-cpu-baseline", "--no-grad", "--no-predict", "--no-train", "--no-pca8",
                              "--no-interactive", "--no-single", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        j = json.loads(lines[0])
        assert j["steps"] == 5 and j["ms_per_step"] > 0
        B = j["evaluations_per_step"]
        got = {p.stem: np.load(p) for p in d.glob("*.npy")}
        assert sorted(got) == ["beta", "info", "logdet", "quad", "sigma2", "status", "value"]
        assert all(a.dtype == np.float64 and a.shape[0] == B for a in got.values())
        assert np.all(np.isfinite(got["value"])) and np.all(got["status"] == 0) and got["beta"].ndim == 2
        assert len(np.unique(got["value"])) == B                        # B distinct thetas, not one result repeated
        dumps.append(got)
    for name, a in dumps[0].items():
        assert a.tobytes() == dumps[1][name].tobytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [1, 2])
def test_plain_bench_runs_the_headline_region_alone(gpus):
    """without --full: set-up, warm-up, the timed steps and the line -- its headline fields, consistent with each other, and
    nothing of the parity gate, the rooflines, the other regions or the CPU baseline; one rank, and two gloo ranks sharing
    the GPU"""
    env = dict(os.environ, BENCH_BACKEND="gloo") if gpus > 1 else None
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--workload", "tiny", "--steps", "4",
                          "--warmup", "2"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["metric"] == "estimate_thetas likelihood-evals/sec + predictions/sec at N=8192 d=8 fp64"
    assert j["unit"] == "likelihood-evals/s" and j["higher_is_better"] is True and j["dtype"] == "f64"
    assert j["n_gpus"] == gpus and j["steps"] == 4 and j["warmup"] == 2 and j["ms_per_step"] > 0
    # value = evaluations per second over the timed steps, all ranks = n_gpus * evaluations_per_step / ms_per_step
    assert abs(j["value"] * j["ms_per_step"] * 1e-3 - gpus * j["evaluations_per_step"]) < 1e-9 * gpus * j["evaluations_per_step"]
    for k in ("parity_gate", "roofline", "roofline_other", "single_evaluation", "predictions", "interactive_mode_cli", "value_grad",
              "estimate_thetas_c_layer", "pca8", "pca8_trained_by_cli_ranks", "cpu_baseline", "speedup_vs_cpu_all_cores"):
        assert k not in j, k
