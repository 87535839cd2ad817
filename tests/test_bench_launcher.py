"""CPU: `python bench.py --gpus N` from a plain interpreter starts its N ranks itself (BASELINE.json configs[4] is an
8-GPU job; the reference's scale-out is one independent job per config, /root/reference/launch_jobs.sh:15-24).
--dry-run replaces the device work by a sleep, everything else -- child processes, gloo rendezvous on 127.0.0.1,
barriers, max-over-ranks timing, the all-gather of per-rank results, rank -> task mapping, one JSON line -- is the
real code path of an N-GPU run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*argv, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_plain_python_launches_its_own_ranks_and_prints_one_line():
    steps, ms = 20, 4.0
    p = run_bench("--gpus", "2", "--backend", "gloo", "--dry-run", "--sweep", "--steps", str(steps), "--warmup", "2",
                  "--dry-run-ms-per-step", str(ms))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == steps and d["warmup"] == 2 and d["scaling"] == "weak" and d["dry_run"] is True
    assert d["metric"].startswith("SAC grad-steps/sec") and d["unit"] == "grad-steps/s" and d["vs_baseline"] is None
    # rank -> task mapping of the sweep (parallel.SWEEP) and independent seeds
    assert [(t["rank"], t["task"], t["obs_dim"], t["act_dim"], t["seed"]) for t in d["config"]["rank_tasks"]] == [
        (0, "Lift", 42, 7, 17), (1, "Door", 46, 7, 18)]
    # every rank's result vector arrived through the all-gather; rank 1 "trains" at half the speed
    assert len(d["per_gpu"]) == 2 and d["per_gpu"][0][1] == 0.5 and d["per_gpu"][1][1] == 1.5
    # (the timed region ends in a barrier: the fast rank waits for the slow one, both clocks read the slow rank's time)
    assert all(abs(x[0] - steps / d["elapsed_max_s"]) <= 0.1 * x[0] for x in d["per_gpu"])
    # timing = MAX over ranks: at least the slow rank's sleep; value = whole-job steps / that time
    assert d["elapsed_max_s"] >= steps * ms * 2 * 1e-3
    assert abs(d["value"] - 2 * steps / d["elapsed_max_s"]) <= 0.01 * d["value"]
    assert abs(d["ms_per_step"] - d["elapsed_max_s"] / steps * 1e3) < 1e-3
    # the ranks of one node line up through shared memory (parallel.NodeBarrier)
    assert d["ranks_barrier"].startswith("shared memory")


def test_the_process_groups_barrier_is_the_fall_back():
    p = run_bench("--gpus", "2", "--backend", "gloo", "--dry-run", "--steps", "5", "--warmup", "1",
                  env_extra=dict(SAC_BENCH_NODE_BARRIER="0"))
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.strip()][0])
    assert d["n_gpus"] == 2 and d["ranks_barrier"] == "torch.distributed barrier (gloo)"


def test_a_failing_rank_makes_the_launcher_fail():
    p = run_bench("--gpus", "2", "--backend", "no-such-backend", "--dry-run", "--steps", "2", "--warmup", "0")
    assert p.returncode != 0
    assert not [l for l in p.stdout.splitlines() if l.strip().startswith("{")]


def test_a_rank_other_than_zero_dying_ends_the_job_at_once_and_is_named():
    """the launcher waited on rank 0 first -- which sat in the rendezvous for its 15-30 minute timeout
    when another rank had died.  All children are polled now: the job ends within seconds, the exit line names the rank
    that failed first and that rank's stderr is shown."""
    import time
    t0 = time.time()
    p = run_bench("--gpus", "3", "--backend", "gloo", "--dry-run", "--steps", "2", "--warmup", "0", "--dry-run-fail-rank", "2",
                  timeout=120)
    assert p.returncode != 0 and time.time() - t0 < 90
    assert "rank 2 failed first" in p.stderr and "exits on purpose" in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.strip().startswith("{")]


def test_torchrun_style_environment_is_still_honoured():
    """Under torch.distributed.run the ranks already exist (RANK / WORLD_SIZE in the environment): no self-launch."""
    p = run_bench("--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1",
                  env_extra=dict(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1"))
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip())
    assert d["n_gpus"] == 1 and d["config"]["parallelism"] == "single GPU"
    p = run_bench("--gpus", "2", "--dry-run", "--steps", "3", env_extra=dict(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1"))
    assert p.returncode != 0 and "does not match" in (p.stderr + p.stdout)


@pytest.mark.gpu
def test_two_ranks_share_the_one_gpu_of_this_box():
    """The N = 2 path end to end on real kernels: two self-launched ranks, both on device 0, gloo for the collective."""
    p = run_bench("--gpus", "2", "--backend", "gloo", "--single-device", "--steps", "60", "--warmup", "10", "--buffer",
                  "50000", "--full", timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.strip().startswith("{")][0])
    assert d["n_gpus"] == 2 and len(d["per_gpu"]) == 2 and d["value"] > 0
    assert "roofline" in d and "roofline_gather" in d
    assert all(x[1] == x[1] for x in d["per_gpu"])          # finite losses from both ranks


def test_concurrent_replicas_are_a_full_run_data_point():
    p = run_bench("--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1", "--replicas-per-gpu", "2")
    assert p.returncode != 0 and "--full" in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.strip().startswith("{")]


@pytest.mark.gpu
@pytest.mark.parametrize("agent", ["SAC", "TD3"])
def test_a_plain_run_reports_the_timed_steps_alone(agent):
    """Without --full the run sets up, warms up, times its steps and prints the line: no profiled replay, CPU baseline or
    other extra data point."""
    p = run_bench("--gpus", "1", "--agent", agent, "--steps", "40", "--warmup", "5", "--buffer", "20000", timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.strip().startswith("{")][0])
    assert d["steps"] == 40 and d["warmup"] == 5 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "grad-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    extras = {"kernels", "roofline_gather", "fixed_call_us", "short_loop", "cpu_baseline",
              "stepwise_interface", "ingest", "general_step", "concurrent_replicas"}
    if agent == "SAC":              # (the TD3 line's roofline is computed from its timed steps alone)
        extras.add("roofline")
    assert not extras & set(d), sorted(extras & set(d))


def test_dump_outputs_writes_the_timed_calls_diagnostics(tmp_path):
    """--dump-outputs DIR: the arrays the timed call returned land as DIR/<name>.npy (here: the dry run's diagnostics)."""
    p = run_bench("--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip())
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    import numpy as np
    last = np.load(tmp_path / "out" / "diag_last.npy")
    assert last.dtype == np.float32 and last.shape == (32,)
    assert float(last[0]) == d["final"]["QF1 Loss"] and float(last[28]) == d["final"]["Alpha"]
    assert sorted(os.listdir(tmp_path / "out")) == ["diag_first.npy", "diag_last.npy"]


@pytest.mark.gpu
@pytest.mark.parametrize("agent", ["SAC", "TD3"])
def test_dump_outputs_on_real_kernels(tmp_path, agent):
    """The dump holds the timed call's last diagnostics (the JSON line's "final") and the trainer state its last step
    left: every network's parameters and Adam moments, the scalars -- float32 / float64, 64 MB at most."""
    import numpy as np
    out = tmp_path / "out"
    p = run_bench("--gpus", "1", "--agent", agent, "--steps", "40", "--warmup", "5", "--buffer", "20000",
                  "--no-cpu-baseline", "--no-stepwise", "--no-peaks", "--dump-outputs", str(out), timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.strip().startswith("{")][0])
    assert d["steps"] == 40 and d["ms_per_step"] > 0
    arrays = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert float(arrays["diag_last"][0]) == d["final"]["QF1 Loss"]
    nets = ["policy", "qf1", "qf2", "target_qf1", "target_qf2"] + (["target_policy"] if agent == "TD3" else [])
    assert {f"params_{n}" for n in nets} <= set(arrays)
    assert {f"adam_{mv}_{n}" for mv in "mv" for n in ("policy", "qf1", "qf2")} <= set(arrays)
    assert arrays["params_policy"].size == (80398 if agent == "SAC" else 78599) and arrays["params_qf1"].size == 78849
    assert all(a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
