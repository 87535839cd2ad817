"""Evaluating the SAC objectives on held-out rows: the device path (k_eval through sac_evaluate / sac_evaluate_many) against
the host path of the SAME trainer -- sac_get_params of the five nets and a float32 NumPy forward, the only route there
was before -- in ONE process.  One JSON line per measurement, appended to --out (default: profiles/evaluate_bench.jsonl).

    python scripts/bench_evaluate.py [--windows 3] [--window-s 1.0] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_evaluate.py --kernel-run 200
    python scripts/bench_evaluate.py --kernel-stats DIR/.../..._kernel_stats.csv [--out FILE]

Every timed call returns with its statistics on the host (the calls end synchronised), so a host clock around a window
of calls measures them; a window lasts at least --window-s seconds after a warm-up, the windows of the two paths
ALTERNATE, and each figure is the median over --windows windows with the smallest and the largest next to it.
(a) SACTrainer.evaluate on the device and (b) its host path, at 1, 256, 1000 and 2500 rows on Lift (42 / 7);
(c) group.evaluate_many over 16 Lift members at 64 rows each and (d) the 16 host evaluations.
--kernel-run N: nothing but N evaluate calls at 1000 rows and N evaluate_many calls of 16 x 64 rows, for a profiler.
--kernel-stats CSV: k_eval's line of that run's kernel statistics, appended as one more record."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy  # noqa: E402
from robosuite_benchmark_amd.group import evaluate_many  # noqa: E402

O, A = 42, 7                                        # Lift


def make_trainer(seed, B=256, hidden=(256, 256)):
    rs = np.random.RandomState(seed)
    qs = [FlattenMlp(list(hidden), 1, O + A, rs=rs) for _ in range(4)]
    pol = TanhGaussianPolicy(list(hidden), O, A, rs=rs, noise=np.random.RandomState(seed))
    return SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], batch_size=B, noise_seed=seed)


def make_batch(rs, n):
    batch = dict(observations=rs.normal(0, 0.5, (n, O)).astype(np.float32),
                 actions=rs.uniform(-1, 1, (n, A)).astype(np.float32),
                 rewards=rs.uniform(0, 1, (n, 1)).astype(np.float32),
                 terminals=(rs.uniform(0, 1, (n, 1)) < 0.1).astype(np.float32),
                 next_observations=rs.normal(0, 0.5, (n, O)).astype(np.float32))
    return batch, (rs.standard_normal((n, A)).astype(np.float32), rs.standard_normal((n, A)).astype(np.float32))


def one_window(fn, window_s):
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(5):
            fn()
        n += 5
        dt = time.perf_counter() - t0
        if dt >= window_s:
            return 1e6 * dt / n


def alternating_windows(fns, n_windows, window_s, warm_s=0.2):
    """us per call of each fn: median, min, max over n_windows windows of at least window_s seconds, the fns taking turns."""
    for fn in fns:
        t_end = time.perf_counter() + warm_s
        while time.perf_counter() < t_end:
            fn()
    per = [[] for _ in fns]
    for _ in range(n_windows):
        for k, fn in enumerate(fns):
            per[k].append(one_window(fn, window_s))
    return [dict(us_median=float(np.median(p)), us_min=float(min(p)), us_max=float(max(p)), windows=n_windows) for p in per]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def on_host(t, batch, eps):
    """The host path of the same trainer, forced through evaluate's private switch."""
    t._evaluate_on_host = True
    try:
        return t.evaluate(batch, eps=eps, rows=True)
    finally:
        t._evaluate_on_host = False


def kernel_run(n_calls):
    rs = np.random.RandomState(0)
    t, ts = make_trainer(1), [make_trainer(10 + i) for i in range(16)]
    batch, eps = make_batch(rs, 1000)
    made = [make_batch(rs, 64) for _ in ts]
    for _ in range(n_calls):
        t.evaluate(batch, eps=eps)
    for _ in range(n_calls):
        evaluate_many(ts, [m[0] for m in made], eps=[m[1] for m in made])


def kernel_stats(path, out):
    for row in csv.DictReader(open(path)):
        if "k_eval" in row["Name"]:
            emit(dict(what="e: k_eval under rocprofv3 --kernel-trace --stats: half of the calls evaluate at 1000 rows (189 "
                           "workgroups), half evaluate_many of 16 members x 64 rows (192 workgroups)", kernel=row["Name"],
                      calls=int(row["Calls"]), us_average=float(row["AverageNs"]) / 1e3, us_min=float(row["MinNs"]) / 1e3,
                      us_max=float(row["MaxNs"]) / 1e3), out)
            return
    raise SystemExit(f"{path}: no k_eval line")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "evaluate_bench.jsonl"))
    ap.add_argument("--kernel-run", dest="kernel_run", type=int, default=0)
    ap.add_argument("--kernel-stats", dest="kernel_stats", type=str, default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args.out)
    if args.kernel_run:
        return kernel_run(args.kernel_run)
    rs = np.random.RandomState(0)
    t = make_trainer(1)
    for n in (1, 256, 1000, 2500):
        batch, eps = make_batch(rs, n)
        dev, host = t.evaluate(batch, eps=eps, rows=True)[1], on_host(t, batch, eps)[1]
        err = max(float(np.max(np.abs(dev[k] - host[k]))) for k in ("q1", "q2", "q1_new", "q2_new", "tq1", "tq2", "log_pi", "y"))
        d, h = alternating_windows([lambda: t.evaluate(batch, eps=eps), lambda: on_host(t, batch, eps)], args.windows,
                                   args.window_s)
        emit(dict(what="a: SACTrainer.evaluate on the device (sac_evaluate), per call", n=n, max_abs_diff_to_host=err, **d),
             args.out)
        emit(dict(what="b: the host path of the same trainer (sac_get_params of five nets + NumPy forward), per call", n=n,
                  **h), args.out)
    ts = [make_trainer(10 + i) for i in range(16)]
    made = [make_batch(rs, 64) for _ in ts]
    batches, eps_l = [m[0] for m in made], [m[1] for m in made]
    d, h = alternating_windows([lambda: evaluate_many(ts, batches, eps=eps_l),
                                lambda: [on_host(x, b, e) for x, b, e in zip(ts, batches, eps_l)]], args.windows, args.window_s)
    emit(dict(what="c: group.evaluate_many (sac_evaluate_many), 16 Lift members x 64 rows, per call", n=64, **d), args.out)
    emit(dict(what="d: 16 host evaluations (sac_get_params of five nets + NumPy forward each), per call", n=64, **h), args.out)


if __name__ == "__main__":
    main()
