"""Evaluating the TD3 objectives on held-out rows: the device path (k_eval_td3 through td3_evaluate / td3_evaluate_many)
against the host path of the SAME trainer -- sac_get_params of the six nets and a float32 NumPy forward -- in ONE process.
One JSON line per measurement, appended to --out (default: profiles/td3_evaluate_bench.jsonl).

    python scripts/bench_td3_evaluate.py [--windows 3] [--window-s 1.0] [--out FILE]

Every timed call returns with its statistics on the host (the calls end synchronised), so a host clock around a window
of calls measures them; a window lasts at least --window-s seconds after a warm-up, the windows of the two paths
ALTERNATE, and each figure is the median over --windows windows with the smallest and the largest next to it.
(a) TD3Trainer.evaluate_td3 on the device and (b) its host path, at 1, 256, 1000 and 2500 rows on Lift (42 / 7);
(c) group.td3_evaluate_many over 16 Lift members at 64 rows each and (d) the 16 host evaluations."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_evaluate import alternating_windows, emit  # noqa: E402
from robosuite_benchmark_amd import FlattenMlp, TanhMlpPolicy, TD3Trainer  # noqa: E402
from robosuite_benchmark_amd.group import td3_evaluate_many  # noqa: E402

O, A = 42, 7                                        # Lift
ROW_KEYS = ("q1", "q2", "q_pi", "tq1", "tq2", "y")


def make_trainer(seed, B=256, hidden=(256, 256)):
    rs = np.random.RandomState(seed)
    qs = [FlattenMlp(list(hidden), 1, O + A, rs=rs) for _ in range(4)]
    pols = [TanhMlpPolicy(list(hidden), A, O, rs=rs) for _ in range(2)]
    return TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1],
                      batch_size=B, noise_seed=seed)


def make_batch(rs, n):
    batch = dict(observations=rs.normal(0, 0.5, (n, O)).astype(np.float32),
                 actions=rs.uniform(-1, 1, (n, A)).astype(np.float32),
                 rewards=rs.uniform(0, 1, (n, 1)).astype(np.float32),
                 terminals=(rs.uniform(0, 1, (n, 1)) < 0.1).astype(np.float32),
                 next_observations=rs.normal(0, 0.5, (n, O)).astype(np.float32))
    return batch, rs.standard_normal((n, A)).astype(np.float32)


def on_host(t, batch, eps):
    """The host path of the same trainer, forced through the evaluation's private switch."""
    t._evaluate_on_host = True
    try:
        return t.evaluate_td3(batch, eps=eps, rows=True)
    finally:
        t._evaluate_on_host = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "td3_evaluate_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    t = make_trainer(1)
    for n in (1, 256, 1000, 2500):
        batch, eps = make_batch(rs, n)
        dev, host = t.evaluate_td3(batch, eps=eps, rows=True)[1], on_host(t, batch, eps)[1]
        err = max(float(np.max(np.abs(dev[k] - host[k]))) for k in ROW_KEYS)
        d, h = alternating_windows([lambda: t.evaluate_td3(batch, eps=eps), lambda: on_host(t, batch, eps)], args.windows,
                                   args.window_s)
        emit(dict(what="a: TD3Trainer.evaluate_td3 on the device (td3_evaluate), per call", n=n, max_abs_diff_to_host=err, **d),
             args.out)
        emit(dict(what="b: the host path of the same trainer (sac_get_params of six nets + NumPy forward), per call", n=n,
                  **h), args.out)
    ts = [make_trainer(10 + i) for i in range(16)]
    made = [make_batch(rs, 64) for _ in ts]
    batches, eps_l = [m[0] for m in made], [m[1] for m in made]
    d, h = alternating_windows([lambda: td3_evaluate_many(ts, batches, eps=eps_l),
                                lambda: [on_host(x, b, e) for x, b, e in zip(ts, batches, eps_l)]], args.windows, args.window_s)
    emit(dict(what="c: group.td3_evaluate_many (td3_evaluate_many), 16 Lift members x 64 rows, per call", n=64, **d), args.out)
    emit(dict(what="d: 16 host evaluations (sac_get_params of six nets + NumPy forward each), per call", n=64, **h), args.out)


if __name__ == "__main__":
    main()
