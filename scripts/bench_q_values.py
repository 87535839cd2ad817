"""Evaluating the critics: the device path (k_qval through sac_q_values / sac_q_values_many) against the only route to a Q
value of a training run there was before it, sac_get_params of the nets and a NumPy forward on the host, in ONE process.
One JSON line per measurement, appended to --out (default: profiles/q_values_bench.jsonl).

    python scripts/bench_q_values.py [--windows 3] [--window-s 0.5] [--out FILE]

Every timed call returns with its values on the host (the calls end synchronised), so a host clock around a window of
calls measures them; a window lasts at least --window-s seconds after a warm-up, and each figure is the median over
--windows windows with the smallest and the largest next to it.  (a) SACTrainer.q_values, qf1 and qf2, at 1, 256 and
1000 rows on Lift (42 / 7); (b) the host alternative at the same rows: sac_get_params of qf1 and qf2, then the float32
NumPy forward of both; (c) group.q_values_many over 16 Lift members, qf1 and qf2 each, at 1 and at 64 rows per member,
and (d) the host alternative for those 16 members."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy  # noqa: E402
from robosuite_benchmark_amd.group import q_values_many  # noqa: E402

O, A = 42, 7                                        # Lift
NETS = ("qf1", "qf2")


def make_trainer(seed, B=256, hidden=(256, 256)):
    rs = np.random.RandomState(seed)
    qs = [FlattenMlp(list(hidden), 1, O + A, rs=rs) for _ in range(4)]
    pol = TanhGaussianPolicy(list(hidden), O, A, rs=rs, noise=np.random.RandomState(seed))
    return SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], batch_size=B, noise_seed=seed)


def windows(fn, n_windows, window_s, warm_s=0.2):
    """us per call of fn(): median, min, max over n_windows windows of at least window_s seconds each."""
    t_end = time.perf_counter() + warm_s
    while time.perf_counter() < t_end:
        fn()
    per = []
    for _ in range(n_windows):
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(10):
                fn()
            n += 10
            dt = time.perf_counter() - t0
            if dt >= window_s:
                break
        per.append(1e6 * dt / n)
    return dict(us_median=float(np.median(per)), us_min=float(min(per)), us_max=float(max(per)), windows=n_windows)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def host_alternative(t, obs, act):
    """What a caller had before: the nets' parameters off the device, then a NumPy forward of each."""
    return t._q_values_host(obs, act, list(NETS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=0.5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "q_values_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    t = make_trainer(1)
    for n in (1, 256, 1000):
        obs, act = rs.normal(0, 0.5, (n, O)).astype(np.float32), np.tanh(rs.normal(size=(n, A))).astype(np.float32)
        dev, host = t.q_values(obs, act, nets=NETS), host_alternative(t, obs, act)
        err = float(np.max(np.abs(dev - host)))
        emit(dict(what="a: SACTrainer.q_values (sac_q_values), qf1 + qf2, per call", n=n, max_abs_diff_to_host=err,
                  **windows(lambda: t.q_values(obs, act, nets=NETS), args.windows, args.window_s)), args.out)
        emit(dict(what="b: sac_get_params of qf1 + qf2 and the NumPy forward, per call", n=n,
                  **windows(lambda: host_alternative(t, obs, act), args.windows, args.window_s)), args.out)
    ts = [make_trainer(10 + i) for i in range(16)]
    for n in (1, 64):
        obs_l = [rs.normal(0, 0.5, (n, O)).astype(np.float32) for _ in ts]
        act_l = [np.tanh(rs.normal(size=(n, A))).astype(np.float32) for _ in ts]
        nets_l = [NETS] * 16
        emit(dict(what="c: group.q_values_many (sac_q_values_many), 16 Lift members, qf1 + qf2, per call", n=n,
                  **windows(lambda: q_values_many(ts, obs_l, act_l, nets_l), args.windows, args.window_s)), args.out)
        emit(dict(what="d: sac_get_params + NumPy forward for each of the 16 members, per call", n=n,
                  **windows(lambda: [host_alternative(x, o, a) for x, o, a in zip(ts, obs_l, act_l)],
                            args.windows, args.window_s)), args.out)


if __name__ == "__main__":
    main()
