"""Per-unit statistics of the hidden layers: the device route (k_units / k_qval_layer and k_unit_moments through
sac_unit_moments[_general][_many]) against the host route of the SAME trainer -- sac_sync, sac_get_params of the nets, a
float32 NumPy forward layer by layer and infer.unit_moments_reference -- in ONE process.  One JSON line per measurement,
appended to --out (default: profiles/unit_statistics_bench.jsonl).

    python scripts/bench_unit_statistics.py [--windows 3] [--window-s 1.0] [--out FILE]

Every timed call returns with its records on the host (each call ends in its own synchronise), so a host clock around a
window of calls measures them.  All shapes are warmed first; then, per case, device and host windows ALTERNATE (device,
host, device, host, ...), each at least --window-s seconds long, and a figure is the median over --windows windows with
the smallest and the largest next to it.  (a) / (b) SACTrainer.unit_moments of policy + qf1 + qf2 on the device / on the
host at 1, 256, 1000 and 2500 rows on Lift (42 / 7), for hidden sizes [256,256] (the fused kernels' shapes), [512,512],
[1024,1024] and [256,256,256]; (c) / (d) group.unit_moments_many over 16 members of 64 rows each against 16 host calls,
for [256,256] and [512,512]."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_q_values import A, O, emit, make_trainer  # noqa: E402
from robosuite_benchmark_amd.group import unit_moments_many  # noqa: E402

NETS = ("policy", "qf1", "qf2")
SHAPES = ((256, 256), (512, 512), (1024, 1024), (256, 256, 256))
ROWS = (1, 256, 1000, 2500)


def alternating(fns, n_windows, window_s):
    """us per call of each fn of `fns`: median, min, max over n_windows windows of at least window_s seconds each, the
    fns' windows taking turns."""
    per = [[] for _ in fns]
    for _ in range(n_windows):
        for k, fn in enumerate(fns):
            n, t0 = 0, time.perf_counter()
            while True:
                fn()
                n += 1
                dt = time.perf_counter() - t0
                if dt >= window_s:
                    break
            per[k].append(1e6 * dt / n)
    return [dict(us_median=float(np.median(p)), us_min=float(min(p)), us_max=float(max(p)), windows=n_windows) for p in per]


def inputs(rs, n):
    return rs.normal(0, 0.5, (n, O)).astype(np.float32), np.tanh(rs.normal(size=(n, A))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "unit_statistics_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    trainers = {hidden: make_trainer(1, hidden=hidden) for hidden in SHAPES}
    groups = {hidden: [make_trainer(10 + i, hidden=hidden) for i in range(16)] for hidden in SHAPES[:2]}
    data = {n: inputs(rs, n) for n in ROWS}
    device = lambda t, obs, act: t.unit_moments(obs, act, nets=NETS, general="device")          # noqa: E731
    host = lambda t, obs, act: t._unit_moments_host(obs, act, list(NETS))                        # noqa: E731
    for t in trainers.values():                                       # all shapes warmed: staging, scratch, both routes
        for n in ROWS:
            device(t, *data[n]), host(t, *data[n])
    for hidden, t in trainers.items():
        for n in ROWS:
            obs, act = data[n]
            d, h = alternating([lambda: device(t, obs, act), lambda: host(t, obs, act)], args.windows, args.window_s)
            emit(dict(what="a: SACTrainer.unit_moments on the device, policy + qf1 + qf2, per call", hidden=list(hidden), n=n,
                      **d), args.out)
            emit(dict(what="b: the host route of the same trainer (sac_get_params of the three nets, NumPy forward, "
                           "unit_moments_reference), per call", hidden=list(hidden), n=n,
                      host_over_device=h["us_median"] / d["us_median"], **h), args.out)
    obs_l, act_l = zip(*[inputs(rs, 64) for _ in range(16)])
    for hidden, ts in groups.items():
        many = lambda: unit_moments_many(ts, obs_l, act_l, [NETS] * 16, general="device")        # noqa: E731
        each = lambda: [host(t, o, a) for t, o, a in zip(ts, obs_l, act_l)]                      # noqa: E731
        many(), each()
        d, h = alternating([many, each], args.windows, args.window_s)
        emit(dict(what="c: group.unit_moments_many on the device, 16 Lift members x 64 rows, policy + qf1 + qf2, per call",
                  hidden=list(hidden), n=64, **d), args.out)
        emit(dict(what="d: 16 host calls (each member's host route), per 16 calls", hidden=list(hidden), n=64,
                  host_over_device=h["us_median"] / d["us_median"], **h), args.out)


if __name__ == "__main__":
    main()
