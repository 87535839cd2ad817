"""Evaluating the critics of general-step trainers: the device path (k_qval_layer through sac_q_values_general /
sac_q_values_general_many, q_values(general="device")) against the default, q_values' host path -- sac_sync,
sac_get_params of the nets and a float32 NumPy forward -- in ONE process.  One JSON line per measurement, appended to
--out (default: profiles/q_values_general_bench.jsonl).

    python scripts/bench_q_values_general.py [--windows 3] [--window-s 0.5] [--out FILE]

The method is scripts/bench_q_values.py's: every timed call returns with its values on the host, so a host clock around
a window of calls measures them; a window lasts at least --window-s seconds after a warm-up, and each figure is the
median over --windows windows with the smallest and the largest next to it.  (a) / (b) SACTrainer.q_values with
general="device" / general="host", qf1 and qf2, at 1, 256 and 1000 rows on Lift (42 / 7), for hidden sizes [512,512],
[1024,1024] and [256,256,256]; (c) / (d) group.q_values_many with general="device" / "host" over 16 [512,512] members,
qf1 and qf2 each, at 1 and at 64 rows per member."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_q_values import A, NETS, O, emit, make_trainer, windows  # noqa: E402
from robosuite_benchmark_amd.group import q_values_many  # noqa: E402

SHAPES = ((512, 512), (1024, 1024), (256, 256, 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=0.5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "q_values_general_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    for hidden in SHAPES:
        t = make_trainer(1, hidden=hidden)
        assert t.fused_mode() == 3, hidden
        for n in (1, 256, 1000):
            obs, act = rs.normal(0, 0.5, (n, O)).astype(np.float32), np.tanh(rs.normal(size=(n, A))).astype(np.float32)
            dev, host = t.q_values(obs, act, nets=NETS, general="device"), t.q_values(obs, act, nets=NETS, general="host")
            err = float(np.max(np.abs(dev - host)))
            d = windows(lambda: t.q_values(obs, act, nets=NETS, general="device"), args.windows, args.window_s)
            h = windows(lambda: t.q_values(obs, act, nets=NETS, general="host"), args.windows, args.window_s)
            emit(dict(what='a: SACTrainer.q_values(general="device") (sac_q_values_general), qf1 + qf2, per call',
                      hidden=list(hidden), n=n, max_abs_diff_to_host=err, max_abs_host=float(np.max(np.abs(host))), **d),
                 args.out)
            emit(dict(what='b: SACTrainer.q_values(general="host") (sac_get_params of qf1 + qf2 and the NumPy forward), per call',
                      hidden=list(hidden), n=n, host_over_device=h["us_median"] / d["us_median"], **h), args.out)
        del t
    ts = [make_trainer(10 + i, hidden=(512, 512)) for i in range(16)]
    for n in (1, 64):
        obs_l = [rs.normal(0, 0.5, (n, O)).astype(np.float32) for _ in ts]
        act_l = [np.tanh(rs.normal(size=(n, A))).astype(np.float32) for _ in ts]
        nets_l = [NETS] * 16
        d = windows(lambda: q_values_many(ts, obs_l, act_l, nets_l, general="device"), args.windows, args.window_s)
        h = windows(lambda: q_values_many(ts, obs_l, act_l, nets_l, general="host"), args.windows, args.window_s)
        emit(dict(what='c: group.q_values_many(general="device") (sac_q_values_general_many), 16 [512,512] Lift members, '
                       'qf1 + qf2, per call', hidden=[512, 512], n=n, **d), args.out)
        emit(dict(what='d: group.q_values_many(general="host") (sac_get_params + NumPy forward for each of the 16 members), '
                       'per call', hidden=[512, 512], n=n, host_over_device=h["us_median"] / d["us_median"], **h), args.out)


if __name__ == "__main__":
    main()
