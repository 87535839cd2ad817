"""Recycling hidden units: the device route (two k_unit_recycle launches through sac_recycle_units[_many]) against the host
route of the SAME trainer -- _export_state, infer.recycle_reference, _import_state: sac_get_params / sac_set_params of the
nets, sac_get_opt_state / sac_set_opt_state of the three trained ones, the scalars -- in ONE process.  One JSON line per
measurement, appended to --out (default: profiles/recycle_units_bench.jsonl).

    python scripts/bench_recycle.py [--windows 3] [--window-s 1.0] [--out FILE]

Every timed call returns with the state written (each ends in its own wait), so a host clock around a window of calls
measures them.  The unit lists and the fresh rows are made once per case, outside the windows, and are the same for both
routes (the argument checks run inside both).  All shapes are warmed first (a few training steps, both routes, their
states compared as bytes); then, per case, device and host windows ALTERNATE, each at least --window-s seconds long, and
a figure is the median over --windows windows with the smallest and the largest next to it.  (a) / (b)
SACTrainer.recycle_units of policy, qf1 and qf2 on the device / on the host on Lift (42 / 7) for hidden sizes [256,256]
(the fused kernels' shapes), [512,512], [1024,1024] and [256,256,256], with 1 %, 10 % and 100 % of every hidden layer's
units listed; (c) / (d) group.recycle_units_many over 16 members against 16 host calls, for [256,256] and [512,512]."""
from __future__ import annotations

import argparse
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_q_values import A, O, emit, make_trainer  # noqa: E402
from bench_unit_statistics import alternating  # noqa: E402
from robosuite_benchmark_amd import infer  # noqa: E402
from robosuite_benchmark_amd.group import recycle_units_many  # noqa: E402

SHAPES = ((256, 256), (512, 512), (1024, 1024), (256, 256, 256))
SHARES = (0.01, 0.10, 1.00)
NETS = ("policy", "qf1", "qf2")


def selection(t, share, rs):
    """(units, fresh rows): max(1, share * N) units of every hidden layer of the three trained nets, drawn without
    replacement, ascending."""
    units = OrderedDict((net, [np.sort(rs.choice(N, max(1, int(round(share * N))), replace=False)).astype(np.int32)
                               for N in t._hidden(net)]) for net in NETS)
    return units, infer.fresh_unit_rows(t, units, rs)


def warm(t, rs, steps=3):
    B = t._batch
    batch = dict(observations=rs.normal(0, 0.5, (B, O)).astype(np.float32), actions=np.tanh(rs.normal(size=(B, A))).astype(np.float32),
                 rewards=rs.normal(size=B).astype(np.float32), terminals=np.zeros(B, np.float32),
                 next_observations=rs.normal(0, 0.5, (B, O)).astype(np.float32))
    for _ in range(steps):
        t.train(batch)
    units, rows = selection(t, 0.10, rs)
    before = t.state_dict()
    t.recycle_units(units, fresh=rows)
    dev = t.state_dict()
    t.load_state_dict(before)
    t.recycle_units(units, fresh=rows, route="host")
    host = t.state_dict()
    for net in dev["params"]:                                          # the two routes write the same state
        assert np.array_equal(dev["params"][net].view(np.uint32), host["params"][net].view(np.uint32)), net
    for net in dev["opt"]:
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(dev["opt"][net], host["opt"][net])), net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "recycle_units_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    trainers = {hidden: make_trainer(1, hidden=hidden) for hidden in SHAPES}
    groups = {hidden: [make_trainer(10 + i, hidden=hidden) for i in range(16)] for hidden in SHAPES[:2]}
    for t in list(trainers.values()) + [t for ts in groups.values() for t in ts]:      # all shapes warmed, both routes
        warm(t, rs)
    for hidden, t in trainers.items():
        for share in SHARES:
            units, rows = selection(t, share, rs)
            listed = int(sum(u.size for us in units.values() for u in us))
            d, h = alternating([lambda: t.recycle_units(units, fresh=rows),
                                lambda: t.recycle_units(units, fresh=rows, route="host")], args.windows, args.window_s)
            emit(dict(what="a: SACTrainer.recycle_units on the device, policy, qf1 and qf2, Adam moments reset, per call",
                      hidden=list(hidden), share=share, units=listed, **d), args.out)
            emit(dict(what="b: the host route of the same trainer (export, recycle_reference, import), per call",
                      hidden=list(hidden), share=share, units=listed, host_over_device=h["us_median"] / d["us_median"], **h),
                 args.out)
    for hidden, ts in groups.items():
        for share in SHARES:
            sel = [selection(t, share, rs) for t in ts]
            units, rows = [s[0] for s in sel], [s[1] for s in sel]
            many = lambda: recycle_units_many(ts, units, fresh_list=rows)                              # noqa: E731
            each = lambda: [t.recycle_units(u, fresh=r, route="host") for t, u, r in zip(ts, units, rows)]   # noqa: E731
            d, h = alternating([many, each], args.windows, args.window_s)
            emit(dict(what="c: group.recycle_units_many on the device, 16 Lift members, three nets each, per call",
                      hidden=list(hidden), share=share, **d), args.out)
            emit(dict(what="d: 16 host calls (each member's host route), per 16 calls", hidden=list(hidden), share=share,
                      host_over_device=h["us_median"] / d["us_median"], **h), args.out)


if __name__ == "__main__":
    main()
