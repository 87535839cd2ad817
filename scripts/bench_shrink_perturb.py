"""Reset and shrink-and-perturb: the device route (one k_param_perturb launch through sac_shrink_perturb[_many]) against the
host route of the SAME trainer -- _export_state, infer.shrink_perturb_reference (the Philox draw in NumPy), _import_state:
sac_get_params / sac_set_params of the nets, sac_get_opt_state / sac_set_opt_state of the three trained ones, the scalars
-- in ONE process.  One JSON line per measurement, appended to --out (default: profiles/shrink_perturb_bench.jsonl).

    python scripts/bench_shrink_perturb.py [--windows 3] [--window-s 1.0] [--out FILE]

Every timed call returns with the state written (each ends in its own wait), so a host clock around a window of calls
measures them.  All shapes are warmed first (a few training steps, both routes, their states compared as bytes); then, per
case, device and host windows ALTERNATE, each at least --window-s seconds long, and a figure is the median over --windows
windows with the smallest and the largest next to it.  (a) / (b) SACTrainer.shrink_perturb of policy, qf1 and qf2 with
opt=True, targets=True on the device / on the host on Lift (42 / 7) for hidden sizes [256,256] (the fused kernels' shapes),
[512,512], [1024,1024] and [256,256,256], as a reset (shrink 0, perturb 1) and as shrink and perturb (0.8 / 0.2); (c) / (d)
group.shrink_perturb_many over 16 members against 16 host calls, for [256,256] and [512,512]."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_q_values import A, O, emit, make_trainer  # noqa: E402
from bench_unit_statistics import alternating  # noqa: E402
from robosuite_benchmark_amd.group import shrink_perturb_many  # noqa: E402

SHAPES = ((256, 256), (512, 512), (1024, 1024), (256, 256, 256))
MODES = (("reset", 0.0, 1.0), ("shrink and perturb", 0.8, 0.2))


def warm(t, rs, steps=3):
    B = t._batch
    batch = dict(observations=rs.normal(0, 0.5, (B, O)).astype(np.float32), actions=np.tanh(rs.normal(size=(B, A))).astype(np.float32),
                 rewards=rs.normal(size=B).astype(np.float32), terminals=np.zeros(B, np.float32),
                 next_observations=rs.normal(0, 0.5, (B, O)).astype(np.float32))
    for _ in range(steps):
        t.train(batch)
    for _, shrink, perturb in MODES:
        kw = dict(shrink=shrink, perturb=perturb, seed=7, draw=1, opt=True, targets=True)
        before = t.state_dict()
        t.shrink_perturb(**kw)
        dev = t.state_dict()
        t.load_state_dict(before)
        t.shrink_perturb(route="host", **kw)
        host = t.state_dict()
        for net in dev["params"]:                                      # the two routes write the same state
            assert np.array_equal(dev["params"][net].view(np.uint32), host["params"][net].view(np.uint32)), net
        for net in dev["opt"]:
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(dev["opt"][net], host["opt"][net])), net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "shrink_perturb_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    trainers = {hidden: make_trainer(1, hidden=hidden) for hidden in SHAPES}
    groups = {hidden: [make_trainer(10 + i, hidden=hidden) for i in range(16)] for hidden in SHAPES[:2]}
    for t in list(trainers.values()) + [t for ts in groups.values() for t in ts]:      # all shapes warmed, both routes
        warm(t, rs)
    for hidden, t in trainers.items():
        n = int(sum(t._get_params(net).size for net in ("policy", "qf1", "qf2")))
        for mode, shrink, perturb in MODES:
            kw = dict(shrink=shrink, perturb=perturb, seed=7, opt=True, targets=True)
            d, h = alternating([lambda: t.shrink_perturb(draw=2, **kw), lambda: t.shrink_perturb(draw=2, route="host", **kw)],
                               args.windows, args.window_s)
            emit(dict(what="a: SACTrainer.shrink_perturb on the device, policy, qf1 and qf2, moments reset, targets written, per call",
                      hidden=list(hidden), mode=mode, parameters=n, **d), args.out)
            emit(dict(what="b: the host route of the same trainer (export, shrink_perturb_reference, import), per call",
                      hidden=list(hidden), mode=mode, parameters=n, host_over_device=h["us_median"] / d["us_median"], **h), args.out)
    for hidden, ts in groups.items():
        for mode, shrink, perturb in MODES:
            kw = dict(shrink=shrink, perturb=perturb, opt=True, targets=True)
            many = lambda: shrink_perturb_many(ts, draws=3, **kw)                                       # noqa: E731
            each = lambda: [t.shrink_perturb(draw=3, route="host", **kw) for t in ts]                   # noqa: E731
            d, h = alternating([many, each], args.windows, args.window_s)
            emit(dict(what="c: group.shrink_perturb_many on the device, 16 Lift members, three nets each, per call",
                      hidden=list(hidden), mode=mode, **d), args.out)
            emit(dict(what="d: 16 host calls (each member's host route), per 16 calls", hidden=list(hidden), mode=mode,
                      host_over_device=h["us_median"] / d["us_median"], **h), args.out)


if __name__ == "__main__":
    main()
