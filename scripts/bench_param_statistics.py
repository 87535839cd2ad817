"""Per-tensor statistics of parameters, Adam moments and target gaps: the device route (k_param_moments / k_param_finish
through sac_param_moments[_many]) against the host route of the SAME trainer -- sac_get_params of the five nets,
sac_get_opt_state of the three trained ones and VECTORISED NumPy over each tensor (np.sum, np.dot, np.max: what a caller
had before; not the chunk-ordered infer.param_moments_reference, whose Python loop would flatter the kernel) -- in ONE
process.  One JSON line per measurement, appended to --out (default: profiles/param_statistics_bench.jsonl).

    python scripts/bench_param_statistics.py [--windows 3] [--window-s 1.0] [--out FILE]

Every timed call returns with its records on the host (each call ends in its own synchronise), so a host clock around a
window of calls measures them.  All shapes are warmed first (a few training steps, both routes); then, per case, device
and host windows ALTERNATE, each at least --window-s seconds long, and a figure is the median over --windows windows
with the smallest and the largest next to it.  (a) / (b) SACTrainer.param_moments of all five nets, opt and gap on, on
the device / on the host on Lift (42 / 7) for hidden sizes [256,256] (the fused kernels' shapes), [512,512],
[1024,1024] and [256,256,256]; (c) / (d) group.param_moments_many over 16 members against 16 host calls, for [256,256]
and [512,512]."""
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
from robosuite_benchmark_amd import _lib, infer  # noqa: E402
from robosuite_benchmark_amd.group import param_moments_many  # noqa: E402

SHAPES = ((256, 256), (512, 512), (1024, 1024), (256, 256, 256))


def host_vectorised(t):
    """The figures' inputs as a caller computed them before: the getters, then NumPy's own reductions per tensor."""
    out = {}
    for name in t.NETS:
        x = t._get_params(name).astype(np.float64)
        m = v = tg = None
        if name in infer.PARAM_TRAINED:
            m32, v32 = np.empty(x.size, np.float32), np.empty(x.size, np.float32)
            _lib.check(t._lib.sac_get_opt_state(t._h, t.NETS[name], _lib.ptr(m32), _lib.ptr(v32), x.size), "sac_get_opt_state")
            m, v = m32.astype(np.float64), v32.astype(np.float64)
        target = infer.param_target(t, name)
        if target is not None:
            tg = t._get_params(target).astype(np.float64)
        rec, off = [], 0
        for _, shape in t.param_tensors(name):
            e = int(np.prod(shape))
            s = slice(off, off + e)
            r = [np.sum(x[s]), np.dot(x[s], x[s]), np.max(np.abs(x[s])), float(e - np.count_nonzero(np.isfinite(x[s])))]
            r += [np.dot(m[s], m[s]), np.max(np.abs(m[s])), np.sum(v[s]), np.max(v[s])] if m is not None else [0.0] * 4
            d = x[s] - tg[s] if tg is not None else None
            r.append(np.dot(d, d) if d is not None else 0.0)
            rec.append(r)
            off += e
        out[name] = np.asarray(rec, np.float64)
    return out


def warm(t, rs, steps=3):
    B = t._batch
    batch = dict(observations=rs.normal(0, 0.5, (B, O)).astype(np.float32), actions=np.tanh(rs.normal(size=(B, A))).astype(np.float32),
                 rewards=rs.normal(size=B).astype(np.float32), terminals=np.zeros(B, np.float32),
                 next_observations=rs.normal(0, 0.5, (B, O)).astype(np.float32))
    for _ in range(steps):
        t.train(batch)
    dev, host = t.param_moments(), host_vectorised(t)
    for name in dev:                                                   # the two routes measure the same thing
        assert np.allclose(dev[name], host[name], rtol=1e-8, atol=1e-6), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "param_statistics_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    trainers = {hidden: make_trainer(1, hidden=hidden) for hidden in SHAPES}
    groups = {hidden: [make_trainer(10 + i, hidden=hidden) for i in range(16)] for hidden in SHAPES[:2]}
    for t in list(trainers.values()) + [t for ts in groups.values() for t in ts]:      # all shapes warmed, both routes
        warm(t, rs)
    for hidden, t in trainers.items():
        n_params = int(sum(np.prod(s) for net in t.NETS for _, s in t.param_tensors(net)))
        d, h = alternating([t.param_moments, lambda: host_vectorised(t)], args.windows, args.window_s)
        emit(dict(what="a: SACTrainer.param_moments on the device, five nets, opt and gap, per call", hidden=list(hidden),
                  parameters=n_params, **d), args.out)
        emit(dict(what="b: the host route of the same trainer (sac_get_params x 7, sac_get_opt_state x 3, vectorised NumPy), "
                       "per call", hidden=list(hidden), parameters=n_params, host_over_device=h["us_median"] / d["us_median"],
                  **h), args.out)
    for hidden, ts in groups.items():
        many = lambda: param_moments_many(ts)                                              # noqa: E731
        each = lambda: [host_vectorised(t) for t in ts]                                    # noqa: E731
        d, h = alternating([many, each], args.windows, args.window_s)
        emit(dict(what="c: group.param_moments_many on the device, 16 Lift members, five nets each, per call",
                  hidden=list(hidden), **d), args.out)
        emit(dict(what="d: 16 host calls (each member's host route, vectorised NumPy), per 16 calls", hidden=list(hidden),
                  host_over_device=h["us_median"] / d["us_median"], **h), args.out)


if __name__ == "__main__":
    main()
