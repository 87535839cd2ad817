"""The TD3 objectives' device statistics and replay evaluation in place, against the routes that existed before, on the
SAME trainer in ONE process.  One JSON line per measurement, appended to --out (default:
profiles/td3_evaluate_replay_bench.jsonl).

    python scripts/bench_td3_evaluate_replay.py [--windows 3] [--window-s 1.0] [--out FILE]

The method is scripts/bench_evaluate.py's: every timed call returns with its statistics on the host (the calls end
synchronised), a window lasts at least --window-s seconds after a warm-up, the windows of the two sides ALTERNATE, and each
figure is the median over --windows windows with the smallest and the largest next to it.  Every trainer is built and
warmed under every route in front of the first window.  Lift (42 / 7); [256,256] (the fused kernels' shapes) and
[512,512] (the general step, general="device"); 1, 256, 1000 and 2500 rows.
(a) evaluate_td3(stats="device") against (b) evaluate_td3(stats="host"), the parent's route unchanged: the yardstick.
(c) evaluate_td3_replay(indices) against (d) evaluate_td3(buffer.gather(indices)) on the same trainer and indices, under
both values of stats.
(e) / (f) and (g) / (h): the same two comparisons for 16 members x 64 rows in one td3_evaluate_many /
td3_evaluate_replay_many call."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from robosuite_benchmark_amd import EnvReplayBuffer  # noqa: E402
from robosuite_benchmark_amd.group import td3_evaluate_many, td3_evaluate_replay_many  # noqa: E402
from bench_evaluate import alternating_windows, emit  # noqa: E402
from bench_td3_evaluate import A, O, make_batch, make_trainer  # noqa: E402

SHAPES = [(256, 256), (512, 512)]
ROWS = (1, 256, 1000, 2500)
BUFFER_ROWS = 20000


def make_buffer(seed):
    rs = np.random.RandomState(seed)
    b, _ = make_batch(rs, BUFFER_ROWS)
    buf = EnvReplayBuffer(BUFFER_ROWS, obs_dim=O, action_dim=A)
    buf.add_block(b["observations"], b["actions"], b["rewards"], b["next_observations"], b["terminals"])
    buf.seed(seed)
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "td3_evaluate_replay_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    kw = dict(general="device")
    solo = {hidden: make_trainer(1, hidden=hidden) for hidden in SHAPES}
    groups = {hidden: [make_trainer(10 + i, hidden=hidden) for i in range(16)] for hidden in SHAPES}
    buf, bufs = make_buffer(3), [make_buffer(20 + i) for i in range(16)]
    assert [t.fused_mode() == 3 for t in solo.values()] == [False, True]
    for hidden in SHAPES:                                             # every shape warmed under every route
        b, e = make_batch(rs, 64)
        for stats in ("host", "device"):
            for t in [solo[hidden]] + groups[hidden]:
                t.evaluate_td3(b, eps=e, stats=stats, **kw)
                t.evaluate_td3_replay(buf, indices=np.arange(64), eps=e, stats=stats, **kw)
    for hidden in SHAPES:
        t, tag = solo[hidden], dict(hidden=list(hidden))
        for n in ROWS:
            batch, eps = make_batch(rs, n)
            idx = rs.randint(0, BUFFER_ROWS, n)
            dev = t.evaluate_td3(batch, eps=eps, stats="device", **kw)
            host = t.evaluate_td3(batch, eps=eps, **kw)
            rel = max(abs(dev[k] - host[k]) / max(abs(host[k]), 1e-300) for k in host)
            d, h = alternating_windows([lambda: t.evaluate_td3(batch, eps=eps, stats="device", **kw),
                                        lambda: t.evaluate_td3(batch, eps=eps, **kw)], args.windows, args.window_s)
            emit(dict(what="a: evaluate_td3(stats='device') (k_eval_moments_td3), per call", n=n, max_rel_diff_to_host=rel,
                      **tag, **d), args.out)
            emit(dict(what="b: evaluate_td3(stats='host'): the columns copied out, td3_eval_statistics, per call", n=n,
                      **tag, **h), args.out)
            for stats in ("host", "device"):
                assert t.evaluate_td3_replay(buf, indices=idx, eps=eps, stats=stats, **kw) == \
                    t.evaluate_td3(buf.gather(idx), eps=eps, stats=stats, **kw)
                r, g = alternating_windows([lambda: t.evaluate_td3_replay(buf, indices=idx, eps=eps, stats=stats, **kw),
                                            lambda: t.evaluate_td3(buf.gather(idx), eps=eps, stats=stats, **kw)],
                                           args.windows, args.window_s)
                emit(dict(what="c: evaluate_td3_replay(indices) (k_eval_rows in front), per call", n=n, stats=stats,
                          **tag, **r), args.out)
                emit(dict(what="d: evaluate_td3(buffer.gather(indices)) on the same trainer and indices, per call", n=n,
                          stats=stats, **tag, **g), args.out)
        ts = groups[hidden]
        made = [make_batch(rs, 64) for _ in ts]
        batches, eps_l = [m[0] for m in made], [m[1] for m in made]
        idxs = [rs.randint(0, BUFFER_ROWS, 64) for _ in ts]
        d, h = alternating_windows([lambda: td3_evaluate_many(ts, batches, eps=eps_l, stats="device", **kw),
                                    lambda: td3_evaluate_many(ts, batches, eps=eps_l, **kw)], args.windows, args.window_s)
        emit(dict(what="e: td3_evaluate_many(stats='device'), 16 Lift members x 64 rows, per call", n=64, **tag, **d), args.out)
        emit(dict(what="f: td3_evaluate_many(stats='host'), the same call, per call", n=64, **tag, **h), args.out)
        for stats in ("host", "device"):
            r, g = alternating_windows(
                [lambda: td3_evaluate_replay_many(ts, bufs, indices=idxs, eps=eps_l, stats=stats, **kw),
                 lambda: td3_evaluate_many(ts, [b.gather(i) for b, i in zip(bufs, idxs)], eps=eps_l, stats=stats, **kw)],
                args.windows, args.window_s)
            emit(dict(what="g: td3_evaluate_replay_many(indices), 16 Lift members x 64 rows, per call", n=64, stats=stats,
                      **tag, **r), args.out)
            emit(dict(what="h: td3_evaluate_many over the 16 gathered batches, per call", n=64, stats=stats, **tag, **g),
                 args.out)


if __name__ == "__main__":
    main()
