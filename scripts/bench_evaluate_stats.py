"""Where evaluate's statistics are reduced: stats="device" (k_eval_moments behind the evaluation's kernels, through
sac_evaluate_stats_many / sac_evaluate_general_stats_many) against stats="host" of the SAME trainer -- the columns copied
out and sac.eval_statistics, the path there was before, unchanged -- in ONE process.  One JSON line per measurement,
appended to --out (default: profiles/evaluate_stats_bench.jsonl).

    python scripts/bench_evaluate_stats.py [--windows 3] [--window-s 1.0] [--out FILE]

Every timed call returns with its statistics on the host (the calls end synchronised), so a host clock around a window of
calls measures them; a window lasts at least --window-s seconds after a warm-up, the windows of the two values ALTERNATE,
and each figure is the median over --windows windows with the smallest and the largest next to it (the method of
scripts/bench_evaluate.py).  Per shape -- Lift 42 / 7 with hidden [256, 256] (the fused kernels' shapes: k_eval) and
[512, 512] (the general step under general="device": k_eval_layer) -- (a) SACTrainer.evaluate at 1, 256, 1000 and 2500
rows, (b) group.evaluate_many over 16 members at 64 rows each.  No figure is promised: slower cases are reported as they
come out."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_evaluate import alternating_windows, emit, make_batch, make_trainer  # noqa: E402
from robosuite_benchmark_amd.group import evaluate_many  # noqa: E402


def largest_difference(a, b):
    """max |a[k] - b[k]| / max(1, |b[k]|) over the statistics of two evaluations of one batch."""
    return max(abs(a[k] - b[k]) / max(1.0, abs(b[k])) for k in b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "evaluate_stats_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    for hidden in ((256, 256), (512, 512)):
        kw = dict(general="device")                  # (decides for the general step only)
        t = make_trainer(1, hidden=hidden)
        path = "k_eval_layer" if t.fused_mode() == 3 else "k_eval"
        for n in (1, 256, 1000, 2500):
            batch, eps = make_batch(rs, n)
            diff = largest_difference(t.evaluate(batch, eps=eps, stats="device", **kw), t.evaluate(batch, eps=eps, **kw))
            d, h = alternating_windows([lambda: t.evaluate(batch, eps=eps, stats="device", **kw),
                                        lambda: t.evaluate(batch, eps=eps, **kw)], args.windows, args.window_s)
            emit(dict(what=f"a: SACTrainer.evaluate(stats='device'), {path}, per call", hidden=list(hidden), n=n,
                      max_rel_diff_to_host_stats=diff, **d), args.out)
            emit(dict(what=f"a: SACTrainer.evaluate(stats='host') of the same trainer, {path}, per call", hidden=list(hidden),
                      n=n, **h), args.out)
        ts = [make_trainer(10 + i, hidden=hidden) for i in range(16)]
        made = [make_batch(rs, 64) for _ in ts]
        batches, eps_l = [m[0] for m in made], [m[1] for m in made]
        d, h = alternating_windows([lambda: evaluate_many(ts, batches, eps=eps_l, stats="device", **kw),
                                    lambda: evaluate_many(ts, batches, eps=eps_l, **kw)], args.windows, args.window_s)
        emit(dict(what=f"b: group.evaluate_many(stats='device'), {path}, 16 Lift members x 64 rows, per call",
                  hidden=list(hidden), n=64, **d), args.out)
        emit(dict(what=f"b: group.evaluate_many(stats='host') of the same members, {path}, per call", hidden=list(hidden),
                  n=64, **h), args.out)
        del t, ts


if __name__ == "__main__":
    main()
