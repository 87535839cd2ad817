"""Evaluating the SAC objectives of GENERAL-STEP trainers on held-out rows: the device path (k_eval_layer through
sac_evaluate_general / sac_evaluate_general_many, evaluate(general="device")) against the host path of the SAME trainer --
sac_get_params of the five nets and a float32 NumPy forward, the default -- in ONE process.  One JSON line per
measurement, appended to --out (default: profiles/evaluate_general_bench.jsonl).

    python scripts/bench_evaluate_general.py [--windows 3] [--window-s 1.0] [--out FILE]

The method is scripts/bench_evaluate.py's: every timed call returns with its statistics on the host, a window lasts at
least --window-s seconds after a warm-up, the windows of the two paths ALTERNATE, and each figure is the median over
--windows windows with the smallest and the largest next to it.
(a) evaluate(general="device") and (b) the host path at 1, 256, 1000 and 2500 rows on Lift (42 / 7), for the hidden sizes
[512,512], [1024,1024] and [256,256,256]; (c) evaluate_many(general="device") over 16 [512,512] members at 64 rows each
and (d) the 16 host evaluations."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from robosuite_benchmark_amd.group import evaluate_many  # noqa: E402
from bench_evaluate import alternating_windows, emit, make_batch, make_trainer  # noqa: E402

SHAPES = [(512, 512), (1024, 1024), (256, 256, 256)]
ROWS = (1, 256, 1000, 2500)
COLUMNS = ("q1", "q2", "q1_new", "q2_new", "tq1", "tq2", "log_pi", "y")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "evaluate_general_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    for hidden in SHAPES:
        t = make_trainer(1, hidden=hidden)
        assert t.fused_mode() == 3, hidden
        for n in ROWS:
            batch, eps = make_batch(rs, n)
            dev, host = t.evaluate(batch, eps=eps, rows=True, general="device")[1], t.evaluate(batch, eps=eps, rows=True)[1]
            err = max(float(np.max(np.abs(dev[k] - host[k]))) for k in COLUMNS)
            d, h = alternating_windows([lambda: t.evaluate(batch, eps=eps, general="device"),
                                        lambda: t.evaluate(batch, eps=eps)], args.windows, args.window_s)
            emit(dict(what="a: SACTrainer.evaluate(general='device') (sac_evaluate_general), per call", hidden=list(hidden),
                      n=n, max_abs_diff_to_host=err, **d), args.out)
            emit(dict(what="b: the host path of the same trainer (sac_get_params of five nets + NumPy forward), per call",
                      hidden=list(hidden), n=n, **h), args.out)
    ts = [make_trainer(10 + i, hidden=(512, 512)) for i in range(16)]
    made = [make_batch(rs, 64) for _ in ts]
    batches, eps_l = [m[0] for m in made], [m[1] for m in made]
    d, h = alternating_windows([lambda: evaluate_many(ts, batches, eps=eps_l, general="device"),
                                lambda: evaluate_many(ts, batches, eps=eps_l)], args.windows, args.window_s)
    emit(dict(what="c: evaluate_many(general='device') (sac_evaluate_general_many), 16 [512,512] Lift members x 64 rows, "
                   "per call", hidden=[512, 512], n=64, **d), args.out)
    emit(dict(what="d: the same call at the default: 16 host evaluations (sac_get_params of five nets + NumPy forward "
                   "each), per call", hidden=[512, 512], n=64, **h), args.out)


if __name__ == "__main__":
    main()
