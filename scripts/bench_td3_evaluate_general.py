"""Evaluating the TD3 objectives of GENERAL-STEP trainers on held-out rows: the device path (k_eval_layer_td3 and
k_eval_layer through td3_evaluate_general / td3_evaluate_general_many, evaluate_td3(general="device")) against the host
path of the SAME trainer -- sac_get_params of the six nets and a float32 NumPy forward, the default -- in ONE process.
One JSON line per measurement, appended to --out (default: profiles/td3_evaluate_general_bench.jsonl).

    python scripts/bench_td3_evaluate_general.py [--windows 3] [--window-s 1.0] [--out FILE]

The method is scripts/bench_evaluate.py's: every timed call returns with its statistics on the host, a window lasts at
least --window-s seconds after a warm-up, the windows of the two paths ALTERNATE, and each figure is the median over
--windows windows with the smallest and the largest next to it.
(a) evaluate_td3(general="device") and (b) the host path at 1, 256, 1000 and 2500 rows on Lift (42 / 7), for the hidden
sizes [512,512], [1024,1024] and [256,256,256]; (c) td3_evaluate_many(general="device") over 16 [512,512] members at 64
rows each and (d) the 16 host evaluations."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from robosuite_benchmark_amd.group import td3_evaluate_many  # noqa: E402
from bench_evaluate import alternating_windows, emit  # noqa: E402
from bench_td3_evaluate import ROW_KEYS, make_batch, make_trainer  # noqa: E402

SHAPES = [(512, 512), (1024, 1024), (256, 256, 256)]
ROWS = (1, 256, 1000, 2500)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", dest="window_s", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "td3_evaluate_general_bench.jsonl"))
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    for hidden in SHAPES:
        t = make_trainer(1, hidden=hidden)
        assert t.fused_mode() == 3, hidden
        for n in ROWS:
            batch, eps = make_batch(rs, n)
            dev = t.evaluate_td3(batch, eps=eps, rows=True, general="device")[1]
            host = t.evaluate_td3(batch, eps=eps, rows=True)[1]
            err = max(float(np.max(np.abs(dev[k] - host[k]))) for k in ROW_KEYS)
            d, h = alternating_windows([lambda: t.evaluate_td3(batch, eps=eps, general="device"),
                                        lambda: t.evaluate_td3(batch, eps=eps)], args.windows, args.window_s)
            emit(dict(what="a: TD3Trainer.evaluate_td3(general='device') (td3_evaluate_general), per call", hidden=list(hidden),
                      n=n, max_abs_diff_to_host=err, **d), args.out)
            emit(dict(what="b: the host path of the same trainer (sac_get_params of six nets + NumPy forward), per call",
                      hidden=list(hidden), n=n, **h), args.out)
    ts = [make_trainer(10 + i, hidden=(512, 512)) for i in range(16)]
    made = [make_batch(rs, 64) for _ in ts]
    batches, eps_l = [m[0] for m in made], [m[1] for m in made]
    d, h = alternating_windows([lambda: td3_evaluate_many(ts, batches, eps=eps_l, general="device"),
                                lambda: td3_evaluate_many(ts, batches, eps=eps_l)], args.windows, args.window_s)
    emit(dict(what="c: td3_evaluate_many(general='device') (td3_evaluate_general_many), 16 [512,512] Lift members x 64 rows, "
                   "per call", hidden=[512, 512], n=64, **d), args.out)
    emit(dict(what="d: the same call at the default: 16 host evaluations (sac_get_params of six nets + NumPy forward "
                   "each), per call", hidden=[512, 512], n=64, **h), args.out)


if __name__ == "__main__":
    main()
