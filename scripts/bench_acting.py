"""Acting: the host path (sac_policy_act, one observation per call) against the device path (k_act through
sac_policy_act_device / sac_policy_act_many), and what the lockstep collection of a 16-seed group epoch gains from it.
One JSON line per measurement, appended to --out (default: stdout only).

    python scripts/bench_acting.py [--windows 3] [--window-s 1.0] [--seeds 16] [--rounds 2] [--out FILE]
    python scripts/bench_acting.py --profile-pass       # a short run of the device calls alone, for a kernel trace
    python scripts/bench_acting.py --sessions [--out FILE]      # acting sessions (GroupActor) beside the calls above
    python scripts/bench_acting.py --profile-pass-sessions      # k_act and k_act_session side by side, for a kernel trace
    python scripts/bench_acting.py --general [--out FILE]       # general-step acting: host forward against k_act_layer
    python scripts/bench_acting.py --profile-pass-general       # a short run of the general-step device calls, for a kernel trace
    python scripts/bench_acting.py --general-sessions [--out FILE]      # general-step acting sessions beside the per-tick calls

Every timed call returns with its actions on the host (the calls end synchronised), so a host clock around a window of
calls measures them; a window lasts at least --window-s seconds after a warm-up, and each figure is the median over
--windows windows with the smallest and the largest next to it.  --sessions measures, in ONE process, (c) again, (c')
the same tick through a GroupActor -- 16 observations and 16 eps rows written into the views, 16 action rows copied out
-- (c'') the bare sac_actor_act call, (b) and (b') a one-member session at n = 1, 16, 256, 1000, and (d') the sampling
phases of the group epoch with sessions=True and sessions=False alternating.  (d) runs experiment_group with --seeds seeds of the
default Lift variant for one epoch at its default step counts, acting="host" and acting="device" alternating --rounds
times, and reports each mode's evaluation + exploration seconds of that epoch.  --general-sessions measures, in ONE
process and with the two paths' windows alternating, (g) the tick of 16 [512,512] members x 1 row through
GroupActor(general="device", general_sessions=False), (g') the same tick with general_sessions=True, (g'') the bare
sac_gactor_act call, one member at n = 1, 16, 1000 on both paths, and the sampling phases of a 16-seed [512,512]
experiment_group epoch with acting="device_all", general_sessions on and off alternating."""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy  # noqa: E402
from robosuite_benchmark_amd.group import act_many  # noqa: E402

O, A = 42, 7                                        # Lift


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
            for _ in range(20):
                fn()
            n += 20
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


def call_benches(args):
    rs = np.random.RandomState(0)
    t = make_trainer(1)
    obs1, eps1 = rs.normal(0, 0.5, (1, O)).astype(np.float32), rs.normal(size=(1, A)).astype(np.float32)
    emit(dict(what="a: sac_policy_act, host, per row", **windows(lambda: t.policy_act(obs1, False, eps1),
                                                                args.windows, args.window_s)), args.out)
    for n in (1, 16, 256, 1000):
        obs, eps = rs.normal(0, 0.5, (n, O)).astype(np.float32), rs.normal(size=(n, A)).astype(np.float32)
        emit(dict(what="b: sac_policy_act_device, per call", n=n,
                  **windows(lambda: t.policy_act_device(obs, False, eps), args.windows, args.window_s)), args.out)
    ts = [make_trainer(10 + i) for i in range(16)]
    obs_l, eps_l = [obs1.copy() for _ in ts], [eps1.copy() for _ in ts]
    det = [False] * 16
    emit(dict(what="c: sac_policy_act_many, 16 Lift members x 1 row, per call (group.act_many)",
              **windows(lambda: act_many(ts, obs_l, det, eps_l), args.windows, args.window_s)), args.out)


def epoch_bench(args):
    from robosuite_benchmark_amd.driver import experiment_group
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=1, batch_size=256)
    v["replay_buffer_size"] = 100000                  # (one epoch never fills it; 16 full-size buffers only cost set-up time)
    seeds = list(range(1, args.seeds + 1))
    res = {"host": [], "device": []}
    for rnd in range(args.rounds):
        for mode in ("host", "device"):
            rows = experiment_group(copy.deepcopy(v), seeds, num_epochs=1, quiet=True, acting=mode)
            ev = [rows[s][0]["time/evaluation sampling (s)"] for s in seeds]
            ex = [rows[s][0]["time/exploration sampling (s)"] for s in seeds]
            # host: the runs collect one after another (the sum over runs); device: one shared phase (any run's column)
            sampling = sum(ev) + sum(ex) if mode == "host" else ev[0] + ex[0]
            res[mode].append(dict(sampling_s=sampling, training_s=rows[seeds[0]][0]["time/training (s)"]))
    ak = v["algorithm_kwargs"]
    emit(dict(what="d: evaluation + exploration seconds of one experiment_group epoch", seeds=args.seeds,
              eval_steps=ak["num_eval_steps_per_epoch"], expl_steps=ak["num_expl_steps_per_train_loop"],
              trains=ak["num_trains_per_train_loop"], rounds=args.rounds,
              host_sampling_s=[r["sampling_s"] for r in res["host"]], device_sampling_s=[r["sampling_s"] for r in res["device"]],
              host_training_s=[r["training_s"] for r in res["host"]], device_training_s=[r["training_s"] for r in res["device"]],
              host_over_device=float(np.median([r["sampling_s"] for r in res["host"]])
                                     / np.median([r["sampling_s"] for r in res["device"]]))), args.out)


def session_benches(args):
    from robosuite_benchmark_amd import GroupActor, _lib
    rs = np.random.RandomState(0)
    ts = [make_trainer(10 + i) for i in range(16)]
    obs64 = [rs.normal(0, 0.5, O) for _ in ts]                        # what an env hands out: float64 rows
    draws = [rs.normal(size=(1, A)) for _ in ts]
    obs_l, eps_l = [o.astype(np.float32)[None] for o in obs64], [e.astype(np.float32) for e in draws]
    det, ones = [False] * 16, [1] * 16
    emit(dict(what="c: sac_policy_act_many, 16 Lift members x 1 row, per call (group.act_many)",
              **windows(lambda: act_many(ts, obs_l, det, eps_l), args.windows, args.window_s)), args.out)
    g = GroupActor(ts, max_rows=1)

    def tick():
        for k in range(16):
            g.obs[k][0] = obs64[k]
            g.eps[k][0] = draws[k][0]
        g.act(ones, det)
        return [g.act[k][0].copy() for k in range(16)]
    emit(dict(what="c': GroupActor tick, 16 Lift members x 1 row: 16 obs + 16 eps rows in, act, 16 action rows out",
              **windows(tick, args.windows, args.window_s)), args.out)
    sess = g._sessions[0]
    sess.n_rows[:], sess.det[:] = ones, [0] * 16
    lib = _lib.load()
    emit(dict(what="c'': sac_actor_act alone, 16 Lift members x 1 row",
              **windows(lambda: lib.sac_actor_act(sess.a, sess.n_rows, sess.det), args.windows, args.window_s)), args.out)
    g.close()
    t = ts[0]
    g1 = GroupActor([t], max_rows=1000)
    for n in (1, 16, 256, 1000):
        o64, e = rs.normal(0, 0.5, (n, O)), rs.normal(size=(n, A)).astype(np.float32)
        o32 = o64.astype(np.float32)
        emit(dict(what="b: sac_policy_act_device, per call", n=n,
                  **windows(lambda: t.policy_act_device(o32, False, e), args.windows, args.window_s)), args.out)

        def tick1():
            g1.obs[0][:n] = o64
            g1.eps[0][:n] = e
            g1.act([n], False)
            return g1.act[0][:n].copy()
        emit(dict(what="b': one-member GroupActor tick (rows in, act, rows out)", n=n,
                  **windows(tick1, args.windows, args.window_s)), args.out)
    g1.close()


def session_epoch_bench(args):
    import robosuite_benchmark_amd.driver as drv
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=1, batch_size=256)
    v["replay_buffer_size"] = 100000
    seeds = list(range(1, args.seeds + 1))
    res = {True: [], False: []}
    for rnd in range(args.rounds):
        for flag in (True, False):
            rows = drv.experiment_group(copy.deepcopy(v), seeds, num_epochs=1, quiet=True, acting="device", sessions=flag)
            r0 = rows[seeds[0]][0]
            res[flag].append(dict(sampling_s=r0["time/evaluation sampling (s)"] + r0["time/exploration sampling (s)"],
                                  training_s=r0["time/training (s)"]))
    ak = v["algorithm_kwargs"]
    on, off = [r["sampling_s"] for r in res[True]], [r["sampling_s"] for r in res[False]]
    emit(dict(what="d': evaluation + exploration seconds of one experiment_group epoch, acting=device, sessions on / off",
              seeds=args.seeds, eval_steps=ak["num_eval_steps_per_epoch"], expl_steps=ak["num_expl_steps_per_train_loop"],
              rounds=args.rounds, sessions_sampling_s=on, act_many_sampling_s=off,
              sessions_training_s=[r["training_s"] for r in res[True]], act_many_training_s=[r["training_s"] for r in res[False]],
              act_many_over_sessions=float(np.median(off) / np.median(on))), args.out)


def profile_pass_sessions():
    """k_act and k_act_session on the same inputs, 200 launches each: 16 members x 1 row, and one member x 1000 rows."""
    from robosuite_benchmark_amd import GroupActor
    rs = np.random.RandomState(0)
    ts = [make_trainer(10 + i) for i in range(16)]
    obs_l = [rs.normal(0, 0.5, (1, O)).astype(np.float32) for _ in ts]
    eps_l = [rs.normal(size=(1, A)).astype(np.float32) for _ in ts]
    g = GroupActor(ts, max_rows=1)
    for k in range(16):
        g.obs[k][...], g.eps[k][...] = obs_l[k], eps_l[k]
    obs, eps = rs.normal(0, 0.5, (1000, O)).astype(np.float32), rs.normal(size=(1000, A)).astype(np.float32)
    g1 = GroupActor([ts[0]], max_rows=1000)
    g1.obs[0][...], g1.eps[0][...] = obs, eps
    for _ in range(4):                                                # interleaved blocks of 50: neither kernel runs "later"
        for _ in range(50):
            act_many(ts, obs_l, [False] * 16, eps_l)
        for _ in range(50):
            g.act([1] * 16, False)
        for _ in range(50):
            ts[0].policy_act_device(obs, False, eps)
        for _ in range(50):
            g1.act([1000], False)
    g.close()
    g1.close()
    print("profile pass: 200 launches each of k_act and k_act_session at 16 x 1 row (16 workgroups) and 1 x 1000 rows (63)",
          flush=True)


def profile_pass():
    rs = np.random.RandomState(0)
    ts = [make_trainer(10 + i) for i in range(16)]
    for n in (1, 16, 256, 1000):
        obs, eps = rs.normal(0, 0.5, (n, O)).astype(np.float32), rs.normal(size=(n, A)).astype(np.float32)
        for _ in range(200):
            ts[0].policy_act_device(obs, False, eps)
    obs_l = [rs.normal(0, 0.5, (1, O)).astype(np.float32) for _ in ts]
    eps_l = [rs.normal(size=(1, A)).astype(np.float32) for _ in ts]
    for _ in range(200):
        act_many(ts, obs_l, [False] * 16, eps_l)
    print("profile pass: 4 x 200 solo calls (n = 1, 16, 256, 1000), 200 grouped calls of 16 x 1 row", flush=True)


GENERAL_SHAPES = ((512, 512), (256, 256, 256), (1024, 1024))


def general_benches(args):
    """(a) the host forward, one row; (b) policy_act_general at n = 1, 16, 256, 1000; (c) a 16-member GroupActor tick with
    the general-step members on the host and on the device."""
    from robosuite_benchmark_amd import GroupActor
    rs = np.random.RandomState(0)
    obs1, eps1 = rs.normal(0, 0.5, (1, O)).astype(np.float32), rs.normal(size=(1, A)).astype(np.float32)
    for hidden in GENERAL_SHAPES:
        t = make_trainer(1, hidden=hidden)
        emit(dict(what="a: sac_policy_act, host, per row", hidden=list(hidden),
                  **windows(lambda: t.policy_act(obs1, False, eps1), args.windows, args.window_s)), args.out)
        for n in (1, 16, 256, 1000):
            obs, eps = rs.normal(0, 0.5, (n, O)).astype(np.float32), rs.normal(size=(n, A)).astype(np.float32)
            emit(dict(what="b: sac_policy_act_general, per call", hidden=list(hidden), n=n,
                      **windows(lambda: t.policy_act_general(obs, False, eps), args.windows, args.window_s)), args.out)
        del t
    ts = [make_trainer(10 + i, hidden=(512, 512)) for i in range(16)]
    obs64, draws = [rs.normal(0, 0.5, O) for _ in ts], [rs.normal(size=(1, A)) for _ in ts]
    det, ones = [False] * 16, [1] * 16
    for general in ("host", "device"):
        g = GroupActor(ts, max_rows=1, general=general, general_sessions=False)      # (sessions: --general-sessions)

        def tick():
            for k in range(16):
                g.obs[k][0] = obs64[k]
                g.eps[k][0] = draws[k][0]
            g.act(ones, det)
            return [g.act[k][0].copy() for k in range(16)]
        emit(dict(what=f"c: GroupActor(general={general!r}) tick, 16 members [512,512] x 1 row: rows in, act, rows out",
                  **windows(tick, args.windows, args.window_s)), args.out)
        g.close()


def general_epoch_bench(args):
    """(d) the evaluation + exploration phases of one experiment_sweep(hidden_sweep=True) epoch over a width sweep,
    acting="device" (the wide members act on the host inside the lockstep ticks) against "device_all", alternating."""
    from robosuite_benchmark_amd.driver import experiment_sweep
    from robosuite_benchmark_amd.variant import default_variant
    widths = [(256, 256), (512, 512), (1024, 1024), (256, 256, 256)]
    runs = []
    for i in range(args.seeds):
        v = default_variant(env="Lift", seed=1 + i, batch_size=256)
        v["replay_buffer_size"] = 100000
        v["policy_kwargs"]["hidden_sizes"] = list(widths[i % len(widths)])
        v["qf_kwargs"]["hidden_sizes"] = list(widths[i % len(widths)])
        if args.epoch_trains:
            v["algorithm_kwargs"]["num_trains_per_train_loop"] = args.epoch_trains
        runs.append((v, 1 + i))
    res = {"device": [], "device_all": []}
    for rnd in range(args.rounds):
        for mode in ("device", "device_all"):
            rows = experiment_sweep(copy.deepcopy(runs), num_epochs=1, quiet=True, hidden_sweep=True, acting=mode)
            r0 = rows[0][0]
            res[mode].append(dict(sampling_s=r0["time/evaluation sampling (s)"] + r0["time/exploration sampling (s)"],
                                  training_s=r0["time/training (s)"]))
    ak = runs[0][0]["algorithm_kwargs"]
    dev, dall = [r["sampling_s"] for r in res["device"]], [r["sampling_s"] for r in res["device_all"]]
    emit(dict(what="d: evaluation + exploration seconds of one experiment_sweep(hidden_sweep=True) epoch, acting=device / device_all",
              members=args.seeds, hidden=[list(widths[i % len(widths)]) for i in range(args.seeds)],
              eval_steps=ak["num_eval_steps_per_epoch"], expl_steps=ak["num_expl_steps_per_train_loop"],
              trains=ak["num_trains_per_train_loop"], rounds=args.rounds, device_sampling_s=dev, device_all_sampling_s=dall,
              device_training_s=[r["training_s"] for r in res["device"]],
              device_all_training_s=[r["training_s"] for r in res["device_all"]],
              device_over_device_all=float(np.median(dev) / np.median(dall))), args.out)


def alternating_windows(fns, n_windows, window_s, warm_s=0.2):
    """windows() for several callables measured in turn: window w of every one, then window w + 1 of every one, so that
    none of them runs "later" than the others.  Returns {name: the figures of windows()}."""
    for fn in fns.values():
        t_end = time.perf_counter() + warm_s
        while time.perf_counter() < t_end:
            fn()
    per = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, fn in fns.items():
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(20):
                    fn()
                n += 20
                dt = time.perf_counter() - t0
                if dt >= window_s:
                    break
            per[k].append(1e6 * dt / n)
    return {k: dict(us_median=float(np.median(v)), us_min=float(min(v)), us_max=float(max(v)), windows=n_windows)
            for k, v in per.items()}


def general_session_benches(args):
    """(g), (g'), (g'') and the one-member rows: GroupActor(general="device") with general_sessions off and on."""
    from robosuite_benchmark_amd import GroupActor, _lib
    rs = np.random.RandomState(0)
    hidden = (512, 512)
    ts = [make_trainer(10 + i, hidden=hidden) for i in range(16)]
    obs64, draws = [rs.normal(0, 0.5, O) for _ in ts], [rs.normal(size=(1, A)) for _ in ts]
    det, ones = [False] * 16, [1] * 16
    gs = {flag: GroupActor(ts, max_rows=1, general="device", general_sessions=flag) for flag in (False, True)}

    def tick_of(g):
        def tick():
            for k in range(16):
                g.obs[k][0] = obs64[k]
                g.eps[k][0] = draws[k][0]
            g.act(ones, det)
            return [g.act[k][0].copy() for k in range(16)]
        return tick
    sess = gs[True]._sessions[0]
    lib = _lib.load()

    def bare():
        sess.n_rows[:], sess.det[:] = ones, [0] * 16
        return lambda: lib.sac_gactor_act(sess.a, sess.n_rows, sess.det)
    a, b = tick_of(gs[False])(), tick_of(gs[True])()
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)), "the two paths disagree"
    res = alternating_windows({"g": tick_of(gs[False]), "g'": tick_of(gs[True]), "g''": bare()}, args.windows, args.window_s)
    what = {"g": "g: GroupActor(general='device', general_sessions=False) tick, 16 members [512,512] x 1 row: rows in, act, rows out",
            "g'": "g': the same tick with general_sessions=True",
            "g''": "g'': sac_gactor_act alone, 16 members [512,512] x 1 row"}
    for k, r in res.items():
        emit(dict(what=what[k], hidden=list(hidden), **r), args.out)
    for g in gs.values():
        g.close()
    t = ts[0]
    g1 = {flag: GroupActor([t], max_rows=1000, general="device", general_sessions=flag) for flag in (False, True)}
    for n in (1, 16, 1000):
        o64, e = rs.normal(0, 0.5, (n, O)), rs.normal(size=(n, A)).astype(np.float32)

        def tick1_of(g):
            def tick1():
                g.obs[0][:n] = o64
                g.eps[0][:n] = e
                g.act([n], False)
                return g.act[0][:n].copy()
            return tick1
        res = alternating_windows({False: tick1_of(g1[False]), True: tick1_of(g1[True])}, args.windows, args.window_s)
        for flag, r in res.items():
            emit(dict(what=f"one-member GroupActor(general='device', general_sessions={flag}) tick (rows in, act, rows out)",
                      hidden=list(hidden), n=n, **r), args.out)
    for g in g1.values():
        g.close()


def general_session_epoch_bench(args):
    """The evaluation + exploration phases of one 16-seed [512,512] experiment_group epoch, acting="device_all", general
    sessions on and off alternating."""
    import robosuite_benchmark_amd.driver as drv
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=1, batch_size=256)
    v["replay_buffer_size"] = 100000
    v["policy_kwargs"]["hidden_sizes"] = [512, 512]
    v["qf_kwargs"]["hidden_sizes"] = [512, 512]
    if args.epoch_trains:
        v["algorithm_kwargs"]["num_trains_per_train_loop"] = args.epoch_trains
    seeds = list(range(1, args.seeds + 1))
    res = {True: [], False: []}
    for rnd in range(args.rounds):
        for flag in (True, False):
            rows = drv.experiment_group(copy.deepcopy(v), seeds, num_epochs=1, quiet=True, acting="device_all", sessions=True,
                                        general_sessions=flag)
            r0 = rows[seeds[0]][0]
            res[flag].append(dict(sampling_s=r0["time/evaluation sampling (s)"] + r0["time/exploration sampling (s)"],
                                  training_s=r0["time/training (s)"]))
    ak = v["algorithm_kwargs"]
    on, off = [r["sampling_s"] for r in res[True]], [r["sampling_s"] for r in res[False]]
    emit(dict(what="evaluation + exploration seconds of one [512,512] experiment_group epoch, acting=device_all, general "
                   "sessions on / off", seeds=args.seeds, eval_steps=ak["num_eval_steps_per_epoch"],
              expl_steps=ak["num_expl_steps_per_train_loop"], trains=ak["num_trains_per_train_loop"], rounds=args.rounds,
              general_sessions_sampling_s=on, general_many_sampling_s=off,
              general_sessions_training_s=[r["training_s"] for r in res[True]],
              general_many_training_s=[r["training_s"] for r in res[False]],
              sessions_below_in_every_round=bool(all(a < b for a, b in zip(on, off))),
              general_many_over_sessions=float(np.median(off) / np.median(on))), args.out)


def profile_pass_general():
    """k_act_layer alone: 200 calls per shape and row count, then 200 grouped calls of 16 x 1 row."""
    rs = np.random.RandomState(0)
    for hidden in GENERAL_SHAPES:
        t = make_trainer(1, hidden=hidden)
        for n in (1, 1000):
            obs, eps = rs.normal(0, 0.5, (n, O)).astype(np.float32), rs.normal(size=(n, A)).astype(np.float32)
            for _ in range(200):
                t.policy_act_general(obs, False, eps)
        del t
    ts = [make_trainer(10 + i, hidden=(512, 512)) for i in range(16)]
    obs_l = [rs.normal(0, 0.5, (1, O)).astype(np.float32) for _ in ts]
    eps_l = [rs.normal(size=(1, A)).astype(np.float32) for _ in ts]
    for _ in range(200):
        act_many(ts, obs_l, [False] * 16, eps_l, general="device")
    print("profile pass: 200 solo calls per shape in", [list(h) for h in GENERAL_SHAPES], "at n = 1 and 1000 (one launch per "
          "layer), 200 grouped calls of 16 x [512,512] x 1 row", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--skip-epoch", action="store_true", help="only the per-call measurements (a) to (c)")
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--sessions", action="store_true", help="the acting-session rows (c), (c'), (c''), (b), (b') and (d')")
    ap.add_argument("--profile-pass-sessions", action="store_true")
    ap.add_argument("--general", action="store_true",
                    help="general-step acting: rows (a) to (d) for [512,512], [256,256,256] and [1024,1024] policies")
    ap.add_argument("--profile-pass-general", action="store_true")
    ap.add_argument("--general-sessions", action="store_true",
                    help="general-step acting sessions: rows (g), (g'), (g''), one member at n = 1, 16, 1000 and the epoch row")
    ap.add_argument("--epoch-trains", type=int, default=0,
                    help="with --general / --general-sessions: gradient steps of the measured epoch (0: the variant's; the sampling phases "
                         "that row (d) reports do not depend on it)")
    args = ap.parse_args()
    if args.profile_pass_general:
        profile_pass_general()
        sys.exit(0)
    if args.general_sessions:
        general_session_benches(args)
        if not args.skip_epoch:
            general_session_epoch_bench(args)
        sys.exit(0)
    if args.general:
        general_benches(args)
        if not args.skip_epoch:
            general_epoch_bench(args)
        sys.exit(0)
    if args.profile_pass_sessions:
        profile_pass_sessions()
        sys.exit(0)
    if args.sessions:
        session_benches(args)
        if not args.skip_epoch:
            session_epoch_bench(args)
        sys.exit(0)
    if args.profile_pass:
        profile_pass()
        sys.exit(0)
    call_benches(args)
    if not args.skip_epoch:
        epoch_bench(args)
