"""Aggregate grad-steps/s of trainer groups (sac_group_train_loop): R SAC (or TD3) runs of Lift (obs 42, act 7) at batch
256 and 128, each with its own 1e6-slot replay buffer, stepped together with grouped launches.  One JSON line per
(batch, R).

    python scripts/bench_group.py [--agent SAC|TD3] [--steps 2000] [--warmup 200] [--batches 256 128]
                                  [--replicas 1 2 4 8 16]

--tasks sweep: the eight tasks of parallel.SWEEP (SAC), --seeds-per-task k runs of each, as ONE mixed trainer group
(MixedSACTrainerGroup) against the same runs trained one after another with solo train_loop.  One JSON line per
(batch, seeds per task): both aggregate rates, every task's solo rate and the step launches per step.

    python scripts/bench_group.py --tasks sweep [--batches 256 128] [--seeds-per-task 1 2] [--buffer 1000000]

--hidden H1 H2 ...: every run's policy and Q nets get these hidden sizes; other than two layers of at most 256 units
they run the general step, and the runs form ONE MLP group (MlpSACTrainerGroup / MlpTD3TrainerGroup), measured against
the same runs trained one after another with solo train_loop (the two alternate per (batch, R)).  One JSON line per
(batch, R) with both aggregate rates.

    python scripts/bench_group.py --hidden 512 512 [--agent SAC|TD3] [--batches 256 128] [--replicas 1 2 4 8 16]

--hidden-sweep H1 H2 ...: a network-size sweep, --seeds-per-arch k runs of every entry (comma-separated widths, e.g.
256,256 512,512 256,256,256 1024; policy and Q nets alike) in three layouts: ONE arch group (ArchSACTrainerGroup /
ArchTD3TrainerGroup), one group per architecture (an MLP group for the general step, a mixed group for the fused
shapes) run one after another, and solo train_loop runs one after another.  The layouts alternate --rounds times; one
JSON line per batch with each layout's best aggregate rate and every round's.

    python scripts/bench_group.py --hidden-sweep 256,256 512,512 256,256,256 1024 [--seeds-per-arch 2] [--rounds 2]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from robosuite_benchmark_amd import (ArchSACTrainerGroup, ArchTD3TrainerGroup, EnvReplayBuffer, FlattenMlp,  # noqa: E402
                                     MixedSACTrainerGroup, MixedTD3TrainerGroup, MlpSACTrainerGroup, MlpTD3TrainerGroup, SACTrainer, SACTrainerGroup, TanhGaussianPolicy, TanhMlpPolicy,
                                     TD3Trainer, TD3TrainerGroup, _lib)
from robosuite_benchmark_amd.group import runs_general_step  # noqa: E402
from robosuite_benchmark_amd.parallel import SWEEP  # noqa: E402
from robosuite_benchmark_amd.variant import parse_hidden_sizes  # noqa: E402


def make_trainer(O, A, B, seed, hidden=(256, 256)):
    rs = np.random.RandomState(seed)
    qs = [FlattenMlp(list(hidden), 1, O + A, rs=rs) for _ in range(4)]
    pol = TanhGaussianPolicy(list(hidden), O, A, rs=rs, noise=np.random.RandomState(seed))
    return SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], discount=0.99,
                      reward_scale=1.0, policy_lr=3e-4, qf_lr=3e-4, soft_target_tau=0.005, target_update_period=1,
                      use_automatic_entropy_tuning=True, batch_size=B, noise_seed=seed)


def make_td3_trainer(O, A, B, seed, hidden=(256, 256)):
    """TD3 with the default variant's trainer_kwargs (bench.py --agent TD3's: policy_and_target_update_period 2)."""
    rs = np.random.RandomState(seed)
    qs = [FlattenMlp(list(hidden), 1, O + A, rs=rs) for _ in range(4)]
    pols = [TanhMlpPolicy(list(hidden), A, O, rs=rs) for _ in range(2)]
    return TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1],
                      target_policy_noise=0.2, discount=0.99, reward_scale=1.0, policy_learning_rate=1e-3,
                      qf_learning_rate=5e-4, policy_and_target_update_period=2, tau=0.005, batch_size=B, noise_seed=seed)


def variant_class(O, A):
    """The kernel variant a SAC trainer's step runs: head tiles (2A outputs in 16-wide tiles) and a first layer wider than
    eight 16-column chunks (the Q input [obs | pad | act | pad] of round_up(O, 16) + 16 columns)."""
    return (-(-2 * A // 16), -(-O // 16) * 16 + 16 >= 129)


def bench_sweep(args):
    N = args.buffer
    gen = np.random.default_rng(1)
    for k in args.seeds_per_task:
        runs = [(task, O, A, s) for task, O, A in SWEEP for s in range(k)]
        bufs = []
        for i, (task, O, A, s) in enumerate(runs):
            b = EnvReplayBuffer(N, obs_dim=O, action_dim=A)
            b.add_block(gen.standard_normal((N, O), dtype=np.float32) * 0.5,
                        gen.uniform(-1, 1, (N, A)).astype(np.float32), gen.uniform(0, 1, (N, 1)).astype(np.float32),
                        gen.standard_normal((N, O), dtype=np.float32) * 0.5, np.zeros((N, 1), np.uint8))
            b.seed(100 + i)
            bufs.append(b)
        for B in args.batches:
            trainers = [make_trainer(O, A, B, 10 + i) for i, (task, O, A, s) in enumerate(runs)]
            group = MixedSACTrainerGroup(trainers)
            group.train_loop(bufs, args.warmup)
            t0 = time.perf_counter()
            _, last = group.train_loop(bufs, args.steps)
            dt_group = time.perf_counter() - t0
            solo, dt_seq = {}, 0.0
            for (task, O, A, s), t, b in zip(runs, trainers, bufs):
                t.train_loop(b, args.warmup, batch_size=B)
                t0 = time.perf_counter()
                t.train_loop(b, args.steps, batch_size=B)
                dt = time.perf_counter() - t0
                dt_seq += dt
                solo.setdefault(task, []).append(round(args.steps / dt, 1))
            n_cls = len({variant_class(O, A) for _, O, A, _ in runs})
            print(json.dumps(dict(metric="mixed_group_sweep_grad_steps_per_s", batch=B, seeds_per_task=k, runs=len(runs),
                                  buffer=N, steps=args.steps, group_seconds=round(dt_group, 4),
                                  group_aggregate_steps_per_s=round(len(runs) * args.steps / dt_group, 1),
                                  sequential_seconds=round(dt_seq, 4),
                                  sequential_aggregate_steps_per_s=round(len(runs) * args.steps / dt_seq, 1),
                                  gain=round(dt_seq / dt_group, 3), solo_steps_per_s=solo, variant_classes=n_cls,
                                  step_launches_per_step=3 * n_cls + 1,
                                  finite=bool(np.all(np.isfinite(last))))), flush=True)
            del group, trainers
        del bufs


def bench_hidden(args, bufs):
    """--hidden: R runs of these hidden sizes as one group (an MLP group for the general step) against the same runs
    trained one after another with solo train_loop."""
    O, A, hidden = args.obs, args.act, tuple(args.hidden)
    td3 = args.agent == "TD3"
    make = make_td3_trainer if td3 else make_trainer
    for B in args.batches:
        for R in args.replicas:
            trainers = [make(O, A, B, 10 + r, hidden) for r in range(R)]
            general = runs_general_step(trainers[0])
            if general:
                group = (MlpTD3TrainerGroup if td3 else MlpSACTrainerGroup)(trainers)
                run = lambda n: group.train_loop(bufs[:R], n, batch_sizes=[B] * R)  # noqa: E731
            else:
                group = (TD3TrainerGroup if td3 else SACTrainerGroup)(trainers)
                run = lambda n: group.train_loop(bufs[:R], n, batch_size=B)  # noqa: E731
            run(args.warmup)
            t0 = time.perf_counter()
            _, last = run(args.steps)
            dt_group = time.perf_counter() - t0
            dt_seq, solo = 0.0, []
            for t, b in zip(trainers, bufs[:R]):
                t.train_loop(b, args.warmup, batch_size=B)
                t0 = time.perf_counter()
                t.train_loop(b, args.steps, batch_size=B)
                dt = time.perf_counter() - t0
                dt_seq += dt
                solo.append(round(args.steps / dt, 1))
            print(json.dumps(dict(metric="mlp_group_grad_steps_per_s" if general else "group_grad_steps_per_s",
                                  agent=args.agent, hidden=list(hidden), batch=B, replicas=R, obs_dim=O, act_dim=A,
                                  buffer=args.buffer, steps=args.steps,
                                  group_seconds=round(dt_group, 4),
                                  group_aggregate_steps_per_s=round(R * args.steps / dt_group, 1),
                                  sequential_seconds=round(dt_seq, 4),
                                  sequential_aggregate_steps_per_s=round(R * args.steps / dt_seq, 1),
                                  gain=round(dt_seq / dt_group, 3), solo_steps_per_s=solo,
                                  finite=bool(np.all(np.isfinite(last))))), flush=True)
            del group, trainers


def bench_hidden_sweep(args, bufs):
    """--hidden-sweep: k runs of every architecture as one arch group, as one group per architecture one after another,
    and as solo train_loop runs one after another (the three alternate, --rounds times)."""
    O, A = args.obs, args.act
    td3 = args.agent == "TD3"
    make = make_td3_trainer if td3 else make_trainer
    archs = [tuple(parse_hidden_sizes(h)) for h in args.hidden_sweep]
    k = args.seeds_per_arch
    runs = [(h, s) for h in archs for s in range(k)]
    R = len(runs)
    if R > 16 or R > len(bufs):
        raise SystemExit(f"{R} runs: an arch group holds at most 16")
    for B in args.batches:
        trainers = [make(O, A, B, 10 + i, h) for i, (h, _) in enumerate(runs)]
        arch = (ArchTD3TrainerGroup if td3 else ArchSACTrainerGroup)(trainers)
        per_arch = []                                       # (member indices, group) per architecture
        for h in archs:
            idx = [i for i, (hh, _) in enumerate(runs) if hh == h]
            ts = [trainers[i] for i in idx]
            kind = ((MlpTD3TrainerGroup if td3 else MlpSACTrainerGroup) if runs_general_step(ts[0])
                    else (MixedTD3TrainerGroup if td3 else MixedSACTrainerGroup))
            per_arch.append((idx, kind(ts)))
        layouts = {
            "arch_group": lambda n: arch.train_loop(bufs[:R], n, batch_sizes=[B] * R),
            "per_arch_groups": lambda n: [g.train_loop([bufs[i] for i in idx], n, batch_sizes=[B] * len(idx))
                                          for idx, g in per_arch],
            "solo": lambda n: [t.train_loop(b, n, batch_size=B) for t, b in zip(trainers, bufs[:R])],
        }
        for run in layouts.values():
            run(args.warmup)
        rates = {name: [] for name in layouts}
        for _ in range(args.rounds):
            for name, run in layouts.items():
                t0 = time.perf_counter()
                out = run(args.steps)
                rates[name].append(round(R * args.steps / (time.perf_counter() - t0), 1))
                if name == "arch_group":
                    last = out[1]
        best = {name: max(v) for name, v in rates.items()}
        general = [sub for idx, sub in arch.subgroups if runs_general_step(trainers[idx[0]])]
        stages = general[0].stage_count() if general else None
        print(json.dumps(dict(metric="arch_group_grad_steps_per_s", agent=args.agent,
                              hidden_sweep=[list(h) for h in archs], seeds_per_arch=k, runs=R, batch=B, obs_dim=O,
                              act_dim=A, buffer=args.buffer, steps=args.steps, rounds=args.rounds,
                              arch_group_aggregate_steps_per_s=best["arch_group"],
                              per_arch_groups_aggregate_steps_per_s=best["per_arch_groups"],
                              solo_aggregate_steps_per_s=best["solo"],
                              gain_vs_per_arch_groups=round(best["arch_group"] / best["per_arch_groups"], 3),
                              gain_vs_solo=round(best["arch_group"] / best["solo"], 3),
                              per_round=rates, arch_group_general_stages=stages,
                              per_arch_general_stages=[g.stage_count() for idx, g in per_arch
                                                       if runs_general_step(trainers[idx[0]])],
                              finite=bool(np.all(np.isfinite(last))))), flush=True)
        del arch, per_arch, trainers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=str, default="lift", choices=["lift", "sweep"])
    ap.add_argument("--seeds-per-task", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--agent", type=str, default="SAC", choices=["SAC", "TD3"])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--buffer", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--obs", type=int, default=42)
    ap.add_argument("--act", type=int, default=7)
    ap.add_argument("--hidden", type=int, nargs="+", default=None)
    ap.add_argument("--hidden-sweep", type=str, nargs="+", default=None)
    ap.add_argument("--seeds-per-arch", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if _lib.device_count() == 0:
        raise SystemExit("bench_group.py needs a GPU")
    if args.tasks == "sweep":
        return bench_sweep(args)
    O, A, N = args.obs, args.act, args.buffer
    rs = np.random.RandomState(1)
    rows = (rs.normal(0, 0.5, (N, O)).astype(np.float32), rs.uniform(-1, 1, (N, A)).astype(np.float32),
            rs.uniform(0, 1, (N, 1)).astype(np.float32), rs.normal(0, 0.5, (N, O)).astype(np.float32),
            np.zeros((N, 1), np.uint8))
    bufs = []
    n_bufs = len(args.hidden_sweep) * args.seeds_per_arch if args.hidden_sweep else max(args.replicas)
    for r in range(n_bufs):
        b = EnvReplayBuffer(N, obs_dim=O, action_dim=A)
        b.add_block(rows[0], rows[1], rows[2], rows[3], rows[4])
        b.seed(100 + r)
        bufs.append(b)
    if args.hidden_sweep:
        return bench_hidden_sweep(args, bufs)
    if args.hidden:
        return bench_hidden(args, bufs)
    for B in args.batches:
        for R in args.replicas:
            make, Group = (make_td3_trainer, TD3TrainerGroup) if args.agent == "TD3" else (make_trainer, SACTrainerGroup)
            trainers = [make(O, A, B, 10 + r) for r in range(R)]
            group = Group(trainers)
            group.train_loop(bufs[:R], args.warmup, batch_size=B)
            t0 = time.perf_counter()
            _, last = group.train_loop(bufs[:R], args.steps, batch_size=B)
            dt = time.perf_counter() - t0
            print(json.dumps(dict(metric="group_grad_steps_per_s", batch=B, replicas=R, obs_dim=O, act_dim=A,
                                  buffer=N, steps=args.steps, seconds=round(dt, 4),
                                  aggregate_steps_per_s=round(R * args.steps / dt, 1),
                                  per_run_steps_per_s=round(args.steps / dt, 1),
                                  fused_members=int(sum(t.is_fused() for t in trainers)),
                                  finite=bool(np.all(np.isfinite(last))))), flush=True)
            del group, trainers


if __name__ == "__main__":
    main()
