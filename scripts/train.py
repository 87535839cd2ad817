#!/usr/bin/env python3
"""Counterpart of the reference's scripts/train.py for the MI355X path:
    python scripts/train.py --variant <variant.json> --seed S --log_dir DIR [--epochs N]
    python scripts/train.py --variant <variant.json> --seeds S1 S2 ... --log_dir DIR [--epochs N] [--checkpoint]
    python scripts/train.py --variants A.json B.json ... --seeds S1 S2 ... --log_dir DIR [--epochs N] [--checkpoint]
    python scripts/train.py --variants A.json ... --hidden_sizes 256,256 512,512 256,256,256 --log_dir DIR [...]
(--seeds: one process trains every seed, the training blocks as one trainer group, SAC or TD3 (--agent);
 DIR/s<seed>/progress.csv each.  --variants: every (variant, seed) pair -- tasks of different dims and batch sizes --
 as one mixed trainer group; DIR/<task>-s<seed>/progress.csv each.  --checkpoint saves the whole group to
 DIR/checkpoint after every epoch; the same command line with --resume DIR instead of --log_dir DIR continues it.
 --hidden_sweep: the --variants may differ in their hidden sizes, one arch trainer group trains them all;
 DIR/<task>-h<sizes>-s<seed>/progress.csv each.  --hidden_sizes H1 H2 ...: every variant once per entry, policy and Q
 nets alike, implies --hidden_sweep.  --acting device: the policies act through the device kernel instead of the
 host forward; grouped runs then collect their paths in lockstep.  --acting device_all: the same, and runs of any
 hidden sizes act on the device.  --q_diagnostics: every epoch, Q1 and Q2 on the evaluation paths from the live
 weights against the discounted returns obtained there: sixteen evaluation/ columns more in progress.csv.
 --q_general device: with --q_diagnostics, runs of any hidden sizes evaluate their critics on the device too.
 --validation: every epoch, the SAC losses, TD errors and targets on the evaluation paths' transitions -- held-out data
 -- from the live weights: validation/ columns in progress.csv; SAC only.
 --eval_general device: with --validation (or --td3_validation), runs of any hidden sizes evaluate these objectives on
 the device too.
 --eval_stats device: with --validation, the statistics of the runs evaluated on the device are reduced there as well.
 --replay_eval [N]: every epoch, the same objectives on N (bare: 1024) rows of the replay buffer, read in place on the
 device: replay/ columns in progress.csv, the training-data figures next to the validation/ ones; SAC only.
 --unit_diagnostics: every epoch, the dormant, dead and active fractions and the feature norm of policy, qf1 and qf2 on
 the evaluation paths, from per-unit reductions of the hidden layers: twelve units/ columns; SAC and TD3.
 --unit_general device: with --unit_diagnostics, runs of any hidden sizes reduce them on the device.
 --td3_validation: --validation for TD3 runs: every epoch, the TD3 losses, TD errors and targets on the evaluation
 paths' transitions from the live weights: validation/ columns in progress.csv; TD3 only.
 --td3_replay_eval [N]: --replay_eval for TD3 runs: every epoch, the TD3 objectives on N (bare: 1024) rows of the replay
 buffer, read in place on the device: replay/ columns in progress.csv; TD3 only.  --eval_stats device applies to both.
 --recycle [E] --recycle_tau T: every E-th epoch the T-dormant hidden units of policy, qf1 and qf2 are recycled on the
 device in front of the training block (ReDo): recycle/ columns in progress.csv; SAC and TD3.
 --reset [E] --reset_shrink S --reset_perturb P: every E-th epoch policy, qf1 and qf2 become S theta + P theta_fresh on
 the device in front of the training block (the defaults 0 and 1: a periodic reset; 0.8 and 0.2: shrink and perturb),
 Adam's moments zero, targets alike: the reset/Networks column in progress.csv; SAC and TD3.)
Runs the variant unchanged (batch size, lrs, tau, period, buffer size ... from the JSON) on the
HIP library with a synthetic environment of the task's dimensions (robosuite is not installed)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robosuite_benchmark_amd.driver import experiment, experiment_group, experiment_sweep  # noqa: E402
from robosuite_benchmark_amd.group_checkpoint import GroupMismatchError  # noqa: E402
from robosuite_benchmark_amd.variant import default_variant, expand_hidden_sizes, load_variant  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", type=str, default=None)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log_dir", type=str, default=None)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--env", type=str, default="Lift")
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--agent", type=str, default="SAC", choices=["SAC", "TD3"])
    ap.add_argument("--resume", type=str, default=None,
                    help="an existing run directory (…_0000--s-0): continue it from its checkpoint/ after the last saved "
                         "epoch; with --seeds / --variants: the group's --log_dir, given the same seeds and variants in "
                         "the same order")
    ap.add_argument("--no_checkpoint", action="store_true", help="do not save <run_dir>/checkpoint after every epoch")
    ap.add_argument("--seeds", type=int, nargs="+", default=None,
                    help="train these seeds of the one configuration together (trainer groups; SAC or TD3)")
    ap.add_argument("--variants", type=str, nargs="+", default=None,
                    help="variant files of different tasks: every (variant, seed of --seeds or --seed) pair trains "
                         "together as one mixed trainer group")
    ap.add_argument("--checkpoint", action="store_true",
                    help="with --seeds / --variants and --log_dir DIR: save the whole group to DIR/checkpoint after "
                         "every epoch (only the replay-buffer chunks changed since the last save are written)")
    ap.add_argument("--hidden_sweep", action="store_true",
                    help="with --variants: the variants may differ in their hidden sizes (a network-size sweep as one "
                         "arch trainer group); run names carry the sizes")
    ap.add_argument("--hidden_sizes", type=str, nargs="+", default=None,
                    help="with --variants: train every variant once per entry (comma-separated widths, e.g. 256,256 "
                         "512,512 256,256,256), policy and Q nets alike; implies --hidden_sweep")
    ap.add_argument("--acting", type=str, default="host", choices=["host", "device", "device_all"],
                    help="where the collectors' policies act: host (sac_policy_act, one observation per call) or device "
                         "(the policy forward as a HIP kernel on the live weights; with --seeds / --variants the runs "
                         "collect in lockstep, all their actions of a tick from one launch of an acting session; runs "
                         "whose hidden sizes are beyond two layers of at most 256 units still act on the host) or "
                         "device_all (device, and those runs act on the device too, one launch per layer)")
    ap.add_argument("--q_diagnostics", action="store_true",
                    help="every epoch, evaluate qf1 and qf2 on the evaluation paths (a HIP kernel on the live weights) and "
                         "log evaluation/Q1 Estimates, Q2 Estimates, Returns To Go and Q Bias = min(Q1, Q2) - discounted "
                         "return to go; off: progress.csv is unchanged")
    ap.add_argument("--q_general", type=str, default="host", choices=["host", "device"],
                    help="with --q_diagnostics: where runs whose hidden sizes are beyond two layers of at most 256 units "
                         "evaluate qf1 and qf2 -- host (a parameter copy and a NumPy forward) or device (one HIP launch per "
                         "layer on the live weights); without --q_diagnostics it has no effect")
    ap.add_argument("--validation", action="store_true",
                    help="every epoch, evaluate the SAC objectives (QF losses, TD errors, Q targets, log pi, policy loss) on "
                         "the transitions of the evaluation paths, which never enter the replay buffer (a HIP kernel on "
                         "the live weights), and log them as validation/<key>; SAC only; off: progress.csv is unchanged")
    ap.add_argument("--eval_general", type=str, default="host", choices=["host", "device"],
                    help="with --validation or --td3_validation: where runs whose hidden sizes are beyond two layers of at "
                         "most 256 units evaluate their objectives (SAC's, or TD3's under --td3_validation) -- host (a "
                         "parameter copy and a NumPy forward) or device (one HIP launch per layer on the live weights); "
                         "without either option it has no effect")
    ap.add_argument("--eval_stats", type=str, default="host", choices=["host", "device"],
                    help="with --validation: where the statistics (means, deviations, extremes, losses) of the runs that are "
                         "evaluated on the device are reduced -- host (the columns are copied out and reduced in NumPy) or "
                         "device (one more HIP launch in front of the call's wait); the same validation/ columns either "
                         "way; it applies to --td3_validation and --td3_replay_eval (the TD3 objectives) in the same way; "
                         "without --validation, --replay_eval and those two it has no effect")
    ap.add_argument("--replay_eval", type=int, nargs="?", const=1024, default=0, metavar="N",
                    help="every epoch, evaluate the same objectives on min(N, buffer size) rows of the replay buffer in "
                         "place (a HIP kernel copies the rows from the replay storage into the evaluation's mapped staging: no "
                         "gather to the host, no host conversion), at the point where --validation is taken, and log them as replay/<key>: "
                         "the training-data figure the validation/ columns stand next to; the bare flag: 1024 rows; SAC "
                         "only; --eval_general and --eval_stats apply to it too; 0 (the default): progress.csv is unchanged")
    ap.add_argument("--unit_diagnostics", action="store_true",
                    help="every epoch, reduce the hidden layers' activations of policy, qf1 and qf2 on the evaluation paths "
                         "per unit, from the live weights, and log units/<Net> Dormant Fraction, Dead Fraction, Active "
                         "Fraction and Feature Norm: how much of each network is alive; SAC and TD3; off: progress.csv is "
                         "unchanged")
    ap.add_argument("--unit_general", type=str, default="host", choices=["host", "device"],
                    help="with --unit_diagnostics: where runs whose hidden sizes are beyond two layers of at most 256 units "
                         "reduce them -- host (a parameter copy and a NumPy forward) or device (per layer one forward "
                         "launch and one reduction launch on the live weights); without --unit_diagnostics it has no effect")
    ap.add_argument("--param_diagnostics", action="store_true",
                    help="every epoch, reduce every net's parameters, Adam moments and target distances per tensor on the "
                         "device where they live (one HIP launch, no parameter copy) and log params/<Net> Weight Norm, "
                         "Weight Abs Max, Adam M Norm, Adam V Mean, Adam V Max, Target Gap and params/Non Finite; SAC and "
                         "TD3; off: progress.csv is unchanged")
    ap.add_argument("--td3_validation", action="store_true",
                    help="every epoch, evaluate the TD3 objectives (QF losses, TD errors, Q targets with target smoothing, "
                         "policy loss) on the transitions of the evaluation paths, which never enter the replay buffer (a "
                         "HIP kernel on the live weights), and log them as validation/<key>; TD3 only (SAC runs take "
                         "--validation); off: progress.csv is unchanged")
    ap.add_argument("--td3_replay_eval", type=int, nargs="?", const=1024, default=0, metavar="N",
                    help="--replay_eval for TD3 runs: every epoch, evaluate the TD3 objectives on min(N, buffer size) rows of "
                         "the replay buffer in place (a HIP kernel copies the rows from the replay storage into the "
                         "evaluation's staging: no gather to the host), at the point where --td3_validation is taken, and "
                         "log them as replay/<key>; the bare flag: 1024 rows; TD3 only (SAC runs take --replay_eval); "
                         "--eval_general and --eval_stats apply to it too; 0 (the default): progress.csv is unchanged")
    ap.add_argument("--recycle", type=int, nargs="?", const=1, default=0, metavar="E",
                    help="every E-th epoch (the bare flag: every epoch; never epoch 0), in front of the training block, "
                         "recycle the dormant hidden units of policy, qf1 and qf2 found on the evaluation paths (ReDo: "
                         "fresh incoming weights, zero outgoing weights, Adam's moments of both reset -- HIP kernels on "
                         "the live state, no parameter copy) and log recycle/<Net> Units; target nets are left alone; "
                         "SAC and TD3; --unit_general applies to it; 0 (the default): the run and progress.csv are unchanged")
    ap.add_argument("--recycle_tau", type=float, default=0.025,
                    help="with --recycle: a unit is dormant when its mean activation is at most this share of its "
                         "layer's (the Dormant Fraction of --unit_diagnostics at the same value)")
    ap.add_argument("--reset", type=int, nargs="?", const=1, default=0, metavar="E",
                    help="every E-th epoch (the bare flag: every epoch; never epoch 0), in front of the training block, set "
                         "policy, qf1 and qf2 to reset_shrink * theta + reset_perturb * theta_fresh (a HIP kernel draws the "
                         "fresh parameters and writes the live state, no parameter copy), zero Adam's moments and give the "
                         "targets the same values; the replay buffer stays; logs reset/Networks; SAC and TD3; 0 (the "
                         "default): the run and progress.csv are unchanged")
    ap.add_argument("--reset_shrink", type=float, default=0.0,
                    help="with --reset: the factor on the trained parameters (0, the default: a full reset)")
    ap.add_argument("--reset_perturb", type=float, default=1.0,
                    help="with --reset: the factor on the fresh parameters (shrink and perturb: 0.8 and 0.2)")
    return ap


if __name__ == "__main__":
    args = build_parser().parse_args()
    # the option keywords of all three entries (driver.EvalOptions, and acting); the later ones are left out at their defaults
    option_kw = dict(acting=args.acting, q_diagnostics=args.q_diagnostics, q_general=args.q_general, validation=args.validation)
    if args.eval_general != "host":
        option_kw["eval_general"] = args.eval_general
    if args.eval_stats != "host":
        option_kw["eval_stats"] = args.eval_stats
    if args.replay_eval:
        option_kw["replay_eval"] = args.replay_eval
    if args.unit_diagnostics:
        option_kw["unit_diagnostics"] = True
    if args.unit_general != "host":
        option_kw["unit_general"] = args.unit_general
    if args.param_diagnostics:
        option_kw["param_diagnostics"] = True
    if args.td3_validation:
        option_kw["td3_validation"] = True
    if args.td3_replay_eval:
        option_kw["td3_replay_eval"] = args.td3_replay_eval
    if args.recycle:
        option_kw.update(recycle_period=args.recycle, recycle_tau=args.recycle_tau)
    if args.reset:
        option_kw.update(reset_period=args.reset, reset_shrink=args.reset_shrink, reset_perturb=args.reset_perturb)
    if (args.hidden_sweep or args.hidden_sizes) and not args.variants:
        raise SystemExit("--hidden_sweep / --hidden_sizes need --variants")
    if args.variants or args.seeds:
        log_dir = args.resume or args.log_dir
        if args.checkpoint and not log_dir:
            raise SystemExit("--checkpoint needs --log_dir (the group is saved to <log_dir>/checkpoint)")
        group_kw = dict(log_dir=log_dir, num_epochs=args.epochs, resume=bool(args.resume),
                        checkpoint_dir=os.path.join(log_dir, "checkpoint") if (args.checkpoint or args.resume) else None,
                        **option_kw)
        try:
            if args.variants:
                seeds = args.seeds or [args.seed]
                variants = [load_variant(v) for v in args.variants]
                if args.hidden_sizes:
                    variants = expand_hidden_sizes(variants, args.hidden_sizes)
                experiment_sweep([(v, s) for v in variants for s in seeds],
                                 hidden_sweep=bool(args.hidden_sweep or args.hidden_sizes), **group_kw)
            else:
                variant = load_variant(args.variant) if args.variant else default_variant(
                    env=args.env, seed=args.seeds[0], batch_size=args.batch_size, agent=args.agent)
                experiment_group(variant, args.seeds, **group_kw)
        except GroupMismatchError as e:
            raise SystemExit(f"--resume {args.resume}: {e}")
        sys.exit(0)
    variant = load_variant(args.variant) if args.variant else default_variant(env=args.env, seed=args.seed,
                                                                              batch_size=args.batch_size, agent=args.agent)
    run_dir = None
    if args.resume:
        import json
        run_dir = args.resume
        variant = json.load(open(os.path.join(run_dir, "variant.json")))
    elif args.log_dir:
        # the reference's run-directory layout (rlkit setup_logger, observed under runs/):
        #   <log_dir>/<Prefix-with-dashes>/<prefix>_<timestamp>_0000--s-0/{variant.json, progress.csv}
        import datetime
        import json
        ek = variant["expl_environment_kwargs"]
        prefix = "{}_{}_{}_SEED{}".format(ek["env_name"], "".join(ek["robots"]), ek["controller"], args.seed)
        stamp = datetime.datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
        run_dir = os.path.join(args.log_dir, prefix.replace("_", "-"), f"{prefix}_{stamp}_0000--s-0")
        os.makedirs(run_dir, exist_ok=True)
        json.dump(variant, open(os.path.join(run_dir, "variant.json"), "w"), indent=2, sort_keys=True)
    ckpt = os.path.join(run_dir, "checkpoint") if (run_dir and not args.no_checkpoint) else None
    experiment(variant, log_dir=run_dir, seed=args.seed, num_epochs=args.epochs, checkpoint_dir=ckpt,
               resume=bool(args.resume), **option_kw)
