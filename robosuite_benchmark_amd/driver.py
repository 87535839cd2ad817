"""Own counterpart of the reference's experiment assembly + epoch loop for boxes without
rlkit / robosuite (the GPU box): variant.json -> nets, trainer, HBM replay buffer -> epochs.

Mirrors /root/reference/util/rlkit_utils.py:31-165 (``experiment``) and
/root/reference/util/rlkit_custom.py:199-301 (``_train`` / ``_log_stats``): prefill, then per
epoch {eval collection, exploration collection, add_paths, num_trains_per_train_loop x
(random_batch; train), end_epoch + one progress.csv row with the reference's column names}.
Environment stepping stays on the host; with no robosuite here the env is a synthetic stand-in
with the task's observation/action sizes (SURVEY.md section 8d synthetic data)."""
from __future__ import annotations

import csv
import os
import time
from collections import OrderedDict
from typing import NamedTuple

import numpy as np

from .checkpoint import checkpoint_exists, load_checkpoint, save_checkpoint
from .group_checkpoint import DEFAULT_CHUNK_ROWS, GroupCheckpoint, member_identity
from .group_checkpoint import checkpoint_exists as _checkpoint_exists
from .networks import (FlattenMlp, GaussianStrategy, MakeDeterministic, PolicyWrappedWithExplorationStrategy,
                       TanhGaussianPolicy, TanhMlpPolicy, check_acting)
from .replay_buffer import EnvReplayBuffer
from .group import (ArchSACTrainerGroup, ArchTD3TrainerGroup, GroupActor, MixedSACTrainerGroup, MixedTD3TrainerGroup,
                    MlpSACTrainerGroup, MlpTD3TrainerGroup, SACTrainerGroup, TD3TrainerGroup, act_many,
                    evaluate_many, evaluate_replay_many, q_values_many, recycle_units_many, runs_general_step, shrink_perturb_many,
                    param_moments_many, param_statistics, td3_evaluate_many, td3_evaluate_replay_many,
                    unit_moments_many, unit_statistics)
from .infer import UNIT_NET_TITLES, check_general, check_stats, dormant_units, param_target
from .infer import td3_eval_statistics
from .sac import SACTrainer, eval_statistics
from .td3 import TD3Trainer
from .variant import env_dims, validate


class SyntheticEnv:
    """Host-side stand-in for NormalizedBoxEnv(GymWrapper(robosuite env)): shaped reward in [0,1],
    never terminates (ignore_done=True in every shipped variant)."""

    def __init__(self, obs_dim, action_dim, horizon=500, seed=0):
        self.obs_dim, self.action_dim, self.horizon = obs_dim, action_dim, horizon
        self._rs = np.random.RandomState(seed)
        self._goal = self._rs.normal(0, 0.5, action_dim)
        self._t = 0

    def reset(self):
        self._t = 0
        self._obs = self._rs.normal(0, 0.5, self.obs_dim)
        return self._obs

    def step(self, action):
        self._t += 1
        rew = float(np.exp(-np.sum((np.asarray(action) - np.tanh(self._goal)) ** 2)))
        self._obs = 0.9 * self._obs + self._rs.normal(0, 0.2, self.obs_dim)
        return self._obs, rew, False, {}


def rollout(env, policy, max_path_length):
    """rlkit rollout contract (rlkit_custom.py:487-495 path dict)."""
    obs_l, act_l, rew_l, nobs_l, term_l = [], [], [], [], []
    o = env.reset()
    policy.reset()
    for _ in range(max_path_length):
        a, _ = policy.get_action(o)
        no, r, d, _ = env.step(a)
        obs_l.append(o); act_l.append(a); rew_l.append(r); nobs_l.append(no); term_l.append(d)
        o = no
        if d:
            break
    n = len(obs_l)
    return dict(observations=np.array(obs_l), actions=np.array(act_l), rewards=np.array(rew_l).reshape(n, 1),
                next_observations=np.array(nobs_l), terminals=np.array(term_l).reshape(n, 1),
                agent_infos=[{}] * n, env_infos=[{}] * n)


class PathCollector:
    """MdpPathCollector.collect_new_paths: the last path is clipped to the remaining step budget and
    kept unless discard_incomplete_paths (pins 'exploration/num paths total' = 12 at epoch 0)."""

    def __init__(self, env, policy):
        self.env, self.policy = env, policy
        self.num_steps_total, self.num_paths_total, self.epoch_paths = 0, 0, []

    def collect_new_paths(self, max_path_length, num_steps, discard_incomplete_paths):
        paths, collected = [], 0
        while collected < num_steps:
            mpl = min(max_path_length, num_steps - collected)
            path = rollout(self.env, self.policy, mpl)
            plen = len(path["actions"])
            if plen != max_path_length and not path["terminals"][-1] and discard_incomplete_paths:
                break
            collected += plen
            paths.append(path)
        self.num_paths_total += len(paths)
        self.num_steps_total += collected
        self.epoch_paths.extend(paths)
        return paths

    def end_epoch(self, epoch):
        self.epoch_paths = []

    def get_diagnostics(self):
        return OrderedDict([("num steps total", self.num_steps_total), ("num paths total", self.num_paths_total)])


def _acting_parts(policy):
    """A collector's policy as (holder, deterministic, exploration wrapper or None): MakeDeterministic(holder), a
    PolicyWrappedWithExplorationStrategy around a holder, or the holder itself."""
    if isinstance(policy, MakeDeterministic):
        return policy.stochastic_policy, True, None
    if isinstance(policy, PolicyWrappedWithExplorationStrategy):
        return policy.policy, False, policy
    return policy, False, None


def _numpy_action(h, obs, eps):
    """One action row of a holder without a trainer handle, from its own NumPy forward (eps: its (1, A) draw or None)."""
    obs = np.asarray(obs, np.float32)[None]
    if isinstance(h, TanhGaussianPolicy):
        mean, log_std = h._trunk(obs)
        return (np.tanh(mean) if eps is None else np.tanh(mean + np.exp(log_std) * eps))[0, :]
    return h.get_actions(obs)[0, :]


def _bound(h):
    """Does holder h act through its trainer's handle (the device, or the trainer's own policy_act)?"""
    tr = h._trainer
    return tr is not None and getattr(tr, "_h", None) is not None and tr.policy is h


def holder_actions(holders, obs_list, deterministic_list, act_many=act_many, general="host"):
    """One action row per holder: what holders[i].get_action(obs_list[i]) (MakeDeterministic: deterministic_list[i])
    returns, for all of them at once.  Every stochastic TanhGaussianPolicy draws its (1, A) exploration noise on the host
    from its own _noise stream, exactly as get_action does; the holders whose trainer has a handle then act through ONE
    act_many call (group.act_many: the fused kernels' shapes in one launch, the general step on the host), holders
    without one through their own NumPy forward.  general="device": act_many(..., general="device"), the holders of
    the general step on the device as well."""
    eps, bound = [], []
    for h, det in zip(holders, deterministic_list):
        stochastic = isinstance(h, TanhGaussianPolicy) and not det
        eps.append(h._noise.standard_normal((1, h.action_dim)).astype(np.float32) if stochastic else None)
        bound.append(_bound(h))
    acts = [None] * len(holders)
    ids = [i for i, b in enumerate(bound) if b]
    if ids:
        got = act_many([holders[i]._trainer for i in ids], [np.asarray(obs_list[i])[None] for i in ids],
                       [deterministic_list[i] for i in ids], [eps[i] for i in ids],
                       **_q_general_kw(general))
        for i, a in zip(ids, got):
            acts[i] = a[0, :]
    for i, h in enumerate(holders):
        if not bound[i]:
            acts[i] = _numpy_action(h, obs_list[i], eps[i])
    return acts


class GroupPathCollector:
    """PathCollector.collect_new_paths for many runs in LOCKSTEP: on every tick the current observation of every member
    that still has steps to take goes through ONE act_many call, then each of those members steps its env.

    collectors: the runs' PathCollectors (env, policy, counters, epoch_paths), which this object fills exactly as their
    own collect_new_paths would: per member the same rollouts -- env.reset / policy.reset at the start of a path, the
    last path clipped to the remaining step budget and dropped under discard_incomplete_paths -- the same paths, and the
    same num_steps_total / num_paths_total.  Members finish at different ticks.  Each member's envs, noise streams and
    weights are its own, so a member's paths do not depend on who else is collected with it.

    sessions=True: the members whose holder is bound to a trainer handle act through a GroupActor (group.py: acting
    sessions, persistent staging) that is built at the first collect_new_paths and kept: per tick each live member's
    observation goes into the session's obs row, each stochastic TanhGaussianPolicy's draw -- the same draw from the same
    stream in the same order as holder_actions' -- into its eps row, one act() call follows and the action rows are
    copied out.  Paths, counters and generator states are those of the default.  `actor` is the GroupActor factory
    (trainers, max_rows=1), injectable as act_many is; close() destroys the sessions.

    general="device" (acting="device_all" of the drivers): act_many and the GroupActor factory are called with
    general="device", so that the members of the general step act on the device too; everything else, the draws from
    the host generators included, is as under the default "host".  general_sessions (True / False; None: GroupActor's
    default) goes to the GroupActor factory with it: acting sessions for the members of the general step too."""

    def __init__(self, collectors, act_many=act_many, sessions=False, actor=GroupActor, general="host", general_sessions=None):
        self.collectors, self._act_many = list(collectors), act_many
        self._general = _q_general_kw(general)
        self._actor_kw = dict(self._general)
        if general == "device" and general_sessions is not None:
            self._actor_kw["general_sessions"] = bool(general_sessions)
        self._sessions, self._actor_factory, self._actor, self._actor_key = bool(sessions), actor, None, None

    def close(self):
        actor, self._actor, self._actor_key = self._actor, None, None
        if actor is not None:
            actor.close()

    def _session_tick(self, parts):
        """The sessions' stand-in for holder_actions: tick(ids, observations) -> one action row per live member."""
        holders = [p[0] for p in parts]
        slot = {i: k for k, i in enumerate(i for i, h in enumerate(holders) if _bound(h))}
        key = tuple(id(holders[i]._trainer) for i in slot)
        if self._actor is None or key != self._actor_key:
            self.close()
            if slot:
                self._actor = self._actor_factory([holders[i]._trainer for i in slot], max_rows=1, **self._actor_kw)
            self._actor_key = key
        actor = self._actor
        det = [bool(parts[i][1]) for i in slot]
        stochastic = [isinstance(h, TanhGaussianPolicy) and not p[1] for h, p in zip(holders, parts)]

        def tick(ids, obs_list):
            n_rows, eps = [0] * len(slot), {}
            for i, o in zip(ids, obs_list):
                if stochastic[i]:
                    eps[i] = holders[i]._noise.standard_normal((1, holders[i].action_dim))
                if i in slot:
                    k = slot[i]
                    actor.obs[k][0] = o
                    if stochastic[i]:
                        actor.eps[k][0] = eps[i][0]
                    n_rows[k] = 1
            if any(n_rows):
                actor.act(n_rows, det)
            return [actor.act[slot[i]][0].copy() if i in slot else
                    _numpy_action(holders[i], o, eps[i].astype(np.float32) if i in eps else None)
                    for i, o in zip(ids, obs_list)]
        return tick

    def collect_new_paths(self, plans):
        """plans[i] = (max_path_length, num_steps, discard_incomplete_paths) of member i.  Returns [paths of member i]."""
        if len(plans) != len(self.collectors):
            raise RuntimeError("GroupPathCollector.collect_new_paths takes one plan per collector")
        parts = [_acting_parts(c.policy) for c in self.collectors]
        S = [dict(c=c, mpl_max=int(p[0]), budget=int(p[1]), discard=bool(p[2]), paths=[], collected=0, live=True)
             for c, p in zip(self.collectors, plans)]

        def begin(m):                                         # the head of PathCollector's while loop + rollout's
            if m["collected"] >= m["budget"]:
                m["live"] = False
                return
            m["mpl"] = min(m["mpl_max"], m["budget"] - m["collected"])
            m["o"] = m["c"].env.reset()
            m["c"].policy.reset()
            m["rec"] = ([], [], [], [], [])

        def finish(m):                                        # the tail of rollout + of the while loop's body
            obs_l, act_l, rew_l, nobs_l, term_l = m["rec"]
            n = len(obs_l)
            path = dict(observations=np.array(obs_l), actions=np.array(act_l), rewards=np.array(rew_l).reshape(n, 1),
                        next_observations=np.array(nobs_l), terminals=np.array(term_l).reshape(n, 1),
                        agent_infos=[{}] * n, env_infos=[{}] * n)
            if n != m["mpl_max"] and not path["terminals"][-1] and m["discard"]:
                m["live"] = False
                return
            m["collected"] += n
            m["paths"].append(path)
            begin(m)

        for m in S:
            begin(m)
        tick = self._session_tick(parts) if self._sessions else None
        while True:
            ids = [i for i, m in enumerate(S) if m["live"]]
            if not ids:
                break
            if tick is not None:
                acts = tick(ids, [S[i]["o"] for i in ids])
            else:
                acts = holder_actions([parts[i][0] for i in ids], [S[i]["o"] for i in ids], [parts[i][1] for i in ids],
                                      self._act_many, **self._general)
            for i, a in zip(ids, acts):
                m, wrapper = S[i], parts[i][2]
                if wrapper is not None:                       # PolicyWrappedWithExplorationStrategy.get_action
                    a = wrapper.es.get_action_from_raw_action(a, wrapper.t)
                no, r, d, _ = m["c"].env.step(a)
                for lst, x in zip(m["rec"], (m["o"], a, r, no, d)):
                    lst.append(x)
                m["o"] = no
                if d or len(m["rec"][0]) == m["mpl"]:
                    finish(m)
        for m in S:
            c = m["c"]
            c.num_paths_total += len(m["paths"])
            c.num_steps_total += m["collected"]
            c.epoch_paths.extend(m["paths"])
        return [m["paths"] for m in S]


def _stats(name, x):
    x = np.asarray(x, dtype=np.float64).ravel()
    return OrderedDict([(name + " Mean", float(np.mean(x))), (name + " Std", float(np.std(x))),
                        (name + " Max", float(np.max(x))), (name + " Min", float(np.min(x)))])


def path_information(paths, prefix, expl_len=None):
    d = OrderedDict()
    d.update(_stats(prefix + "path length", [len(p["actions"]) for p in paths]))
    d.update(_stats(prefix + "Rewards", np.vstack([p["rewards"] for p in paths])))
    d.update(_stats(prefix + "Returns", [np.sum(p["rewards"]) for p in paths]))
    if expl_len is not None:      # evaluation/ExplReturns: return truncated at the exploration horizon
        d.update(_stats(prefix + "ExplReturns", [np.sum(p["rewards"][:expl_len]) for p in paths]))
    d.update(_stats(prefix + "Actions", np.vstack([p["actions"] for p in paths])))
    d[prefix + "Num Paths"] = len(paths)
    d[prefix + "Average Returns"] = float(np.mean([np.sum(p["rewards"]) for p in paths]))
    return d


def q_bias_information(paths, q1, q2, discount, reward_scale):
    """The critics against the returns actually obtained on `paths` (the overestimation bias of the TD3 and SAC papers),
    in float64.  q1 / q2: Q1 / Q2(s_t, a_t) for every step of every path, the paths one behind the other.  For each step
    G_t = sum_{k >= t} discount^(k - t) * reward_scale * r_k over the path AS COLLECTED: a path cut by the time limit (or
    by the epoch's step budget) lacks its tail, so its G_t is short of the return the critics estimate by up to
    discount^(T - t) * V(s_T), most of all near the path's end.  Columns, each Mean / Std / Max / Min (_stats):
    evaluation/Q1 Estimates, evaluation/Q2 Estimates, evaluation/Returns To Go, evaluation/Q Bias = min(q1, q2) - G."""
    q1, q2 = np.asarray(q1, np.float64).ravel(), np.asarray(q2, np.float64).ravel()
    G = []
    for p in paths:
        r = float(reward_scale) * np.asarray(p["rewards"], np.float64).ravel()
        g, acc = np.empty(r.size, np.float64), 0.0
        for t in range(r.size - 1, -1, -1):
            acc = r[t] + float(discount) * acc
            g[t] = acc
        G.append(g)
    G = np.concatenate(G) if G else np.empty(0, np.float64)
    if not (q1.size == q2.size == G.size):
        raise ValueError(f"q_bias_information: {q1.size} / {q2.size} Q values for {G.size} steps")
    d = OrderedDict()
    d.update(_stats("evaluation/Q1 Estimates", q1))
    d.update(_stats("evaluation/Q2 Estimates", q2))
    d.update(_stats("evaluation/Returns To Go", G))
    d.update(_stats("evaluation/Q Bias", np.minimum(q1, q2) - G))
    return d


def _path_steps(paths, O, A):
    """Every (observation, action) of `paths`, the paths one behind the other: (n, O), (n, A) float32."""
    if not paths:
        return np.empty((0, O), np.float32), np.empty((0, A), np.float32)
    return (np.concatenate([np.asarray(p["observations"], np.float32).reshape(-1, O) for p in paths]),
            np.concatenate([np.asarray(p["actions"], np.float32).reshape(-1, A) for p in paths]))


VALIDATION_STREAM = 0x56414C      # "VAL": the third seed word of an epoch's validation draws


def _validation_batch(paths, O, A):
    """Every transition of `paths`, the paths one behind the other, as the dict SACTrainer.evaluate takes (None without
    paths)."""
    if not paths:
        return None
    cat = lambda k, w: np.concatenate([np.asarray(p[k], np.float32).reshape(-1, w) for p in paths])  # noqa: E731
    return dict(observations=cat("observations", O), actions=cat("actions", A), rewards=cat("rewards", 1),
                terminals=cat("terminals", 1), next_observations=cat("next_observations", O))


def _validation_eps(seed, epoch, batch, A):
    """(eps, eps_next) of a run's validation in `epoch`: a function of (seed, epoch) alone, so nothing needs checkpointing
    and a resumed run logs the same rows."""
    if batch is None:
        return None
    rs = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(epoch), VALIDATION_STREAM])
    n = batch["observations"].shape[0]
    return rs.standard_normal((n, A)), rs.standard_normal((n, A))


def _td3_validation_eps(seed, epoch, batch, A):
    """The smoothing draw of a TD3 run's validation in `epoch`: the first draw of _validation_eps' generator, a function
    of (seed, epoch) alone."""
    if batch is None:
        return None
    rs = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(epoch), VALIDATION_STREAM])
    return rs.standard_normal((batch["observations"].shape[0], A))


def _td3_objective_columns(prefix, stats, n):
    """<prefix><key> for every key of td3_eval_statistics, and <prefix>Num Transitions = n.  stats None (nothing to
    evaluate this epoch: no evaluation path, an empty buffer): the columns stay, empty."""
    if stats is None:
        stats = OrderedDict((k, float("nan")) for k in td3_eval_statistics(np.zeros((6, 1)), np.zeros((1, 1))))
    d = OrderedDict((prefix + k, v) for k, v in stats.items())
    d[prefix + "Num Transitions"] = int(n)
    return d


def _td3_validation_columns(stats, batch):
    """The validation block of a TD3 run's row: validation/<key> for every key of td3_eval_statistics and
    validation/Num Transitions.  stats None (no evaluation path this epoch): the columns stay, empty."""
    return _td3_objective_columns("validation/", stats, 0 if batch is None else batch["observations"].shape[0])


def _td3_replay_columns(stats, n):
    """The replay block of a TD3 run's row: the statistics of n replay rows (0: an empty buffer this epoch)."""
    return _td3_objective_columns("replay/", stats, n)


def _objective_columns(prefix, stats, n):
    """<prefix><key> for every key of SACTrainer.evaluate, and <prefix>Num Transitions = n.  stats None (nothing to evaluate
    this epoch: no evaluation path, an empty buffer): the columns stay, empty."""
    if stats is None:
        z = np.zeros((1, 1))
        stats = OrderedDict((k, float("nan")) for k in eval_statistics(np.zeros((9, 1)), z, z, 1.0, 0.0, 0.0, False))
    d = OrderedDict((prefix + k, v) for k, v in stats.items())
    d[prefix + "Num Transitions"] = int(n)
    return d


def _validation_columns(stats, batch):
    """The validation block of a row: the statistics of `batch` (None: no evaluation path this epoch)."""
    return _objective_columns("validation/", stats, 0 if batch is None else batch["observations"].shape[0])


REPLAY_STREAM = 0x52504C          # "RPL": the third seed word of an epoch's replay-evaluation draws


def check_replay_eval(replay_eval, name="replay_eval"):
    if isinstance(replay_eval, bool) or not isinstance(replay_eval, (int, np.integer)) or replay_eval < 0:
        raise RuntimeError(f"{name} is a row count (0: off), got {replay_eval!r}")
    return int(replay_eval)


def check_recycle_period(recycle_period):
    if isinstance(recycle_period, bool) or not isinstance(recycle_period, (int, np.integer)) or recycle_period < 0:
        raise RuntimeError(f"recycle_period is a number of epochs (0: off), got {recycle_period!r}")
    return int(recycle_period)


def _recycle_rng(seed, epoch):
    """The generator of an epoch's fresh rows: a function of (seed, epoch), so there is nothing to checkpoint."""
    return np.random.RandomState([seed, epoch, 0x524344])


def check_reset(reset_period, reset_shrink, reset_perturb):
    if isinstance(reset_period, bool) or not isinstance(reset_period, (int, np.integer)) or reset_period < 0:
        raise RuntimeError(f"reset_period is a number of epochs (0: off), got {reset_period!r}")
    sh, pe = float(reset_shrink), float(reset_perturb)
    if not (np.isfinite(sh) and np.isfinite(pe) and sh >= 0.0 and pe >= 0.0 and (sh > 0.0 or pe > 0.0)):
        raise RuntimeError(f"reset_shrink and reset_perturb are finite factors >= 0, not both 0, got {reset_shrink!r} and "
                           f"{reset_perturb!r}")
    return int(reset_period), sh, pe


def _reset_words(seed, epoch):
    """(seed, draw) of an epoch's reset, two 64-bit words: a function of (seed, epoch), so there is nothing to checkpoint."""
    w = [int(x) for x in np.random.RandomState([seed, epoch, 0x525354]).randint(0, 2**32, 4)]
    return w[0] | w[1] << 32, w[2] | w[3] << 32


def _replay_rows(replay_eval, buf):
    """The replay rows of an epoch's evaluation: min(replay_eval, buffer size)."""
    return min(int(replay_eval), int(buf.num_steps_can_sample()))


def _replay_rng(seed, epoch):
    """The generator of a run's replay evaluation in `epoch` (the indices, then eps, then eps_next): a function of
    (seed, epoch) alone, so nothing needs checkpointing and a resumed run logs the same rows."""
    return np.random.RandomState([int(seed) & 0xFFFFFFFF, int(epoch), REPLAY_STREAM])


def _replay_columns(stats, n):
    """The replay block of a row: the statistics of n replay rows (0: an empty buffer this epoch)."""
    return _objective_columns("replay/", stats, n)


def _rs_pack(rs):
    st = rs.get_state()
    return dict(key=[int(x) for x in st[1]], pos=int(st[2]), has_gauss=int(st[3]), cached=float(st[4]))


def _rs_unpack(rs, d):
    rs.set_state(("MT19937", np.asarray(d["key"], np.uint32), d["pos"], d["has_gauss"], d["cached"]))


def _q_general_kw(q_general):
    """q_general (eval_general) as the `general` keyword of q_values / q_values_many (evaluate / evaluate_many): left out
    at the default, so the call is what it was."""
    return {} if q_general == "host" else {"general": q_general}


def _eval_stats_kw(eval_stats):
    """eval_stats as the `stats` keyword of evaluate / evaluate_many: left out at the default, as _q_general_kw does."""
    return {} if eval_stats == "host" else {"stats": eval_stats}


class EvalOptions(NamedTuple):
    """The per-epoch evaluations of experiment(), experiment_group() and experiment_sweep(): each is taken right behind
    the epoch's evaluation paths and in front of the training block (policy and critics of one moment), adds a block of
    columns in front of time/* -- Q bias, validation, replay, in this order -- and counts under
    `time/evaluation sampling (s)`.  With all of them off (the defaults) the row, every generator and every column are
    exactly what they were.  experiment() calls the trainer's own methods; the group entries make ONE q_values_many,
    evaluate_many and evaluate_replay_many call per epoch over all runs, and each run's columns are its solo ones.

    q_diagnostics=True: qf1 and qf2 on every (observation, action) of the epoch's evaluation paths (q_values: on the
    device from the live weights) and q_bias_information's sixteen columns behind the evaluation/ block.
    q_general ("host" or "device") is q_values' `general`: where a run of the general step evaluates its critics --
    sac_get_params and a NumPy forward, or sac_q_values_general (one k_qval_layer launch per layer on the live weights;
    in a group one sac_q_values_general_many call per 16 such runs).  Without q_diagnostics, and for a run with the
    fused kernels' shapes, it has no effect.

    validation=True: the SAC objectives on the transitions of the epoch's evaluation paths -- collected
    deterministically, never in the replay buffer: a held-out set -- by evaluate (on the device from the live weights
    and the current entropy coefficient; a run of the general step on the host), with the N(0,1) draws of
    RandomState([seed, epoch, 0x56414C]): nothing to checkpoint, and a resumed run logs the same rows.  The row gains
    validation/<key> for every key of evaluate and validation/Num Transitions.  A TD3 variant is refused.
    eval_general ("host" or "device") is evaluate's `general`: where a run of the general step evaluates its objectives
    -- sac_get_params and a NumPy forward, or sac_evaluate_general (one k_eval_layer launch per layer on the live
    weights; in a group one sac_evaluate_general_many call per 16 such runs).  Without validation, td3_validation and
    replay_eval, and for a run with the fused kernels' shapes, it has no effect.
    eval_stats ("host" or "device") is evaluate's `stats`: where the statistics of a run that is evaluated on the device
    are reduced -- eval_statistics on the columns copied out, or k_eval_moments on the device (the same columns of
    progress.csv, equal up to the rounding of a float64 sum in another order).  It applies to td3_validation and
    td3_replay_eval in the same way (evaluate_td3's `stats`: k_eval_moments_td3).  Without validation, replay_eval,
    td3_validation and td3_replay_eval it has no effect.

    replay_eval=N > 0: the same objectives on min(N, buffer size) rows of the REPLAY buffer in place (evaluate_replay: a
    kernel copies the rows into the evaluation's staging, no gather to the host), in front of the epoch's exploration
    paths -- the figure validation/QF1 Loss stands next to, at the same parameters.  Indices and N(0,1) draws come from
    RandomState([seed, epoch, 0x52504C]).  The row gains replay/<key> for every key of evaluate and
    replay/Num Transitions.  eval_general and eval_stats apply to it as to validation.  A TD3 variant is refused.

    unit_diagnostics=True: how much of each network is alive -- the per-unit records of policy, qf1 and qf2 on every
    (observation, action) of the epoch's evaluation paths (unit_moments: the same steps as q_diagnostics, so no
    generator is used and nothing needs a checkpoint) and unit_statistics' twelve columns units/<Net> Dormant Fraction /
    Dead Fraction / Active Fraction / Feature Norm behind the replay/ block.  unit_general ("host" or "device") is
    unit_moments' `general`: where a run of the general step reduces them -- sac_get_params and a NumPy forward, or
    sac_unit_moments_general (in a group one sac_unit_moments_general_many call per 16 such runs); a run with the
    fused kernels' shapes reduces them on the device either way (sac_unit_moments).  TD3 variants are served.

    param_diagnostics=True: the state the step kernels write -- every net's parameters, Adam's moments, the distance of
    each target to its online net -- reduced per tensor on the device where it lives (param_moments: no parameter copy,
    no generator, nothing to checkpoint), at the point of the epoch where validation is taken, and param_statistics'
    columns params/<Net> Weight Norm / Weight Abs Max / Adam M Norm / Adam V Mean / Adam V Max / Target Gap and
    params/Non Finite behind the units/ block.  The group entries make ONE param_moments_many call per epoch.  SAC and TD3
    variants are served (a TD3 policy has a Target Gap too).

    td3_validation=True: validation for TD3 runs -- the TD3 objectives (a deterministic policy, target smoothing, no
    entropy term) on the transitions of the epoch's evaluation paths by evaluate_td3 (on the device from the live
    weights: td3_evaluate, k_eval_td3; a run of the general step on the host), with the smoothing draw
    RandomState([seed, epoch, 0x56414C]).standard_normal((n, A)): nothing to checkpoint, and a resumed run logs the same
    rows.  The row gains validation/<key> for every key of td3_eval_statistics and validation/Num Transitions where the
    SAC validation block sits; the group entries make ONE td3_evaluate_many call per epoch.  Every run must be a TD3
    variant: a SAC variant is refused (validation=True is its option).  eval_general applies to it as to validation:
    under "device" a TD3 run of the general step evaluates on the device as well (td3_evaluate_general: k_eval_layer_td3
    and k_eval_layer, one launch per layer on the live weights; in a group one td3_evaluate_general_many call per 16
    such runs).  eval_stats applies too: under "device" the statistics of a run that is evaluated on the device are
    reduced there (td3_evaluate_stats_many / td3_evaluate_general_stats_many).

    td3_replay_eval=N > 0: the TD3 objectives on min(N, buffer size) rows of the REPLAY buffer in place
    (evaluate_td3_replay: k_eval_rows copies the rows into the evaluation's staging, no gather to the host), taken where
    validation is taken -- the figure validation/QF1 Loss stands next to, at the same parameters.  Indices and the
    smoothing draw come from RandomState([seed, epoch, 0x52504C]), the indices first: nothing to checkpoint.  The row
    gains replay/<key> for every key of td3_eval_statistics and replay/Num Transitions where the SAC replay block sits;
    the group entries make ONE td3_evaluate_replay_many call per epoch, and only when some run has rows.  eval_general
    and eval_stats apply to it as to td3_validation.  Every run must be a TD3 variant: a SAC variant is refused
    (replay_eval=N is its option).

    recycle_period=E > 0 (no evaluation: the one option here that CHANGES the run): on the epochs with epoch > 0 and
    epoch % E == 0 the recycle_tau-dormant hidden units of policy, qf1 and qf2 are recycled (ReDo;
    SACTrainer.recycle_dormant: fresh incoming weights, zero outgoing weights, Adam's moments of both reset, on the
    device) directly in front of the training block -- _epoch_recycle.  The row gains a last block recycle/Policy Units /
    QF1 Units / QF2 Units.  Target nets are left alone, so params/* Target Gap jumps on such an epoch.  SAC and TD3.

    reset_period=E > 0 (it CHANGES the run too): on the epochs with epoch > 0 and epoch % E == 0 policy, qf1 and qf2 become
    reset_shrink * theta + reset_perturb * theta_fresh (the defaults 0 and 1: a full reset, Nikishin et al. 2022; 0.8 and
    0.2: shrink and perturb, Ash & Adams 2020), Adam's moments +0.0 and the targets the same bits, on the device
    (SACTrainer.shrink_perturb) directly in front of the training block, behind _epoch_recycle -- _epoch_reset.  The
    replay buffer, the step counts and the entropy coefficient stay.  The row gains a last block reset/Networks, the
    number of nets written that epoch.  SAC and TD3."""
    q_diagnostics: bool = False
    q_general: str = "host"
    validation: bool = False
    eval_general: str = "host"
    eval_stats: str = "host"
    replay_eval: int = 0
    unit_diagnostics: bool = False
    unit_general: str = "host"
    param_diagnostics: bool = False
    td3_replay_eval: int = 0
    recycle_period: int = 0
    recycle_tau: float = 0.025
    reset_period: int = 0
    reset_shrink: float = 0.0
    reset_perturb: float = 1.0
    td3_validation: bool = False


def _refuse_td3(variant, what, call, reason):
    if variant.get("algorithm", "SAC") == "TD3":
        raise RuntimeError(f"{what}({call}): {reason}; a TD3 variant has no such evaluation")


def _options(what, specs, acting, q_diagnostics, q_general, validation, eval_general, eval_stats, replay_eval,
             unit_diagnostics=False, unit_general="host", param_diagnostics=False, td3_replay_eval=0,
             recycle_period=0, recycle_tau=0.025, reset_period=0, reset_shrink=0.0, reset_perturb=1.0, td3_validation=False):
    """The EvalOptions of entry `what`, after the value checks of its keywords (acting's too) and, for the variant at
    the head of every run spec in `specs`, the TD3 refusals: all of it in front of anything that builds a run."""
    check_stats(eval_stats)
    check_acting(acting)
    check_general(q_general)
    check_general(eval_general)
    check_general(unit_general)
    opts = EvalOptions(q_diagnostics, q_general, validation, eval_general, eval_stats, check_replay_eval(replay_eval),
                       bool(unit_diagnostics), unit_general, bool(param_diagnostics),
                       check_replay_eval(td3_replay_eval, "td3_replay_eval"), check_recycle_period(recycle_period),
                       float(recycle_tau), *check_reset(reset_period, reset_shrink, reset_perturb), bool(td3_validation))
    if not opts.recycle_tau >= 0.0:
        raise RuntimeError(f"recycle_tau is a threshold >= 0, got {recycle_tau!r}")
    for spec in specs if opts.validation else ():
        _refuse_td3(tuple(spec)[0], what, "validation=True", "validation evaluates the SAC objective (SACTrainer.evaluate)")
    for spec in specs if opts.replay_eval else ():
        _refuse_td3(tuple(spec)[0], what, "replay_eval=N",
                    "the replay evaluation computes the SAC objective (SACTrainer.evaluate_replay)")
    for spec in specs if opts.td3_validation else ():
        if tuple(spec)[0].get("algorithm", "SAC") != "TD3":
            raise RuntimeError(f"{what}(td3_validation=True): td3_validation evaluates the TD3 objective "
                               "(TD3Trainer.evaluate_td3); a SAC variant takes validation=True")
    for spec in specs if opts.td3_replay_eval else ():
        if tuple(spec)[0].get("algorithm", "SAC") != "TD3":
            raise RuntimeError(f"{what}(td3_replay_eval=N): td3_replay_eval evaluates the TD3 objective "
                               "(TD3Trainer.evaluate_td3_replay); a SAC variant takes replay_eval=N")
    return opts


EVAL_BLOCKS = ("q", "validation", "replay", "units")          # the optional column blocks, in the row's order
UNIT_NETS = ("policy", "qf1", "qf2")                          # the nets of the units/ block
ALL_BLOCKS = EVAL_BLOCKS + ("params",)                        # ... and the params/ block behind them


def _unit_columns(moments):
    """The units block of a row: unit_statistics of a run's records (None: no evaluation path this epoch, the columns
    stay, empty)."""
    if moments is None:
        z = dict(count=1.0, sum=np.zeros(1), sumsq=np.zeros(1), active=np.zeros(1), max=np.zeros(1))
        return OrderedDict(("units/" + k, float("nan")) for k in unit_statistics(OrderedDict((n, [z]) for n in UNIT_NETS)))
    return OrderedDict(("units/" + k, v) for k, v in unit_statistics(moments).items())


def _param_columns(t, moments):
    """The params block of a row: param_statistics of a run's records, over every net of its trainer."""
    sizes = {net: [int(np.prod(shape)) for _, shape in t.param_tensors(net)] for net in moments}
    targets = tuple(net for net in moments if param_target(t, net) is not None)
    return OrderedDict(("params/" + k, v) for k, v in param_statistics(moments, sizes, targets).items())


def _epoch_evaluations(runs, epoch, opts, take=ALL_BLOCKS, many=True):
    """The blocks of `take` that `opts` switches on, for every run at this moment of `epoch`: ([{block: columns} per
    run], seconds spent).  many: ONE q_values_many / evaluate_many / evaluate_replay_many / unit_moments_many
    / param_moments_many call over all runs (evaluate_replay_many only when some run has rows); otherwise each trainer's
    own q_values / evaluate / evaluate_replay / unit_moments / param_moments.  For TD3 runs (td3_validation,
    td3_replay_eval) td3_evaluate_many and td3_evaluate_replay_many stand in the same two places, or the trainer's own
    evaluate_td3 / evaluate_td3_replay."""
    s0 = time.time()
    cols, trainers = [{} for _ in runs], [r["trainer"] for r in runs]
    paths = [r["evalc"].epoch_paths for r in runs]
    gen, stats_kw = _q_general_kw(opts.eval_general), _eval_stats_kw(opts.eval_stats)
    if opts.q_diagnostics and "q" in take:
        steps = [_path_steps(p, t.obs_dim, t.act_dim) for p, t in zip(paths, trainers)]
        kw = _q_general_kw(opts.q_general)
        qs = (q_values_many(trainers, [s[0] for s in steps], [s[1] for s in steps], [("qf1", "qf2")] * len(runs), **kw)
              if many else [t.q_values(*s, nets=("qf1", "qf2"), **kw) for t, s in zip(trainers, steps)])
        for c, p, t, q in zip(cols, paths, trainers, qs):
            c["q"] = q_bias_information(p, q[0], q[1], t.discount, t.reward_scale)
    if opts.validation and "validation" in take:
        batches = [_validation_batch(p, t.obs_dim, t.act_dim) for p, t in zip(paths, trainers)]
        eps = [_validation_eps(r["seed"], epoch, b, t.act_dim) for r, b, t in zip(runs, batches, trainers)]
        got = (evaluate_many(trainers, batches, eps=eps, **gen, **stats_kw) if many else
               [None if b is None else t.evaluate(b, eps=e, **gen, **stats_kw) for t, b, e in zip(trainers, batches, eps)])
        for c, s, b in zip(cols, got, batches):
            c["validation"] = _validation_columns(s, b)
    if opts.td3_validation and "validation" in take:
        batches = [_validation_batch(p, t.obs_dim, t.act_dim) for p, t in zip(paths, trainers)]
        eps = [_td3_validation_eps(r["seed"], epoch, b, t.act_dim) for r, b, t in zip(runs, batches, trainers)]
        got = (td3_evaluate_many(trainers, batches, eps=eps, **gen, **stats_kw) if many else
               [None if b is None else t.evaluate_td3(b, eps=e, **gen, **stats_kw) for t, b, e in zip(trainers, batches, eps)])
        for c, s, b in zip(cols, got, batches):
            c["validation"] = _td3_validation_columns(s, b)
    if opts.td3_replay_eval and "replay" in take:               # (the row's replay block, taken where SAC's is)
        bufs, ns = [r["buf"] for r in runs], [_replay_rows(opts.td3_replay_eval, r["buf"]) for r in runs]
        got = [None] * len(runs)
        if any(ns):
            rngs = [_replay_rng(r["seed"], epoch) for r in runs]
            got = (td3_evaluate_replay_many(trainers, bufs, n=ns, rngs=rngs, **gen, **stats_kw) if many else
                   [t.evaluate_td3_replay(b, n=n, rng=g, **gen, **stats_kw) if n else None
                    for t, b, n, g in zip(trainers, bufs, ns, rngs)])
        for c, s, n in zip(cols, got, ns):
            c["replay"] = _td3_replay_columns(s, n)
    if opts.replay_eval and "replay" in take:
        bufs, ns = [r["buf"] for r in runs], [_replay_rows(opts.replay_eval, r["buf"]) for r in runs]
        got = [None] * len(runs)
        if any(ns):
            rngs = [_replay_rng(r["seed"], epoch) for r in runs]
            got = (evaluate_replay_many(trainers, bufs, n=ns, rngs=rngs, **gen, **stats_kw) if many else
                   [t.evaluate_replay(b, n=n, rng=g, **gen, **stats_kw) for t, b, n, g in zip(trainers, bufs, ns, rngs)])
        for c, s, n in zip(cols, got, ns):
            c["replay"] = _replay_columns(s, n)
    if opts.unit_diagnostics and "units" in take:
        steps = [_path_steps(p, t.obs_dim, t.act_dim) for p, t in zip(paths, trainers)]
        kw = _q_general_kw(opts.unit_general)
        got = (unit_moments_many(trainers, [s[0] for s in steps], [s[1] for s in steps], [UNIT_NETS] * len(runs), **kw)
               if many else [t.unit_moments(*s, nets=UNIT_NETS, **kw) if s[0].shape[0] else None
                             for t, s in zip(trainers, steps)])
        for c, m in zip(cols, got):
            c["units"] = _unit_columns(m)
    if opts.param_diagnostics and "params" in take:
        got = param_moments_many(trainers) if many else [t.param_moments() for t in trainers]
        for c, t, m in zip(cols, trainers, got):
            c["params"] = _param_columns(t, m)
    return cols, time.time() - s0


ROW_BLOCKS = ALL_BLOCKS + ("recycle",)                        # ... and the recycle/ block, the row's last in front of time/*


def _epoch_recycle(runs, blocks, epoch, opts, many=True):
    """recycle_period=E > 0: on the epochs with epoch > 0 and epoch % E == 0 the recycle_tau-dormant units of policy, qf1
    and qf2 of every run are recycled (SACTrainer.recycle_dormant) -- directly in front of the training block, behind
    every evaluation block and both collections, so the row's blocks and paths show the state before.  The records come
    from the steps of the epoch's evaluation paths (_path_steps) under unit_general, the fresh rows from
    RandomState([seed, epoch, 0x524344]): nothing to checkpoint.  many: ONE unit_moments_many and ONE recycle_units_many
    call over all runs.  Every row gains blocks["recycle"]: recycle/Policy Units, QF1 Units, QF2 Units -- the counts, 0
    on the other epochs.  With the option at 0 nothing is called and nothing is added."""
    if not opts.recycle_period:
        return
    counts = [None] * len(runs)
    if epoch > 0 and epoch % opts.recycle_period == 0:
        trainers = [r["trainer"] for r in runs]
        steps = [_path_steps(r["evalc"].epoch_paths, t.obs_dim, t.act_dim) for r, t in zip(runs, trainers)]
        rngs = [_recycle_rng(r["seed"], epoch) for r in runs]
        kw = _q_general_kw(opts.unit_general)
        if many:
            moments = unit_moments_many(trainers, [s[0] for s in steps], [s[1] for s in steps], [UNIT_NETS] * len(runs), **kw)
            units = [None if m is None else dormant_units(m, opts.recycle_tau) for m in moments]
            counts = recycle_units_many(trainers, units, rngs=rngs)
        else:
            counts = [t.recycle_dormant(*s, nets=UNIT_NETS, tau=opts.recycle_tau, rng=g, **kw) if s[0].shape[0] else None
                      for t, s, g in zip(trainers, steps, rngs)]
    for b, c in zip(blocks, counts):
        b["recycle"] = OrderedDict((f"recycle/{UNIT_NET_TITLES[n]} Units", 0 if c is None else int(c[n])) for n in UNIT_NETS)


RESET_BLOCKS = ROW_BLOCKS + ("reset",)                        # ... and the reset/ block behind it


def _epoch_reset(runs, blocks, epoch, opts, many=True):
    """reset_period=E > 0: on the epochs with epoch > 0 and epoch % E == 0 policy, qf1 and qf2 of every run become
    reset_shrink * theta + reset_perturb * theta_fresh with opt=True, targets=True (SACTrainer.shrink_perturb) -- directly
    in front of the training block, behind _epoch_recycle.  (seed, draw) are _reset_words(run seed, epoch): nothing to
    checkpoint.  many: ONE shrink_perturb_many call over all runs.  Every row gains blocks["reset"]: reset/Networks, the
    number of nets written, 0 on the other epochs.  With the option at 0 nothing is called and nothing is added."""
    if not opts.reset_period:
        return
    done = [None] * len(runs)
    if epoch > 0 and epoch % opts.reset_period == 0:
        trainers = [r["trainer"] for r in runs]
        words = [_reset_words(r["seed"], epoch) for r in runs]
        kw = dict(shrink=opts.reset_shrink, perturb=opts.reset_perturb, opt=True, targets=True)
        if many:
            done = shrink_perturb_many(trainers, [UNIT_NETS] * len(runs), seeds=[w[0] for w in words],
                                       draws=[w[1] for w in words], **kw)
        else:
            done = [t.shrink_perturb(UNIT_NETS, seed=w[0], draw=w[1], **kw) for t, w in zip(trainers, words)]
    for b, d in zip(blocks, done):
        b["reset"] = OrderedDict([("reset/Networks", 0 if d is None else len(d))])


def _end_epoch_row(r, blocks, epoch):
    """Run r's progress.csv columns of `epoch` in the reference's order up to the time/* block, the blocks of
    _epoch_evaluations, _epoch_recycle and _epoch_reset behind them in RESET_BLOCKS' order; then the run's parts end
    their epoch."""
    buf, trainer, expl, evalc = r["buf"], r["trainer"], r["expl"], r["evalc"]
    row = OrderedDict()
    row.update(("replay_buffer/" + k, v) for k, v in buf.get_diagnostics().items())
    row.update(("trainer/" + k, v) for k, v in trainer.get_diagnostics().items())
    row.update(("exploration/" + k, v) for k, v in expl.get_diagnostics().items())
    row.update(path_information(expl.epoch_paths, "exploration/"))
    row.update(("evaluation/" + k, v) for k, v in evalc.get_diagnostics().items())
    row.update(path_information(evalc.epoch_paths, "evaluation/", r["ak"]["expl_max_path_length"]))
    for name in RESET_BLOCKS:
        row.update(blocks.get(name, ()))
    for x in (trainer, buf, expl, evalc):
        x.end_epoch(epoch)
    return row


def _stamp_times(row, epoch, storing, evaluation, exploration, logging, saving, training, epoch_s, total):
    """The row's last nine columns, in the reference's order."""
    row["time/data storing (s)"] = storing
    row["time/evaluation sampling (s)"] = evaluation
    row["time/exploration sampling (s)"] = exploration
    row["time/logging (s)"] = logging
    row["time/saving (s)"] = saving
    row["time/training (s)"] = training
    row["time/epoch (s)"] = epoch_s
    row["time/total (s)"] = total
    row["Epoch"] = epoch


def _log_row(r, row, log_dir, first_epoch):
    """Run r keeps the row and, with log_dir, writes it to <log_dir>/progress.csv: opened at the run's first row, with
    the row's columns as the header -- or, after a resume (first_epoch > 0) onto an existing file, appended to without
    one."""
    r["rows"].append(row)
    if log_dir is None:
        return
    if r["writer"] is None:
        os.makedirs(log_dir, exist_ok=True)
        path = os.path.join(log_dir, "progress.csv")
        appending = first_epoch > 0 and os.path.exists(path)
        r["fh"] = open(path, "a" if appending else "w", newline="")
        r["writer"] = csv.DictWriter(r["fh"], fieldnames=list(row.keys()))
        if not appending:
            r["writer"].writeheader()
    r["writer"].writerow(row)
    r["fh"].flush()


def _pack_extra(r, epoch):
    """What a checkpoint keeps of run r next to its trainer and buffer: the epoch, the seed, the collectors' totals and
    the host generators."""
    extra = dict(epoch=epoch, seed=r["seed"], expl_totals=[r["expl"].num_steps_total, r["expl"].num_paths_total],
                 eval_totals=[r["evalc"].num_steps_total, r["evalc"].num_paths_total])
    extra.update({k: _rs_pack(rs) for k, rs in r["host_rngs"].items()})
    return extra


def _restore_extra(r, extra):
    """_pack_extra's counterpart on a run whose trainer and buffer have been restored; returns the first epoch to run."""
    for k, rs in r["host_rngs"].items():
        _rs_unpack(rs, extra[k])
    r["expl"].num_steps_total, r["expl"].num_paths_total = extra["expl_totals"]
    r["evalc"].num_steps_total, r["evalc"].num_paths_total = extra["eval_totals"]
    r["trainer"].end_epoch(int(extra["epoch"]))
    return int(extra["epoch"]) + 1


def _build_run(variant, seed, O, A, device, acting, rs):
    """The run record of (variant, seed): seed, ak (the variant's algorithm_kwargs), trainer, buf, expl and evalc (the
    two PathCollectors), rows, fh and writer (its progress.csv), variant, host_rngs (the host generators a checkpoint
    keeps: policy noise and the two environments').  The synthetic environments and every noise stream come from `seed`,
    the initial weights from the generator `rs`: qf1, qf2, target_qf1, target_qf2, then the policy or policies.  The
    buffer is empty.  acting: see experiment()."""
    ak, tk = variant["algorithm_kwargs"], variant["trainer_kwargs"]
    expl_env = SyntheticEnv(O, A, variant["expl_environment_kwargs"].get("horizon", 500), seed)
    eval_env = SyntheticEnv(O, A, variant["eval_environment_kwargs"].get("horizon", 500), seed + 1)
    qf1, qf2, tqf1, tqf2 = (FlattenMlp(input_size=O + A, output_size=1, rs=rs, **variant["qf_kwargs"]) for _ in range(4))
    if variant.get("algorithm", "SAC") == "TD3":                  # rlkit_utils.py:107-135
        policy = TanhMlpPolicy(input_size=O, output_size=A, rs=rs, **variant["policy_kwargs"])
        target_policy = TanhMlpPolicy(input_size=O, output_size=A, rs=rs, **variant["policy_kwargs"])
        eval_policy = policy
        expl_policy = PolicyWrappedWithExplorationStrategy(
            exploration_strategy=GaussianStrategy(max_sigma=0.1, min_sigma=0.1, seed=seed), policy=policy)
        trainer = TD3Trainer(policy=policy, qf1=qf1, qf2=qf2, target_qf1=tqf1, target_qf2=tqf2, target_policy=target_policy,
                             batch_size=ak["batch_size"], noise_seed=seed, device=device, **tk)
        policy._noise = expl_policy.es._rs                        # (the generator a checkpoint saves as policy_noise)
    else:
        policy = TanhGaussianPolicy(obs_dim=O, action_dim=A, rs=rs, noise=np.random.RandomState(seed),
                                    **variant["policy_kwargs"])
        eval_policy, expl_policy = MakeDeterministic(policy), policy
        trainer = SACTrainer(env=eval_env, policy=policy, qf1=qf1, qf2=qf2, target_qf1=tqf1, target_qf2=tqf2,
                             batch_size=ak["batch_size"], noise_seed=seed, device=device, **tk)
    if acting != "host" and not runs_general_step(trainer):
        policy.acting = "device"
    elif acting == "device_all":
        policy.acting = "device_all"
    buf = EnvReplayBuffer(variant["replay_buffer_size"], obs_dim=O, action_dim=A, device=device)
    expl, evalc = PathCollector(expl_env, expl_policy), PathCollector(eval_env, eval_policy)
    host_rngs = dict(policy_noise=policy._noise, expl_env=expl_env._rs, eval_env=eval_env._rs)
    return dict(seed=seed, ak=ak, trainer=trainer, buf=buf, expl=expl, evalc=evalc, rows=[], fh=None, writer=None,
                variant=variant, host_rngs=host_rngs)


def _prefill(r):
    """min_num_steps_before_training exploration steps into the buffer, in front of epoch 0 (the run's own get_action
    calls)."""
    ak = r["ak"]
    if ak.get("min_num_steps_before_training", 0) > 0:
        r["buf"].add_paths(r["expl"].collect_new_paths(ak["expl_max_path_length"], ak["min_num_steps_before_training"], False))
        r["expl"].end_epoch(-1)


def experiment(variant, log_dir=None, seed=1, obs_dim=None, action_dim=None, num_epochs=None, device=0,
               fused_loop=True, quiet=False, checkpoint_dir=None, resume=False, acting="host", q_diagnostics=False,
               q_general="host", validation=False, eval_general="host", eval_stats="host", replay_eval=0,
               unit_diagnostics=False, unit_general="host", param_diagnostics=False, td3_replay_eval=0,
               recycle_period=0, recycle_tau=0.025, reset_period=0, reset_shrink=0.0, reset_perturb=1.0,
               td3_validation=False):
    """variant.json -> training run.  Returns the list of progress rows (also written to
    <log_dir>/progress.csv when log_dir is given).

    checkpoint_dir: after every epoch the full run state (networks, Adam moments, entropy coefficient, step
    counters, replay buffer, sampling stream, host generators) is saved there (`time/saving (s)`); with
    resume=True a run picks up after the last saved epoch and continues bit for bit -- the reference's own
    snapshots (rlkit_custom.py:68-82) hold the networks only and cannot resume.

    acting: "host" (the default: sac_policy_act, one observation per call from the mirrored weights) or "device"
    (sac_policy_act_device: the collectors' get_action calls run k_act on the live weights).  A run of the general step
    acts on the host either way ("device" serves the fused kernels' shapes, and its results are pinned).
    "device_all" is "device", and a run of the general step acts on the device too (sac_policy_act_general: one
    k_act_layer launch per layer on the live weights).  The exploration noise comes from the same host stream, in the
    same amounts, whichever value is given.

    q_diagnostics, q_general, validation, eval_general, eval_stats, replay_eval, unit_diagnostics, unit_general,
    param_diagnostics, td3_replay_eval, td3_validation: the
    per-epoch evaluations, EvalOptions; here from the trainer's own q_values, evaluate, evaluate_replay and unit_moments."""
    opts = _options("experiment", [(variant,)], acting, q_diagnostics, q_general, validation, eval_general, eval_stats,
                    replay_eval, unit_diagnostics, unit_general, param_diagnostics, td3_replay_eval,
                    recycle_period, recycle_tau, reset_period, reset_shrink, reset_perturb, td3_validation)
    validate(variant)
    # This driver's runs are a function of `seed` alone: initial weights come from np.random (seeded here), every noise
    # stream from `seed` -- whether or not torch happens to be loaded in the process (the reference's own scripts seed
    # torch as well, train.py:113, and the holders then follow torch's generator by themselves: networks.process_stream).
    np.random.seed(seed)                                          # scripts/train.py:112 (args.seed, not variant seed)
    O, A = env_dims(variant["expl_environment_kwargs"], obs_dim, action_dim)
    # (no private stream for the buffer: it samples np.random itself -- bound to its state words)
    r = _build_run(variant, seed, O, A, device, acting, np.random)
    ak, trainer, buf, expl, evalc = r["ak"], r["trainer"], r["buf"], r["expl"], r["evalc"]
    first_epoch, t_start = 0, time.time()
    if resume and checkpoint_dir and checkpoint_exists(checkpoint_dir):
        extra = load_checkpoint(checkpoint_dir, trainer, buf)
        _rs_unpack(np.random, extra["np_random"])
        first_epoch = _restore_extra(r, extra)
    else:
        _prefill(r)
    n_train = ak["num_trains_per_train_loop"]
    for epoch in range(first_epoch, num_epochs if num_epochs is not None else ak["num_epochs"]):
        t0 = time.time()
        evalc.collect_new_paths(ak["eval_max_path_length"], ak["num_eval_steps_per_epoch"], True)
        blocks, _ = _epoch_evaluations([r], epoch, opts, many=False)
        t1 = time.time()
        new_paths = expl.collect_new_paths(ak["expl_max_path_length"], ak["num_expl_steps_per_train_loop"], False)
        t2 = time.time()
        buf.add_paths(new_paths)
        t3 = time.time()
        _epoch_recycle([r], blocks, epoch, opts, many=False)
        _epoch_reset([r], blocks, epoch, opts, many=False)
        recycle_s = time.time() - t3                              # (counted as evaluation: it reads the evaluation paths)
        if fused_loop:
            trainer.train_loop(buf, n_train, batch_size=ak["batch_size"])
        else:
            for _ in range(n_train):
                trainer.train(buf.random_batch(ak["batch_size"]))
        t4 = time.time()
        row = _end_epoch_row(r, blocks[0], epoch)
        t5 = time.time()
        if checkpoint_dir:
            save_checkpoint(checkpoint_dir, trainer, buf, dict(_pack_extra(r, epoch), np_random=_rs_pack(np.random)))
        t6 = time.time()
        _stamp_times(row, epoch, storing=t3 - t2, evaluation=t1 - t0 + recycle_s, exploration=t2 - t1, logging=t5 - t4,
                     saving=t6 - t5, training=t4 - t3 - recycle_s, epoch_s=t6 - t0, total=t6 - t_start)
        _log_row(r, row, log_dir, first_epoch)
        if not quiet:
            print(f"epoch {epoch}: buffer {row['replay_buffer/size']}  QF1 {row['trainer/QF1 Loss']:.4f}  "
                  f"policy loss {row['trainer/Policy Loss']:.4f}  training {row['time/training (s)']:.3f}s "
                  f"({n_train / max(row['time/training (s)'], 1e-9):.0f} steps/s)", flush=True)
    if r["fh"]:
        r["fh"].close()
    return r["rows"]


def _group_run(variant, seed, O, A, device, prefill=True, acting="host"):
    """One run of a grouped experiment, set up as experiment(variant, seed=seed) sets it up (_build_run), but for the
    generators: the weights come from a private RandomState(seed), in the order experiment() draws them from np.random,
    and the replay buffer samples a private stream continued from that generator.  Prefilled unless the run is about to
    be restored from a checkpoint (the prefill is this run's alone: its get_action calls)."""
    rs = np.random.RandomState(seed)                          # experiment(): np.random.seed(seed), then the weights
    r = _build_run(variant, seed, O, A, device, acting, rs)
    r["buf"].seed_from_numpy(rs)                              # (the stream np.random would continue with)
    if prefill:
        _prefill(r)
    return r


def _group_checkpoint(runs, checkpoint_dir, restore, chunk_rows):
    """The group checkpoint of a grouped experiment (None without checkpoint_dir) and the first epoch to run.  With
    restore (resume=True and a checkpoint in checkpoint_dir), every run is restored from it -- trainer, buffer, host generators and
    collector totals -- and continues after the saved epoch; the live group must be the saved one (same members in the
    same order), which the loader checks before it touches any state."""
    if not checkpoint_dir:
        return None, 0
    ck = GroupCheckpoint(checkpoint_dir, chunk_rows)
    for r in runs:
        r["identity"] = member_identity(r["sub"], r["seed"], r["variant"], r["trainer"])
    if not restore:
        return ck, 0
    extras = ck.load([r["trainer"] for r in runs], [r["buf"] for r in runs], [r["identity"] for r in runs])
    first_epochs = [_restore_extra(r, extra) for r, extra in zip(runs, extras)]
    return ck, first_epochs[0]                                # (one generation: every run saved the same epoch)


def _group_epochs(*, runs, train_block, n_epochs, n_train, log_dir, quiet, what, opts, acting, sessions, general_sessions,
                  ck, first_epoch):
    """The epoch loop of a grouped experiment: each run collects its paths, then train_block() trains every run at once,
    then every run ends its epoch, the group is saved (with a GroupCheckpoint `ck`: one generation for the whole group,
    and the epoch ends behind the save), and each run writes its row (to <log_dir>/<run["sub"]>/progress.csv with
    log_dir; appended to after a resume).
    acting="host": the runs collect one after the other -- evaluation paths, exploration paths, add_paths each.  The
    replay evaluation of all runs stands in front of them all (each buffer as the run's own experiment() sees it there),
    Q bias, validation and the unit statistics of all runs behind them all (nobody has trained since the first run's
    evaluation paths).  The
    seconds of these calls are added to every run's time/evaluation sampling (s); the replay evaluation's also to its
    time/epoch (s), the run's start taken that much earlier: a row's phases stay inside its epoch.
    acting="device": the runs collect in lockstep (GroupPathCollector) -- the evaluation phase of all runs, the
    evaluations of `opts` (EvalOptions) in experiment()'s order, then the exploration phase of all runs, every tick's
    actions from one act_many call (sessions=True: from one acting-session call, GroupActor, one session for each
    phase's collectors; the rows are the same); each run's time/*sampling (s) columns then hold the shared phase time.
    acting="device_all": the same, and the lockstep collectors send the runs of the general step to the device as well
    (general="device"; with sessions=True, general_sessions says whether they get acting sessions of their own, None:
    GroupActor's default -- the rows are the same either way)."""
    t_start = time.time()
    lockstep = acting != "host"
    lock_kw = dict(sessions=sessions, general="device" if acting == "device_all" else "host", general_sessions=general_sessions)
    lock_eval = GroupPathCollector([r["evalc"] for r in runs], **lock_kw) if lockstep else None
    lock_expl = GroupPathCollector([r["expl"] for r in runs], **lock_kw) if lockstep else None
    try:
        for epoch in range(first_epoch, n_epochs):
            times = []                                        # per run: (start, evaluation s, exploration s, storing s)
            if lockstep:
                t0 = time.time()
                lock_eval.collect_new_paths([(r["ak"]["eval_max_path_length"], r["ak"]["num_eval_steps_per_epoch"], True)
                                             for r in runs])
                blocks, _ = _epoch_evaluations(runs, epoch, opts)
                t1 = time.time()
                new = lock_expl.collect_new_paths([(r["ak"]["expl_max_path_length"],
                                                    r["ak"]["num_expl_steps_per_train_loop"], False) for r in runs])
                t2 = time.time()
                for r, new_paths in zip(runs, new):
                    s0 = time.time()
                    r["buf"].add_paths(new_paths)
                    times.append((t0, t1 - t0, t2 - t1, time.time() - s0))
            else:
                blocks, r_s = _epoch_evaluations(runs, epoch, opts, take=("replay",))
                for r in runs:
                    ak = r["ak"]
                    t0 = time.time()
                    r["evalc"].collect_new_paths(ak["eval_max_path_length"], ak["num_eval_steps_per_epoch"], True)
                    t1 = time.time()
                    new_paths = r["expl"].collect_new_paths(ak["expl_max_path_length"], ak["num_expl_steps_per_train_loop"], False)
                    t2 = time.time()
                    r["buf"].add_paths(new_paths)
                    times.append((t0 - r_s, t1 - t0 + r_s, t2 - t1, time.time() - t2))
                behind, b_s = _epoch_evaluations(runs, epoch, opts, take=("q", "validation", "units", "params"))
                for b, more in zip(blocks, behind):
                    b.update(more)
                times = [(a0, eval_s + b_s, expl_s, store_s) for a0, eval_s, expl_s, store_s in times]
            t2r = time.time()
            _epoch_recycle(runs, blocks, epoch, opts)         # (in front of the training block: ONE call pair for all runs)
            _epoch_reset(runs, blocks, epoch, opts)           # (behind it: ONE shrink_perturb_many call for all runs)
            if opts.recycle_period or opts.reset_period:
                times = [(a0, eval_s + time.time() - t2r, expl_s, store_s) for a0, eval_s, expl_s, store_s in times]
            t3 = time.time()
            train_block()
            t4 = time.time()
            ended = [(_end_epoch_row(r, b, epoch), time.time()) for r, b in zip(runs, blocks)]
            t6 = time.time()
            if ck is not None:
                ck.save([r["trainer"] for r in runs], [r["buf"] for r in runs], [r["identity"] for r in runs],
                        [_pack_extra(r, epoch) for r in runs])
            t7 = time.time()
            for r, (a0, eval_s, expl_s, store_s), (row, t5) in zip(runs, times, ended):
                t_end = t7 if ck is not None else t5
                _stamp_times(row, epoch, storing=store_s, evaluation=eval_s, exploration=expl_s, logging=t5 - t4,
                             saving=t7 - t6 if ck is not None else 0.0, training=t4 - t3,   # (the group's block)
                             epoch_s=t_end - a0, total=t_end - t_start)
                _log_row(r, row, None if log_dir is None else os.path.join(log_dir, r["sub"]), first_epoch)
            if not quiet:
                print(f"epoch {epoch}: {len(runs)} {what}, training {t4 - t3:.3f}s "
                      f"({len(runs) * n_train / max(t4 - t3, 1e-9):.0f} steps/s together)", flush=True)
    finally:
        for lock in (lock_eval, lock_expl):
            if lock is not None:
                lock.close()
        for r in runs:
            if r["fh"]:
                r["fh"].close()


def experiment_group(variant, seeds, log_dir=None, num_epochs=None, obs_dim=None, action_dim=None, device=0,
                     quiet=False, checkpoint_dir=None, resume=False, chunk_rows=DEFAULT_CHUNK_ROWS, acting="host", sessions=True,
                     general_sessions=None, q_diagnostics=False, q_general="host", validation=False,
                     eval_general="host", eval_stats="host", replay_eval=0, unit_diagnostics=False, unit_general="host",
                     param_diagnostics=False, td3_replay_eval=0, recycle_period=0, recycle_tau=0.025, reset_period=0,
                     reset_shrink=0.0, reset_perturb=1.0, td3_validation=False):
    """One configuration, several seeds, one process: each seed is the run ``experiment(variant, seed=s)`` would make --
    its own synthetic environments, collectors, weights and replay buffer -- and every epoch's training block is ONE
    SACTrainerGroup.train_loop (TD3 variants: TD3TrainerGroup; hidden sizes other than two layers of at most 256 units:
    MlpSACTrainerGroup / MlpTD3TrainerGroup) over all seeds (grouped launches; each run's result is bit for bit its solo
    one).
    Weights come from a private RandomState(s) in the order experiment() draws them from np.random, and the buffer
    samples a private stream continued from that generator (np.random is neither read nor written).  Returns
    {seed: progress rows}; with log_dir, each seed's rows also go to <log_dir>/s<seed>/progress.csv.
    checkpoint_dir: after every epoch the whole group is saved there as one generation (group_checkpoint.py: each
    buffer in chunks of `chunk_rows` rows, only the chunks changed since the last save rewritten; `time/saving (s)`).
    resume=True continues the group saved in checkpoint_dir after its last saved epoch, bit for bit, appending to each
    seed's progress.csv; the seeds must be the saved ones in the saved order.  Without a checkpoint there it starts
    afresh.
    acting: "host" (the default: every run collects its own paths, one sac_policy_act call per step) or "device": the
    runs collect in lockstep (GroupPathCollector), every tick's actions of all runs from ONE launch on the live weights
    (sessions=True, the default: one acting-session call, group.GroupActor; False: one sac_policy_act_many call, the
    slower path kept for measuring against -- same rows); each run's rows are those of
    experiment(variant, seed=s, acting="device").  "device_all": the same, with the runs of the general step acting on the
    device too (one sac_policy_act_general_many call per tick and 16 of them; with sessions and general_sessions=True one
    sac_gactor_act call, None: GroupActor's default); rows as experiment(..., acting="device_all").
    q_diagnostics, q_general, validation, eval_general, eval_stats, replay_eval, unit_diagnostics, unit_general,
    param_diagnostics, td3_replay_eval, td3_validation: the
    per-epoch evaluations, EvalOptions; each seed's rows are those of experiment(variant, seed=s) with the same options."""
    opts = _options("experiment_group", [(variant,)], acting, q_diagnostics, q_general, validation, eval_general,
                    eval_stats, replay_eval, unit_diagnostics, unit_general, param_diagnostics, td3_replay_eval,
                    recycle_period, recycle_tau, reset_period, reset_shrink, reset_perturb, td3_validation)
    if resume and not checkpoint_dir:
        raise RuntimeError("experiment_group(resume=True) needs the checkpoint_dir to resume from")
    validate(variant)
    td3 = variant.get("algorithm", "SAC") == "TD3"
    seeds = [int(s) for s in seeds]
    if not seeds or len(set(seeds)) != len(seeds):
        raise RuntimeError(f"experiment_group needs distinct seeds (got {seeds})")
    O, A = env_dims(variant["expl_environment_kwargs"], obs_dim, action_dim)
    ak = variant["algorithm_kwargs"]
    runs = []
    restoring = bool(resume) and _checkpoint_exists(checkpoint_dir)
    for seed in seeds:
        runs.append(_group_run(variant, seed, O, A, device, prefill=not restoring, acting=acting))
        runs[-1]["sub"] = f"s{seed}"
    ck, first_epoch = _group_checkpoint(runs, checkpoint_dir, restoring, chunk_rows)
    n_train = ak["num_trains_per_train_loop"]
    if runs_general_step(runs[0]["trainer"]):                 # (hidden sizes of the general step: an MLP group)
        group = (MlpTD3TrainerGroup if td3 else MlpSACTrainerGroup)([r["trainer"] for r in runs])
        batches = [ak["batch_size"]] * len(runs)
        train_block = lambda: group.train_loop([r["buf"] for r in runs], n_train, batch_sizes=batches)  # noqa: E731
    else:
        group = (TD3TrainerGroup if td3 else SACTrainerGroup)([r["trainer"] for r in runs])
        train_block = lambda: group.train_loop([r["buf"] for r in runs], n_train, batch_size=ak["batch_size"])  # noqa: E731
    _group_epochs(runs=runs, train_block=train_block, n_epochs=num_epochs if num_epochs is not None else ak["num_epochs"],
                  n_train=n_train, log_dir=log_dir, quiet=quiet, what="seeds", opts=opts, acting=acting, sessions=sessions,
                  general_sessions=general_sessions, ck=ck, first_epoch=first_epoch)
    return {r["seed"]: r["rows"] for r in runs}


def task_label(variant):
    """The task of a variant as a directory name: <env_name>-<robots>, e.g. Lift-Panda, TwoArmLift-PandaPanda."""
    env = variant["expl_environment_kwargs"]
    robots = env["robots"]
    robots = [robots] if isinstance(robots, str) else list(robots)
    return f"{env['env_name']}-{''.join(robots)}"


def hidden_label(variant):
    """The hidden sizes of a variant as a name part: h512x512, or p<policy>-q<qf> when the two differ
    (p256x256-q512x512x512)."""
    hp, hq = ("x".join(str(int(h)) for h in variant[kw]["hidden_sizes"]) for kw in ("policy_kwargs", "qf_kwargs"))
    return f"h{hp}" if hp == hq else f"p{hp}-q{hq}"


def sweep_label(variant, seed, hidden_sweep=False):
    """A sweep run's name (its log directory): <task>-s<seed>, or <task>-<hidden sizes>-s<seed> in a hidden-size sweep
    (Lift-Panda-h512x512-s1)."""
    return f"{task_label(variant)}-{hidden_label(variant)}-s{seed}" if hidden_sweep else f"{task_label(variant)}-s{seed}"


def experiment_sweep(runs, log_dir=None, num_epochs=None, device=0, quiet=False, checkpoint_dir=None, resume=False,
                     chunk_rows=DEFAULT_CHUNK_ROWS, hidden_sweep=False, acting="host", sessions=True, general_sessions=None,
                     q_diagnostics=False, q_general="host", validation=False,
                     eval_general="host", eval_stats="host", replay_eval=0, unit_diagnostics=False, unit_general="host",
                     param_diagnostics=False, td3_replay_eval=0, recycle_period=0, recycle_tau=0.025, reset_period=0,
                     reset_shrink=0.0, reset_perturb=1.0, td3_validation=False):
    """Several tasks x seeds, one process, one device: every entry of ``runs`` -- (variant, seed), or (variant, seed,
    obs_dim, action_dim) for a task without pinned dims -- is the run ``experiment(variant, seed=seed)`` would make, and
    every epoch's training block is ONE MixedSACTrainerGroup.train_loop (TD3 variants: MixedTD3TrainerGroup; hidden sizes
    of the general step: MlpSACTrainerGroup / MlpTD3TrainerGroup) over all runs, each on its own batch size (bit for bit
    its solo result).
    The runs must share the algorithm, the hidden sizes and the epoch plan (num_trains_per_train_loop, and num_epochs
    unless it is given here); dims and batch sizes may differ.  Returns the runs' progress rows, a list in the order of
    ``runs``; with log_dir, each run's rows also go to <log_dir>/<task>-s<seed>/progress.csv.  checkpoint_dir, resume
    and chunk_rows as for experiment_group: one generation for every run of the sweep, and a resume needs the saved
    runs in the saved order.
    hidden_sweep=True: the runs may also differ in their policy / Q hidden sizes (a network-size sweep), the training
    block is ONE ArchSACTrainerGroup.train_loop (TD3: ArchTD3TrainerGroup), and each run's name carries its hidden
    sizes: <task>-h<sizes>-s<seed>, or <task>-p<policy sizes>-q<Q sizes>-s<seed> (sweep_label).
    acting as for experiment_group; in a hidden sweep the runs of the general step act on the host inside the same
    lockstep ticks (act_many), so each run's rows stay those of its solo experiment(..., acting="device").  Under
    "device_all" those runs act on the device inside the same ticks, and each run's rows are those of its solo
    experiment(..., acting="device_all").
    q_diagnostics, q_general, validation, eval_general, eval_stats, replay_eval, unit_diagnostics, unit_general,
    param_diagnostics, td3_replay_eval, td3_validation: the
    per-epoch evaluations, EvalOptions, as for experiment_group; in a hidden sweep the runs of the general step take the
    host path inside the same call, or
    the device's under q_general / eval_general "device".  A sweep with a TD3 run refuses validation and replay_eval."""
    opts = _options("experiment_sweep", runs, acting, q_diagnostics, q_general, validation, eval_general, eval_stats,
                    replay_eval, unit_diagnostics, unit_general, param_diagnostics, td3_replay_eval,
                    recycle_period, recycle_tau, reset_period, reset_shrink, reset_perturb, td3_validation)
    if resume and not checkpoint_dir:
        raise RuntimeError("experiment_sweep(resume=True) needs the checkpoint_dir to resume from")
    specs = []
    for spec in runs:
        spec = tuple(spec)
        if len(spec) not in (2, 4):
            raise RuntimeError(f"a sweep run is (variant, seed) or (variant, seed, obs_dim, action_dim), got {len(spec)} items")
        v, seed = spec[0], int(spec[1])
        validate(v)
        O, A = env_dims(v["expl_environment_kwargs"], *(spec[2:] if len(spec) == 4 else (None, None)))
        specs.append((v, seed, O, A))
    if not specs:
        raise RuntimeError("experiment_sweep needs at least one run")
    v0 = specs[0][0]
    algo0, ak0 = v0.get("algorithm", "SAC"), v0["algorithm_kwargs"]
    labels = set()
    for i, (v, seed, _, _) in enumerate(specs):
        ak = v["algorithm_kwargs"]
        if v.get("algorithm", "SAC") != algo0:
            raise RuntimeError(f"sweep run {i} is {v.get('algorithm', 'SAC')}, run 0 {algo0}: a sweep runs one algorithm")
        for kw in ("policy_kwargs", "qf_kwargs") if not hidden_sweep else ():
            if list(v[kw]["hidden_sizes"]) != list(v0[kw]["hidden_sizes"]):
                raise RuntimeError(f"sweep run {i} has {kw} hidden sizes {v[kw]['hidden_sizes']}, run 0 "
                                   f"{v0[kw]['hidden_sizes']}")
        plan = ("num_trains_per_train_loop",) + (("num_epochs",) if num_epochs is None else ())
        for k in plan:
            if ak[k] != ak0[k]:
                raise RuntimeError(f"sweep run {i} has {k} {ak[k]}, run 0 {ak0[k]}: a sweep runs one epoch plan")
        label = sweep_label(v, seed, hidden_sweep)
        if label in labels:
            raise RuntimeError(f"sweep run {i} repeats {label}")
        labels.add(label)
    group_runs = []
    restoring = bool(resume) and _checkpoint_exists(checkpoint_dir)
    for v, seed, O, A in specs:
        group_runs.append(_group_run(v, seed, O, A, device, prefill=not restoring, acting=acting))
        group_runs[-1]["sub"] = sweep_label(v, seed, hidden_sweep)
    ck, first_epoch = _group_checkpoint(group_runs, checkpoint_dir, restoring, chunk_rows)
    td3 = algo0 == "TD3"
    if hidden_sweep:                                          # (any hidden sizes: an arch group)
        group = (ArchTD3TrainerGroup if td3 else ArchSACTrainerGroup)([r["trainer"] for r in group_runs])
    elif runs_general_step(group_runs[0]["trainer"]):         # (hidden sizes of the general step: an MLP group)
        group = (MlpTD3TrainerGroup if td3 else MlpSACTrainerGroup)([r["trainer"] for r in group_runs])
    else:
        group = (MixedTD3TrainerGroup if td3 else MixedSACTrainerGroup)([r["trainer"] for r in group_runs])
    n_train = ak0["num_trains_per_train_loop"]
    batches = [r["ak"]["batch_size"] for r in group_runs]
    _group_epochs(runs=group_runs, n_epochs=num_epochs if num_epochs is not None else ak0["num_epochs"], n_train=n_train,
                  train_block=lambda: group.train_loop([r["buf"] for r in group_runs], n_train, batch_sizes=batches),
                  log_dir=log_dir, quiet=quiet, what="runs", opts=opts, acting=acting, sessions=sessions,
                  general_sessions=general_sessions, ck=ck, first_epoch=first_epoch)
    return [r["rows"] for r in group_runs]
