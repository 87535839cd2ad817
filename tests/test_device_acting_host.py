"""Host side of device acting (no GPU): the lockstep collector against PathCollector, the acting= switch and the
command line.  The policies here are holders without a trainer: they act through their NumPy forward, and the act_many
callable is injected (or never reached, since no member has a handle)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from robosuite_benchmark_amd import (GaussianStrategy, MakeDeterministic, PolicyWrappedWithExplorationStrategy,
                                     TanhGaussianPolicy, TanhMlpPolicy)
from robosuite_benchmark_amd.driver import GroupPathCollector, PathCollector, SyntheticEnv, holder_actions
from robosuite_benchmark_amd.networks import check_acting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH_KEYS = ("observations", "actions", "rewards", "next_observations", "terminals")


class EndingEnv(SyntheticEnv):
    """A SyntheticEnv whose episodes end by themselves now and then (terminal paths shorter than the horizon)."""

    def step(self, action):
        o, r, _, info = super().step(action)
        return o, r, bool(self._rs.uniform() < 0.04), info


def member(kind, seed, O, A, env_cls=SyntheticEnv):
    """(env, collector policy) of one run, seeded: SAC exploration, SAC evaluation or TD3 exploration."""
    env = env_cls(O, A, 500, seed)
    rs = np.random.RandomState(seed)
    if kind == "td3":
        pol = TanhMlpPolicy([32, 16], A, O, rs=rs)
        return env, PolicyWrappedWithExplorationStrategy(GaussianStrategy(max_sigma=0.1, min_sigma=0.1, seed=seed), pol)
    pol = TanhGaussianPolicy([32, 16], O, A, rs=rs, noise=np.random.RandomState(seed + 100))
    return env, (MakeDeterministic(pol) if kind == "eval" else pol)


SPECS = [  # kind, seed, O, A, env, (max_path_length, num_steps, discard_incomplete_paths)
    ("expl", 1, 11, 3, SyntheticEnv, (20, 75, False)),
    ("eval", 2, 7, 2, SyntheticEnv, (20, 75, True)),
    ("expl", 3, 5, 4, EndingEnv, (30, 100, False)),
    ("eval", 4, 9, 3, EndingEnv, (25, 110, True)),
    ("td3", 5, 6, 2, SyntheticEnv, (10, 10, False)),
    ("td3", 6, 6, 2, EndingEnv, (40, 95, True)),
    ("expl", 7, 8, 1, SyntheticEnv, (50, 7, True)),              # nothing but one incomplete path: dropped
]


def assert_same_paths(got, want, where):
    assert len(got) == len(want), where
    for pg, pw in zip(got, want):
        for k in PATH_KEYS:
            assert pg[k].dtype == pw[k].dtype and pg[k].shape == pw[k].shape and np.array_equal(pg[k], pw[k]), (where, k)
        assert pg["agent_infos"] == pw["agent_infos"] and pg["env_infos"] == pw["env_infos"], where


@pytest.mark.parametrize("inject", [False, True])
def test_lockstep_collector_equals_path_collector(inject):
    solo = [PathCollector(*member(k, s, O, A, env)) for k, s, O, A, env, _ in SPECS]
    lock = [PathCollector(*member(k, s, O, A, env)) for k, s, O, A, env, _ in SPECS]
    calls = []

    def injected(trainers, obs_list, deterministic_list, eps_list):      # never reached: no member has a handle
        calls.append(len(trainers))
        raise AssertionError("holders without a trainer act on the host")

    group = GroupPathCollector(lock, act_many=injected) if inject else GroupPathCollector(lock)
    for rnd in range(3):                                                  # (three phases: the counters accumulate)
        want = [c.collect_new_paths(*plan) for c, (*_, plan) in zip(solo, SPECS)]
        got = group.collect_new_paths([plan for *_, plan in SPECS])
        for i, (c, l) in enumerate(zip(solo, lock)):
            assert_same_paths(got[i], want[i], (rnd, i))
            assert_same_paths(l.epoch_paths, c.epoch_paths, (rnd, i, "epoch_paths"))
            assert l.get_diagnostics() == c.get_diagnostics(), (rnd, i)
        if rnd == 1:
            for c in solo + lock:
                c.end_epoch(0)
    assert solo[6].num_paths_total == 0 and solo[0].num_paths_total == 12 and not calls
    assert len({len(p) for p in want}) > 1                               # members really finish at different ticks
    with pytest.raises(RuntimeError, match="one plan per collector"):
        group.collect_new_paths([SPECS[0][-1]])


class FakeTrainer:
    """A trainer look-alike with a handle: holder_actions must send its holder through act_many."""

    def __init__(self, policy):
        self.policy, self._h, self.act_dim = policy, object(), policy.action_dim
        policy._trainer = self


def test_members_with_a_handle_go_through_one_act_many_call_per_tick():
    envs_pols = [member("expl", 1, 11, 3), member("eval", 2, 7, 2), member("expl", 3, 5, 4)]
    twins = [member("expl", 1, 11, 3), member("eval", 2, 7, 2), member("expl", 3, 5, 4)]
    plans = [(10, 25, False), (10, 31, True), (10, 18, False)]
    calls = []

    def fake_act_many(trainers, obs_list, deterministic_list, eps_list):
        calls.append([t.policy for t in trainers])
        out = []
        for t, o, det, eps in zip(trainers, obs_list, deterministic_list, eps_list):
            assert o.shape == (1, t.policy.obs_dim) and (eps is None) == bool(det)
            mean, log_std = t.policy._trunk(o)
            out.append(np.tanh(mean) if det else np.tanh(mean + np.exp(log_std) * eps))
        return out

    holders = [p.stochastic_policy if isinstance(p, MakeDeterministic) else p for _, p in envs_pols]
    for h in holders[:2]:                                                 # two bound members, one without a trainer
        FakeTrainer(h)
    lock = [PathCollector(e, p) for e, p in envs_pols]
    got = GroupPathCollector(lock, act_many=fake_act_many).collect_new_paths(plans)
    for i, ((e, p), plan) in enumerate(zip(twins, plans)):
        assert_same_paths(got[i], PathCollector(e, p).collect_new_paths(*plan), i)
    # one call per tick, holding exactly the bound members still collecting: 25 ticks with member 0, 31 with member 1
    # (whose last, one-step path is taken and then dropped)
    assert len(calls) == 31 and all(holders[2] not in c for c in calls)
    assert sum(holders[0] in c for c in calls) == 25 and sum(holders[1] in c for c in calls) == 31
    # holder_actions alone: the noise of a stochastic member is drawn from its own stream, (1, A) per call
    h = member("expl", 9, 4, 2)[1]
    a = holder_actions([h], [np.zeros(4)], [False])[0]
    h2 = member("expl", 9, 4, 2)[1]
    assert np.array_equal(a, h2.get_action(np.zeros(4))[0])
    assert np.array_equal(h._noise.standard_normal(3), h2._noise.standard_normal(3))


def test_acting_values():
    assert check_acting("host") == "host" and check_acting("device") == "device"
    assert TanhGaussianPolicy([8, 8], 3, 2).acting == "host" and TanhMlpPolicy([8, 8], 2, 3).acting == "host"
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="acting"):
            check_acting(bad)
    from robosuite_benchmark_amd.driver import experiment, experiment_group, experiment_sweep
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant()
    for call in (lambda: experiment(v, acting="cuda"), lambda: experiment_group(v, [1, 2], acting="cuda"),
                 lambda: experiment_sweep([(v, 1)], acting="cuda")):
        with pytest.raises(ValueError, match="acting"):                   # refused before anything is built
            call()


def test_bindings_and_header_name_the_entry_points():
    from robosuite_benchmark_amd import _lib
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    for name in ("sac_policy_act_device", "sac_policy_act_many"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    assert _lib.ACT_MAX_ROWS == 1024


def test_train_script_names_acting():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--acting" in out and "device" in out
