"""Host side of acting sessions (no GPU): GroupPathCollector(..., sessions=True) against the default path, with a NumPy
stand-in for group.GroupActor (injected through `actor=`, as act_many is injected).  The envs and holders are those of
tests/test_device_acting_host.py; holders bound to a FakeTrainer go through the session (or through act_many on the
default path), the others keep their NumPy forward on both."""
import pickle

import numpy as np
import pytest

from robosuite_benchmark_amd import MakeDeterministic, PolicyWrappedWithExplorationStrategy, TanhGaussianPolicy
from robosuite_benchmark_amd.driver import GroupPathCollector, PathCollector, SyntheticEnv
from tests.test_device_acting_host import SPECS, EndingEnv, FakeTrainer, assert_same_paths, member


def forward(policy, obs32, deterministic, eps):
    """The holder's own NumPy forward on float32 observations (what a trainer handle would compute on the device)."""
    if isinstance(policy, TanhGaussianPolicy):
        mean, log_std = policy._trunk(obs32)
        return np.tanh(mean) if deterministic else np.tanh(mean + np.exp(log_std) * eps)
    h, names = obs32, list(policy.layers)
    for n in names[:-1]:
        w, b = policy.layers[n]
        h = np.maximum(h @ w.T + b, 0)
    w, b = policy.layers[names[-1]]
    return np.tanh(h @ w.T + b)


def numpy_act_many(trainers, obs_list, deterministic_list, eps_list):
    return [forward(t.policy, np.asarray(o, np.float32), det, eps).astype(np.float32)
            for t, o, det, eps in zip(trainers, obs_list, deterministic_list, eps_list)]


class _Rows(list):
    """One name for the action arrays and the tick, as on GroupActor: act[k] and act(n_rows, deterministic)."""

    def __call__(self, n_rows, deterministic):
        return self.tick(n_rows, deterministic)


class NumpyActor:
    """group.GroupActor's interface on ordinary arrays: obs float64, eps / act float32, act(n_rows, deterministic)."""
    made = []

    def __init__(self, trainers, max_rows=1):
        self.trainers, self.closed, self.ticks = list(trainers), False, []
        self.obs = [np.full((max_rows, t.policy.obs_dim), np.nan, np.float64) for t in self.trainers]
        self.eps = [np.full((max_rows, t.act_dim), np.nan, np.float32) for t in self.trainers]
        self.act = _Rows(np.full((max_rows, t.act_dim), np.nan, np.float32) for t in self.trainers)
        self.act.tick = self.tick
        NumpyActor.made.append(self)

    def tick(self, n_rows, deterministic):
        assert not self.closed and len(n_rows) == len(deterministic) == len(self.trainers) and any(n_rows)
        self.ticks.append(list(n_rows))
        for k, (t, n) in enumerate(zip(self.trainers, n_rows)):
            if n:
                stochastic = isinstance(t.policy, TanhGaussianPolicy) and not deterministic[k]
                assert np.all(np.isfinite(self.obs[k][:n])) and (not stochastic or np.all(np.isfinite(self.eps[k][:n])))
                self.act[k][:n] = forward(t.policy, self.obs[k][:n].astype(np.float32), deterministic[k], self.eps[k][:n])

    def close(self):
        self.closed = True


numpy_actor = NumpyActor


def holder_of(policy):
    if isinstance(policy, MakeDeterministic):
        return policy.stochastic_policy
    return policy.policy if isinstance(policy, PolicyWrappedWithExplorationStrategy) else policy


def collectors(bind):
    """PathCollectors of SPECS; the members in `bind` get a FakeTrainer (a handle), the others act on their own."""
    out = []
    for i, (k, s, O, A, env, _) in enumerate(SPECS):
        e, p = member(k, s, O, A, env)
        if i in bind:
            FakeTrainer(holder_of(p))
        out.append(PathCollector(e, p))
    return out


def rng_states(cs):
    out = []
    for c in cs:
        h = holder_of(c.policy)
        rs = [c.env._rs] + ([h._noise] if hasattr(h, "_noise") else [])
        if isinstance(c.policy, PolicyWrappedWithExplorationStrategy):
            rs.append(c.policy.es._rs)
        out.append([r.get_state() for r in rs])
    return out


def same_states(a, b):
    return all(x[0] == y[0] and np.array_equal(x[1], y[1]) and x[2:] == y[2:] for sa, sb in zip(a, b) for x, y in zip(sa, sb))


BIND = (0, 1, 3, 4, 5, 6)                    # member 2 stays unbound: its NumPy forward, inside the same ticks


def test_session_collector_equals_the_default_collector():
    NumpyActor.made.clear()
    plans = [plan for *_, plan in SPECS]
    base, sess = collectors(BIND), collectors(BIND)
    g0 = GroupPathCollector(base, act_many=numpy_act_many)
    g1 = GroupPathCollector(sess, sessions=True, actor=numpy_actor)
    for rnd in range(3):                                                  # (three phases: the counters accumulate)
        want, got = g0.collect_new_paths(plans), g1.collect_new_paths(plans)
        for i, (c, l) in enumerate(zip(base, sess)):
            assert_same_paths(got[i], want[i], (rnd, i))
            assert_same_paths(l.epoch_paths, c.epoch_paths, (rnd, i, "epoch_paths"))
            assert l.get_diagnostics() == c.get_diagnostics(), (rnd, i)
        assert same_states(rng_states(base), rng_states(sess)), rnd
    assert len(NumpyActor.made) == 1                                      # built at the first collect, then kept
    assert [t.policy for t in NumpyActor.made[0].trainers] == [holder_of(sess[i].policy) for i in BIND]
    assert sum(len(p) for p in want) > 0 and len({len(p) for p in want}) > 1
    g1.close()
    assert NumpyActor.made[0].closed
    # the default (sessions=False) never builds an actor, with or without an injected act_many
    GroupPathCollector(collectors(BIND), act_many=numpy_act_many, actor=numpy_actor).collect_new_paths(plans)
    assert len(NumpyActor.made) == 1
    with pytest.raises(RuntimeError, match="one plan per collector"):
        g1.collect_new_paths(plans[:1])


def test_only_live_members_have_rows_on_every_tick():
    """Members finish at different ticks; member 1 ends under discard_incomplete_paths (its last, one-step path is taken
    and dropped).  The row counts of every tick are exactly the members still collecting."""
    NumpyActor.made.clear()
    specs = [("expl", 1, 11, 3, SyntheticEnv), ("eval", 2, 7, 2, SyntheticEnv), ("td3", 5, 6, 2, SyntheticEnv),
             ("expl", 3, 5, 4, EndingEnv)]
    plans = [(10, 25, False), (10, 31, True), (10, 18, False), (12, 40, False)]
    pairs = [member(*s) for s in specs]
    for _, p in pairs[:3]:                                                # member 3 is unbound
        FakeTrainer(holder_of(p))
    lock = [PathCollector(e, p) for e, p in pairs]
    got = GroupPathCollector(lock, sessions=True, actor=numpy_actor).collect_new_paths(plans)
    for i, (s, plan) in enumerate(zip(specs, plans)):
        assert_same_paths(got[i], PathCollector(*member(*s)).collect_new_paths(*plan), i)
    ticks = NumpyActor.made[0].ticks
    assert len(NumpyActor.made[0].trainers) == 3 and len(ticks) == 31
    for tk, rows in enumerate(ticks):
        assert rows == [int(tk < 25), 1, int(tk < 18)], (tk, rows)
    assert sum(len(p["actions"]) for p in got[1]) == 30 and lock[1].num_steps_total == 30


def test_paths_hold_no_views_of_the_staging():
    NumpyActor.made.clear()
    plans = [plan for *_, plan in SPECS]
    sess = collectors(BIND)
    got = GroupPathCollector(sess, sessions=True, actor=numpy_actor).collect_new_paths(plans)
    frozen = pickle.loads(pickle.dumps(got))
    actor = NumpyActor.made[0]
    staging = actor.obs + actor.eps + list(actor.act)
    for paths in got:
        for p in paths:
            for k in ("observations", "actions", "next_observations"):
                assert p[k].flags["OWNDATA"] and not any(np.shares_memory(p[k], s) for s in staging), k
    for s in staging:                                                     # the next tick would overwrite these
        s[...] = 123.0
    for i, (g, f) in enumerate(zip(got, frozen)):
        assert_same_paths(g, f, i)
    assert_same_paths(sess[0].epoch_paths, frozen[0], "epoch_paths")
