"""The driver's epoch loops end to end over recording stand-ins, without a library: what experiment(), experiment_group()
and experiment_sweep() call per epoch and in which order (solo, sequential group, lockstep group), that every run's rows
are its solo rows, where the optional column blocks stand, which keywords the evaluation calls get, that a row's phases
lie inside its epoch, and that a resumed run continues the straight one.

The stand-in trainers have no handle, so the policies act through their own NumPy forward -- in the collectors' own
get_action calls and in the lockstep collectors alike -- and the real collectors, environments, noise streams and row
code run.  Every stand-in appends to one call log."""
import copy
import csv
import json
import math
import os
from collections import OrderedDict

import numpy as np
import pytest

from robosuite_benchmark_amd import driver
from robosuite_benchmark_amd.variant import default_variant

O, A, SEEDS, EPOCHS = 7, 3, (3, 4), 2
ALL_ON = dict(q_diagnostics=True, q_general="device", validation=True, eval_general="device", eval_stats="device",
              replay_eval=16)
LOG = []                                                          # (name, run's seed or None, keywords of the call)


def variant(prefill=25):
    v = default_variant()
    v["algorithm_kwargs"].update(num_epochs=EPOCHS, num_eval_steps_per_epoch=40, num_expl_steps_per_train_loop=30,
                                 eval_max_path_length=20, expl_max_path_length=20, min_num_steps_before_training=prefill,
                                 num_trains_per_train_loop=5, batch_size=8)
    v["replay_buffer_size"] = 500
    v["eval_environment_kwargs"]["horizon"] = 501                 # (how LoggingEnv tells a run's two environments apart)
    return v


class LoggingEnv(driver.SyntheticEnv):
    """SyntheticEnv that logs the start of every path: ("eval" | "expl", the run's seed)."""

    def __init__(self, obs_dim, action_dim, horizon=500, seed=0):
        super().__init__(obs_dim, action_dim, horizon, seed)
        self.kind, self.run_seed = ("eval", seed - 1) if horizon == 501 else ("expl", seed)

    def reset(self):
        LOG.append((self.kind, self.run_seed, {}))
        return super().reset()


class FakeTrainer:
    """SACTrainer's face towards the driver, without a handle: the policy holder stays unbound and acts by itself."""
    made = []

    def __init__(self, env, policy, qf1, qf2, target_qf1, target_qf2, batch_size, noise_seed, device, discount=0.99,
                 reward_scale=1.0, **kw):
        self.policy, self.seed, self._h, self._batch, self.steps = policy, noise_seed, None, batch_size, 0
        self.obs_dim, self.act_dim, self.discount, self.reward_scale = policy.obs_dim, policy.action_dim, discount, reward_scale
        self.init_sums = [float(np.sum(n.flat(), dtype=np.float64)) for n in (qf1, qf2, target_qf1, target_qf2, policy)]
        FakeTrainer.made.append(self)

    def _hidden(self, name="policy"):
        return (256, 256)

    def _train(self, buf, n):                                     # (a deterministic function of the weights and the buffer)
        p = self.policy.flat()
        self.policy.load_flat(p * np.float32(0.999) + np.float32(1e-3) * np.sin(np.arange(p.size, dtype=np.float32))
                              + np.float32(1e-6 * buf.num_steps_can_sample()))
        self.steps += n

    def train_loop(self, buf, n, batch_size=None):
        LOG.append(("train", self.seed, {}))
        self._train(buf, n)

    def get_diagnostics(self):
        p = self.policy.flat().astype(np.float64)
        return OrderedDict([("QF1 Loss", float(p.sum())), ("Policy Loss", float(np.abs(p).sum())),
                            ("Init Sum", sum(self.init_sums)), ("num train steps", self.steps)])

    def end_epoch(self, epoch):
        self.ended = epoch

    def _q(self, obs, act):
        q = np.asarray(obs, np.float64).sum(1) + np.asarray(act, np.float64).sum(1) + float(self.policy.flat()[0])
        return np.stack([q, 0.5 * q])

    def _evaluate(self, batch, eps):
        x = sum(float(np.sum(batch[k], dtype=np.float64)) for k in sorted(batch))
        return OrderedDict([("QF1 Loss", x + float(eps[0].sum())), ("Policy Loss", float(eps[1].sum()) - x),
                            ("Weights", float(np.sum(self.policy.flat(), dtype=np.float64)))])

    def _evaluate_replay(self, buf, n, rng):
        idx = rng.randint(0, buf.num_steps_can_sample(), n)
        eps = rng.standard_normal((n, self.act_dim)), rng.standard_normal((n, self.act_dim))
        return self._evaluate({k: v[idx] for k, v in buf.rows().items()}, eps)

    def q_values(self, obs, act, nets=("qf1", "qf2"), **kw):
        LOG.append(("q_values", self.seed, kw))
        assert tuple(nets) == ("qf1", "qf2")
        return self._q(obs, act)

    def evaluate(self, batch, eps=None, **kw):
        LOG.append(("evaluate", self.seed, kw))
        return self._evaluate(batch, eps)

    def evaluate_replay(self, buf, n=None, rng=None, **kw):
        LOG.append(("evaluate_replay", self.seed, kw))
        return self._evaluate_replay(buf, n, rng)


class FakeBuffer:
    KEYS = ("observations", "actions", "rewards", "next_observations", "terminals")

    def __init__(self, size, obs_dim, action_dim, device=0):
        self.paths, self.epoch = [], None

    def add_paths(self, paths):
        LOG.append(("add_paths", None, {}))
        self.paths.extend(paths)

    def seed_from_numpy(self, rs):
        self.stream = rs.randint(0, 2 ** 31 - 1)

    def num_steps_can_sample(self):
        return sum(len(p["actions"]) for p in self.paths)

    def rows(self):
        return {k: np.concatenate([np.asarray(p[k], np.float64) for p in self.paths]) for k in self.KEYS}

    def get_diagnostics(self):
        return OrderedDict([("size", self.num_steps_can_sample())])

    def end_epoch(self, epoch):
        self.epoch = epoch


class FakeGroup:
    def __init__(self, trainers):
        self.trainers = list(trainers)

    def train_loop(self, bufs, n, batch_size=None, batch_sizes=None):
        assert (batch_size is None) != (batch_sizes is None)
        LOG.append(("train_group", None, {}))
        for t, b in zip(self.trainers, bufs):
            t._train(b, n)


def fake_q_values_many(trainers, obs, act, nets, **kw):
    LOG.append(("q_values_many", None, kw))
    assert all(tuple(n) == ("qf1", "qf2") for n in nets)
    return [t._q(o, a) for t, o, a in zip(trainers, obs, act)]


def fake_evaluate_many(trainers, batches, eps=None, **kw):
    LOG.append(("evaluate_many", None, kw))
    return [None if b is None else t._evaluate(b, e) for t, b, e in zip(trainers, batches, eps)]


def fake_evaluate_replay_many(trainers, bufs, n=None, rngs=None, **kw):
    LOG.append(("evaluate_replay_many", None, kw))
    return [None if k == 0 else t._evaluate_replay(b, k, r) for t, b, k, r in zip(trainers, bufs, n, rngs)]


class FakeStore:
    """The group checkpoint's and the solo checkpoint's stand-in: trainer and buffer state by directory name, and the
    `extra` dicts as JSON text (what a manifest keeps)."""
    saved = {}

    def __init__(self, dirname, chunk_rows=None):
        self.dirname = dirname

    @staticmethod
    def _state(t, b):
        return dict(flat=t.policy.flat().copy(), steps=t.steps, paths=copy.deepcopy(b.paths))

    @staticmethod
    def _restore(t, b, st):
        t.policy.load_flat(st["flat"])
        t.steps, b.paths = st["steps"], copy.deepcopy(st["paths"])

    def save(self, trainers, bufs, identities, extras):
        LOG.append(("save", None, {}))
        FakeStore.saved[self.dirname] = ([self._state(t, b) for t, b in zip(trainers, bufs)], json.dumps(extras),
                                         json.dumps(identities))

    def load(self, trainers, bufs, identities):
        states, extras, saved_ids = FakeStore.saved[self.dirname]
        assert json.loads(saved_ids) == json.loads(json.dumps(identities))
        for t, b, st in zip(trainers, bufs, states):
            self._restore(t, b, st)
        return json.loads(extras)


def fake_save_checkpoint(dirname, trainer, buf, extra):
    FakeStore(dirname).save([trainer], [buf], [None], [extra])


def fake_load_checkpoint(dirname, trainer, buf):
    return FakeStore(dirname).load([trainer], [buf], [None])[0]


@pytest.fixture(autouse=True)
def stand_ins(monkeypatch):
    for name, fake in dict(SACTrainer=FakeTrainer, EnvReplayBuffer=FakeBuffer, SACTrainerGroup=FakeGroup,
                           MixedSACTrainerGroup=FakeGroup, q_values_many=fake_q_values_many,
                           evaluate_many=fake_evaluate_many, evaluate_replay_many=fake_evaluate_replay_many,
                           SyntheticEnv=LoggingEnv, GroupCheckpoint=FakeStore, save_checkpoint=fake_save_checkpoint,
                           load_checkpoint=fake_load_checkpoint, checkpoint_exists=lambda d: d in FakeStore.saved,
                           _checkpoint_exists=lambda d: d in FakeStore.saved).items():
        assert hasattr(driver, name), name
        monkeypatch.setattr(driver, name, fake)
    FakeStore.saved.clear()
    del LOG[:], FakeTrainer.made[:]


# ---- the runs ---------------------------------------------------------------------------------------------------------
def solo(seed, v=None, **kw):
    return driver.experiment(copy.deepcopy(v or variant()), seed=seed, obs_dim=O, action_dim=A, quiet=True,
                             **{**dict(num_epochs=EPOCHS), **kw})


def group(v=None, **kw):
    return driver.experiment_group(copy.deepcopy(v or variant()), SEEDS, obs_dim=O, action_dim=A, quiet=True,
                                   **{**dict(num_epochs=EPOCHS), **kw})


def sweep(v=None, **kw):
    rows = driver.experiment_sweep([(copy.deepcopy(v or variant()), s, O, A) for s in SEEDS], quiet=True,
                                   **{**dict(num_epochs=EPOCHS), **kw})
    return dict(zip(SEEDS, rows))


def logged(fn, *a, **kw):
    del LOG[:]
    got = fn(*a, **kw)
    return got, list(LOG)


def calls(log, by_seed=True):
    """The log's names in order, a path's start as ("eval" | "expl", seed) (by_seed) or "eval" | "expl", and a phase's
    consecutive starts as one entry."""
    out = []
    for name, seed, _ in log:
        tok = ((name, seed) if by_seed else name) if name in ("eval", "expl") else name
        if not (out and out[-1] == tok and name in ("eval", "expl")):
            out.append(tok)
    return out


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def assert_rows_equal(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert list(g.keys()) == list(w.keys()), what
        for k in w:
            assert k.startswith("time/") or same(g[k], w[k]), (what, k, g[k], w[k])


def assert_times(rows, what):
    for row in rows:
        t = {k: v for k, v in row.items() if k.startswith("time/")}
        assert list(t) == ["time/" + k + " (s)" for k in ("data storing", "evaluation sampling", "exploration sampling",
                                                           "logging", "saving", "training", "epoch", "total")], what
        assert list(row)[-1] == "Epoch" and list(row)[-9:-1] == list(t), what
        assert all(v >= 0 for v in t.values()), (what, t)
        phases = sum(t["time/" + k + " (s)"] for k in ("evaluation sampling", "exploration sampling", "data storing", "training"))
        assert phases <= t["time/epoch (s)"] + 1e-9, (what, t)     # (1e-9 s: the rounding of a handful of float64 sums)


@pytest.fixture
def solo_rows():
    """The solo runs of both seeds with every option on: the rows every grouped run has to give."""
    return {s: solo(s, **ALL_ON) for s in SEEDS}


# ---- call order -------------------------------------------------------------------------------------------------------
def test_solo_call_order():
    _, log = logged(solo, 3, **ALL_ON)
    epoch = [("eval", 3), "q_values", "evaluate", "evaluate_replay", ("expl", 3), "add_paths", "train"]
    assert calls(log) == [("expl", 3), "add_paths"] + epoch * EPOCHS
    _, log = logged(solo, 3)
    assert calls(log) == [("expl", 3), "add_paths"] + [("eval", 3), ("expl", 3), "add_paths", "train"] * EPOCHS


@pytest.mark.parametrize("entry", [group, sweep])
def test_sequential_group_call_order(entry):
    _, log = logged(entry, acting="host", **ALL_ON)
    prefill = [tok for s in SEEDS for tok in (("expl", s), "add_paths")]
    epoch = (["evaluate_replay_many"] + [tok for s in SEEDS for tok in (("eval", s), ("expl", s), "add_paths")]
             + ["q_values_many", "evaluate_many", "train_group"])
    assert calls(log) == prefill + epoch * EPOCHS
    _, log = logged(entry, acting="host")
    assert calls(log) == prefill + ([tok for s in SEEDS for tok in (("eval", s), ("expl", s), "add_paths")]
                                    + ["train_group"]) * EPOCHS


@pytest.mark.parametrize("sessions", [False, True])
@pytest.mark.parametrize("entry", [group, sweep])
def test_lockstep_call_order(entry, sessions):
    _, log = logged(entry, acting="device", sessions=sessions, **ALL_ON)
    prefill = ["expl", "add_paths"] * len(SEEDS)
    epoch = (["eval", "q_values_many", "evaluate_many", "evaluate_replay_many", "expl"] + ["add_paths"] * len(SEEDS)
             + ["train_group"])
    assert calls(log, by_seed=False) == prefill + epoch * EPOCHS
    # within a phase the runs' paths start tick by tick, side by side: both runs' first paths before anyone's second
    starts = [(n, s) for n, s, _ in log if n == "eval"][:2 * len(SEEDS)]
    assert starts == [("eval", s) for s in SEEDS] * 2


def test_replay_evaluation_is_skipped_while_every_buffer_is_empty():
    v = variant(prefill=0)
    want = {s: solo(s, v, replay_eval=16) for s in SEEDS}
    for s in SEEDS:
        assert want[s][0]["replay/Num Transitions"] == 0 and want[s][1]["replay/Num Transitions"] == 16
        assert math.isnan(want[s][0]["replay/QF1 Loss"]) and math.isfinite(want[s][1]["replay/QF1 Loss"])
    _, log = logged(solo, 3, v, replay_eval=16)
    assert calls(log).count("evaluate_replay") == EPOCHS - 1
    for acting in ("host", "device"):
        got, log = logged(group, v, acting=acting, replay_eval=16)
        assert calls(log).count("evaluate_replay_many") == EPOCHS - 1
        for s in SEEDS:
            assert_rows_equal(got[s], want[s], (acting, s))


# ---- rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,kw", [(group, dict(acting="host")), (sweep, dict(acting="host")),
                                      (group, dict(acting="device", sessions=False)),
                                      (group, dict(acting="device", sessions=True)),
                                      (sweep, dict(acting="device", sessions=True))])
def test_rows_match_the_solo_run(entry, kw, solo_rows):
    got = entry(**kw, **ALL_ON)
    for s in SEEDS:
        assert len(got[s]) == EPOCHS
        assert_rows_equal(got[s], solo_rows[s], (entry.__name__, kw, s))
        assert_times(got[s], (entry.__name__, kw, s))
    assert solo_rows[3][0]["trainer/QF1 Loss"] != solo_rows[4][0]["trainer/QF1 Loss"]
    assert solo_rows[3][0]["trainer/QF1 Loss"] != solo_rows[3][1]["trainer/QF1 Loss"]


def test_weights_are_drawn_in_one_order():
    """qf1, qf2, target_qf1, target_qf2, then the policy: from np.random (solo) and from RandomState(seed) (group)."""
    solo(3)
    group()
    a, b = FakeTrainer.made[0], FakeTrainer.made[1]
    assert a.seed == b.seed == 3 and a.init_sums == b.init_sums
    from robosuite_benchmark_amd.networks import FlattenMlp, TanhGaussianPolicy
    rs = np.random.RandomState(3)
    hs = dict(hidden_sizes=[256, 256])
    nets = [FlattenMlp(input_size=O + A, output_size=1, rs=rs, **hs) for _ in range(4)]
    nets.append(TanhGaussianPolicy(obs_dim=O, action_dim=A, rs=rs, **hs))
    assert a.init_sums == [float(np.sum(n.flat(), dtype=np.float64)) for n in nets]


def test_column_placement(solo_rows):
    on = list(solo_rows[3][0].keys())
    off = list(solo(3)[0].keys())
    at = off.index("time/data storing (s)")
    extra = [k for k in on if k not in off]
    assert on == off[:at] + extra + off[at:]                      # (directly in front of time/data storing (s))
    assert not any(k.startswith(("validation/", "replay/", "evaluation/Q")) for k in off)
    q, v, r = extra[:16], [k for k in extra if k.startswith("validation/")], [k for k in extra if k.startswith("replay/")]
    assert extra == q + v + r                                     # (Q bias, validation, replay)
    assert q == [f"evaluation/{n} {s}" for n in ("Q1 Estimates", "Q2 Estimates", "Returns To Go", "Q Bias")
                 for s in ("Mean", "Std", "Max", "Min")]
    stats = ["QF1 Loss", "Policy Loss", "Weights", "Num Transitions"]
    assert v == ["validation/" + k for k in stats] and r == ["replay/" + k for k in stats]
    for row in solo_rows[3]:
        assert row["validation/Num Transitions"] == 40 and row["replay/Num Transitions"] == 16
    # each block alone stands at the same place
    for kw, block in ((dict(q_diagnostics=True), q), (dict(validation=True), v), (dict(replay_eval=16), r)):
        assert list(solo(3, num_epochs=1, **kw)[0].keys()) == off[:at] + block + off[at:], kw
        assert list(group(num_epochs=1, **kw)[3][0].keys()) == off[:at] + block + off[at:], kw
    assert_times(solo_rows[3], "solo")


# ---- keywords ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", [solo, group, sweep])
def test_keyword_hygiene(entry):
    args = (3,) if entry is solo else ()
    q, e, r = ("q_values", "evaluate", "evaluate_replay") if entry is solo else ("q_values_many", "evaluate_many",
                                                                                 "evaluate_replay_many")
    _, log = logged(entry, *args, q_diagnostics=True, validation=True, replay_eval=16)
    kws = [(n, kw) for n, _, kw in log if n in (q, e, r)]
    assert len(kws) == 3 * EPOCHS and all(kw == {} for _, kw in kws)
    _, log = logged(entry, *args, **ALL_ON)
    kws = [(n, kw) for n, _, kw in log if n in (q, e, r)]
    assert len(kws) == 3 * EPOCHS
    for n, kw in kws:
        assert kw == (dict(general="device") if n == q else dict(general="device", stats="device")), n


# ---- resume -----------------------------------------------------------------------------------------------------------
def read_csv(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


@pytest.mark.parametrize("kw", [dict(acting="host"), dict(acting="device")])
def test_group_resume_gives_the_straight_rows(kw, tmp_path, solo_rows):
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    first, log = logged(group, num_epochs=1, log_dir=logs, checkpoint_dir=ck, **kw, **ALL_ON)
    assert calls(log)[-1] == "save"                               # (behind the epoch's rows and end_epoch calls)
    extras = json.loads(FakeStore.saved[ck][1])
    for s, extra in zip(SEEDS, extras):
        assert set(extra) == {"epoch", "seed", "expl_totals", "eval_totals", "policy_noise", "expl_env", "eval_env"}
        assert extra["epoch"] == 0 and extra["seed"] == s
        assert extra["expl_totals"] == [55, 4] and extra["eval_totals"] == [40, 2]
    resumed, log = logged(group, num_epochs=2, log_dir=logs, checkpoint_dir=ck, resume=True, **kw, **ALL_ON)
    assert calls(log, by_seed=False)[0] == ("evaluate_replay_many" if kw["acting"] == "host" else "eval")  # (no prefill)
    for s in SEEDS:
        assert_rows_equal(first[s] + resumed[s], solo_rows[s], (kw, s))
        assert resumed[s][0]["Epoch"] == 1 and resumed[s][0]["time/saving (s)"] >= 0
        lines = read_csv(os.path.join(logs, f"s{s}", "progress.csv"))
        assert len(lines) == 1 + EPOCHS and lines[0] == list(solo_rows[s][0].keys())
        assert [ln[-1] for ln in lines] == ["Epoch", "0", "1"]    # (appended to: one header)
        assert_times(first[s] + resumed[s], (kw, s))
    assert FakeTrainer.made[-1].ended == 1


def test_solo_resume_gives_the_straight_rows(tmp_path, solo_rows):
    logs, ck = str(tmp_path / "logs"), str(tmp_path / "ck")
    first = solo(3, num_epochs=1, log_dir=logs, checkpoint_dir=ck, **ALL_ON)
    extra = json.loads(FakeStore.saved[ck][1])[0]
    assert set(extra) == {"epoch", "seed", "np_random", "expl_totals", "eval_totals", "policy_noise", "expl_env", "eval_env"}
    resumed, log = logged(solo, 3, num_epochs=2, log_dir=logs, checkpoint_dir=ck, resume=True, **ALL_ON)
    assert calls(log)[0] == ("eval", 3)                           # (no prefill on a restore)
    assert_rows_equal(first + resumed, solo_rows[3], "solo")
    lines = read_csv(os.path.join(logs, "progress.csv"))
    assert len(lines) == 1 + EPOCHS and lines[0] == list(solo_rows[3][0].keys())
    assert [ln[-1] for ln in lines] == ["Epoch", "0", "1"]
    assert_times(first + resumed, "solo")
    assert first[0]["time/saving (s)"] >= 0 and solo_rows[3][0]["time/saving (s)"] >= 0


@pytest.mark.parametrize("acting", ["host", "device"])
def test_a_group_without_a_checkpoint_saves_in_no_time(acting):
    for rows in group(acting=acting, **ALL_ON).values():
        assert [row["time/saving (s)"] for row in rows] == [0.0] * EPOCHS
