"""CPU: evaluate_replay above the library -- the declarations, the defaults, the rule "exactly one of n / indices", the
draw order (indices in front of eps, never from np.random), the route of handle-less trainers and of buffers without
device storage, TD3's refusal, the replay/ columns and scripts/train.py --replay_eval."""
import ctypes as C
import importlib.util
import inspect
import os

import numpy as np
import pytest

from robosuite_benchmark_amd import FlattenMlp, TanhMlpPolicy, TD3Trainer, _lib, driver, infer
from robosuite_benchmark_amd.group import ArchSACTrainerGroup, evaluate_replay_many
from robosuite_benchmark_amd.sac import SACTrainer
from tests.eval_reference import COLUMNS, batch_dict
from tests.helpers import synth_transitions
from tests.test_evaluate_general_host import group_of
from tests.test_evaluate_host import handle_less
from tests.test_q_values_host import NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostBuffer:
    """A replay buffer without device storage (no handle): the rows as NumPy arrays, gather as EnvReplayBuffer's."""
    _h = None

    def __init__(self, size, O, A, seed=3):
        self.rows = synth_transitions(size, O, A, seed=seed, term_frac=0.2)
        self.gathered = []

    def num_steps_can_sample(self):
        return self.rows[0].shape[0]

    def gather(self, indices):
        idx = np.asarray(indices, np.int64)
        self.gathered.append(idx.copy())
        obs, act, rew, term, nobs = (a[idx] for a in self.rows)
        return dict(observations=obs, actions=act, rewards=rew.astype(np.float32), terminals=term.astype(np.float32),
                    next_observations=nobs)


def no_library(monkeypatch, *trainers):
    for t in trainers:
        t._lib = NoLibrary()
    monkeypatch.setattr(_lib, "load", lambda: NoLibrary())


def eps_pair(n, A, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((n, A)).astype(np.float32), rs.standard_normal((n, A)).astype(np.float32)


def td3_trainer(O=5, A=2):
    pols = [TanhMlpPolicy([8, 8], A, O) for _ in range(2)]
    qs = [FlattenMlp([8, 8], 1, O + A) for _ in range(4)]
    return TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1])


def test_bindings_and_header_declare_the_feature():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    assert "typedef struct { sac_buffer_t *buf; const int64_t *idx; } sac_eval_src_t;" in header
    for name in ("sac_evaluate_replay_many", "sac_evaluate_replay_general_many"):
        assert f"int {name}(" in header
        # trainers, n_trainers, n_rows, src, io, stats
        assert _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4)
    assert [f[0] for f in _lib.SacEvalSrc._fields_] == ["buf", "idx"] and C.sizeof(_lib.SacEvalSrc) == 16
    assert infer.EVAL_REPLAY_ENTRIES == {infer.FUSED: "sac_evaluate_replay_many",
                                         infer.GENERAL_STEP: "sac_evaluate_replay_general_many"}
    csrc = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")
    kernel = open(os.path.join(csrc, "sac_eval_rows.h")).read()
    assert "k_eval_rows" in kernel and "asm" not in kernel and "__shared__" not in kernel
    assert '#include "sac_eval_rows.h"' in open(os.path.join(csrc, "sac_trainer.hip")).read()


def test_defaults():
    for fn in (SACTrainer.evaluate_replay, TD3Trainer.evaluate_replay, evaluate_replay_many, infer.evaluate_replay_many,
               ArchSACTrainerGroup.evaluate_replay_many):
        p = inspect.signature(fn).parameters
        assert p["general"].default == "host" and p["stats"].default == "host", fn.__qualname__
        assert p["n"].default is None and p["indices"].default is None and p["rows"].default is False, fn.__qualname__
    for fn in (driver.experiment, driver.experiment_group, driver.experiment_sweep):
        assert inspect.signature(fn).parameters["replay_eval"].default == 0, fn.__name__
    assert driver.EvalOptions._field_defaults["replay_eval"] == 0
    for bad in (-1, 1.5, "many", True):
        for fn, args in ((driver.experiment, (None,)), (driver.experiment_group, (None, None)), (driver.experiment_sweep, (None,))):
            with pytest.raises(RuntimeError, match="replay_eval is a row count"):
                fn(*args, replay_eval=bad)


def test_exactly_one_of_n_and_indices(monkeypatch):
    t = handle_less(5, 2, (8, 8))
    no_library(monkeypatch, t)
    buf = HostBuffer(20, 5, 2)
    for kw in (dict(), dict(n=3, indices=[0, 1, 2])):
        with pytest.raises(ValueError, match="exactly one of n and indices"):
            t.evaluate_replay(buf, **kw)
        with pytest.raises(ValueError, match="exactly one of n and indices"):
            evaluate_replay_many([t], [buf], **{k: ([v] if k == "indices" else v) for k, v in kw.items()})
        with pytest.raises(ValueError, match="exactly one of n and indices"):
            group_of([t]).evaluate_replay_many([buf], **{k: ([v] if k == "indices" else v) for k, v in kw.items()})
    assert buf.gathered == []
    # the other argument checks, all in front of the gather
    for idx in ([20], [-1], [0, 5, 20]):
        with pytest.raises(RuntimeError, match="out of range"):
            t.evaluate_replay(buf, indices=idx)
    with pytest.raises(ValueError, match="eps"):
        t.evaluate_replay(buf, indices=[1, 2, 3], eps=eps_pair(2, 2, 0))
    with pytest.raises(ValueError, match="at least one row"):
        t.evaluate_replay(buf, n=0)
    with pytest.raises(RuntimeError, match="empty"):
        t.evaluate_replay(HostBuffer(0, 5, 2), n=4)
    with pytest.raises(RuntimeError, match="stats must be"):
        t.evaluate_replay(buf, n=4, stats="gpu", general="gpu")
    with pytest.raises(RuntimeError, match="general must be"):
        t.evaluate_replay(buf, n=4, general="gpu")
    with pytest.raises(RuntimeError, match="twice"):
        evaluate_replay_many([t, t], [buf, buf], n=4)
    assert buf.gathered == []


def test_indices_are_drawn_in_front_of_eps_and_never_from_np_random(monkeypatch):
    O, A, size, n = 5, 2, 37, 11
    t = handle_less(O, A, (8, 8))
    no_library(monkeypatch, t)
    buf = HostBuffer(size, O, A)
    np.random.seed(123)
    before = np.random.get_state()
    stats, cols = t.evaluate_replay(buf, n=n, rng=np.random.RandomState(9), rows=True)
    rs = np.random.RandomState(9)
    idx = rs.randint(0, size, n)
    eps = (rs.standard_normal((n, A)), rs.standard_normal((n, A)))
    assert cols["indices"].dtype == np.int64 and np.array_equal(cols["indices"], idx)
    assert np.array_equal(buf.gathered[-1], idx)
    want_stats, want = t.evaluate(buf.gather(idx), eps=eps, rows=True)
    assert stats == want_stats and all(np.array_equal(cols[k], want[k]) for k in COLUMNS)
    assert list(cols.keys()) == list(want.keys()) + ["indices"]
    # rng=None: evaluate's private stream (seeded from noise_seed), indices first
    t2 = handle_less(O, A, (8, 8))
    no_library(monkeypatch, t2)
    _, cols2 = t2.evaluate_replay(buf, n=n, rows=True)
    rs = np.random.RandomState([int(t2.noise_seed & 0xFFFFFFFF), int(t2.noise_seed >> 32), 0x4556414C])
    idx2 = rs.randint(0, size, n)
    eps2 = (rs.standard_normal((n, A)), rs.standard_normal((n, A)))
    assert np.array_equal(cols2["indices"], idx2)
    _, want2 = handle_less(O, A, (8, 8)).evaluate(buf.gather(idx2), eps=eps2, rows=True)
    assert all(np.array_equal(cols2[k], want2[k]) for k in COLUMNS)
    # given indices: only the eps pair is drawn
    _, cols3 = t.evaluate_replay(buf, indices=[3, 3, 36, 0], rng=np.random.RandomState(4), rows=True)
    rs = np.random.RandomState(4)
    _, want3 = t.evaluate(buf.gather([3, 3, 36, 0]), eps=(rs.standard_normal((4, A)), rs.standard_normal((4, A))), rows=True)
    assert all(np.array_equal(cols3[k], want3[k]) for k in COLUMNS) and cols3["indices"].tolist() == [3, 3, 36, 0]
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]


class Handle:
    """A trainer with a handle's face: route asks nothing else of it."""
    _evaluate_on_host = False

    def __init__(self, hidden, h=1):
        self._h, self.hidden = h, list(hidden)

    def _hidden(self, name):
        return self.hidden


class DeviceBuffer:
    _h = C.c_void_p(1)


def test_route_sends_handle_less_trainers_and_host_buffers_to_the_host():
    fused, general = Handle((256, 256)), Handle((512, 512))
    for g in infer.GENERAL:
        assert infer.replay_route(Handle((256, 256), h=None), DeviceBuffer(), g) == infer.HOST
        assert infer.replay_route(Handle((512, 512), h=None), DeviceBuffer(), g) == infer.HOST
        assert infer.replay_route(fused, HostBuffer(4, 2, 1), g) == infer.HOST
        assert infer.replay_route(general, HostBuffer(4, 2, 1), g) == infer.HOST
        assert infer.replay_route(fused, DeviceBuffer(), g) == infer.FUSED
    assert infer.replay_route(general, DeviceBuffer(), "host") == infer.HOST
    assert infer.replay_route(general, DeviceBuffer(), "device") == infer.GENERAL_STEP
    fused._evaluate_on_host = True
    assert infer.replay_route(fused, DeviceBuffer(), "device") == infer.HOST


@pytest.mark.parametrize("hidden", [(8, 8), (24, 12, 20)])
def test_the_host_route_is_evaluate_on_the_gathered_batch(monkeypatch, hidden):
    O, A, size = 9, 3, 50
    t, u = handle_less(O, A, hidden, reward_scale=1.5, discount=0.97), handle_less(O, A, hidden, seed=6)
    no_library(monkeypatch, t, u)
    buf = HostBuffer(size, O, A)
    idx = np.array([0, size - 1, 7, 7, 31, 2], np.int64)
    eps = eps_pair(idx.size, A, 5)
    want_stats, want = t.evaluate(buf.gather(idx), eps=eps, rows=True)
    for general in infer.GENERAL:
        for stats in infer.STATS:
            s, c = t.evaluate_replay(buf, indices=idx, eps=eps, rows=True, general=general, stats=stats)
            assert s == want_stats and all(np.array_equal(c[k], want[k]) for k in COLUMNS)
            assert np.array_equal(c["indices"], idx) and c["alpha"] == want["alpha"]
            assert t.evaluate_replay(buf, indices=idx, eps=eps, general=general, stats=stats) == want_stats
    # many: member 1 sits out, two members share one buffer
    for got in (evaluate_replay_many([t, u, handle_less(O, A, hidden, seed=8)], [buf, buf, buf],
                                     indices=[idx, None, idx[:2]], eps=[eps, None, (eps[0][:2], eps[1][:2])], rows=True),
                group_of([t, u, handle_less(O, A, hidden, seed=8)]).evaluate_replay_many(
                    [buf, buf, buf], indices=[idx, [], idx[:2]], eps=[eps, None, (eps[0][:2], eps[1][:2])], rows=True)):
        assert got[1] is None and got[0][0] == want_stats
        assert all(np.array_equal(got[0][1][k], want[k]) for k in COLUMNS)
        w2 = handle_less(O, A, hidden, seed=8).evaluate(buf.gather(idx[:2]), eps=(eps[0][:2], eps[1][:2]), rows=True)
        assert got[2][0] == w2[0] and all(np.array_equal(got[2][1][k], w2[1][k]) for k in COLUMNS)
    # n per member, 0 sits out; one n for all
    got = evaluate_replay_many([t, u], [buf, buf], n=[4, 0], rngs=[np.random.RandomState(1), None], rows=True)
    assert got[1] is None and np.array_equal(got[0][1]["indices"], np.random.RandomState(1).randint(0, size, 4))
    got = evaluate_replay_many([t, u], [buf, buf], n=3, rngs=[np.random.RandomState(1), np.random.RandomState(2)], rows=True)
    assert [g[1]["indices"].size for g in got] == [3, 3]


def test_td3_is_refused():
    t = td3_trainer()
    buf = HostBuffer(10, 5, 2)
    for kw in (dict(n=4), dict(indices=[0, 1])):
        with pytest.raises(NotImplementedError, match="SAC objective"):
            t.evaluate_replay(buf, **kw)
    with pytest.raises(NotImplementedError, match="SAC objective"):
        evaluate_replay_many([t], [buf], n=4)
    with pytest.raises(NotImplementedError, match="SAC objective"):
        evaluate_replay_many([t], [buf], indices=[[0, 1]])
    assert buf.gathered == []
    # TD3Trainer.evaluate itself is what it was
    with pytest.raises(NotImplementedError, match="TD3Trainer.evaluate: "):
        t.evaluate(batch_dict(synth_transitions(4, 5, 2, seed=1)))
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=1, batch_size=64, agent="TD3")
    with pytest.raises(RuntimeError, match="replay_eval=N.*SAC objective"):
        driver.experiment(v, replay_eval=64, obs_dim=5, action_dim=2)
    with pytest.raises(RuntimeError, match="replay_eval=N.*SAC objective"):
        driver.experiment_group(v, [1, 2], replay_eval=64, obs_dim=5, action_dim=2)
    with pytest.raises(RuntimeError, match="replay_eval=N.*SAC objective"):
        driver.experiment_sweep([(v, 1, 5, 2)], replay_eval=64)


def test_replay_columns_have_the_keys_of_the_validation_columns():
    val = driver._validation_columns(None, None)
    rep = driver._replay_columns(None, 0)
    assert [k.replace("validation/", "replay/", 1) for k in val] == list(rep)
    assert rep["replay/Num Transitions"] == 0 and all(np.isnan(v) for k, v in rep.items() if k != "replay/Num Transitions")
    t = handle_less(5, 2, (8, 8))
    stats = t.evaluate(batch_dict(synth_transitions(6, 5, 2, seed=2)), eps=eps_pair(6, 2, 1))
    rep = driver._replay_columns(stats, 6)
    assert list(rep) == ["replay/" + k for k in stats] + ["replay/Num Transitions"] and rep["replay/Num Transitions"] == 6
    assert all(rep["replay/" + k] == v for k, v in stats.items())
    assert driver.REPLAY_STREAM == 0x52504C
    a, b = driver._replay_rng(3, 7), np.random.RandomState([3, 7, 0x52504C])
    assert np.array_equal(a.randint(0, 1000, 50), b.randint(0, 1000, 50))


def test_train_script_parses_replay_eval():
    spec = importlib.util.spec_from_file_location("train_script", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args([]).replay_eval == 0
    assert ap.parse_args(["--replay_eval"]).replay_eval == 1024
    assert ap.parse_args(["--replay_eval", "300"]).replay_eval == 300
    assert ap.parse_args(["--replay_eval", "--validation"]).replay_eval == 1024
