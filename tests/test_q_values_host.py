"""Host side of the critics' evaluation (no GPU): driver.q_bias_information against a plain loop, the net-mask helper,
the argument checks that come before any library call, and the declarations."""
import os
import subprocess
import sys

import numpy as np
import pytest

from robosuite_benchmark_amd import FlattenMlp, _lib
from robosuite_benchmark_amd.driver import _stats, q_bias_information
from robosuite_benchmark_amd.group import q_values_many
from robosuite_benchmark_amd.sac import SACTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_COLUMNS = [f"evaluation/{name} {s}" for name in ("Q1 Estimates", "Q2 Estimates", "Returns To Go", "Q Bias")
             for s in ("Mean", "Std", "Max", "Min")]


def plain_returns_to_go(paths, discount, reward_scale):
    out = []
    for p in paths:
        r = [float(x) for x in np.asarray(p["rewards"]).ravel()]
        for t in range(len(r)):
            g = 0.0
            for k in range(t, len(r)):
                g += discount ** (k - t) * reward_scale * r[k]
            out.append(g)
    return out


def make_paths(lengths, seed):
    rs = np.random.RandomState(seed)
    return [dict(rewards=rs.uniform(0, 1, (n, 1)), observations=rs.normal(size=(n, 3)), actions=rs.normal(size=(n, 2)))
            for n in lengths]


@pytest.mark.parametrize("lengths", [(1,), (5,), (4, 1, 9, 2)])
@pytest.mark.parametrize("discount,reward_scale", [(1.0, 1.0), (0.99, 1.0), (0.99, 2.5), (0.5, 0.1)])
def test_q_bias_information_against_a_plain_loop(lengths, discount, reward_scale):
    paths = make_paths(lengths, sum(lengths))
    n = sum(lengths)
    rs = np.random.RandomState(n)
    q1 = rs.normal(3, 2, n).astype(np.float32)
    q2 = (q1 + np.where(np.arange(n) % 2 == 0, 0.5, -0.5)).astype(np.float32)      # q1 < q2 and q1 > q2 rows
    G = plain_returns_to_go(paths, discount, reward_scale)
    info = q_bias_information(paths, q1, q2, discount, reward_scale)
    assert list(info.keys()) == Q_COLUMNS
    bias = [min(float(a), float(b)) - g for a, b, g in zip(q1, q2, G)]
    if n > 1:
        assert any(a < b for a, b in zip(q1, q2)) and any(a > b for a, b in zip(q1, q2))
    want = {}
    for name, x in (("Q1 Estimates", q1), ("Q2 Estimates", q2), ("Returns To Go", G), ("Q Bias", bias)):
        want.update(_stats("evaluation/" + name, x))
    for k in Q_COLUMNS:
        assert isinstance(info[k], float) and info[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k
    # exact where the arithmetic is: the Q columns are plain float64 statistics of the float32 values
    assert info["evaluation/Q1 Estimates Mean"] == float(np.mean(q1.astype(np.float64)))
    assert info["evaluation/Q2 Estimates Max"] == float(np.max(q2))


def test_q_bias_information_by_hand():
    paths = [dict(rewards=np.array([[1.0], [2.0], [4.0]])), dict(rewards=np.array([[3.0]]))]
    info = q_bias_information(paths, [10, 0, 1, 5], [9, 2, 3, 7], 0.5, 2.0)
    # G = 2 * (1 + .5 * 2 + .25 * 4), 2 * (2 + .5 * 4), 2 * 4 | 2 * 3
    assert info["evaluation/Returns To Go Max"] == 8.0 and info["evaluation/Returns To Go Min"] == 6.0
    assert info["evaluation/Returns To Go Mean"] == (6.0 + 8.0 + 8.0 + 6.0) / 4
    # min(q1, q2) - G = 9 - 6, 0 - 8, 1 - 8, 5 - 6
    assert info["evaluation/Q Bias Max"] == 3.0 and info["evaluation/Q Bias Min"] == -8.0
    assert info["evaluation/Q Bias Mean"] == (3.0 - 8.0 - 7.0 - 1.0) / 4
    with pytest.raises(ValueError, match="Q values"):
        q_bias_information(paths, [1, 2, 3], [1, 2, 3], 0.99, 1.0)
    assert "time limit" in q_bias_information.__doc__ and "tail" in q_bias_information.__doc__


def test_net_masks():
    assert _lib.Q_NET_BITS == {"qf1": 1, "qf2": 2, "target_qf1": 4, "target_qf2": 8}
    assert all(bit == 1 << (_lib.NET_IDS[name] - 1) for name, bit in _lib.Q_NET_BITS.items())
    assert _lib.q_net_mask(("qf1", "qf2")) == (3, [0, 1])
    assert _lib.q_net_mask(("qf2", "qf1")) == (3, [1, 0])
    assert _lib.q_net_mask("target_qf1") == (4, [0])
    assert _lib.q_net_mask(["target_qf2", "qf2", "target_qf1"]) == (14, [2, 0, 1])
    assert _lib.q_net_mask(("target_qf2", "target_qf1", "qf2", "qf1")) == (15, [3, 2, 1, 0])
    for bad in ((), [], ("policy",), ("qf3",), ("qf1", "qf1"), ("qf1", None)):
        with pytest.raises(ValueError, match="Q network"):
            _lib.q_net_mask(bad)


class NoLibrary:
    """Stands in for the loaded library: any call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


def handle_less_trainer(O=5, A=2):
    """A SACTrainer that was never given a batch size: holders and host metadata, no handle."""
    from robosuite_benchmark_amd import TanhGaussianPolicy
    rs = np.random.RandomState(3)
    qs = [FlattenMlp([8, 4], 1, O + A, rs=rs) for _ in range(4)]
    t = SACTrainer.__new__(SACTrainer)
    t.policy, (t.qf1, t.qf2, t.target_qf1, t.target_qf2) = TanhGaussianPolicy([8, 4], O, A, rs=rs), qs
    t.obs_dim, t.act_dim, t._h, t._lib = O, A, None, NoLibrary()
    for q in qs:
        q._trainer = t
    return t


def test_bad_arguments_raise_before_any_library_call():
    t = handle_less_trainer()
    obs, act = np.zeros((6, 5), np.float32), np.zeros((6, 2), np.float32)
    for nets in ((), ("policy",), ("qf1", "qf1")):
        with pytest.raises(ValueError, match="Q network"):
            t.q_values(obs, act, nets=nets)
    for o, a in ((obs[:, :4], act), (obs, act[:, :1]), (obs[:5], act), (obs[:0], act[:0]), (np.zeros((2, 3, 5)), act)):
        with pytest.raises(ValueError, match="q_values"):
            t.q_values(o, a)
    with pytest.raises(ValueError, match="Q network"):
        q_values_many([t], [obs], [act], [("qf9",)])
    with pytest.raises(ValueError, match="q_values"):
        q_values_many([t], [obs], [act[:3]], [("qf1",)])
    with pytest.raises(RuntimeError, match="per trainer"):
        q_values_many([t], [obs, obs], [act], [("qf1",)])
    with pytest.raises(RuntimeError, match="twice"):
        q_values_many([t, t], [obs, obs], [act, act], [("qf1",), ("qf1",)])


def test_without_a_handle_the_holders_own_weights_answer():
    t = handle_less_trainer()
    rs = np.random.RandomState(1)
    obs, act = rs.normal(size=(7, 5)).astype(np.float32), rs.normal(size=(7, 2)).astype(np.float32)
    got = t.q_values(obs, act, nets=("target_qf1", "qf1"))
    assert got.shape == (2, 7) and got.dtype == np.float32
    assert np.allclose(got[0], t.target_qf1.forward_np(obs, act)[:, 0], rtol=1e-6, atol=1e-7)
    assert np.allclose(got[1], t.qf1.forward_np(obs, act)[:, 0], rtol=1e-6, atol=1e-7)
    many = q_values_many([t], [obs], [act], [("target_qf1", "qf1")])
    assert np.array_equal(many[0], got)
    assert q_values_many([t], [None], [None], [("qf1", "qf2")])[0].shape == (2, 0)
    # a holder: (n, 1) through forward_np while there is no handle, bound or not
    free = FlattenMlp([8, 4], 1, 7, rs=rs)
    for q in (t.qf2, free):
        assert q(obs, act).shape == (7, 1) and np.array_equal(q(obs, act), q.forward_np(obs, act))
    # a one-row call may come without the row dimension
    assert np.array_equal(t.q_values(obs[0], act[0]), t.q_values(obs[:1], act[:1]))


def test_bindings_and_header_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    for name in ("sac_q_values", "sac_q_values_many"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    assert "enum { SAC_Q_QF1 = 1, SAC_Q_QF2 = 2, SAC_Q_TARGET_QF1 = 4, SAC_Q_TARGET_QF2 = 8 }" in header
    assert len(_lib.SYMBOLS["sac_q_values"][1]) == 6 and len(_lib.SYMBOLS["sac_q_values_many"][1]) == 7


def test_drivers_take_q_diagnostics():
    import inspect
    from robosuite_benchmark_amd import driver
    for fn in (driver.experiment, driver.experiment_group, driver.experiment_sweep):
        assert inspect.signature(fn).parameters["q_diagnostics"].default is False, fn.__name__
    assert driver.EvalOptions._field_defaults["q_diagnostics"] is False
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--q_diagnostics" in out
