"""Host side of evaluate's device statistics (no GPU): sac.eval_moments / merge_moments / moments_statistics against
sac.eval_statistics under the bound of tests/eval_stats_bound.py, the exact cases (a constant column, a NaN element), the
declarations of sac_evaluate_stats_many / sac_evaluate_general_stats_many, the `stats` argument checked before anything
else, the handle-less path under both values, eval_stats on the drivers and scripts/train.py, and TD3's refusal."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from robosuite_benchmark_amd import FlattenMlp, TanhMlpPolicy, TD3Trainer, _lib, sac
from robosuite_benchmark_amd.group import ArchSACTrainerGroup, evaluate_many
from robosuite_benchmark_amd.sac import SACTrainer, eval_moments, eval_statistics, merge_moments, moments_statistics
from tests.eval_reference import COLUMNS, batch_dict
from tests.eval_stats_bound import check_statistics
from tests.helpers import synth_transitions
from tests.test_evaluate_general_host import group_of, inputs
from tests.test_evaluate_host import handle_less
from tests.test_q_values_host import NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024


def columns(n, A, seed, scale=1.0, offset=0.0):
    """Random float32 columns: rows (9, n), mu and log_std (n, A)."""
    rs = np.random.RandomState(seed)
    f = lambda *shape: (offset + scale * rs.standard_normal(shape)).astype(np.float32)       # noqa: E731
    return f(9, n), f(n, A), np.clip(f(n, A), -20, 2)


def merged(rows, mu, log_std):
    """eval_moments of 1024-row chunks, merged in order: what a call above 1024 rows does."""
    out = None
    for i in range(0, rows.shape[1], CHUNK):
        part = eval_moments(rows[:, i:i + CHUNK], mu[i:i + CHUNK], log_std[i:i + CHUNK])
        out = part if out is None else {k: merge_moments(out[k], part[k]) for k in out}
    return out


@pytest.mark.parametrize("n,A", [(1, 1), (2, 3), (255, 7), (1024, 16)])
@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (1e-3, 5.0), (1e3, -1e4)])
def test_moments_statistics_agree_with_eval_statistics(n, A, scale, offset):
    rows, mu, log_std = columns(n, A, n + A, scale, offset)
    for auto, log_alpha in ((True, -0.37), (False, 0.0)):
        want = eval_statistics(rows, mu, log_std, 0.7, log_alpha, -float(A), auto)
        M = eval_moments(rows, mu, log_std)
        assert list(M.keys()) == _lib.EVAL_MOMENTS and all(list(m.keys()) == _lib.EVAL_MOMENT_FIELDS for m in M.values())
        assert M["q1"]["count"] == n and M["mu"]["count"] == n * A
        got = moments_statistics(M, 0.7, log_alpha, -float(A), auto)
        check_statistics(got, want, rows, mu, log_std, log_alpha, -float(A), (n, A, auto))
        assert got["Alpha"] == 0.7 and (auto or got["Alpha Loss"] == 0.0)
        for k in want:                                               # Max and Min are exact
            assert not k.endswith((" Max", " Min")) or got[k] == want[k], k
    if n == 1:
        assert all(got[k] == 0.0 for k in got if k.endswith(" Std"))


@pytest.mark.parametrize("n", [1025, 2500])
def test_merged_chunks_agree_with_the_whole(n):
    for scale, offset in ((1.0, 0.0), (1e-3, 1e4)):
        rows, mu, log_std = columns(n, 5, n, scale, offset)
        M = merged(rows, mu, log_std)
        assert M["q1"]["count"] == n and M["log_std"]["count"] == 5 * n
        want = eval_statistics(rows, mu, log_std, 1.3, 0.21, -5.0, True)
        check_statistics(moments_statistics(M, 1.3, 0.21, -5.0, True), want, rows, mu, log_std, 0.21, -5.0, (n, scale))
        whole = moments_statistics(eval_moments(rows, mu, log_std), 1.3, 0.21, -5.0, True)
        check_statistics(moments_statistics(M, 1.3, 0.21, -5.0, True), whole, rows, mu, log_std, 0.21, -5.0, (n, scale))


@pytest.mark.parametrize("n", [1, 1000, 2500])
def test_a_constant_column_has_no_deviation(n):
    c = np.float32(0.1)
    rows, mu, log_std = columns(n, 3, 4)
    rows[0] = c
    log_std[:] = np.float32(2.0)
    for M in (eval_moments(rows, mu, log_std), merged(rows, mu, log_std)):
        got = moments_statistics(M, 1.0, 0.0, -3.0, True)
        assert got["Q1 Predictions Std"] == 0.0 and got["Q1 Predictions Mean"] == float(c)
        assert got["Q1 Predictions Max"] == got["Q1 Predictions Min"] == float(c)
        assert got["Policy log std Std"] == 0.0 and got["Policy log std Mean"] == 2.0


def test_a_nan_element_makes_its_statistics_nan():
    rows, mu, log_std = columns(40, 3, 6)
    rows[0, 17] = np.nan                                             # q1: its own statistics, TD Error 1 and QF1 Loss
    mu[39, 2] = np.nan
    want = eval_statistics(rows, mu, log_std, 1.0, 0.1, -3.0, True)
    for M in (eval_moments(rows, mu, log_std), merged(rows, mu, log_std)):
        got = moments_statistics(M, 1.0, 0.1, -3.0, True)
        for name in ("Q1 Predictions", "Policy mu", "TD Error 1"):
            assert all(np.isnan(got[f"{name} {s}"]) for s in ("Mean", "Std", "Max", "Min")), name
        assert np.isnan(got["QF1 Loss"]) and not np.isnan(got["QF2 Loss"])
        check_statistics(got, want, rows, mu, log_std, 0.1, -3.0)
    rows, mu, log_std = columns(2500, 2, 6)
    rows[8, 2000] = np.nan                                           # a NaN in the second chunk survives the merge
    got = moments_statistics(merged(rows, mu, log_std), 1.0, 0.1, -2.0, True)
    assert all(np.isnan(got[f"Q Targets {s}"]) for s in ("Mean", "Std", "Max", "Min")) and np.isnan(got["QF2 Loss"])
    assert not np.isnan(got["Log Pis Max"])


def test_bindings_and_header_declare_the_feature():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    assert ("enum { SAC_EVAL_M_Q1, SAC_EVAL_M_Q2, SAC_EVAL_M_Y, SAC_EVAL_M_LOG_PI, SAC_EVAL_M_MU, SAC_EVAL_M_LOG_STD,\n"
            "       SAC_EVAL_M_TD1, SAC_EVAL_M_TD2, SAC_EVAL_M_POLICY, SAC_EVAL_MOMENTS_N };") in header
    assert "typedef struct { double count, sum, m2, sumsq, max, min; } sac_eval_moment_t;" in header
    assert ("typedef struct { sac_eval_moment_t m[SAC_EVAL_MOMENTS_N]; double alpha, log_alpha; } sac_eval_stats_t;"
            in header)
    for name in ("sac_evaluate_stats_many", "sac_evaluate_general_stats_many"):
        assert f"int {name}(" in header and _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 3)
    assert _lib.EVAL_MOMENTS == ["q1", "q2", "y", "log_pi", "mu", "log_std", "td1", "td2", "policy"]
    assert _lib.EVAL_MOMENT_FIELDS == ["count", "sum", "m2", "sumsq", "max", "min"]
    assert C.sizeof(_lib.SacEvalMoment) == 6 * 8 and C.sizeof(_lib.SacEvalStats) == 9 * 6 * 8 + 2 * 8
    assert _lib.SacEvalStats.alpha.offset == 9 * 6 * 8 and _lib.SacEvalStats.log_alpha.offset == 9 * 6 * 8 + 8
    assert len(_lib.SacEvalIO._fields_) == 13                        # (sac_eval_io_t is what it was)
    csrc = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")
    kernel = open(os.path.join(csrc, "sac_eval_moments.h")).read()
    assert "k_eval_moments" in kernel and "atomic" not in kernel.replace("No atomics", "") and "asm" not in kernel
    assert '#include "sac_eval_moments.h"' in open(os.path.join(csrc, "sac_trainer.hip")).read()


def test_stats_defaults_to_host_everywhere():
    from robosuite_benchmark_amd import driver
    assert sac.STATS == ("host", "device")
    for fn in (SACTrainer.evaluate, TD3Trainer.evaluate, evaluate_many, ArchSACTrainerGroup.evaluate_many):
        assert inspect.signature(fn).parameters["stats"].default == "host", fn.__qualname__
    for fn in (driver.experiment, driver.experiment_group, driver.experiment_sweep):
        assert inspect.signature(fn).parameters["eval_stats"].default == "host", fn.__name__
    assert driver.EvalOptions._field_defaults["eval_stats"] == "host"
    # the keyword is left out of the calls at the default: a replacement of evaluate with the old signature still serves
    assert driver._eval_stats_kw("host") == {} and driver._eval_stats_kw("device") == dict(stats="device")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--eval_stats" in out and out.count("{host,device}") >= 3


def test_stats_is_checked_before_everything_else(monkeypatch):
    from robosuite_benchmark_amd import driver
    t = handle_less(5, 2, (8, 8))
    t._lib = NoLibrary()
    monkeypatch.setattr(_lib, "load", lambda: NoLibrary())
    batch, eps = inputs(6, 5, 2, 1)
    for bad in ("gpu", "", None, "Device", 1):
        # (in front of the check of `general` and of the arguments)
        with pytest.raises(RuntimeError, match="stats must be"):
            t.evaluate(batch_dict(batch), eps=(eps[0], eps[1][:5]), general="gpu", stats=bad)
        with pytest.raises(RuntimeError, match="stats must be"):
            evaluate_many([t, t], [batch_dict(batch)], eps=[eps], general="gpu", stats=bad)
        with pytest.raises(RuntimeError, match="stats must be"):
            group_of([t]).evaluate_many([batch_dict(batch)], eps=[eps], general="gpu", stats=bad)
    for fn, args in ((driver.experiment, (None,)), (driver.experiment_group, (None, None)), (driver.experiment_sweep, (None,))):
        with pytest.raises(RuntimeError, match="stats must be"):
            fn(*args, eval_stats="gpu", eval_general="gpu", acting="nowhere")
    # the other checks still come before the library under "device"
    with pytest.raises(RuntimeError, match="general"):
        t.evaluate(batch_dict(batch), eps=eps, general="gpu", stats="device")
    with pytest.raises(ValueError, match="eps"):
        t.evaluate(batch_dict(batch), eps=(eps[0], eps[1][:5]), stats="device")
    with pytest.raises(RuntimeError, match="twice"):
        evaluate_many([t, t], [batch_dict(batch)] * 2, stats="device")


@pytest.mark.parametrize("hidden", [(8, 8), (24, 12, 20)])
def test_without_a_handle_the_host_path_answers_under_both_values(monkeypatch, hidden):
    O, A, n = 9, 3, 17
    t = handle_less(O, A, hidden, reward_scale=1.5, discount=0.97)
    assert t._h is None
    t._lib = NoLibrary()
    monkeypatch.setattr(_lib, "load", lambda: NoLibrary())
    batch, eps = inputs(n, O, A, 3)
    stats, cols = t.evaluate(batch_dict(batch), eps=eps, rows=True)
    assert stats == eval_statistics(np.stack([cols[k] for k in _lib.EVAL_ROWS]), cols["mu"], cols["log_std"], cols["alpha"],
                                    0.0, t.target_entropy, True)
    for value in sac.STATS:
        s, c = t.evaluate(batch_dict(batch), eps=eps, rows=True, stats=value)
        assert s == stats and all(np.array_equal(c[k], cols[k]) for k in COLUMNS), value
        assert t.evaluate(batch_dict(batch), eps=eps, stats=value) == stats
        for got in (evaluate_many([t], [batch_dict(batch)], eps=[eps], rows=True, stats=value),
                    group_of([t]).evaluate_many([batch_dict(batch)], eps=[eps], rows=True, stats=value)):
            assert got[0][0] == stats and all(np.array_equal(got[0][1][k], cols[k]) for k in COLUMNS), value
        assert evaluate_many([t], [None], stats=value) == [None]


def test_td3_still_refuses():
    O, A = 5, 2
    pols = [TanhMlpPolicy([8, 8], A, O) for _ in range(2)]
    qs = [FlattenMlp([8, 8], 1, O + A) for _ in range(4)]
    t = TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1])
    batch = batch_dict(synth_transitions(4, O, A, seed=1))
    for value in sac.STATS:
        with pytest.raises(NotImplementedError, match="SAC objective"):
            t.evaluate(batch, stats=value)
        with pytest.raises(NotImplementedError, match="SAC objective"):
            evaluate_many([t], [batch], stats=value)
