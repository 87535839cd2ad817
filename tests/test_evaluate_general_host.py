"""Host side of the loss evaluation for general-step trainers (no GPU): the declarations of sac_evaluate_general /
sac_evaluate_general_many, the `general` argument of evaluate / evaluate_many checked before any library call, the
handle-less path under both values (general shapes included, against tests/eval_reference_general.py), eval_general on
the drivers and scripts/train.py, and TD3's refusal."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from robosuite_benchmark_amd import FlattenMlp, TanhMlpPolicy, TD3Trainer, _lib
from robosuite_benchmark_amd.group import GENERAL, ArchSACTrainerGroup, evaluate_many
from robosuite_benchmark_amd.sac import SACTrainer
from tests.eval_reference import COLUMNS, batch_dict
from tests.eval_reference_general import check_columns
from tests.helpers import synth_transitions
from tests.test_evaluate_host import handle_less
from tests.test_q_values_host import NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inputs(n, O, A, seed):
    batch = synth_transitions(n, O, A, seed=seed, term_frac=0.1)
    rs = np.random.RandomState(seed + 7)
    return batch, (rs.standard_normal((n, A)).astype(np.float32), rs.standard_normal((n, A)).astype(np.float32))


def group_of(trainers):
    group = ArchSACTrainerGroup.__new__(ArchSACTrainerGroup)
    group.trainers = list(trainers)
    return group


def test_bindings_and_header_name_the_general_entry_points():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    for name in ("sac_evaluate_general", "sac_evaluate_general_many"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    # the signatures of sac_evaluate / sac_evaluate_many
    assert _lib.SYMBOLS["sac_evaluate_general"] == _lib.SYMBOLS["sac_evaluate"]
    assert _lib.SYMBOLS["sac_evaluate_general_many"] == _lib.SYMBOLS["sac_evaluate_many"]
    # the two families point at each other, and the fused entries keep the texts their refusals are matched by
    csrc = os.path.join(ROOT, "robosuite_benchmark_amd", "csrc")
    fused, infer = open(os.path.join(csrc, "sac_eval.h")).read(), open(os.path.join(csrc, "sac_infer.h")).read()
    assert "sac_evaluate_general" in fused and "k_eval_layer" in header
    assert "forward on the host" in fused and "general step" in infer and "SAC objective" in infer
    general = open(os.path.join(csrc, "sac_eval_general.h")).read()
    # one alpha read for both entries: the SAC description's per-call preparation, which the body of either family runs
    assert fused.count("eval_read_alpha(") == 2 and "return eval_read_alpha(" in fused.split("int prepare(")[1].split("}")[0]
    assert "eval_read_alpha" not in general and "C.prepare(" in general and "C.prepare(" in fused


def test_general_is_checked_before_any_library_call(monkeypatch):
    t = handle_less(5, 2, (8, 8))
    t._lib = NoLibrary()
    monkeypatch.setattr(_lib, "load", lambda: NoLibrary())
    batch, eps = inputs(6, 5, 2, 1)
    for bad in ("gpu", "", None, "Device", 1):
        with pytest.raises(RuntimeError, match="general"):
            t.evaluate(batch_dict(batch), eps=eps, general=bad)
        with pytest.raises(RuntimeError, match="general"):
            evaluate_many([t], [batch_dict(batch)], eps=[eps], general=bad)
        with pytest.raises(RuntimeError, match="general"):
            group_of([t]).evaluate_many([batch_dict(batch)], eps=[eps], general=bad)
    # the other argument checks still come before the library under "device"
    with pytest.raises(ValueError, match="eps"):
        t.evaluate(batch_dict(batch), eps=(eps[0], eps[1][:5]), general="device")
    with pytest.raises(RuntimeError, match="twice"):
        evaluate_many([t, t], [batch_dict(batch)] * 2, general="device")


@pytest.mark.parametrize("hidden", [(8, 8), (24, 12, 20), (300,)])
def test_without_a_handle_the_holders_answer_under_both_values(monkeypatch, hidden):
    O, A, n = 9, 3, 17
    t = handle_less(O, A, hidden, reward_scale=1.5, discount=0.97)
    assert t._h is None
    t._lib = NoLibrary()
    monkeypatch.setattr(_lib, "load", lambda: NoLibrary())
    batch, eps = inputs(n, O, A, 3)
    stats, cols = t.evaluate(batch_dict(batch), eps=eps, rows=True)
    check_columns(cols, t, batch, eps, ("host", hidden),
                  state=dict(scalars=np.zeros(6), params={k: getattr(t, k).flat() for k in t.NETS}))
    for general in GENERAL:
        s, c = t.evaluate(batch_dict(batch), eps=eps, rows=True, general=general)
        assert s == stats and all(np.array_equal(c[k], cols[k]) for k in COLUMNS), general
        for got in (evaluate_many([t], [batch_dict(batch)], eps=[eps], rows=True, general=general),
                    group_of([t]).evaluate_many([batch_dict(batch)], eps=[eps], rows=True, general=general)):
            assert got[0][0] == stats and all(np.array_equal(got[0][1][k], cols[k]) for k in COLUMNS), general
        assert evaluate_many([t], [None], general=general) == [None]


def test_drivers_and_train_script_take_eval_general():
    from robosuite_benchmark_amd import driver
    for fn, args in ((driver.experiment, (None,)), (driver.experiment_group, (None, None)), (driver.experiment_sweep, (None,))):
        assert inspect.signature(fn).parameters["eval_general"].default == "host", fn.__name__
        with pytest.raises(RuntimeError, match="general"):       # (checked in front of everything else)
            fn(*args, eval_general="gpu")
    assert driver.EvalOptions._field_defaults["eval_general"] == "host"
    for fn in (SACTrainer.evaluate, TD3Trainer.evaluate, evaluate_many, ArchSACTrainerGroup.evaluate_many):
        assert inspect.signature(fn).parameters["general"].default == "host", fn.__qualname__
    # the keyword is left out of the calls at the default: a replacement of evaluate with the old signature still serves
    assert driver._q_general_kw("host") == {} and driver._q_general_kw("device") == dict(general="device")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--eval_general" in out and out.count("{host,device}") >= 2


def test_td3_still_refuses():
    O, A = 5, 2
    pols = [TanhMlpPolicy([8, 8], A, O) for _ in range(2)]
    qs = [FlattenMlp([8, 8], 1, O + A) for _ in range(4)]
    t = TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1])
    batch = batch_dict(synth_transitions(4, O, A, seed=1))
    for general in GENERAL:
        with pytest.raises(NotImplementedError, match="SAC objective"):
            t.evaluate(batch, general=general)
        with pytest.raises(NotImplementedError, match="SAC objective"):
            evaluate_many([t], [batch], general=general)
