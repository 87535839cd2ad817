"""Host side of the critics' evaluation for general-step trainers (no GPU): the declarations of sac_q_values_general /
sac_q_values_general_many, the `general` argument of q_values / q_values_many / q_many checked before any library call,
the handle-less path under both values, and q_general on the drivers and scripts/train.py."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from robosuite_benchmark_amd import _lib
from robosuite_benchmark_amd.group import GENERAL, ArchSACTrainerGroup, q_values_many
from tests.test_q_values_host import NoLibrary, handle_less_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bindings_and_header_name_the_general_entry_points():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    for name in ("sac_q_values_general", "sac_q_values_general_many"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    # the signatures of sac_q_values / sac_q_values_many
    assert _lib.SYMBOLS["sac_q_values_general"] == _lib.SYMBOLS["sac_q_values"]
    assert _lib.SYMBOLS["sac_q_values_general_many"] == _lib.SYMBOLS["sac_q_values_many"]
    # the two families point at each other
    kernel = open(os.path.join(ROOT, "robosuite_benchmark_amd", "csrc", "sac_qval.h")).read()
    assert "sac_q_values_general" in kernel and "k_qval_layer" in header


def test_general_is_checked_before_any_library_call(monkeypatch):
    assert GENERAL == ("host", "device")
    t = handle_less_trainer()
    obs, act = np.zeros((6, 5), np.float32), np.zeros((6, 2), np.float32)
    monkeypatch.setattr(_lib, "load", lambda: NoLibrary())
    for bad in ("gpu", "", None, "Device", 1):
        with pytest.raises(RuntimeError, match="general"):
            t.q_values(obs, act, general=bad)
        with pytest.raises(RuntimeError, match="general"):
            q_values_many([t], [obs], [act], [("qf1",)], general=bad)
        group = ArchSACTrainerGroup.__new__(ArchSACTrainerGroup)
        group.trainers = [t]
        with pytest.raises(RuntimeError, match="general"):
            group.q_many([obs], [act], general=bad)
    # the other argument checks still come before the library under "device"
    with pytest.raises(ValueError, match="Q network"):
        t.q_values(obs, act, nets=("qf9",), general="device")
    with pytest.raises(ValueError, match="q_values"):
        q_values_many([t], [obs], [act[:3]], [("qf1",)], general="device")


def test_without_a_handle_the_holders_answer_under_both_values(monkeypatch):
    t = handle_less_trainer()
    monkeypatch.setattr(_lib, "load", lambda: NoLibrary())
    rs = np.random.RandomState(1)
    obs, act = rs.normal(size=(7, 5)).astype(np.float32), rs.normal(size=(7, 2)).astype(np.float32)
    nets = ("target_qf1", "qf1")
    want = t.q_values(obs, act, nets=nets)
    assert np.allclose(want[0], t.target_qf1.forward_np(obs, act)[:, 0], rtol=1e-6, atol=1e-7)
    for general in GENERAL:
        assert np.array_equal(t.q_values(obs, act, nets=nets, general=general), want), general
        assert np.array_equal(q_values_many([t], [obs], [act], [nets], general=general)[0], want), general
        assert q_values_many([t], [None], [None], [nets], general=general)[0].shape == (2, 0)
        group = ArchSACTrainerGroup.__new__(ArchSACTrainerGroup)
        group.trainers = [t]
        assert np.array_equal(group.q_many([obs], [act], [nets], general=general)[0], want), general


def test_drivers_and_train_script_take_q_general():
    from robosuite_benchmark_amd import driver
    from robosuite_benchmark_amd.sac import SACTrainer
    from robosuite_benchmark_amd.td3 import TD3Trainer
    for fn, args in ((driver.experiment, (None,)), (driver.experiment_group, (None, None)), (driver.experiment_sweep, (None,))):
        assert inspect.signature(fn).parameters["q_general"].default == "host", fn.__name__
        with pytest.raises(RuntimeError, match="general"):       # (checked in front of everything else)
            fn(*args, q_general="gpu")
    for fn in (SACTrainer.q_values, TD3Trainer.q_values, q_values_many, ArchSACTrainerGroup.q_many):
        assert inspect.signature(fn).parameters["general"].default == "host", fn.__qualname__
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--q_general" in out and "{host,device}" in out
