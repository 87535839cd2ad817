"""Host side of device acting for general-step policies (no GPU): the acting value "device_all", the two new entry points
in the bindings, the header and the built library, the command line, and the lockstep collector's general= switch on
holders without a trainer (which keep their NumPy forward whatever the value)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from robosuite_benchmark_amd import TanhGaussianPolicy, TanhMlpPolicy, _lib
from robosuite_benchmark_amd.driver import GroupPathCollector, PathCollector
from robosuite_benchmark_amd.networks import ACTING, check_acting
from tests.test_device_acting_host import SPECS, assert_same_paths, member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sac_policy_act_general", "sac_policy_act_general_many")


def test_acting_values():
    assert ACTING == ("host", "device", "device_all")
    assert check_acting("device_all") == "device_all" and check_acting("device") == "device" and check_acting("host") == "host"
    assert TanhGaussianPolicy([8, 8], 3, 2).acting == "host" and TanhMlpPolicy([8, 8, 8], 2, 3).acting == "host"
    for bad in ("gpu", "", None, "Device", "device_general", "DEVICE_ALL"):
        with pytest.raises(ValueError, match="acting"):
            check_acting(bad)


def test_drivers_still_refuse_unknown_values_before_anything_is_built():
    from robosuite_benchmark_amd.driver import experiment, experiment_group, experiment_sweep
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant()
    for call in (lambda: experiment(v, acting="cuda"), lambda: experiment_group(v, [1, 2], acting="cuda"),
                 lambda: experiment_sweep([(v, 1)], acting="cuda")):
        with pytest.raises(ValueError, match="acting"):
            call()


def test_bindings_header_and_library_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and f"int {name}(" in header
        assert getattr(lib, name) is not None                           # (AttributeError if the library lacks it)
    res, args = _lib.SYMBOLS["sac_policy_act_general"]
    assert res is C.c_int and args == _lib.SYMBOLS["sac_policy_act_device"][1]
    assert _lib.SYMBOLS["sac_policy_act_general_many"] == _lib.SYMBOLS["sac_policy_act_many"]
    assert _lib.ACT_MAX_ROWS == 1024


def test_train_script_names_device_all():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--acting" in out and "device_all" in out


@pytest.mark.parametrize("sessions", [False, True])
def test_unbound_holders_collect_the_same_paths_under_device_and_device_all(sessions):
    """What acting="device" and acting="device_all" make of the lockstep collectors: general="host" and "device".  No
    member has a trainer handle here, so neither act_many nor a GroupActor is ever reached and the paths, counters and
    generator states are the same."""
    def boom(*a, **kw):
        raise AssertionError("holders without a trainer act on the host")

    groups = {}
    for general in ("host", "device"):
        cols = [PathCollector(*member(k, s, O, A, env)) for k, s, O, A, env, _ in SPECS]
        for c in cols:                                                     # the value the drivers give the holders
            h = getattr(c.policy, "stochastic_policy", None) or getattr(c.policy, "policy", c.policy)
            h.acting = "device_all" if general == "device" else "device"
        groups[general] = (cols, GroupPathCollector(cols, act_many=boom, actor=boom, sessions=sessions, general=general))
    for rnd in range(2):
        got = {g: grp.collect_new_paths([plan for *_, plan in SPECS]) for g, (_, grp) in groups.items()}
        for i in range(len(SPECS)):
            assert_same_paths(got["device"][i], got["host"][i], (rnd, i))
            assert groups["device"][0][i].get_diagnostics() == groups["host"][0][i].get_diagnostics(), (rnd, i)
    for a, b in zip(*(cols for cols, _ in groups.values())):
        ha = getattr(a.policy, "stochastic_policy", None) or getattr(a.policy, "policy", a.policy)
        hb = getattr(b.policy, "stochastic_policy", None) or getattr(b.policy, "policy", b.policy)
        if isinstance(ha, TanhGaussianPolicy):
            assert (ha._noise.standard_normal(3) == hb._noise.standard_normal(3)).all()
