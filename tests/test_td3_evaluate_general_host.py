"""Host side of the device evaluation of general-step TD3 trainers (no GPU): where evaluate_td3 / td3_evaluate_many send
each kind of trainer under general="host" and "device" (route, TD3_EVAL_ENTRIES; a recording stand-in takes the library's
place), the keyword the drivers pass, the any-depth reference's layer shapes, the conditioning rule on the oracle's fresh
nets at every shape and row count of tests/test_gpu_td3_evaluate_general.py, and the two new symbols."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

from robosuite_benchmark_amd import _lib, driver, group, infer
from robosuite_benchmark_amd.infer import FUSED, GENERAL_STEP, HOST, TD3_EVAL_ENTRIES, route
from tests import td3_eval_reference as two_layer
from tests.td3_eval_reference import make_td3_trainer
from tests.td3_eval_reference_general import SHAPES, column_scales, conditioned_inputs, net_layers, rows_of, shape_id
from tests.test_infer_routing_host import A, O, DeviceBuffer, Lib, entries, f32_view, make, request, value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Td3Lib(Lib):
    """test_infer_routing_host's stand-in with the two TD3 evaluation entries (logged: entry, handles, n_rows)."""

    def _td3_many(self, entry, handles, n, n_rows, ios):
        for k, (h, r) in enumerate(zip(*self._note(entry, handles, n, n_rows))):
            io = ios[k]
            v = value(h, f32_view(io.obs, r, O)[:, 0])
            f32_view(io.rows, len(_lib.TD3_EVAL_ROWS), r)[...] = v[None, :] + 10000.0 * np.arange(len(_lib.TD3_EVAL_ROWS))[:, None]
            for name in _lib.TD3_EVAL_ARRAYS:
                f32_view(getattr(io, name), r, A)[...] = v[:, None]
        return 0

    def td3_evaluate_many(self, *a):
        return self._td3_many("td3_evaluate_many", *a)

    def td3_evaluate_general_many(self, *a):
        return self._td3_many("td3_evaluate_general_many", *a)

    def td3_evaluate_replay_many(self, *a):
        return self._replay_many("td3_evaluate_replay_many", *a)


@pytest.fixture
def lib(monkeypatch):
    fake = Td3Lib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    return fake


def td3(lib, **kw):
    t = make(lib, td3=True, **kw)
    t.target_policy_noise, t.target_policy_noise_clip = 0.2, 0.5
    return t


KINDS = {"no handle": dict(handle=False), "fused": dict(), "general": dict(hidden=(8, 8, 8), kind=3), "on host": dict(on_host=True)}
ROUTES = {("no handle", "host"): HOST, ("no handle", "device"): HOST, ("fused", "host"): FUSED, ("fused", "device"): FUSED,
          ("general", "host"): HOST, ("general", "device"): GENERAL_STEP, ("on host", "host"): HOST, ("on host", "device"): HOST}


def test_the_entry_table():
    assert TD3_EVAL_ENTRIES == {FUSED: "td3_evaluate_many", GENERAL_STEP: "td3_evaluate_general_many"}
    assert all(name in _lib.SYMBOLS for name in TD3_EVAL_ENTRIES.values())
    assert "no general one" not in inspect.getdoc(route)


@pytest.mark.parametrize("kind,general", list(ROUTES))
def test_route_table(lib, kind, general):
    t = td3(lib, **KINDS[kind])
    want = ROUTES[(kind, general)]
    assert route(t, general, t._evaluate_on_host) == want
    called = [] if want == HOST else [TD3_EVAL_ENTRIES[want]]
    _, _, batch, eps = request(3)
    solo = t.evaluate_td3(batch, eps=eps[0], rows=True, general=general)
    assert entries(lib) == called
    got = infer.td3_evaluate_many([t], [batch], eps=[eps[0]], rows=True, general=general)
    assert entries(lib) == called
    assert got[0][0] == solo[0] and all(np.array_equal(got[0][1][k], solo[1][k]) for k in solo[1])
    if want != HOST:                                  # the stand-in's values landed in their rows
        assert np.array_equal(solo[1]["q2"], value(t._h.value, np.arange(3)) + np.float32(10000.0))
    # the default is "host": the call without the keyword is the call with it
    t.evaluate_td3(batch, eps=eps[0])
    assert entries(lib) == ([] if ROUTES[(kind, "host")] == HOST else ["td3_evaluate_many"])


def test_a_member_served_on_the_device_is_settled(lib):
    """As for the SAC objective (tests/test_infer_routing_host.py): one call path settles the members of both."""
    t = td3(lib)
    _, _, batch, eps = request(3)
    for call, entry in ((lambda: t.evaluate_td3(batch, eps=eps[0]), "td3_evaluate_many"),
                        (lambda: t.evaluate_td3_replay(DeviceBuffer(), indices=[0, 9, 9], eps=eps[0]), "td3_evaluate_replay_many")):
        t._stepped_buffers = (object(),)
        call()
        assert entries(lib) == [entry] and t._stepped_buffers == ()


def test_a_mixed_call_serves_each_family_in_its_own_windows(lib):
    ts = [td3(lib), td3(lib, hidden=(8, 8, 8), kind=3), td3(lib, handle=False), td3(lib, hidden=(300,), kind=3)]
    reqs = [request(n) for n in (5, 1030, 4, 7)]
    got = infer.td3_evaluate_many(ts, [r[2] for r in reqs], eps=[r[3][0] for r in reqs], rows=True, general="device")
    h = [None if t._h is None else t._h.value for t in ts]
    assert lib.log == [("td3_evaluate_many", [h[0]], [5]), ("td3_evaluate_general_many", [h[1], h[3]], [1024, 7]),
                       ("td3_evaluate_general_many", [h[1]], [6])]
    assert np.array_equal(got[1][1]["q1"], value(h[1], np.arange(1030)))
    del lib.log[:]
    infer.td3_evaluate_many(ts, [r[2] for r in reqs], eps=[r[3][0] for r in reqs])
    assert lib.log == [("td3_evaluate_many", [h[0]], [5])]
    for call in (lambda: infer.td3_evaluate_many(ts, [r[2] for r in reqs], general="gpu"),
                 lambda: ts[0].evaluate_td3(reqs[0][2], general="gpu")):
        with pytest.raises(RuntimeError, match="general must be one of"):
            call()
    for kind in (group.TD3TrainerGroup, group.MixedTD3TrainerGroup, group.MlpTD3TrainerGroup, group.ArchTD3TrainerGroup):
        assert inspect.signature(kind.td3_evaluate_many).parameters["general"].default == "host"


def test_the_driver_leaves_the_keyword_out_at_the_default(monkeypatch):
    seen = []

    def without_general(trainers, batches, eps=None, rngs=None, rows=False):
        seen.append("default")
        return [None] * len(trainers)

    def with_general(trainers, batches, eps=None, rngs=None, rows=False, general="host"):
        seen.append(general)
        return [None] * len(trainers)

    class T:
        obs_dim, act_dim = O, A

        def evaluate_td3(self, batch, eps=None, **kw):
            seen.append(("solo", kw))
            return None

    n = 3
    path = dict(observations=np.zeros((n, O)), actions=np.zeros((n, A)), rewards=np.zeros((n, 1)), terminals=np.zeros((n, 1)),
                next_observations=np.zeros((n, O)))
    runs = [dict(trainer=T(), evalc=types.SimpleNamespace(epoch_paths=[path]), seed=1)]
    opts = driver.EvalOptions(td3_validation=True)
    monkeypatch.setattr(driver, "td3_evaluate_many", without_general)
    driver._epoch_evaluations(runs, 0, opts)                          # (a TypeError if the keyword were passed)
    monkeypatch.setattr(driver, "td3_evaluate_many", with_general)
    driver._epoch_evaluations(runs, 0, opts._replace(eval_general="device"))
    driver._epoch_evaluations(runs, 0, opts, many=False)
    driver._epoch_evaluations(runs, 0, opts._replace(eval_general="device"), many=False)
    assert seen == ["default", "device", ("solo", {}), ("solo", dict(general="device"))]
    assert "td3_evaluate_general" in inspect.getdoc(driver.EvalOptions)
    assert "TD3" in open(os.path.join(ROOT, "scripts", "train.py")).read().split('"--eval_general"')[1].split("add_argument")[0]


@pytest.mark.parametrize("O_,A_,hidden,hidden_q", [(42, 7, (256, 256), None), (46, 16, (240, 256), None), (42, 7, (64, 32), (256, 256))])
def test_the_general_layers_are_the_two_layer_ones(O_, A_, hidden, hidden_q):
    t = make_td3_trainer(O_, A_, hidden, hidden_q, seed=5)
    params = {k: getattr(t, k).flat() for k in t.NETS}
    mine, theirs = net_layers(params, O_, A_, hidden, hidden_q), two_layer.net_layers(params, O_, A_, hidden, hidden_q)
    assert list(mine) == list(theirs)
    for name in theirs:
        assert len(mine[name]) == len(theirs[name]) == 3
        for (w, b), (w2, b2) in zip(mine[name], theirs[name]):
            assert w.shape == w2.shape and np.array_equal(w, w2) and np.array_equal(b, b2)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_conditioned_inputs_finds_a_draw_on_fresh_nets(shape):
    """The seeds are the parity test's (tests/test_gpu_td3_evaluate_general.py, fresh weights)."""
    hp, hq, O_, A_ = shape
    t = make_td3_trainer(O_, A_, hp, hq, seed=5)
    layers = net_layers({k: getattr(t, k).flat() for k in t.NETS}, O_, A_, hp, hq)
    assert [w.shape for w, _ in layers["policy"]] == [(n, k) for n, k in zip(list(hp) + [A_], [O_] + list(hp))]
    assert [w.shape for w, _ in layers["target_qf2"]] == [(n, k) for n, k in zip(list(hq or hp) + [1], [O_ + A_] + list(hq or hp))]
    scales = column_scales(t, O_ + A_)
    assert set(rows_of(shape)) <= {1, 15, 16, 17, 33, 1000, 1024}
    for n in (1, 15, 16, 17, 33, 1000, 1024):
        batch, eps = conditioned_inputs(t, n, O_ + A_ + n, scales)
        assert batch[0].shape == (n, O_) and eps.shape == (n, A_)


def test_both_symbols_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    for name in ("td3_evaluate_general", "td3_evaluate_general_many"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[name.replace("_general", "")]
    assert _lib.SYMBOLS["td3_evaluate_general"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p])
    src = open(os.path.join(ROOT, "robosuite_benchmark_amd", "csrc", "td3_eval_general.h")).read()
    assert "k_eval_layer_td3" in src and "td3_eval_smooth(" in src and "atomic" not in src.replace("no atomics", "")
    for doc in ("README.md", "DESIGN.md"):
        assert "td3_evaluate_general" in open(os.path.join(ROOT, doc)).read(), doc
    sig = inspect.signature
    assert all(sig(f).parameters["general"].default == "host"
               for f in (infer.td3_evaluate_many, infer.td3_evaluate_of, group.td3_evaluate_many))
    from robosuite_benchmark_amd import TD3Trainer
    assert sig(TD3Trainer.evaluate_td3).parameters["general"].default == "host"
