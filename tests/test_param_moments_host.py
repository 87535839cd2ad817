"""Host side of the per-tensor parameter statistics (no GPU, no library): infer.param_moments_reference against math.fsum
and against a plain loop over lanes, its edges, param_statistics on hand-made records, the declarations (header, ctypes
mirror, keywords), the host route of trainers without a handle, and where the driver puts the params/ block."""
import ctypes
import importlib.util
import inspect
import math
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

from robosuite_benchmark_amd import _lib, driver, infer
from robosuite_benchmark_amd.group import (SACTrainerGroup, param_moments_many, param_moments_reference, param_statistics)
from tests import test_driver_epochs_host as epochs
from tests.param_reference import CH, F, loop_record, same_bytes, same_values
from tests.test_infer_routing_host import Lib, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("sum", "sumsq", "absmax", "nonfinite", "m_sumsq", "m_absmax", "v_sum", "v_max", "gap_sumsq")
SIZES = [1, 255, 256, 257, CH - 1, CH, CH + 1, 3 * CH + 5]


def tensors(E, seed=0):
    rs = np.random.RandomState(1000 + E + seed)
    x = rs.normal(0, 1, E).astype(np.float32)
    m = rs.normal(0, 1e-2, E).astype(np.float32)
    v = (rs.normal(0, 1e-2, E) ** 2).astype(np.float32)
    t = (x + rs.normal(0, 1e-3, E)).astype(np.float32)
    return x, m, v, t


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", SIZES)
def test_sums_stay_within_the_bound_of_fsum(E):
    """Any order of E float64 additions stays within (E - 1) u sum|x| (1 + O(E u)) of the exact sum, u = 2^-53 (Higham,
    Accuracy and Stability, 4.2); 8 E 2^-53 sum|x| is that with room.  The elements themselves (x, x x, m m, v) are exact
    float64 values; the gap's (x - t)^2 is rounded once, which 8 E u sum|.| covers too."""
    x, m, v, t = tensors(E)
    rec = param_moments_reference(x, m, v, t)
    assert rec.shape == (9,) and rec.dtype == np.float64
    xd, md, vd, td = (a.astype(np.float64) for a in (x, m, v, t))
    for field, elems in (("sum", xd), ("sumsq", xd * xd), ("m_sumsq", md * md), ("v_sum", vd), ("gap_sumsq", (xd - td) ** 2)):
        exact = math.fsum(elems.tolist())
        bound = 8 * E * 2.0 ** -53 * math.fsum(np.abs(elems).tolist())
        assert abs(rec[F[field]] - exact) <= bound, (field, rec[F[field]], exact, bound)
    assert rec[F["absmax"]] == float(np.max(np.abs(x))) and rec[F["nonfinite"]] == 0.0
    assert rec[F["m_absmax"]] == float(np.max(np.abs(m))) and rec[F["v_max"]] == float(np.max(v))


@pytest.mark.parametrize("E", SIZES)
def test_reference_is_the_plain_loop_across_the_chunk_boundary(E):
    x, m, v, t = tensors(E, 1)
    assert same_bytes(param_moments_reference(x, m, v, t), loop_record(x, m, v, t))
    assert same_bytes(param_moments_reference(x), loop_record(x))
    # what is not given is exactly 0.0, and the other fields do not move
    full, bare = param_moments_reference(x, m, v, t), param_moments_reference(x)
    assert same_bytes(bare[:4], full[:4]) and np.all(bare[4:] == 0.0) and not np.any(np.signbit(bare[4:]))
    assert same_bytes(param_moments_reference(x, m, v)[:8], full[:8]) and param_moments_reference(x, m, v)[8] == 0.0
    # a tensor given as a matrix is its flat order
    if E % 3 == 0:
        assert same_bytes(param_moments_reference(x.reshape(3, -1)), bare)


@pytest.mark.parametrize("E", [1, 257, CH + 1])
def test_the_order_is_a_function_of_the_element_count_alone(E):
    """A prefix of a longer tensor's elements, reduced as a tensor of its own, gives the record of that count: nothing of
    the longer tensor's chunking leaks in."""
    x = tensors(3 * CH + 5)[0]
    assert same_bytes(param_moments_reference(x[:E]), loop_record(x[:E]))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", [0, 300, CH, CH + 77])
def test_a_planted_non_finite_is_counted_and_a_nan_stays(bad, where):
    x, m, v, t = tensors(CH + 100, 2)
    clean = param_moments_reference(x, m, v, t)
    x[where] = bad
    rec = param_moments_reference(x, m, v, t)
    assert same_values(rec, loop_record(x, m, v, t))
    assert rec[F["nonfinite"]] == 1.0
    if np.isnan(bad):
        assert np.isnan(rec[F["absmax"]]) and np.isnan(rec[F["sum"]]) and np.isnan(rec[F["sumsq"]]) and np.isnan(rec[F["gap_sumsq"]])
    else:
        assert rec[F["absmax"]] == np.inf and rec[F["sum"]] == bad and rec[F["sumsq"]] == np.inf
    assert same_bytes(rec[4:8], clean[4:8])               # Adam's fields read m and v only
    x[where + 1 if where + 1 < x.size else 0] = np.nan
    x[5] = np.inf
    assert param_moments_reference(x)[F["nonfinite"]] == 3.0 and np.isnan(param_moments_reference(x)[F["absmax"]])
    # in the moments: theirs alone
    x, m, v, t = tensors(CH + 100, 2)
    m[where] = bad
    rec = param_moments_reference(x, m, v, t)
    assert same_bytes(rec[:4], clean[:4]) and rec[F["nonfinite"]] == 0.0
    assert np.isnan(rec[F["m_absmax"]]) if np.isnan(bad) else rec[F["m_absmax"]] == np.inf


@pytest.mark.parametrize("E", [1, 256, CH + 3])
def test_an_all_zero_tensor_gives_all_zero_fields(E):
    z = np.zeros(E, np.float32)
    rec = param_moments_reference(z, z, z, z)
    assert np.all(rec == 0.0) and not np.any(np.signbit(rec))
    assert same_bytes(rec, loop_record(z, z, z, z))
    # a negative second moment (only a setter can plant one) is still the largest value, not 0
    assert param_moments_reference(z, z, z - np.float32(2.0))[F["v_max"]] == -2.0
    with pytest.raises(ValueError):
        param_moments_reference(np.zeros(0, np.float32))
    with pytest.raises(ValueError):
        param_moments_reference(z, z[:-1] if E > 1 else np.zeros(2, np.float32), z)


def test_known_values():
    x = np.array([3.0, -4.0], np.float32)
    rec = param_moments_reference(x, np.array([1.0, -2.0], np.float32), np.array([0.5, 0.25], np.float32),
                                  np.array([3.0, -4.5], np.float32))
    assert rec.tolist() == [-1.0, 25.0, 4.0, 0.0, 5.0, 2.0, 0.75, 0.5, 0.25]
    # one element moved by a float32 amount: the gap is that amount squared, exactly
    x = tensors(CH + 9)[0]
    t = x.copy()
    d = np.float32(2.0 ** -10)
    x[CH + 1] = np.float32(1.5)
    t[CH + 1] = np.float32(1.5) + d
    assert param_moments_reference(x, target=t)[F["gap_sumsq"]] == float(d) * float(d)
    assert param_moments_reference(x, target=x)[F["gap_sumsq"]] == 0.0


# ---- the figures ------------------------------------------------------------------------------------------------------------
def test_param_statistics_on_hand_made_records():
    def rec(**kw):
        r = np.zeros(9)
        for k, v in kw.items():
            r[F[k]] = v
        return r
    moments = OrderedDict([
        ("policy", np.stack([rec(sumsq=9.0, absmax=2.0, m_sumsq=1.0, m_absmax=1.0, v_sum=6.0, v_max=0.5),
                             rec(sumsq=16.0, absmax=3.0, m_sumsq=3.0, v_sum=2.0, v_max=0.25)])),
        ("qf1", np.stack([rec(sumsq=4.0, absmax=1.0, nonfinite=2.0, gap_sumsq=1.0, v_sum=1.0, v_max=1.0)])),
        ("target_qf1", np.stack([rec(sumsq=100.0, absmax=9.0, nonfinite=1.0)])),
    ])
    sizes = dict(policy=[6, 2], qf1=[4], target_qf1=[4])
    d = param_statistics(moments, sizes)
    assert list(d) == ["Policy " + f for f in infer.PARAM_FIGURES] + ["QF1 " + f for f in infer.PARAM_FIGURES] + [
        "QF1 Target Gap", "Non Finite"]
    assert d["Policy Weight Norm"] == 5.0 and d["Policy Weight Abs Max"] == 3.0 and d["Policy Adam M Norm"] == 2.0
    assert d["Policy Adam V Mean"] == 1.0 and d["Policy Adam V Max"] == 0.5
    assert d["QF1 Weight Norm"] == 2.0 and d["QF1 Target Gap"] == 0.5 and d["QF1 Adam V Mean"] == 0.25
    assert d["Non Finite"] == 3.0
    # a TD3 trainer's policy has a target too
    d3 = param_statistics(moments, sizes, targets=("policy", "qf1"))
    assert d3["Policy Target Gap"] == 0.0 and list(d3).index("Policy Target Gap") == 5
    # a NaN stays in the maximum
    moments["qf1"][0, F["absmax"]] = np.nan
    assert math.isnan(param_statistics(moments, sizes)["QF1 Weight Abs Max"])


# ---- declarations -----------------------------------------------------------------------------------------------------------
def test_declarations():
    text = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    m = re.search(r"typedef struct sac_params_io \{(.*?)\} sac_params_io_t;", text, flags=re.S)
    assert m, "sac_params_io_t is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t nets", "uint32_t flags", "double *moments"]
    assert [(n, c) for n, c in _lib.SacParamsIO._fields_] == [("nets", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                                                              ("moments", ctypes.c_void_p)]
    assert ctypes.sizeof(_lib.SacParamsIO) == 16 and _lib.SacParamsIO.flags.offset == 4 and _lib.SacParamsIO.moments.offset == 8
    assert re.search(r"enum \{ SAC_PARAM_SUM, SAC_PARAM_SUMSQ, SAC_PARAM_ABSMAX, SAC_PARAM_NONFINITE, SAC_PARAM_M_SUMSQ, "
                     r"SAC_PARAM_M_ABSMAX,\s+SAC_PARAM_V_SUM, SAC_PARAM_V_MAX, SAC_PARAM_GAP_SUMSQ, SAC_PARAM_FIELDS_N \};", text)
    assert re.search(r"enum \{ SAC_PARAMS_OPT = 1, SAC_PARAMS_GAP = 2 \};", text)
    assert _lib.PARAM_FIELDS == FIELDS and (_lib.PARAMS_OPT, _lib.PARAMS_GAP) == (1, 2)
    for name in ("sac_param_tensors", "sac_param_moments", "sac_param_moments_many"):
        assert re.search(r"\bint " + name + r"\(", text) and name in _lib.SYMBOLS
    src = open(os.path.join(ROOT, "robosuite_benchmark_amd", "csrc", "sac_params.h")).read()
    assert re.search(r"constexpr int PM_CH = (\d+);", src).group(1) == str(infer.PARAM_CH) == "16384"
    assert re.search(r"constexpr int PM_LANES = (\d+);", src).group(1) == str(infer.PARAM_LANES) == "256"


def test_the_keywords_and_their_defaults():
    for fn in (driver.experiment, driver.experiment_group, driver.experiment_sweep):
        assert inspect.signature(fn).parameters["param_diagnostics"].default is False, fn.__name__
    assert driver.EvalOptions._field_defaults["param_diagnostics"] is False
    from robosuite_benchmark_amd import TD3Trainer
    from robosuite_benchmark_amd.sac import SACTrainer
    for cls in (SACTrainer, TD3Trainer):
        p = inspect.signature(cls.param_moments).parameters
        assert [(k, v.default) for k, v in p.items()][1:] == [("nets", None), ("opt", True), ("gap", True), ("route", "device")]
        assert "net" in inspect.signature(cls.param_tensors).parameters
    p = inspect.signature(param_moments_many).parameters
    assert p["route"].default == "device" and p["opt"].default is True and p["gap"].default is True
    assert inspect.signature(SACTrainerGroup.param_moments_many).parameters["route"].default == "device"
    assert infer.param_moments_many is param_moments_many and infer.PARAM_ROUTES == ("device", "host")


def test_train_script_parses_the_option():
    spec = importlib.util.spec_from_file_location("train_script_params", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args([]).param_diagnostics is False
    assert ap.parse_args(["--param_diagnostics"]).param_diagnostics is True
    src = open(os.path.join(ROOT, "scripts", "train.py")).read()
    assert 'option_kw["param_diagnostics"] = True' in src


# ---- trainers without a handle ----------------------------------------------------------------------------------------------
class NoParamLib(Lib):
    """The stand-in library without the device entry: whoever reaches for it fails."""

    def sac_param_moments_many(self, *a):
        raise AssertionError("the device entry was called for a trainer without a handle")


@pytest.fixture
def lib(monkeypatch):
    fake = NoParamLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    return fake


@pytest.mark.parametrize("td3", [False, True])
@pytest.mark.parametrize("hidden", [(8, 8), (8, 8, 8)])
def test_trainers_without_a_handle_take_the_host_route(lib, td3, hidden):
    t = make(lib, hidden=hidden, handle=False, td3=td3)
    names = [n for n, _ in t.param_tensors("policy")]
    heads = ["last_fc.weight", "last_fc.bias"] + ([] if td3 else ["last_fc_log_std.weight", "last_fc_log_std.bias"])
    assert names == [f"fc{i}.{k}" for i in range(len(hidden)) for k in ("weight", "bias")] + heads
    assert t.param_tensors("qf1")[0] == ("fc0.weight", (hidden[0], 6)) and t.param_tensors("qf1")[-1] == ("last_fc.bias", (1,))
    for route in ("device", "host"):
        got = t.param_moments(route=route)
        assert list(got) == list(t.NETS)
        for net, rec in got.items():
            flat = getattr(t, net).flat()
            shapes = t.param_tensors(net)
            assert rec.shape == (len(shapes), 9) and rec.dtype == np.float64
            target = getattr(t, infer.param_target(t, net)).flat() if infer.param_target(t, net) else None
            off = 0
            for row, (_, shape) in zip(rec, shapes):
                e = int(np.prod(shape))
                z = np.zeros(e, np.float32) if net in infer.PARAM_TRAINED else None      # (fresh Adam moments)
                assert same_bytes(row, param_moments_reference(flat[off:off + e], z, z,
                                                               None if target is None else target[off:off + e]))
                off += e
            assert off == flat.size
    assert infer.param_target(t, "policy") == ("target_policy" if td3 else None)
    # a selection, its order, the flags
    got = t.param_moments(nets=("qf2", "policy"), opt=False, gap=False)
    assert list(got) == ["qf2", "policy"] and np.all(got["qf2"][:, 4:] == 0.0)
    assert same_bytes(got["qf2"][:, :4], t.param_moments()["qf2"][:, :4])
    many = param_moments_many([t, make(lib, handle=False)], [("qf1",), None])
    assert list(many[0]) == ["qf1"] and many[1] is None
    for bad, err in ((dict(nets=()), ValueError), (dict(nets=("qf9",)), ValueError), (dict(nets=("qf1", "qf1")), ValueError),
                     (dict(route="gpu"), RuntimeError)):
        with pytest.raises(err):
            t.param_moments(**bad)
    if not td3:
        with pytest.raises(ValueError):
            t.param_moments(nets=("target_policy",))
    with pytest.raises(RuntimeError, match="twice"):
        param_moments_many([t, t])


# ---- the driver -------------------------------------------------------------------------------------------------------------
PARENT_HEADER = [
    "replay_buffer/size", "trainer/QF1 Loss", "trainer/Policy Loss", "trainer/Init Sum", "trainer/num train steps"]


class ParamTrainer(epochs.FakeTrainer):
    NETS = _lib.NET_IDS

    def _params(self):
        x = float(self.policy.flat()[0])
        rec = np.zeros((2, 9))
        rec[:, F["sumsq"]] = (x * x, 1.0)
        rec[:, F["absmax"]] = (abs(x), 1.0)
        rec[:, F["v_sum"]] = (2.0, 4.0)
        rec[:, F["gap_sumsq"]] = (1.0, 0.0)
        return OrderedDict((n, rec.copy()) for n in _lib.NET_IDS)

    def param_tensors(self, net):
        return [("fc0.weight", (2, 2)), ("fc0.bias", (2,))]

    def param_moments(self, **kw):
        epochs.LOG.append(("param_moments", self.seed, kw))
        return self._params()


def fake_param_moments_many(trainers, **kw):
    epochs.LOG.append(("param_moments_many", None, kw))
    return [t._params() for t in trainers]


PARAM_KEYS = [f"params/{t} {f}" for t in ("Policy", "QF1", "QF2")
              for f in infer.PARAM_FIGURES + (("Target Gap",) if t != "Policy" else ())] + ["params/Non Finite"]


@pytest.fixture
def stand_ins(monkeypatch):
    for name, fake in dict(SACTrainer=ParamTrainer, EnvReplayBuffer=epochs.FakeBuffer, SACTrainerGroup=epochs.FakeGroup,
                           MixedSACTrainerGroup=epochs.FakeGroup, q_values_many=epochs.fake_q_values_many,
                           evaluate_many=epochs.fake_evaluate_many, evaluate_replay_many=epochs.fake_evaluate_replay_many,
                           param_moments_many=fake_param_moments_many, SyntheticEnv=epochs.LoggingEnv).items():
        assert hasattr(driver, name), name
        monkeypatch.setattr(driver, name, fake)
    del epochs.LOG[:], epochs.FakeTrainer.made[:]


def test_with_the_option_off_the_header_is_the_parents(stand_ins):
    rows = epochs.solo(3)
    keys = list(rows[0])
    assert keys[:5] == PARENT_HEADER and keys[-9:] == ["time/" + k + " (s)" for k in (
        "data storing", "evaluation sampling", "exploration sampling", "logging", "saving", "training", "epoch", "total")] + ["Epoch"]
    assert all(k.split("/")[0] in ("replay_buffer", "trainer", "exploration", "evaluation", "time") or k == "Epoch" for k in keys)
    assert len(keys) == len(set(keys)) and not [k for k in keys if k.startswith("params/")]
    for entry in (epochs.group, epochs.sweep):
        got = entry()
        for s in epochs.SEEDS:
            epochs.assert_rows_equal(got[s], epochs.solo(s), (entry.__name__, s))
    _, log = epochs.logged(epochs.solo, 3, **epochs.ALL_ON)
    assert not [n for n, _, _ in log if n.startswith("param")]


def test_the_params_block_stands_last_in_front_of_time(stand_ins):
    off = epochs.solo(3, **epochs.ALL_ON)
    on = epochs.solo(3, param_diagnostics=True, **epochs.ALL_ON)
    plain, only = epochs.solo(3), epochs.solo(3, param_diagnostics=True)
    n = len(PARAM_KEYS)
    for with_params, without in ((on, off), (only, plain)):
        for row, ref in zip(with_params, without):
            keys = list(row)
            i = keys.index(PARAM_KEYS[0])
            assert keys[i:i + n] == PARAM_KEYS and keys[i + n] == "time/data storing (s)"
            assert keys[:i] + keys[i + n:] == list(ref)
            assert all(k.startswith("time/") or epochs.same(row[k], ref[k]) for k in ref)
            assert row["params/QF1 Adam V Mean"] == 1.0 and row["params/Non Finite"] == 0.0
            assert row["params/QF1 Target Gap"] == 1.0 / row["params/QF1 Weight Norm"]
    assert list(on[0])[list(on[0]).index(PARAM_KEYS[0]) - 1].startswith("replay/")


@pytest.mark.parametrize("entry", ["group", "sweep"])
@pytest.mark.parametrize("acting", ["host", "device"])
def test_group_rows_are_solo_rows_and_one_call_per_epoch(stand_ins, entry, acting):
    solo_rows = {s: epochs.solo(s, param_diagnostics=True, validation=True) for s in epochs.SEEDS}
    _, log = epochs.logged(epochs.solo, 3, param_diagnostics=True)
    assert [(n, kw) for n, _, kw in log if n.startswith("param")] == [("param_moments", {})] * epochs.EPOCHS
    rows, log = epochs.logged(getattr(epochs, entry), acting=acting, param_diagnostics=True, validation=True)
    assert [(n, k) for n, _, k in log if n.startswith("param")] == [("param_moments_many", {})] * epochs.EPOCHS
    names = epochs.calls(log, by_seed=False)
    assert names.index("param_moments_many") == names.index("evaluate_many") + 1       # (where validation is taken)
    for s in epochs.SEEDS:
        epochs.assert_rows_equal(rows[s], solo_rows[s], (entry, acting, s))
        epochs.assert_times(rows[s], (entry, acting, s))
