"""Host side of the per-unit statistics (no GPU, no library): infer.unit_moments_reference against a plain Python loop,
merge_unit_moments, unit_statistics on hand-built records, the routing and the windows of unit_moments /
unit_moments_many over a recording stand-in library, the declarations (header, ctypes mirror, EvalOptions), and where
the driver puts the units/ block and how scripts/train.py passes the options on."""
import ctypes
import importlib.util
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

from robosuite_benchmark_amd import _lib, driver, infer
from robosuite_benchmark_amd.group import (ArchSACTrainerGroup, merge_unit_moments, unit_moments_many, unit_moments_reference,
                                           unit_statistics)
from tests import test_driver_epochs_host as epochs
from tests.test_infer_routing_host import O, Lib, f32_view, make, request, value, window_log
from tests.unit_reference import loop_moments, same_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("sum", "sumsq", "active", "max")


# ---- the reference against a plain loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1024])
def test_reference_is_the_plain_loop(n):
    rs = np.random.RandomState(n)
    N = 70 if n < 1024 else 5
    h = np.maximum(rs.normal(0, 1, (n, N)), 0).astype(np.float32)
    got = unit_moments_reference(h)
    assert got["count"] == n and all(got[f].shape == (N,) and got[f].dtype == np.float64 for f in FIELDS)
    assert same_record(got, loop_moments(h))
    assert np.array_equal(got["active"], (h > 0).sum(0)) and np.array_equal(got["max"], h.max(0).astype(np.float64))
    assert np.allclose(got["sum"], h.astype(np.float64).sum(0), rtol=1e-12, atol=0)


def test_reference_edges():
    # a constant column: sum = n b exactly when b is a float32 (every partial sum is a multiple of b below 2^53)
    for n in (1, 5, 1024):
        b = np.float32(0.3)
        rec = unit_moments_reference(np.full((n, 3), b, np.float32))
        assert np.all(rec["sum"] == n * float(b)) and np.all(rec["sumsq"] == n * (float(b) * float(b)))
        assert np.all(rec["active"] == n) and np.all(rec["max"] == float(b))
    # a NaN element: sum, sumsq and max NaN, not active; the other units untouched
    h = np.ones((9, 4), np.float32)
    h[6, 2] = np.nan
    rec = unit_moments_reference(h)
    assert same_record(rec, loop_moments(h))
    assert np.isnan(rec["sum"][2]) and np.isnan(rec["sumsq"][2]) and np.isnan(rec["max"][2]) and rec["active"][2] == 8
    assert np.all(rec["sum"][[0, 1, 3]] == 9) and np.all(rec["max"][[0, 1, 3]] == 1)
    # a NaN in the first row and in the last one
    for r in (0, 8):
        h = np.ones((9, 2), np.float32)
        h[r, 0] = np.nan
        assert np.isnan(unit_moments_reference(h)["max"][0]) and same_record(unit_moments_reference(h), loop_moments(h))
    # +-0: not active, sum and max are zeros of the loop's signs
    h = np.array([[0.0, -0.0], [-0.0, -0.0], [0.0, -0.0]], np.float32)
    rec = unit_moments_reference(h)
    assert same_record(rec, loop_moments(h))
    assert np.all(rec["active"] == 0) and np.all(rec["sum"] == 0) and np.all(rec["max"] == 0)
    with pytest.raises(ValueError):
        unit_moments_reference(np.zeros((0, 3), np.float32))


def test_merge_of_two_windows():
    rs = np.random.RandomState(2)
    for na, nb in ((1024, 6), (5, 1), (1024, 1024)):
        h = np.maximum(rs.normal(0.2, 1, (na + nb, 33)), 0).astype(np.float32)
        h[3, 7] = 0.0
        whole = unit_moments_reference(h)
        a, b = unit_moments_reference(h[:na]), unit_moments_reference(h[na:])
        got = merge_unit_moments(dict(a, h=h[:na]), dict(b, h=h[na:]))
        n = na + nb
        assert got["count"] == n and np.array_equal(got["h"], h)
        assert np.array_equal(got["active"], whole["active"]) and np.array_equal(got["max"], whole["max"])
        bound = 8 * n * 2.0 ** -53 * float(np.max(np.abs(h)))
        assert np.all(np.abs(got["sum"] - whole["sum"]) <= bound)
        assert np.all(np.abs(got["sumsq"] - whole["sumsq"]) <= bound * float(np.max(np.abs(h))))
    nan = unit_moments_reference(np.array([[np.nan, 1.0]], np.float32))
    one = unit_moments_reference(np.array([[2.0, 2.0]], np.float32))
    for m in (merge_unit_moments(nan, one), merge_unit_moments(one, nan)):
        assert np.isnan(m["max"][0]) and np.isnan(m["sum"][0]) and m["max"][1] == 2 and m["active"][0] == 1


# ---- unit_statistics ----------------------------------------------------------------------------------------------------------
def record(h):
    return unit_moments_reference(np.asarray(h, np.float32))


def test_unit_statistics_on_hand_built_records():
    zero = record(np.zeros((4, 5)))
    d = unit_statistics(OrderedDict(policy=[zero]))
    assert list(d) == ["Policy Dormant Fraction", "Policy Dead Fraction", "Policy Active Fraction", "Policy Feature Norm"]
    assert d["Policy Dormant Fraction"] == 1 and d["Policy Dead Fraction"] == 1
    assert d["Policy Active Fraction"] == 0 and d["Policy Feature Norm"] == 0
    # one live unit among dead ones: the layer's mean is a quarter of it
    h = np.zeros((4, 4))
    h[:2, 1] = 2.0
    d = unit_statistics(OrderedDict(qf1=[record(h)]))
    assert d["QF1 Dormant Fraction"] == 0.75 and d["QF1 Dead Fraction"] == 0.75
    assert d["QF1 Active Fraction"] == 0.5 / 4 and d["QF1 Feature Norm"] == np.sqrt(8.0 / 4)
    # a weak unit: dormant at tau = 0.025 when its mean is at most 2.5 % of the layer's; tau = 0 counts the zero sums alone
    h = np.ones((2, 4))
    h[:, 0], h[:, 3] = 0.01, 0.0
    rec = record(h)
    assert unit_statistics(OrderedDict(qf2=[rec]))["QF2 Dormant Fraction"] == 0.5
    assert unit_statistics(OrderedDict(qf2=[rec]), tau=0)["QF2 Dormant Fraction"] == 0.25
    assert unit_statistics(OrderedDict(qf2=[rec]), tau=0.01)["QF2 Dormant Fraction"] == 0.25
    # over all hidden units of a net, each layer against its own mean; the feature norm is the last layer's
    two = unit_statistics(OrderedDict(policy=[zero, record(np.full((4, 15), 3.0))]))
    assert two["Policy Dormant Fraction"] == 5 / 20 and two["Policy Dead Fraction"] == 5 / 20
    assert two["Policy Active Fraction"] == 15 / 20 and two["Policy Feature Norm"] == np.sqrt(15 * 9.0)
    # keys and their order: the nets as given, four figures each
    d = unit_statistics(OrderedDict([("target_policy", [zero]), ("policy", [zero]), ("target_qf2", [zero])]))
    assert list(d) == [f"{t} {f}" for t in ("Target Policy", "Policy", "Target QF2") for f in infer.UNIT_FIGURES]
    # NaN follows NumPy
    d = unit_statistics(OrderedDict(qf1=[record([[np.nan, 1.0], [1.0, 1.0]])]))
    assert d["QF1 Dormant Fraction"] == 0 and d["QF1 Dead Fraction"] == 0 and d["QF1 Active Fraction"] == 0.75
    assert np.isnan(d["QF1 Feature Norm"])


# ---- routing and windows over a stand-in library ------------------------------------------------------------------------------
FUSED_ENTRY, GENERAL_ENTRY = "sac_unit_moments_many", "sac_unit_moments_general_many"
NET_OF_BIT = {k: name for name, k in _lib.TD3_NET_IDS.items()}


def fake_h(handle, rows, net_id, layer, N):
    """The stand-in's activations: a function of (handle, row index, net, layer, unit), exact in float32."""
    return (value(handle % 64, rows)[:, None] + np.float32(100 * net_id + 10 * layer) + np.arange(N, dtype=np.float32)[None, :] / 4)


class UnitLib(Lib):
    def sac_unit_moments_many(self, *a):
        return self._unit_many(FUSED_ENTRY, *a)

    def sac_unit_moments_general_many(self, *a):
        return self._unit_many(GENERAL_ENTRY, *a)

    def _unit_many(self, entry, handles, n, n_rows, ios):
        for k, (h, r) in enumerate(zip(*self._note(entry, handles, n, n_rows))):
            io, t = ios[k], self.by_handle[h][0]
            rows = f32_view(io.obs, r, O)[:, 0]
            assert io.nets and (io.act or not io.nets & 0x1e)
            widths = [t._hidden(NET_OF_BIT[b]) for b in range(6) if io.nets >> b & 1]
            units = sum(sum(w) for w in widths)
            mom = np.ctypeslib.as_array((C_DOUBLE * (4 * units)).from_address(io.moments))
            taps = f32_view(io.activations, r * units) if io.activations else None
            m0 = h0 = 0
            for b in [b for b in range(6) if io.nets >> b & 1]:
                for l, N in enumerate(t._hidden(NET_OF_BIT[b])):
                    x = fake_h(h, rows, b, l, N)
                    rec = unit_moments_reference(x)
                    for f in FIELDS:
                        mom[m0:m0 + N] = rec[f]
                        m0 += N
                    if taps is not None:
                        taps[h0:h0 + r * N] = x.ravel()
                        h0 += r * N
        return 0


C_DOUBLE = ctypes.c_double


@pytest.fixture
def lib(monkeypatch):
    fake = UnitLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    return fake


def entries(lib):
    got = [c[0] for c in lib.log]
    del lib.log[:]
    return got


KINDS = {"no handle": dict(handle=False), "fused": dict(), "general": dict(hidden=(8, 8, 8), kind=3),
         "td3": dict(td3=True), "td3 general": dict(td3=True, hidden=(8, 8, 8), kind=3)}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("general", ["host", "device"])
def test_route_table(lib, kind, general):
    t = make(lib, **KINDS[kind])
    obs, act, _, _ = request(3)
    want = [] if kind == "no handle" else [FUSED_ENTRY] if "general" not in kind else [GENERAL_ENTRY] if general == "device" else []
    nets = ("qf2", "policy") + (("target_policy",) if "td3" in kind else ())
    got = t.unit_moments(obs, act, nets=nets, general=general)
    assert entries(lib) == want and list(got) == list(nets)
    many = unit_moments_many([t], [obs], [act], [nets], general=general)
    assert entries(lib) == want
    assert ArchSACTrainerGroup.unit_moments_many.__defaults__ == (None, False, "host")
    for net in nets:
        assert [r["sum"].size for r in got[net]] == list(t._hidden(net)) and all(r["count"] == 3 for r in got[net])
        for x, y in zip(got[net], many[0][net]):
            assert same_record(x, y)
    if not want:                                  # the host path: the float32 NumPy forward and the reference
        full = t.unit_moments(obs, act, nets=nets, activations=True, general=general)
        for net in nets:
            layers = t._host_hidden(net)
            h = np.concatenate([obs, act], axis=1) if net in _lib.UNIT_Q_NETS else obs
            for (w, b), r, r0 in zip(layers, full[net], got[net]):
                h = h @ w.T + b
                h = np.where(h < 0, np.float32(0), h)
                assert r["h"].dtype == np.float32 and np.array_equal(r["h"], h) and "h" not in r0
                assert same_record(r, unit_moments_reference(h)) and same_record(r, r0)
    # `general` is checked in front of everything, and the argument checks in front of any call
    with pytest.raises(RuntimeError, match="general"):
        t.unit_moments(obs, act, general="gpu")
    with pytest.raises(ValueError, match="unknown network"):
        t.unit_moments(obs, act, nets=("qf9",), general=general)
    if "td3" not in kind:
        with pytest.raises(ValueError, match="unknown network"):
            t.unit_moments(obs, act, nets=("target_policy",), general=general)
    with pytest.raises(ValueError, match="twice"):
        t.unit_moments(obs, act, nets=("qf1", "qf1"), general=general)
    with pytest.raises(ValueError, match="actions are None"):
        t.unit_moments(obs, None, nets=("policy", "qf1"), general=general)
    with pytest.raises(ValueError, match="actions"):
        t.unit_moments(obs, act[:2], nets=("qf1",), general=general)
    with pytest.raises(RuntimeError, match="twice"):
        unit_moments_many([t, t], [obs, obs], [act, act], [nets, nets], general=general)
    assert entries(lib) == []
    assert t.unit_moments(obs, nets="policy", general=general)["policy"][0]["count"] == 3      # (no actions needed)
    assert unit_moments_many([t], [None], [None], [nets], general=general) == [None]
    del lib.log[:]


@pytest.mark.parametrize("R,members_per_call", [(35, [16, 12, 14, 7]), (42, [16, 16, 1, 16, 8])])
@pytest.mark.parametrize("entry,general,hidden,kind", [(FUSED_ENTRY, "host", (8, 3), 1), (GENERAL_ENTRY, "device", (8, 3, 8), 3)])
def test_windows_of_1024_rows_and_16_members(lib, R, members_per_call, entry, general, hidden, kind):
    ts = [make(lib, hidden=hidden, kind=kind, td3=bool(i % 3 == 0)) for i in range(R)]
    hs = [t._h.value for t in ts]
    n_rows = [(0, 1, 1024, 1025, 2049)[i % 5] for i in range(R)]
    reqs = [request(n) for n in n_rows]
    nets = [("qf2", "policy") if i % 2 else ("target_qf1",) for i in range(R)]
    got = unit_moments_many(ts, [r[0] for r in reqs], [r[1] for r in reqs], nets, activations=True, general=general)
    assert [len(c[1]) for c in lib.log] == members_per_call
    assert lib.log == window_log(entry, hs, n_rows)
    for i, n in enumerate(n_rows):
        if n == 0:
            assert got[i] is None
            continue
        assert list(got[i]) == list(nets[i])
        for net in nets[i]:
            assert len(got[i][net]) == len(hidden)
            for l, (N, r) in enumerate(zip(hidden, got[i][net])):
                h = fake_h(hs[i], np.arange(n, dtype=np.float32), _lib.TD3_NET_IDS[net], l, N)
                assert r["count"] == n and np.array_equal(r["h"], h), (i, net, l)
                want = None
                for r0 in range(0, n, 1024):      # the windows' records, joined
                    part = unit_moments_reference(h[r0:r0 + 1024])
                    want = part if want is None else merge_unit_moments(want, part)
                assert same_record(r, want), (i, net, l)


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_declarations():
    text = open(os.path.join(ROOT, "include", "sac_hip.h")).read()
    m = re.search(r"typedef struct sac_units_io \{(.*?)\} sac_units_io_t;", text, flags=re.S)
    assert m, "sac_units_io_t is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["const float *obs", "const float *act", "uint32_t nets, reserved", "double *moments", "float *activations"]
    assert [f[0] for f in _lib.SacUnitsIO._fields_] == ["obs", "act", "nets", "reserved", "moments", "activations"]
    assert ctypes.sizeof(_lib.SacUnitsIO) == 40 and _lib.SacUnitsIO.nets.offset == 16 and _lib.SacUnitsIO.moments.offset == 24
    assert re.search(r"enum \{ SAC_UNIT_SUM, SAC_UNIT_SUMSQ, SAC_UNIT_ACTIVE, SAC_UNIT_MAX, SAC_UNIT_FIELDS_N \};", text)
    assert _lib.UNIT_FIELDS == FIELDS
    assert _lib.UNIT_NET_BITS == dict(policy=1, qf1=2, qf2=4, target_qf1=8, target_qf2=16, target_policy=32)
    for name in ("sac_unit_moments", "sac_unit_moments_many", "sac_unit_moments_general", "sac_unit_moments_general_many"):
        assert re.search(r"\bint " + name + r"\(", text) and name in _lib.SYMBOLS
    assert infer.UNIT_ENTRIES == {infer.FUSED: "sac_unit_moments_many", infer.GENERAL_STEP: "sac_unit_moments_general_many"}
    assert _lib.SYMBOLS["sac_unit_moments"] == _lib.SYMBOLS["sac_unit_moments_general"]
    assert _lib.SYMBOLS["sac_unit_moments_many"] == _lib.SYMBOLS["sac_unit_moments_general_many"]
    assert driver.EvalOptions._field_defaults["unit_diagnostics"] is False
    assert driver.EvalOptions._field_defaults["unit_general"] == "host"
    assert driver.EVAL_BLOCKS[-1] == "units" and driver.EVAL_BLOCKS[:3] == ("q", "validation", "replay")


# ---- the driver: where the block stands, what the calls get ---------------------------------------------------------------------
UNIT_KEYS = [f"units/{t} {f}" for t in ("Policy", "QF1", "QF2") for f in infer.UNIT_FIGURES]


class UnitTrainer(epochs.FakeTrainer):
    def _units(self, obs, act):
        x = float(np.sum(obs, dtype=np.float64) + np.sum(act, dtype=np.float64)) + float(self.policy.flat()[0])
        rec = dict(count=float(len(obs)), sum=np.array([1.0, 0.0, abs(x)]), sumsq=np.array([2.0, 0.0, x * x]),
                   active=np.array([float(len(obs)), 0.0, 1.0]), max=np.array([1.0, 0.0, abs(x)]))
        return OrderedDict((n, [rec]) for n in driver.UNIT_NETS)

    def unit_moments(self, obs, act=None, nets=None, **kw):
        epochs.LOG.append(("unit_moments", self.seed, kw))
        assert tuple(nets) == ("policy", "qf1", "qf2")
        return self._units(obs, act)


def fake_unit_moments_many(trainers, obs, act, nets, **kw):
    epochs.LOG.append(("unit_moments_many", None, kw))
    assert all(tuple(n) == ("policy", "qf1", "qf2") for n in nets)
    return [t._units(o, a) for t, o, a in zip(trainers, obs, act)]


@pytest.fixture
def stand_ins(monkeypatch):
    for name, fake in dict(SACTrainer=UnitTrainer, EnvReplayBuffer=epochs.FakeBuffer, SACTrainerGroup=epochs.FakeGroup,
                           MixedSACTrainerGroup=epochs.FakeGroup, q_values_many=epochs.fake_q_values_many,
                           evaluate_many=epochs.fake_evaluate_many, evaluate_replay_many=epochs.fake_evaluate_replay_many,
                           unit_moments_many=fake_unit_moments_many, SyntheticEnv=epochs.LoggingEnv).items():
        assert hasattr(driver, name), name
        monkeypatch.setattr(driver, name, fake)
    del epochs.LOG[:], epochs.FakeTrainer.made[:]


def test_the_units_block_stands_behind_replay_and_in_front_of_time(stand_ins):
    off = epochs.solo(3, **epochs.ALL_ON)
    on = epochs.solo(3, unit_diagnostics=True, **epochs.ALL_ON)
    plain, only = epochs.solo(3), epochs.solo(3, unit_diagnostics=True)
    for with_units, without in ((on, off), (only, plain)):
        for row, ref in zip(with_units, without):
            keys = list(row)
            i = keys.index(UNIT_KEYS[0])
            assert keys[i:i + 12] == UNIT_KEYS and keys[i + 12] == "time/data storing (s)"
            assert keys[:i] + keys[i + 12:] == list(ref)
            assert all(k.startswith("time/") or epochs.same(row[k], ref[k]) for k in ref)
            assert row["units/Policy Dead Fraction"] == 1 / 3 and row["units/QF2 Dead Fraction"] == 1 / 3
            assert 1 / 3 < row["units/QF1 Active Fraction"] < 2 / 3 and row["units/QF1 Feature Norm"] > 0
    assert list(on[0])[list(on[0]).index(UNIT_KEYS[0]) - 1].startswith("replay/")
    assert not [k for k in plain[0] if k.startswith("units/")]


@pytest.mark.parametrize("entry", ["group", "sweep"])
@pytest.mark.parametrize("acting", ["host", "device"])
def test_group_rows_are_solo_rows_and_one_call_per_epoch(stand_ins, entry, acting):
    solo_rows = {s: epochs.solo(s, unit_diagnostics=True, q_diagnostics=True) for s in epochs.SEEDS}
    _, log = epochs.logged(epochs.solo, 3, unit_diagnostics=True, unit_general="device")
    assert [(n, kw) for n, _, kw in log if n.startswith("unit")] == [("unit_moments", dict(general="device"))] * epochs.EPOCHS
    _, log = epochs.logged(epochs.solo, 3, unit_diagnostics=True)
    assert [(n, kw) for n, _, kw in log if n.startswith("unit")] == [("unit_moments", {})] * epochs.EPOCHS     # (left out at the default)
    for kw, seen in ((dict(), {}), (dict(unit_general="device"), dict(general="device"))):
        rows, log = epochs.logged(getattr(epochs, entry), acting=acting, unit_diagnostics=True, q_diagnostics=True, **kw)
        assert [(n, k) for n, _, k in log if n.startswith("unit")] == [("unit_moments_many", seen)] * epochs.EPOCHS
        names = epochs.calls(log, by_seed=False)
        assert names.index("unit_moments_many") == names.index("q_values_many") + 1
        for s in epochs.SEEDS:
            epochs.assert_rows_equal(rows[s], solo_rows[s], (entry, acting, s))
            epochs.assert_times(rows[s], (entry, acting, s))
    with pytest.raises(RuntimeError, match="general"):
        getattr(epochs, entry)(unit_diagnostics=True, unit_general="gpu")
    # unit_general alone switches nothing on
    rows = getattr(epochs, entry)(unit_general="device")
    assert not [k for k in rows[epochs.SEEDS[0]][0] if k.startswith("units/")]


def test_train_script_passes_the_options_on():
    spec = importlib.util.spec_from_file_location("train_script_units", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    args = ap.parse_args([])
    assert args.unit_diagnostics is False and args.unit_general == "host"
    args = ap.parse_args(["--unit_diagnostics", "--unit_general", "device"])
    assert args.unit_diagnostics is True and args.unit_general == "device"
    with pytest.raises(SystemExit):
        ap.parse_args(["--unit_general", "gpu"])
    src = open(os.path.join(ROOT, "scripts", "train.py")).read()
    assert 'option_kw["unit_diagnostics"] = True' in src and 'option_kw["unit_general"] = args.unit_general' in src
