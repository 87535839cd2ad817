"""Recycling dormant units on the host: infer.dormant_units against unit_statistics, infer.recycle_reference (the NumPy
statement of sac_recycle_units) on small SAC and TD3 states, function preservation for exactly dead units,
fresh_unit_rows against a freshly built holder, and the argument refusals -- none of which needs a device."""
from collections import OrderedDict

import numpy as np
import pytest

from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy, TanhMlpPolicy, TD3Trainer, infer
from robosuite_benchmark_amd.group import recycle_units_many


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def sac_trainer(O=5, A=3, hp=(6, 4), hq=(5, 7, 3), seed=0):
    rs = np.random.RandomState(seed)
    pol = TanhGaussianPolicy(list(hp), O, A, rs=rs, noise=rs)
    qs = [FlattenMlp(list(hq), 1, O + A, rs=rs) for _ in range(4)]
    return SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3])


def td3_trainer(O=5, A=3, hp=(6, 4), hq=(5, 7, 3), seed=0):
    rs = np.random.RandomState(seed)
    pols = [TanhMlpPolicy(list(hp), A, O, rs=rs) for _ in range(2)]
    qs = [FlattenMlp(list(hq), 1, O + A, rs=rs) for _ in range(4)]
    return TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1])


def state_of(t, seed=1):
    """An _export_state() look-alike of a trainer without a handle: the holders' parameters, non-zero moments."""
    rs = np.random.RandomState(seed)
    params = {k: np.ascontiguousarray(getattr(t, k).flat(), np.float32) for k in t.NETS}
    opt = {k: (rs.standard_normal(params[k].size).astype(np.float32) + 3,
               rs.uniform(0.5, 1.5, params[k].size).astype(np.float32)) for k in ("policy", "qf1", "qf2")}
    return dict(params=params, opt=opt, scalars=rs.uniform(1, 2, 6))


def tensors_of(t, net, flat):
    out, off = OrderedDict(), 0
    for name, shape in t.param_tensors(net):
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].reshape(shape)
        off += n
    assert off == flat.size
    return out


# ---- dormant_units ----------------------------------------------------------------------------------------------------------
def record(sums):
    s = np.asarray(sums, np.float64)
    return dict(count=8.0, sum=s, sumsq=s * s, active=(s > 0) * 8.0, max=s)


def test_dormant_units_is_unit_statistics_predicate():
    tau = 0.25
    tie = record([1.0, 4.0, 7.0, 4.0])               # mean 4: tau * mean = 1.0 -- unit 0 sits exactly on it
    zero = record([0.0, 0.0, 0.0])                   # an all-zero layer: all listed
    nan = record([np.nan, 0.0, 5.0])                 # a NaN unit: it and its layer list nothing
    moments = OrderedDict(policy=[tie, zero], qf1=[nan, tie], qf2=[zero])
    got = infer.dormant_units(moments, tau)
    assert list(got) == ["policy", "qf1", "qf2"]
    assert [u.tolist() for u in got["policy"]] == [[0], [0, 1, 2]]
    assert [u.tolist() for u in got["qf1"]] == [[], [0]]
    assert [u.tolist() for u in got["qf2"]] == [[0, 1, 2]]
    assert all(u.dtype == np.int32 for us in got.values() for u in us)
    stats = infer.unit_statistics(moments, tau)
    for net, title in (("policy", "Policy"), ("qf1", "QF1"), ("qf2", "QF2")):
        units = sum(r["sum"].size for r in moments[net])
        assert sum(u.size for u in got[net]) / units == stats[title + " Dormant Fraction"]
    # just above the tie nothing of that layer is listed
    assert infer.dormant_units(OrderedDict(policy=[record([1.0000001, 4.0, 7.0, 4.0 - 1e-7])]), tau)["policy"][0].size == 0


# ---- recycle_reference ------------------------------------------------------------------------------------------------------
UNITS = OrderedDict(policy=[[0, 5], [1, 3]], qf1=[[4], [0, 1, 2, 3, 4, 5, 6], [2]], qf2=[[], [6], []])


@pytest.mark.parametrize("make", [sac_trainer, td3_trainer])
@pytest.mark.parametrize("opt", [True, False])
def test_recycle_reference(make, opt):
    t = make()
    st = state_of(t)
    fresh = infer.fresh_unit_rows(t, UNITS, np.random.RandomState(7))
    before = {k: v.copy() for k, v in st["params"].items()}
    new = infer.recycle_reference(st, t, UNITS, fresh, opt=opt)
    for k in st["params"]:                           # the given state is left alone
        assert np.array_equal(bits(st["params"][k]), bits(before[k]))
    for net, lists in UNITS.items():
        old, got = tensors_of(t, net, st["params"][net]), tensors_of(t, net, new["params"][net])
        written = {name: np.zeros(x.shape, bool) for name, x in old.items()}
        nh = len(lists)
        heads = [n for n in old if n.endswith(".weight") and not n.startswith("fc")]
        assert heads == (["last_fc.weight", "last_fc_log_std.weight"] if net == "policy" and make is sac_trainer
                         else ["last_fc.weight"])
        for l, us in enumerate(lists):
            readers = [f"fc{l + 1}.weight"] if l + 1 < nh else heads
            for j, u in enumerate(us):
                written[f"fc{l}.weight"][u, :] = True
                written[f"fc{l}.bias"][u] = True
                for r in readers:
                    written[r][:, u] = True
                    assert not bits(got[r][:, u]).any()                          # listed columns are +0.0, every head
                K = old[f"fc{l}.weight"].shape[1]
                crossed = np.zeros(K, bool)
                if l:
                    crossed[list(lists[l - 1])] = True                          # zero wins at a crossing
                assert np.array_equal(bits(got[f"fc{l}.weight"][u, ~crossed]), bits(fresh[net][l][j, :K][~crossed]))
                assert not bits(got[f"fc{l}.weight"][u, crossed]).any()
                assert bits(got[f"fc{l}.bias"][u]) == bits(fresh[net][l][j, K])
        m_old, v_old = (tensors_of(t, net, x) for x in st["opt"][net])
        m_new, v_new = (tensors_of(t, net, x) for x in new["opt"][net])
        for name in old:
            w = written[name]
            assert np.array_equal(bits(got[name][~w]), bits(old[name][~w]))      # every other byte is unchanged
            for a, b in ((m_old, m_new), (v_old, v_new)):
                assert np.array_equal(bits(b[name][~w]), bits(a[name][~w]))
                if opt:
                    assert not bits(b[name][w]).any()                            # exactly the written elements' moments
                else:
                    assert np.array_equal(bits(b[name][w]), bits(a[name][w]))
    assert written["fc1.weight"].any()
    for net in set(st["params"]) - set(UNITS):                                  # target nets included
        assert np.array_equal(bits(new["params"][net]), bits(st["params"][net]))
    assert np.array_equal(new["scalars"].view(np.uint64), np.asarray(st["scalars"]).view(np.uint64))


def test_recycling_exactly_dead_units_preserves_the_function():
    t = sac_trainer(hp=(8, 6), hq=(8, 6))
    dead = OrderedDict(policy=[[2, 7], [0]], qf1=[[1], [4, 5]])
    rs = np.random.RandomState(3)
    X = np.abs(rs.standard_normal((16, 5))).astype(np.float32)                  # non-negative rows
    act = np.abs(rs.standard_normal((16, 3))).astype(np.float32)
    for net, lists in dead.items():                                             # make the units exactly dead on X
        holder = getattr(t, net)
        for l, us in enumerate(lists):
            w, b = holder.layers[f"fc{l}"]
            w[us, :] = -np.abs(w[us, :])                                        # (post-ReLU inputs are non-negative too)
            b[us] = -1.0
    moments = t.unit_moments(X, act, nets=tuple(dead))
    for net, lists in dead.items():
        for l, us in enumerate(lists):
            assert (moments[net][l]["active"][us] == 0).all()

    def forward(params, net):
        h = X if net == "policy" else np.concatenate([X, act], axis=1)
        ten = tensors_of(t, net, params[net])
        for l in range(2):
            h = h @ ten[f"fc{l}.weight"].T + ten[f"fc{l}.bias"]
            h = np.where(h < 0, np.float32(0), h).astype(np.float32)
        return [h @ ten[n].T + ten[n[:-6] + "bias"] for n in ten if n.endswith(".weight") and not n.startswith("fc")]

    st = state_of(t)
    new = infer.recycle_reference(st, t, dead, infer.fresh_unit_rows(t, dead, np.random.RandomState(5)))
    for net in dead:
        assert not np.array_equal(bits(new["params"][net]), bits(st["params"][net]))
        for a, b in zip(forward(st["params"], net), forward(new["params"], net)):
            assert np.array_equal(bits(a), bits(b))


# ---- fresh_unit_rows ---------------------------------------------------------------------------------------------------------
def test_fresh_unit_rows_are_reproducible_and_drawn_like_a_fresh_holder():
    t = sac_trainer()
    a = infer.fresh_unit_rows(t, UNITS, np.random.RandomState(11))
    b = infer.fresh_unit_rows(t, UNITS, np.random.RandomState(11))
    for net in UNITS:
        assert [x.shape for x in a[net]] == [(len(us), w.shape[1] + 1) for us, (w, _) in
                                             zip(UNITS[net], getattr(t, net).as_layer_list())]
        for x, y in zip(a[net], b[net]):
            assert x.dtype == np.float32 and np.array_equal(bits(x), bits(y))
    # the draws, in order: one uniform per (net, layer) with units -- qf2's empty layers draw nothing
    rs = np.random.RandomState(11)
    for net in UNITS:
        for l, us in enumerate(UNITS[net]):
            w, _ = getattr(t, net).layers[f"fc{l}"]
            if us:
                bound = 1.0 / np.sqrt(w.shape[0])
                want = rs.uniform(-bound, bound, (len(us), w.shape[1])).astype(np.float32)
                assert np.array_equal(bits(a[net][l][:, :-1]), bits(want))
    # bound and bias of a freshly built holder's layer: a whole layer listed with the holder's own generator is that layer
    holder = FlattenMlp([7], 1, 4, rs=np.random.RandomState(2))
    tr = sac_trainer(O=3, A=1, hp=(7,), hq=(7,))
    rows = infer.fresh_unit_rows(tr, dict(qf1=[list(range(7))]), np.random.RandomState(2))["qf1"][0]
    assert np.array_equal(bits(rows[:, :-1]), bits(holder.layers["fc0"][0]))
    assert np.array_equal(bits(rows[:, -1]), bits(holder.layers["fc0"][1]))
    assert (np.abs(rows[:, :-1]) <= 1.0 / np.sqrt(7)).all()


# ---- refusals, before any library call -----------------------------------------------------------------------------------------
class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.mark.parametrize("units, match", [
    (dict(target_qf1=[[0], [0], [0]]), "not recycled"),
    (dict(target_policy=[[0], [0]]), "not recycled"),
    (dict(critic=[[0]]), "not recycled"),
    (dict(), "at least one network"),
    ([[0], [1]], "mapping"),
    (dict(policy=[[0]]), "2 hidden layers"),
    (dict(policy=[[0], [4]]), "outside"),
    (dict(policy=[[-1], []]), "outside"),
    (dict(policy=[[6], []]), "outside"),
    (dict(policy=[[1, 1], []]), "strictly ascending"),
    (dict(policy=[[2, 1], []]), "strictly ascending"),
    (dict(policy=[[0.5], []]), "integers"),
])
def test_argument_refusals(units, match):
    for t in (sac_trainer(), td3_trainer()):
        t._lib = NoLibrary()
        rng = np.random.RandomState(0)
        with pytest.raises(ValueError, match=match):
            t.recycle_units(units, rng=rng)
        with pytest.raises(ValueError, match=match):
            recycle_units_many([t], [units], rngs=[rng])
        with pytest.raises(ValueError, match=match):
            infer.fresh_unit_rows(t, units, rng)
        assert rng.get_state()[2] == 624 and np.array_equal(rng.get_state()[1], np.random.RandomState(0).get_state()[1])


def test_more_refusals():
    t = sac_trainer()
    t._lib = NoLibrary()
    ok = dict(policy=[[0], [1]])
    with pytest.raises(ValueError, match="fresh rows or a generator"):
        t.recycle_units(ok)
    with pytest.raises(ValueError, match="fresh rows must be"):
        t.recycle_units(ok, fresh=dict(policy=[np.zeros((1, 5)), np.zeros((1, 7))]))
    with pytest.raises(RuntimeError, match="route"):
        t.recycle_units(ok, rng=np.random.RandomState(0), route="gpu")
    with pytest.raises(RuntimeError, match="twice"):
        recycle_units_many([t, t], [ok, ok], rngs=[np.random.RandomState(0)] * 2)
    with pytest.raises(RuntimeError, match="one unit selection"):
        recycle_units_many([t], [ok, ok])
    with pytest.raises(ValueError, match="generator"):
        t.recycle_dormant(np.zeros((2, 5), np.float32), np.zeros((2, 3), np.float32))


def test_a_trainer_without_a_handle_takes_the_host_route():
    t, twin = sac_trainer(), sac_trainer()
    fresh = infer.fresh_unit_rows(t, UNITS, np.random.RandomState(7))
    counts = t.recycle_units(UNITS, fresh=fresh)             # route="device" asked, no handle: the host
    assert counts == OrderedDict(policy=4, qf1=9, qf2=1)
    st = dict(params={k: np.ascontiguousarray(getattr(twin, k).flat(), np.float32) for k in twin.NETS},
              opt={k: (np.zeros(getattr(twin, k).flat().size, np.float32),) * 2 for k in ("policy", "qf1", "qf2")},
              scalars=np.zeros(6))
    want = infer.recycle_reference(st, twin, UNITS, fresh)
    for k in t.NETS:
        assert np.array_equal(bits(getattr(t, k).flat()), bits(want["params"][k]))
    assert recycle_units_many([t, twin], [None, dict(qf2=[[], [], []])], rngs=[None, np.random.RandomState(0)]) == \
        [None, OrderedDict(qf2=0)]
