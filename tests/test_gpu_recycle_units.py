"""GPU: recycling hidden units on the device -- sac_recycle_units / sac_recycle_units_many (k_unit_recycle,
csrc/sac_recycle.h), SACTrainer.recycle_units / recycle_dormant, group.recycle_units_many and the drivers' recycle_period.

There is NO tolerance anywhere but in the one float64-referenced step: what _export_state() returns after a recycle is
compared as bytes with infer.recycle_reference of what it returned before -- every net, both moments, the scalars -- for
both step families and both algorithms; the fused kernels' transposed copy and pads are read back too; grouped == solo;
exactly dead units leave every inference entry bit for bit; the next steps of the recycled trainer are those of a twin that
got the reference's state from the host; refusals write nothing."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

from robosuite_benchmark_amd import _lib, driver, infer
from robosuite_benchmark_amd.group import ArchSACTrainerGroup, recycle_units_many
from tests.helpers import F64_ERRORS, filled_buffer, full_state, synth_transitions
from tests.test_gpu_optimizer_step import _batch
from tests.test_gpu_param_moments import B, build, variant
from tests.test_gpu_step_edges import PATHS
from tests.test_gpu_written_state import _buffer, _leg_c, _of_path, _set_env, _trainer
from tests.written_state import check_copies_and_pads

pytestmark = pytest.mark.gpu

# name -> (algorithm, policy hidden, Q hidden (None: the policy's), O, A, general step?)
SHAPES = {
    "fused 42-7 (256,256)": ("sac", (256, 256), None, 42, 7, False),
    "fused 17-5 (64,32)": ("sac", (64, 32), None, 17, 5, False),                         # units 0 and N - 1 next to the pads
    "fused 379-6 (256,256)": ("sac", (256, 256), None, 379, 6, False),                   # action columns at KP = 384
    "fused 46-16 (256,256)": ("sac", (256, 256), None, 46, 16, False),                   # A = 16: two head tiles
    "fused td3 (240,256)": ("td3", (240, 256), None, 42, 7, False),
    "general (512,512)": ("sac", (512, 512), None, 45, 7, True),
    "general (300,7,129)": ("sac", (300, 7, 129), None, 123, 7, True),
    "general (1,)": ("sac", (1,), None, 1, 1, True),
    "general (64,)x7": ("sac", (64,) * 7, None, 42, 7, True),
    "general (4096,)": ("sac", (4096,), None, 42, 7, True),
    "general policy deeper": ("sac", (96, 80, 72), (128, 112), 42, 7, True),
    "general td3 (300,200,100)": ("td3", (300, 200, 100), None, 17, 5, True),
}


def fresh(name, seed=5):
    algo, hp, hq, O, A, general = SHAPES[name]
    t = build(algo, hp, hq, O, A, seed)
    assert t.runs_general_step() == general, name
    return t


def steps(t, n, seed=50):
    o, a, r, d, no = synth_transitions(B, t.obs_dim, t.act_dim, seed=seed)
    for _ in range(n):
        t.train(dict(observations=o, actions=a, rewards=r, terminals=d, next_observations=no))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def same_state(got, want, where):
    assert list(got["params"]) == list(want["params"])
    for k in got["params"]:
        assert np.array_equal(bits(got["params"][k]), bits(want["params"][k])), (where, "params", k)
    for k in got["opt"]:
        for what, x, y in zip("mv", got["opt"][k], want["opt"][k]):
            assert np.array_equal(bits(x), bits(y)), (where, "adam " + what, k)
    assert np.array_equal(bits(np.asarray(got["scalars"], np.float64)), bits(np.asarray(want["scalars"], np.float64))), where


def unit_lists(t):
    """Per net the lists that hit the edges: 15/16/17 and 63/64/65, first and last unit, a whole layer behind a listed
    one (adjacent layers that cross), an empty layer -- nets given out of id order."""
    def edge(N):
        return sorted({u for u in (0, 15, 16, 17, 63, 64, 65, N - 1) if u < N})
    out = OrderedDict()
    for net in ("qf2", "policy", "qf1"):
        ws = t._hidden(net)
        if net == "policy":
            lists = [edge(N) for N in ws]
            lists[-1] = list(range(ws[-1]))                      # a whole layer; it crosses the layer in front of it
        elif net == "qf1":
            lists = [[] for _ in ws]
            lists[0] = sorted({0, ws[0] - 1})
        else:
            lists = [edge(N) for N in ws]
            if len(ws) > 1:
                lists[0] = []
        out[net] = lists
    return out


# ---- 1. the state is the reference of the state before ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_state_equals_the_reference(name):
    t = fresh(name)
    steps(t, 20)
    units = unit_lists(t)
    for opt, seed in ((False, 3), (True, 4)):
        before = t.state_dict()
        for net in ("policy", "qf1", "qf2"):                     # (behind 20 steps the moments are not zero)
            assert all(np.count_nonzero(x) > 0 for x in before["opt"][net]), (name, net)
        rows = infer.fresh_unit_rows(t, units, np.random.RandomState(seed))
        counts = t.recycle_units(units, fresh=rows, opt=opt)
        assert counts == OrderedDict((n, sum(len(u) for u in units[n])) for n in units) and counts["policy"] > 0
        after, want = t.state_dict(), infer.recycle_reference(before, t, units, rows, opt=opt)
        same_state(after, want, (name, opt))
        assert not np.array_equal(bits(after["params"]["qf2"]), bits(before["params"]["qf2"]))
        if not opt:                                              # the moment bytes are left
            for net in ("policy", "qf1", "qf2"):
                for x, y in zip(after["opt"][net], before["opt"][net]):
                    assert np.array_equal(bits(x), bits(y)), (name, net)
        else:
            assert not np.array_equal(bits(after["opt"]["policy"][1]), bits(before["opt"]["policy"][1]))
        if not t.runs_general_step():                            # "pt_<net>" against sac_get_params, "pad_nonzero" all 0
            check_copies_and_pads(t, f"{name}, behind recycle_units(opt={opt})")
    # the host route on a twin: the same bytes
    twin = fresh(name)
    steps(twin, 20)
    for opt, seed in ((False, 3), (True, 4)):
        twin.recycle_units(units, rng=np.random.RandomState(seed), opt=opt, route="host")
    same_state(twin.state_dict(), t.state_dict(), (name, "host route"))


# ---- 2. grouped == solo -----------------------------------------------------------------------------------------------------
def test_grouped_is_solo():
    names = (list(SHAPES) + list(SHAPES))[:16]
    ts = [fresh(n, seed=20 + i) for i, n in enumerate(names)]
    twins = [fresh(n, seed=20 + i) for i, n in enumerate(names)]
    assert {t.runs_general_step() for t in ts} == {True, False} and {"target_policy" in t.NETS for t in ts} == {True, False}
    for t in ts + twins:
        steps(t, 3, seed=60)
    units = [unit_lists(t) for t in ts]
    units[5] = None                                              # a member that sits out
    units[6] = OrderedDict(qf1=[[] for _ in ts[6]._hidden("qf1")])          # a member whose every list is empty
    rows = [None if u is None else infer.fresh_unit_rows(t, u, np.random.RandomState(70 + i))
            for i, (t, u) in enumerate(zip(ts, units))]
    got = recycle_units_many(ts, units, fresh_list=rows)
    for i, (t, twin) in enumerate(zip(ts, twins)):
        if units[i] is None:
            assert got[i] is None
        else:
            assert got[i] == twin.recycle_units(units[i], fresh=rows[i])
        same_state(t.state_dict(), twin.state_dict(), names[i])
    # a group's own method, rows drawn from the members' generators: the members' solo recycle_units with the same seeds
    sub = [i for i, t in enumerate(ts) if "target_policy" not in t.NETS and t.runs_general_step()][::-1]
    group = ArchSACTrainerGroup([ts[i] for i in sub])
    sel = [OrderedDict(policy=[[0]] + [[] for _ in ts[i]._hidden("policy")[1:]]) for i in sub]
    group.recycle_units_many(sel, rngs=[np.random.RandomState(90 + i) for i in sub], opt=False)
    for i, s in zip(sub, sel):
        twins[i].recycle_units(s, rng=np.random.RandomState(90 + i), opt=False)
        same_state(ts[i].state_dict(), twins[i].state_dict(), (names[i], "group method"))


# ---- 3. exactly dead units: every inference entry is left bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("name", ["fused 42-7 (256,256)", "fused 17-5 (64,32)", "fused td3 (240,256)", "general (300,7,129)"])
def test_dead_units_leave_the_function(name):
    t = fresh(name)
    steps(t, 4)
    td3, general = "target_policy" in t.NETS, t.runs_general_step()
    dead = OrderedDict((net, [sorted({0, N // 2, N - 1}) for N in t._hidden(net)]) for net in ("policy", "qf1", "qf2"))
    for net, lists in dead.items():                              # a zero row and a negative bias: dead on every input
        flat = t._get_params(net)
        hidden, _, _ = infer._recycle_layers(t, net)
        for us, (N, K, ow, ob) in zip(lists, hidden):
            for u in us:
                flat[ow + u * K:ow + (u + 1) * K] = 0.0
                flat[ob + u] = -1.0
        t._set_params(net, flat)
    n = 40
    o, a, r, d, no = synth_transitions(n, t.obs_dim, t.act_dim, seed=9)
    kw = dict(general="device") if general else {}
    moments = t.unit_moments(o, a, nets=tuple(dead), **kw)
    for net, lists in dead.items():
        for l, us in enumerate(lists):
            assert (moments[net][l]["active"][us] == 0).all(), (net, l)
    rs = np.random.RandomState(2)
    eps = rs.standard_normal((n, t.act_dim)).astype(np.float32)
    batch = dict(observations=o, actions=a, rewards=r, terminals=d.astype(np.float32), next_observations=no)

    def outputs():
        act = t.policy_act_general(o, True, None) if general else t.policy_act_device(o, True, None)
        out = [t.q_values(o, a, nets=("qf1", "qf2"), **kw), act]
        if td3:
            _, cols = t.evaluate_td3(batch, eps=eps, rows=True, **kw)
        else:
            _, cols = t.evaluate(batch, eps=(eps, eps[::-1].copy()), rows=True, **kw)
        return out + [np.asarray(cols[k]) for k in sorted(cols)]

    before, state = outputs(), t.state_dict()
    t.recycle_units(dead, rng=np.random.RandomState(6))
    assert not np.array_equal(bits(t.state_dict()["params"]["qf1"]), bits(state["params"]["qf1"]))
    for x, y in zip(before, outputs()):
        assert np.array_equal(bits(np.asarray(x, np.float32)), bits(np.asarray(y, np.float32))), name


# ---- 4. the next steps ---------------------------------------------------------------------------------------------------------
STEP_CASES = [_of_path(p) for p in PATHS if p[0] in ("sac kind 1", "sac kind 0", "sac kind 2", "sac kind 4", "sac kind 3 deep",
                                                     "td3 fused critic", "td3 general")]
assert len(STEP_CASES) == 7


@pytest.mark.parametrize("c", STEP_CASES, ids=[c["label"] for c in STEP_CASES])
def test_the_next_steps_are_the_twins(c, monkeypatch):
    label, (O, A, Bc), td3 = c["label"], c["shape"], c["algo"] == "td3"
    _set_env(c["env"], monkeypatch)
    hip, twin = _trainer(c), _trainer(c)
    assert hip.fused_mode() == c["kind"], (label, hip.fused_mode())
    buf, tbuf = _buffer(O, A, 70), _buffer(O, A, 70)
    hip.train_loop(buf, 4, batch_size=Bc)
    twin.train_loop(tbuf, 4, batch_size=Bc)                      # (the twin's buffer draws along)
    before, units = hip.state_dict(), unit_lists(hip)
    rows = infer.fresh_unit_rows(hip, units, np.random.RandomState(12))
    hip.recycle_units(units, fresh=rows)
    want = infer.recycle_reference(before, hip, units, rows)
    twin.load_state_dict(want)                                   # (the host uploads both copies and the moments)
    # one step against the float64 oracle rebuilt from the state the recycle left: a stale transposed copy fails here
    state = hip.state_dict()
    same_state(state, want, label)
    batch, eps = _batch(O, A, Bc, 7)
    eps = eps[0] if td3 else eps
    diag, diag_twin = hip.train(batch, eps=eps), twin.train(batch, eps=eps)
    assert np.array_equal(diag, diag_twin, equal_nan=True), label
    _leg_c(f"recycled {label}", hip, state, batch, eps, diag, td3, True)      # (step 4: a TD3 policy step)
    assert F64_ERRORS.get(f"written state recycled {label}") is not None
    first, last = hip.train_loop(buf, 6, batch_size=Bc)
    tfirst, tlast = twin.train_loop(tbuf, 6, batch_size=Bc)
    assert np.array_equal(first, tfirst, equal_nan=True) and np.array_equal(last, tlast, equal_nan=True), label
    for x, y in zip(full_state(hip, buf), full_state(twin, tbuf)):
        assert np.array_equal(x, y), label
    if c["kind"] != 3:
        check_copies_and_pads(hip, f"{label}, six steps behind a recycle")


# ---- 5. behind unsettled steps; the host acting mirror -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused 42-7 (256,256)", "fused td3 (240,256)"])
def test_behind_unsettled_device_batch_steps(name):
    a, b = fresh(name, seed=12), fresh(name, seed=12)
    ba, bb = filled_buffer(2000, a.obs_dim, a.act_dim, 8), filled_buffer(2000, a.obs_dim, a.act_dim, 8)
    units = unit_lists(a)
    rows = infer.fresh_unit_rows(a, units, np.random.RandomState(1))
    for _ in range(5):                                           # device batches, stepwise: nothing read, no sac_sync
        a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
    _lib.check(_lib.load().sac_sync(b._h), "sac_sync")
    a.recycle_units(units, fresh=rows)
    b.recycle_units(units, fresh=rows)
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y), name
    a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("name", ["fused 42-7 (256,256)", "general (300,7,129)", "fused td3 (240,256)"])
def test_host_acting_sees_the_recycled_policy(name):
    t, twin = fresh(name, seed=3), fresh(name, seed=3)
    steps(t, 2)
    obs = synth_transitions(6, t.obs_dim, t.act_dim, seed=4)[0]
    old = t.policy_act(obs, True, None)                          # (the mirror is valid now)
    before, units = t.state_dict(), unit_lists(t)
    rows = infer.fresh_unit_rows(t, units, np.random.RandomState(2))
    t.recycle_units(units, fresh=rows)
    twin.load_state_dict(infer.recycle_reference(before, t, units, rows))
    got, want = t.policy_act(obs, True, None), twin.policy_act(obs, True, None)
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(got), bits(old)), name
    holder = (t.policy.get_action(obs[0], deterministic=True) if "target_policy" not in t.NETS else t.policy.get_action(obs[0]))[0]
    assert np.array_equal(bits(np.asarray(holder, np.float32)), bits(want[0]))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def recycle_c(ts, ios):
    R = len(ts)
    return _lib.load().sac_recycle_units_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                              (_lib.SacRecycleIO * R)(*ios))


def test_refusals_write_nothing():
    lib = _lib.load()
    a, g, narrow = fresh("fused 42-7 (256,256)", seed=1), fresh("general (300,7,129)", seed=1), fresh("fused 17-5 (64,32)", seed=1)
    buf = filled_buffer(500, 42, 7, 2)
    a.train_loop(buf, 3, batch_size=B)
    steps(g, 2); steps(narrow, 2)
    states = [(t, t.state_dict()) for t in (a, g, narrow)]
    state_a = full_state(a, buf)
    counts = np.array([2, 1, 9, 9, 9, 9], np.int32)              # policy of (256, 256): two layers; 9: a sentinel behind them
    units = np.array([3, 200, 7, -5, -5, -5], np.int32)
    rows = np.full(4096, 7.0, np.float32)
    kept = [x.copy() for x in (counts, units, rows)]

    alive = []                                                   # (the arrays behind every io's pointers)

    def io(nets=1, flags=1, c=counts, u=units, f=rows):
        alive.extend((c, u, f))
        return _lib.SacRecycleIO(nets, flags, *[None if x is None else x.ctypes.data for x in (c, u, f)])

    def untouched(what):
        for x, y in zip((counts, units, rows), kept):
            assert np.array_equal(x, y), what
        for t, st in states:
            same_state(t.state_dict(), st, what)
        for x, y in zip(full_state(a, buf), state_a):
            assert np.array_equal(x, y), what

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        untouched(what)

    g_io = io(2, 1, np.array([1, 0, 0], np.int32), np.array([5], np.int32))
    refused(recycle_c([a, g], [io(0), g_io]), "selects no network")
    for bit in (3, 4, 5):
        refused(recycle_c([a, g], [io(1 | 1 << bit), g_io]), "target nets are not recycled")
    refused(recycle_c([g, a], [g_io, io(1 << 6)]), "unknown bit")
    refused(recycle_c([a, g], [io(flags=2), g_io]), "unknown flags")
    refused(recycle_c([a, g], [io(c=None), g_io]), "null counts")
    refused(recycle_c([a, g], [io(u=None), g_io]), "null units or fresh")
    refused(recycle_c([a, g], [io(f=None), g_io]), "null units or fresh")
    refused(recycle_c([a], [io(u=np.array([3, 256, 7], np.int32))]), "outside the layer's true width")
    refused(recycle_c([a], [io(u=np.array([-1, 5, 7], np.int32))]), "outside the layer's true width")
    refused(recycle_c([narrow], [io(c=np.array([1, 0], np.int32), u=np.array([64], np.int32))]), "pads are not units")
    refused(recycle_c([narrow], [io(c=np.array([0, 1], np.int32), u=np.array([32], np.int32))]), "pads are not units")
    refused(recycle_c([a], [io(u=np.array([200, 3, 7], np.int32))]), "not strictly ascending")
    refused(recycle_c([a], [io(u=np.array([3, 3, 7], np.int32))]), "not strictly ascending")
    refused(recycle_c([a], [io(c=np.array([257, 0], np.int32))]), "units listed")
    refused(recycle_c([a, a], [io(), io()]), "again")
    refused(recycle_c([a, None], [io(), io()]), "null")
    refused(lib.sac_recycle_units_many((C.c_void_p * 17)(*[a._h.value] * 17), 17, (_lib.SacRecycleIO * 17)(*[io()] * 17)), "1..16")
    _lib.check(lib.sac_trainer_set_xcd_mask(g._h, 0x0f), "sac_trainer_set_xcd_mask")
    refused(recycle_c([a, g], [io(), g_io]), "trainer 1 is confined by sac_trainer_set_xcd[_mask]")
    _lib.check(lib.sac_trainer_set_xcd_mask(g._h, 0xff), "sac_trainer_set_xcd_mask")
    states[1] = (g, g.state_dict())
    refused(lib.sac_recycle_units(None, C.byref(io())), "bad arguments")
    refused(lib.sac_recycle_units(a._h, None), "bad arguments")
    # every list empty: 0, nothing launched, nothing changed -- null units and fresh are fine then
    zeros = np.zeros(2, np.int32)
    assert recycle_c([a, g], [io(7, 1, np.zeros(6, np.int32), None, None), io(1, 0, np.zeros(3, np.int32), None, None)]) == 0
    assert lib.sac_recycle_units(a._h, C.byref(io(1, 1, zeros, None, None))) == 0
    untouched("every list empty")
    # a valid call with the same arrays: exactly the reference
    before = a.state_dict()
    assert recycle_c([a], [io()]) == 0
    K = [42, 256]
    fresh_rows = OrderedDict(policy=[rows[:2 * 43].reshape(2, 43), rows[2 * 43:2 * 43 + 257].reshape(1, 257)])
    want = infer.recycle_reference(before, a, OrderedDict(policy=[[3, 200], [7]]), fresh_rows)
    same_state(a.state_dict(), want, "a valid call")
    assert K == [r.shape[1] - 1 for r in fresh_rows["policy"]]


# ---- 7. the drivers ------------------------------------------------------------------------------------------------------------
KEYS = ["recycle/Policy Units", "recycle/QF1 Units", "recycle/QF2 Units"]


def final_states(monkeypatch, run):
    """run() with every trainer the driver builds kept: (its result, the trainers' final states in build order)."""
    made, build_run = [], driver._build_run

    def keeping(*a, **k):
        r = build_run(*a, **k)
        made.append(r["trainer"])
        return r

    monkeypatch.setattr(driver, "_build_run", keeping)
    out = run()
    monkeypatch.setattr(driver, "_build_run", build_run)
    return out, [t.state_dict() for t in made]


@pytest.mark.parametrize("algo,hidden", [("SAC", (256, 256)), ("TD3", (256, 256)), ("SAC", (64, 64, 64))])
def test_the_drivers_recycle(algo, hidden, monkeypatch, tmp_path):
    O, A, seeds = 11, 3, [3, 4]
    kw = dict(obs_dim=O, action_dim=A, quiet=True, num_epochs=3)
    on = dict(recycle_period=1, recycle_tau=1.0)
    calls, seen = dict(moments=0, recycle=0), []
    many, moments_many = driver.recycle_units_many, driver.unit_moments_many

    def recycling(trainers, units, **k):
        calls["recycle"] += 1
        got = many(trainers, units, **k)
        seen.append(got)
        return got

    def reducing(*a, **k):
        calls["moments"] += 1
        return moments_many(*a, **k)

    monkeypatch.setattr(driver, "recycle_units_many", recycling)
    monkeypatch.setattr(driver, "unit_moments_many", reducing)
    rows, states = final_states(monkeypatch, lambda: driver.experiment_group(variant(hidden, algo), seeds, **on, **kw))
    assert calls == dict(moments=2, recycle=2)                   # ONE call pair per recycle epoch (1 and 2) over all runs
    for i, s in enumerate(seeds):
        solo, solo_state = final_states(monkeypatch, lambda: driver.experiment(variant(hidden, algo), seed=s, **on, **kw))
        same_state(states[i], solo_state[0], (algo, hidden, s))
        for e, (row, want) in enumerate(zip(rows[s], solo)):
            cols = list(row)
            j = cols.index(KEYS[0])
            assert cols[j:j + 3] == KEYS and cols[j + 3] == "time/data storing (s)"          # the row's last block
            assert [row[k] for k in KEYS] == [want[k] for k in KEYS]                         # a solo twin's recycle_dormant
            if e == 0:
                assert [row[k] for k in KEYS] == [0, 0, 0]
            else:
                assert all(row[k] > 0 for k in KEYS), (s, e, [row[k] for k in KEYS])         # (tau = 1: the layer minimum)
                assert [row[k] for k in KEYS] == [seen[e - 1][i][n] for n in ("policy", "qf1", "qf2")]
            assert all(k.startswith("time/") or row[k] == want[k] or (row[k] != row[k] and want[k] != want[k]) for k in want)
    # the option off: header and rows of a run without the keyword
    monkeypatch.setattr(driver, "recycle_units_many", many)
    monkeypatch.setattr(driver, "unit_moments_many", moments_many)
    plain = driver.experiment_group(variant(hidden, algo), seeds, **kw)
    off = driver.experiment_group(variant(hidden, algo), seeds, recycle_period=0, recycle_tau=1.0, **kw)
    for s in seeds:
        assert [list(r) for r in off[s]] == [list(r) for r in plain[s]]
        assert all(k.startswith("time/") or a[k] == b[k] or (a[k] != a[k] and b[k] != b[k])
                   for a, b in zip(off[s], plain[s]) for k in a)
        assert any(a["trainer/QF1 Loss"] != b["trainer/QF1 Loss"] for a, b in zip(rows[s], plain[s]))   # (it does change the run)
    # a group checkpointed and resumed across a recycle epoch continues bit for bit
    if algo == "SAC" and hidden == (256, 256):
        ck = str(tmp_path / "ck")
        driver.experiment_group(variant(hidden, algo), seeds, checkpoint_dir=ck, **on, **dict(kw, num_epochs=1))
        resumed, rstates = final_states(monkeypatch, lambda: driver.experiment_group(
            variant(hidden, algo), seeds, checkpoint_dir=ck, resume=True, **on, **kw))
        for i, s in enumerate(seeds):
            same_state(rstates[i], states[i], ("resumed", s))
            assert [[r[k] for k in KEYS] for r in resumed[s]] == [[r[k] for k in KEYS] for r in rows[s][1:]]


def test_a_hidden_sweep_recycles(monkeypatch):
    kw = dict(quiet=True, num_epochs=2, recycle_period=1, recycle_tau=1.0)
    specs = [(variant((256, 256)), 3, 11, 3), (variant((64, 64, 64)), 4, 9, 2)]
    rows, states = final_states(monkeypatch, lambda: driver.experiment_sweep(specs, hidden_sweep=True, **kw))
    for i, (v, s, O, A) in enumerate(specs):
        solo, solo_state = final_states(monkeypatch, lambda: driver.experiment(v, seed=s, obs_dim=O, action_dim=A, **kw))
        same_state(states[i], solo_state[0], ("sweep", i))
        assert [[r[k] for k in KEYS] for r in rows[i]] == [[r[k] for k in KEYS] for r in solo]
        assert [rows[i][0][k] for k in KEYS] == [0, 0, 0] and all(rows[i][1][k] > 0 for k in KEYS)
