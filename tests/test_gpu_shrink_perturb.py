"""GPU: whole-network reset and shrink-and-perturb on the device -- sac_shrink_perturb / sac_shrink_perturb_many
(k_param_perturb, csrc/sac_perturb.h), SACTrainer.shrink_perturb / reset_networks, group.shrink_perturb_many and the
drivers' reset_period.

There is NO tolerance anywhere but in the one float64-referenced step: what state_dict() returns after a call is compared
as bytes with infer.shrink_perturb_reference of what it returned before -- every net, both moments, the scalars -- for both
step families and both algorithms; the fused kernels' transposed copy and pads are read back too; a reset clears planted
NaN and Inf; grouped == solo; the same (seed, draw) gives the same bytes; the next steps are those of a twin that got the
reference's state from the host; every reader sees the new weights; refusals write nothing."""
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import _lib, driver, infer
from robosuite_benchmark_amd.group import ArchSACTrainerGroup, GroupActor, shrink_perturb_many
from tests.helpers import F64_ERRORS, filled_buffer, full_state, synth_transitions
from tests.test_gpu_optimizer_step import _batch
from tests.test_gpu_param_moments import B, build, variant
from tests.test_gpu_recycle_units import SHAPES as RECYCLE_SHAPES
from tests.test_gpu_recycle_units import STEP_CASES, bits, final_states, same_state, steps
from tests.test_gpu_written_state import _buffer, _leg_c, _set_env, _trainer
from tests.written_state import check_copies_and_pads

pytestmark = pytest.mark.gpu

# recycle's twelve, and two general shapes whose fc1.weight is one chunk exactly (16384) and one element short of it
SHAPES = dict(RECYCLE_SHAPES)
SHAPES["general (128,128)"] = ("sac", (128, 128), None, 42, 7, True)
SHAPES["general (127,129)"] = ("sac", (127, 129), None, 42, 7, True)
FORCED = ("general (128,128)", "general (127,129)")              # two layers of at most 256 units: the fused kernels' otherwise
assert len(SHAPES) == 14 and 128 * 128 == infer.PARAM_CH and 129 * 127 == infer.PARAM_CH - 1
TRAINED = ("policy", "qf1", "qf2")
SEED, DRAW = 0xF1E2D3C4B5A69788, 0x0123456789ABCDEF


def fresh(name, monkeypatch, seed=5):
    algo, hp, hq, O, A, general = SHAPES[name]
    if name in FORCED:
        monkeypatch.setenv("SAC_GENERAL", "1")
    t = build(algo, hp, hq, O, A, seed)
    if name in FORCED:
        monkeypatch.delenv("SAC_GENERAL")
    assert t.runs_general_step() == general, name
    return t


def differs(a, b, net):
    return not np.array_equal(bits(a["params"][net]), bits(b["params"][net]))


# the calls of test 1, in an order that keeps the moments non-zero in front of every opt=False call
CALLS = [
    dict(nets=None, shrink=0.8, perturb=0.2, seed=SEED, draw=DRAW, opt=False, targets=False),
    dict(nets=("qf2", "policy"), shrink=0.5, perturb=0.0, seed=SEED, draw=1, opt=False, targets=True),
    dict(nets=("qf1",), shrink=0.8, perturb=0.2, seed=None, draw=2, opt=True, targets=False, init_w=dict(qf1=0.05), b_init=-0.25),
    dict(nets=None, shrink=0.8, perturb=0.2, seed=3, draw=DRAW, opt=True, targets=True),
]


# ---- 1. the state is the reference of the state before ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_state_equals_the_reference(name, monkeypatch):
    t, twin = fresh(name, monkeypatch), fresh(name, monkeypatch)
    td3 = "target_policy" in t.NETS
    steps(t, 20)
    steps(twin, 20)
    for kw in CALLS:
        before = t.state_dict()
        if not kw["opt"]:                                        # (behind 20 steps the moments are not zero)
            assert all(np.count_nonzero(x) > 0 for net in TRAINED for x in before["opt"][net]), name
        nets = TRAINED if kw["nets"] is None else tuple(n for n in TRAINED if n in kw["nets"])
        assert t.shrink_perturb(**kw) == nets
        after, want = t.state_dict(), infer.shrink_perturb_reference(before, t, **kw)
        same_state(after, want, (name, kw))
        for net in TRAINED:
            assert differs(after, before, net) == (net in nets), (name, net)
            for x, y in zip(after["opt"][net], before["opt"][net]):
                if kw["opt"] and net in nets:
                    assert not x.any()
                else:
                    assert np.array_equal(bits(x), bits(y)), (name, net)
            tg = infer.param_target(t, net)
            if tg is not None:
                assert differs(after, before, tg) == (kw["targets"] and net in nets), (name, tg)
        if not t.runs_general_step():                            # "pt_<net>" against sac_get_params, "pad_nonzero" all 0
            check_copies_and_pads(t, f"{name}, behind shrink_perturb({kw})")
        twin.shrink_perturb(route="host", **kw)
    # a reset, behind two more steps (non-zero moments again): the fresh values themselves, targets alike
    steps(t, 2)
    steps(twin, 2)
    before = t.state_dict()
    assert all(np.count_nonzero(x) > 0 for net in TRAINED for x in before["opt"][net]), name
    assert t.reset_networks(seed=SEED, draw=7) == TRAINED
    after = t.state_dict()
    same_state(after, infer.shrink_perturb_reference(before, t, None, 0.0, 1.0, SEED, 7, opt=True, targets=True), (name, "reset"))
    for net in TRAINED:
        f = infer.fresh_params(t, net, SEED, 7)
        assert np.array_equal(bits(after["params"][net]), bits(f)) and not any(x.any() for x in after["opt"][net])
        tg = infer.param_target(t, net)
        assert (tg is None) == (net == "policy" and not td3)
        if tg is not None:
            assert np.array_equal(bits(after["params"][tg]), bits(f))
    assert np.array_equal(after["scalars"], before["scalars"])
    if not t.runs_general_step():
        check_copies_and_pads(t, f"{name}, behind reset_networks")
    # the host route on the twin: the same bytes
    twin.reset_networks(seed=SEED, draw=7, route="host")
    same_state(twin.state_dict(), after, (name, "host route"))


def test_reset_networks_alpha():
    t = build("sac", (256, 256), None, 42, 7, 5)
    steps(t, 6)
    before = t.state_dict()
    assert before["scalars"][0] != 0.0 and before["scalars"][1] != 0.0 and before["scalars"][2] != 0.0
    t.reset_networks(nets=("qf1",), alpha=True)
    sc = t.state_dict()["scalars"]
    assert list(sc[:3]) == [0.0, 0.0, 0.0] and sc[5] == 1.0 and list(sc[3:5]) == list(before["scalars"][3:5])
    td3 = build("td3", (240, 256), None, 42, 7, 5)
    steps(td3, 6)
    before = td3.state_dict()
    td3.reset_networks(alpha=True)                               # (a TD3 trainer has no entropy coefficient: counters stay)
    assert np.array_equal(td3.state_dict()["scalars"], before["scalars"])


# ---- 2. a reset clears planted NaN and Inf -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused 42-7 (256,256)", "fused td3 (240,256)", "general (300,7,129)"])
def test_a_reset_clears_nan_and_inf(name, monkeypatch):
    t = fresh(name, monkeypatch)
    steps(t, 2)

    def plant():
        for net, at, v in (("qf1", 0, np.nan), ("qf1", -1, np.inf), ("policy", 5, -np.inf), ("target_qf2", 7, np.nan)):
            flat = t._get_params(net)                            # a weight, a bias (the head's), a weight, a target
            flat[at] = v
            t._set_params(net, flat)

    def non_finite():
        return sum(float(m[:, _lib.PARAM_FIELDS.index("nonfinite")].sum()) for m in t.param_moments().values())

    plant()
    assert non_finite() == 4
    before = t.state_dict()
    t.shrink_perturb(shrink=0.8, perturb=0.2, seed=1, draw=2, targets=False)       # they stay
    assert non_finite() == 4
    same_state(t.state_dict(), infer.shrink_perturb_reference(before, t, None, 0.8, 0.2, 1, 2), (name, "0.8 / 0.2"))
    before = t.state_dict()
    t.shrink_perturb(shrink=0.8, perturb=0.2, seed=1, draw=3, targets=True)        # ... and reach the targets
    assert non_finite() == 3 + 2 + (1 if "target_policy" in t.NETS else 0)
    same_state(t.state_dict(), infer.shrink_perturb_reference(before, t, None, 0.8, 0.2, 1, 3, targets=True), (name, "targets"))
    before = t.state_dict()
    t.reset_networks(seed=1, draw=4)
    assert non_finite() == 0
    same_state(t.state_dict(), infer.shrink_perturb_reference(before, t, None, 0.0, 1.0, 1, 4, targets=True), (name, "reset"))
    assert all(np.isfinite(v).all() for v in t.state_dict()["params"].values())


# ---- 3. grouped == solo; 4. (seed, draw) ------------------------------------------------------------------------------------------
def test_grouped_is_solo(monkeypatch):
    names = (list(RECYCLE_SHAPES) + list(SHAPES))[:16]
    ts = [fresh(n, monkeypatch, seed=20 + i) for i, n in enumerate(names)]
    twins = [fresh(n, monkeypatch, seed=20 + i) for i, n in enumerate(names)]
    assert {t.runs_general_step() for t in ts} == {True, False} and {"target_policy" in t.NETS for t in ts} == {True, False}
    for t in ts + twins:
        steps(t, 3, seed=60)
    nets = [TRAINED, ("qf1",), ("policy", "qf2"), None] * 4
    nets[5] = None                                               # (members 3, 5, 7, 11, 15 sit out)
    shrink = [(0.0, 0.8, 0.5, 1.0)[i % 4] for i in range(16)]
    perturb = [(1.0, 0.2, 0.0, 0.25)[i % 4] for i in range(16)]
    seeds = [None if i % 3 == 0 else 100 + i for i in range(16)]
    opt, targets = [i % 2 == 0 for i in range(16)], [i % 5 != 0 for i in range(16)]
    got = shrink_perturb_many(ts, nets, shrink, perturb, seeds, 9, opt, targets)
    for i, (t, twin) in enumerate(zip(ts, twins)):
        if nets[i] is None:
            assert got[i] is None
        else:
            assert got[i] == twin.shrink_perturb(nets[i], shrink[i], perturb[i], seeds[i], 9, opt[i], targets[i])
        same_state(t.state_dict(), twin.state_dict(), names[i])
    # a group's own method
    sub = [i for i, t in enumerate(ts) if "target_policy" not in t.NETS and t.runs_general_step()][::-1]
    group = ArchSACTrainerGroup([ts[i] for i in sub])
    group.shrink_perturb_many(shrink=0.0, perturb=1.0, seeds=[50 + i for i in sub], draws=3, targets=True)
    for i in sub:
        twins[i].reset_networks(seed=50 + i, draw=3)
        same_state(ts[i].state_dict(), twins[i].state_dict(), (names[i], "group method"))


@pytest.mark.parametrize("name", ["fused 379-6 (256,256)", "general (300,7,129)"])
def test_the_same_seed_and_draw_give_the_same_bytes(name, monkeypatch):
    a, b = fresh(name, monkeypatch, seed=1), fresh(name, monkeypatch, seed=2)      # different weights and noise seeds
    steps(a, 1)
    a.reset_networks(seed=77, draw=5)
    b.reset_networks(seed=77, draw=5)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa["params"]:
        assert np.array_equal(bits(sa["params"][k]), bits(sb["params"][k])), k
    a.reset_networks(seed=77, draw=5)
    same_state(a.state_dict(), sa, name)
    a.reset_networks(seed=77, draw=6)
    assert all(differs(a.state_dict(), sa, k) for k in sa["params"])
    b.reset_networks(draw=5)                                     # (seed None: the trainer's noise seed, not 77)
    assert all(differs(b.state_dict(), sb, k) for k in sb["params"])


# ---- 5. the next steps ---------------------------------------------------------------------------------------------------------
MODES = {"reset": dict(shrink=0.0, perturb=1.0, opt=True, targets=True), "0.8-0.2": dict(shrink=0.8, perturb=0.2, opt=True, targets=False)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("c", STEP_CASES, ids=[c["label"] for c in STEP_CASES])
def test_the_next_steps_are_the_twins(c, mode, monkeypatch):
    label, (O, A, Bc), td3 = f"{c['label']} {mode}", c["shape"], c["algo"] == "td3"
    _set_env(c["env"], monkeypatch)
    hip, twin = _trainer(c), _trainer(c)
    assert hip.fused_mode() == c["kind"], (label, hip.fused_mode())
    buf, tbuf = _buffer(O, A, 70), _buffer(O, A, 70)
    hip.train_loop(buf, 4, batch_size=Bc)
    twin.train_loop(tbuf, 4, batch_size=Bc)                      # (the twin's buffer draws along)
    before = hip.state_dict()
    hip.shrink_perturb(seed=SEED, draw=DRAW, **MODES[mode])
    want = infer.shrink_perturb_reference(before, hip, seed=SEED, draw=DRAW, **MODES[mode])
    twin.load_state_dict(want)                                   # (the host uploads both copies and the moments)
    state = hip.state_dict()
    same_state(state, want, label)
    # one step against the float64 oracle rebuilt from the state the call left: a stale transposed copy fails here
    batch, eps = _batch(O, A, Bc, 7)
    eps = eps[0] if td3 else eps
    diag, diag_twin = hip.train(batch, eps=eps), twin.train(batch, eps=eps)
    assert np.array_equal(diag, diag_twin, equal_nan=True), label
    _leg_c(f"perturbed {label}", hip, state, batch, eps, diag, td3, True)      # (step 4: a TD3 policy step)
    assert F64_ERRORS.get(f"written state perturbed {label}") is not None
    first, last = hip.train_loop(buf, 10, batch_size=Bc)
    tfirst, tlast = twin.train_loop(tbuf, 10, batch_size=Bc)
    assert np.array_equal(first, tfirst, equal_nan=True) and np.array_equal(last, tlast, equal_nan=True), label
    for x, y in zip(full_state(hip, buf), full_state(twin, tbuf)):
        assert np.array_equal(x, y), label
    if c["kind"] != 3:
        check_copies_and_pads(hip, f"{label}, eleven steps behind the call")


# ---- 6. the readers of the new state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fused 42-7 (256,256)", "fused td3 (240,256)", "general (300,7,129)", "general td3 (300,200,100)"])
def test_readers_see_the_new_weights(name, monkeypatch):
    t, twin = fresh(name, monkeypatch, seed=3), fresh(name, monkeypatch, seed=3)
    td3, general = "target_policy" in t.NETS, t.runs_general_step()
    steps(t, 2)
    n = 40
    o, a, r, d, no = synth_transitions(n, t.obs_dim, t.act_dim, seed=9)
    eps = np.random.RandomState(2).standard_normal((n, t.act_dim)).astype(np.float32)
    batch = dict(observations=o, actions=a, rewards=r, terminals=d.astype(np.float32), next_observations=no)
    kw = dict(general="device") if general else {}
    session, tsession = (GroupActor([x], max_rows=8, **kw) for x in (t, twin))

    def outputs(x, s):
        act = x.policy_act_general(o, True, None) if general else x.policy_act_device(o, True, None)
        out = [x.q_values(o, a, nets=("qf1", "qf2"), **kw), act, x.policy_act(o[:6], True, None)]
        if td3:
            _, cols = x.evaluate_td3(batch, eps=eps, rows=True, **kw)
        else:
            _, cols = x.evaluate(batch, eps=(eps, eps[::-1].copy()), rows=True, **kw)
        s.obs[0][:8] = o[:8]
        s.act([8], True)
        out.append(np.array(s.act[0][:8]))
        return out + [np.asarray(cols[k]) for k in sorted(cols)]

    old = outputs(t, session)                                    # (the mirror and the session are live now)
    for mode in MODES.values():
        before = t.state_dict()
        t.shrink_perturb(seed=SEED, draw=DRAW, **mode)
        twin.load_state_dict(infer.shrink_perturb_reference(before, t, seed=SEED, draw=DRAW, **mode))
        got, want = outputs(t, session), outputs(twin, tsession)
        for x, y in zip(got, want):
            assert np.array_equal(bits(np.asarray(x, np.float32)), bits(np.asarray(y, np.float32))), (name, mode)
        assert all(not np.array_equal(bits(np.asarray(x, np.float32)), bits(np.asarray(y, np.float32))) for x, y in zip(got[:4], old))
        old = got
    session.close()
    tsession.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def perturb_c(ts, ios):
    R = len(ts)
    return _lib.load().sac_shrink_perturb_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                               (_lib.SacPerturbIO * R)(*ios))


def io(nets=7, flags=3, shrink=0.8, perturb=0.2, seed=1, draw=2, init_w=(1e-3, 3e-3, 3e-3), b_init=(0.1, 0.1, 0.1)):
    return _lib.SacPerturbIO(nets, flags, shrink, perturb, seed, draw, (C.c_float * 3)(*init_w), (C.c_float * 3)(*b_init))


def test_refusals_write_nothing(monkeypatch):
    lib = _lib.load()
    a, g = fresh("fused 42-7 (256,256)", monkeypatch, seed=1), fresh("general (300,7,129)", monkeypatch, seed=1)
    buf = filled_buffer(500, 42, 7, 2)
    a.train_loop(buf, 3, batch_size=B)
    steps(g, 2)
    states = [(t, t.state_dict()) for t in (a, g)]
    state_a = full_state(a, buf)
    nan, inf = float("nan"), float("inf")

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        for t, st in states:
            same_state(t.state_dict(), st, what)
        for x, y in zip(full_state(a, buf), state_a):
            assert np.array_equal(x, y), what

    refused(perturb_c([a, g], [io(0), io()]), "selects no network")
    for bit in (3, 4, 5):
        refused(perturb_c([a, g], [io(), io(1 | 1 << bit)]), "selects a target net")
    refused(perturb_c([g, a], [io(), io(1 << 6)]), "unknown bit")
    refused(perturb_c([a, g], [io(flags=4), io()]), "unknown flags")
    refused(perturb_c([a, g], [io(flags=8 | 1), io()]), "unknown flags")
    for kw in (dict(shrink=nan), dict(perturb=nan), dict(shrink=inf), dict(perturb=-inf), dict(shrink=-0.5), dict(perturb=-1e-9)):
        refused(perturb_c([g, a], [io(), io(**kw)]), "must be finite and not negative")
    refused(perturb_c([a, g], [io(), io(shrink=0.0, perturb=0.0)]), "both zero")
    refused(perturb_c([a], [io(init_w=(nan, 3e-3, 3e-3))]), "init_w")
    refused(perturb_c([a], [io(init_w=(1e-3, -1.0, 3e-3))]), "init_w")
    refused(perturb_c([a], [io(init_w=(1e-3, 3e-3, inf))]), "init_w")
    refused(perturb_c([a], [io(b_init=(0.1, nan, 0.1))]), "b_init")
    refused(perturb_c([a], [io(b_init=(-inf, 0.1, 0.1))]), "b_init")
    refused(perturb_c([a, a], [io(), io()]), "again")
    refused(perturb_c([a, None], [io(), io()]), "null")
    refused(lib.sac_shrink_perturb_many((C.c_void_p * 17)(*[a._h.value] * 17), 17, (_lib.SacPerturbIO * 17)(*[io()] * 17)), "1..16")
    _lib.check(lib.sac_trainer_set_xcd_mask(g._h, 0x0f), "sac_trainer_set_xcd_mask")
    refused(perturb_c([a, g], [io(), io()]), "trainer 1 is confined by sac_trainer_set_xcd[_mask]")
    _lib.check(lib.sac_trainer_set_xcd_mask(g._h, 0xff), "sac_trainer_set_xcd_mask")
    states[1] = (g, g.state_dict())
    refused(lib.sac_shrink_perturb(None, C.byref(io())), "bad arguments")
    refused(lib.sac_shrink_perturb(a._h, None), "bad arguments")
    # the values of nets that are NOT selected are not read; a valid call: exactly the reference
    before = a.state_dict()
    assert perturb_c([a], [io(nets=2, init_w=(nan, 0.5, -1.0), b_init=(inf, 0.25, nan))]) == 0
    want = infer.shrink_perturb_reference(before, a, ("qf1",), 0.8, 0.2, 1, 2, opt=True, targets=True, init_w=0.5, b_init=0.25)
    same_state(a.state_dict(), want, "a valid call")


# ---- 8. the drivers ------------------------------------------------------------------------------------------------------------
KEY = "reset/Networks"


@pytest.mark.parametrize("algo,hidden", [("SAC", (256, 256)), ("TD3", (256, 256)), ("SAC", (64, 64, 64))])
def test_the_drivers_reset(algo, hidden, monkeypatch, tmp_path):
    O, A, seeds = 11, 3, [3, 4]
    kw = dict(obs_dim=O, action_dim=A, quiet=True, num_epochs=3)
    on = dict(reset_period=2) if algo == "TD3" else dict(reset_period=1, reset_shrink=0.8, reset_perturb=0.2)
    due = [e for e in range(3) if e > 0 and e % on["reset_period"] == 0]
    calls, many = [], driver.shrink_perturb_many

    def counting(trainers, *a, **k):
        calls.append(len(trainers))
        return many(trainers, *a, **k)

    monkeypatch.setattr(driver, "shrink_perturb_many", counting)
    rows, states = final_states(monkeypatch, lambda: driver.experiment_group(variant(hidden, algo), seeds, **on, **kw))
    assert calls == [len(seeds)] * len(due)                      # ONE call per reset epoch over all runs
    for i, s in enumerate(seeds):
        solo, solo_state = final_states(monkeypatch, lambda: driver.experiment(variant(hidden, algo), seed=s, **on, **kw))
        same_state(states[i], solo_state[0], (algo, hidden, s))
        for e, (row, want) in enumerate(zip(rows[s], solo)):
            cols = list(row)
            assert cols[cols.index(KEY) + 1] == "time/data storing (s)"                      # the row's last block
            assert row[KEY] == want[KEY] == (3 if e in due else 0)
            assert all(k.startswith("time/") or row[k] == want[k] or (row[k] != row[k] and want[k] != want[k]) for k in want)
    assert len(calls) == len(due)                                # (the solo runs call the trainer's own method)
    # the option off: header and rows of a run without the keyword
    plain = driver.experiment_group(variant(hidden, algo), seeds, **kw)
    off = driver.experiment_group(variant(hidden, algo), seeds, reset_period=0, reset_shrink=0.8, reset_perturb=0.2, **kw)
    for s in seeds:
        assert [list(r) for r in off[s]] == [list(r) for r in plain[s]]
        assert all(k.startswith("time/") or a[k] == b[k] or (a[k] != a[k] and b[k] != b[k])
                   for a, b in zip(off[s], plain[s]) for k in a)
        assert any(a["trainer/QF1 Loss"] != b["trainer/QF1 Loss"] for a, b in zip(rows[s], plain[s]))   # (it does change the run)
    # a group checkpointed and resumed across a reset epoch continues bit for bit
    if algo == "SAC" and hidden == (256, 256):
        ck = str(tmp_path / "ck")
        driver.experiment_group(variant(hidden, algo), seeds, checkpoint_dir=ck, **on, **dict(kw, num_epochs=1))
        resumed, rstates = final_states(monkeypatch, lambda: driver.experiment_group(
            variant(hidden, algo), seeds, checkpoint_dir=ck, resume=True, **on, **kw))
        for i, s in enumerate(seeds):
            same_state(rstates[i], states[i], ("resumed", s))
            assert [r[KEY] for r in resumed[s]] == [r[KEY] for r in rows[s][1:]]


def test_a_hidden_sweep_resets(monkeypatch):
    kw = dict(quiet=True, num_epochs=2, reset_period=1)
    specs = [(variant((256, 256)), 3, 11, 3), (variant((64, 64, 64)), 4, 9, 2),
             (variant((256, 256), "TD3"), 5, 11, 3), (variant((64, 64, 64), "TD3"), 6, 9, 2)]
    for group in (specs[:2], specs[2:]):
        rows, states = final_states(monkeypatch, lambda: driver.experiment_sweep(group, hidden_sweep=True, **kw))
        for i, (v, s, O, A) in enumerate(group):
            solo, solo_state = final_states(monkeypatch, lambda: driver.experiment(v, seed=s, obs_dim=O, action_dim=A, **kw))
            same_state(states[i], solo_state[0], ("sweep", s))
            assert [r[KEY] for r in rows[i]] == [r[KEY] for r in solo] == [0, 3]
