"""GPU: the TD3 objectives on held-out transitions for general-step trainers -- td3_evaluate_general /
td3_evaluate_general_many (k_eval_layer_td3, k_eval_layer, k_eval_y_td3: csrc/td3_eval_general.h), the Python entries over
them (TD3Trainer.evaluate_td3 / td3_evaluate_many with general="device") and the drivers' eval_general="device" under
td3_validation.

Reference: tests/td3_eval_reference_general.py -- td3_eval_reference.evaluate_reference on nets of any depth built from the
weights the device holds now, in float32 (P) and float64 (R).  Bound of every column: the project's per-tensor rule
helpers.check_f64 as it stands, max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5), K == 0 where R == 0, on inputs
at which max|R| is a meaningful unit (conditioned_inputs: chosen from the float64 reference alone, at most 64 seeds).
Everything else -- against sac_q_values_general and sac_policy_act_general, a_smooth and y against their float32 NumPy
restatements, row independence, grouped == solo, isolation of a NaN, "disturbs nothing", the statistics -- is bit for bit
(uint32 views).
On an MI355X the largest |K - f64| / max|R| seen per column is q1 3.7e-6, q2 4.7e-6, q_pi 1.0e-5, tq1 1.7e-6, tq2 3.6e-6,
y 6.8e-8, a_pi 2.2e-6, a_target 2.6e-6, a_smooth 5.6e-7; test_zz_report_the_largest_errors prints the largest error per column and shape (run with -s)."""
import copy
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import ArchTD3TrainerGroup, MlpTD3TrainerGroup, _lib
from robosuite_benchmark_amd.checkpoint import load_checkpoint, save_checkpoint
from robosuite_benchmark_amd.group import runs_general_step, td3_evaluate_many
from robosuite_benchmark_amd.infer import td3_eval_statistics, td3_eval_target, td3_smooth
from tests.helpers import filled_buffer, make_pair, make_td3_pair, synth_transitions
from tests.td3_eval_reference import ARRAY_COLUMNS, COLUMNS, ROW_COLUMNS, batch_dict, inputs, make_td3_trainer
from tests.td3_eval_reference_general import (SHAPES, check_columns, column_scales, conditioned_inputs, rows_of, shape_id)
from tests.test_gpu_td3_evaluate import as_columns, make_io, td3_state

pytestmark = pytest.mark.gpu
TARGETS = ("target_qf1", "target_qf2")
EVAL_ERRORS = {}            # shape id -> {column: largest |K - f64| / max|R| seen in the parity tests}
SIGMA, CLIP = 0.3, 0.25     # non-default smoothing: draws beyond clip / sigma = 0.83 clip, the others do not
LRS = dict(policy_learning_rate=1e-3, qf_learning_rate=5e-4)


def fresh(hp, hq=None, O=42, A=7, seed=5, B=32, **kw):
    """A general-step TD3 trainer: the oracle's fresh nets (critics from `seed`, the two policies from seed + 1000)."""
    t = make_td3_trainer(O, A, tuple(hp), None if hq is None else tuple(hq), seed=seed, batch_size=B, **dict(LRS, **kw))
    assert runs_general_step(t) and t.fused_mode() == 3
    return t


_TRAINERS = {}


def trainer(hp, hq=None, O=42, A=7, seed=5):
    """A general-step TD3 trainer of one shape, weights as created (shared by the tests that do not change them)."""
    key = (tuple(hp), None if hq is None else tuple(hq), O, A, seed)
    if key not in _TRAINERS:
        _TRAINERS[key] = fresh(hp, hq, O, A, seed)
    return _TRAINERS[key]


def eval_g(t, batch, eps, arrays=ARRAY_COLUMNS):
    """td3_evaluate_general through the C ABI: the nine arrays (or fewer)."""
    io, out, _keep = make_io(t, batch, eps, arrays=arrays)
    _lib.check(_lib.load().td3_evaluate_general(t._h, batch[0].shape[0], C.byref(io)), "td3_evaluate_general")
    return as_columns(out)


def many_g(ts, n_rows, ios):
    R = len(ts)
    arr = (_lib.Td3EvalIO * R)(*ios)
    return _lib.load().td3_evaluate_general_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                                 (C.c_int32 * R)(*n_rows), arr)


def bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same(a, b, keys=COLUMNS):
    return all(bits(a[k], b[k]) for k in keys)


def sweep_rows(t, shape, seed, case):
    errors = EVAL_ERRORS.setdefault(shape_id(shape), {})
    params = t.state_dict()["params"]
    scales = column_scales(t, seed, params)
    for n in rows_of(shape):
        batch, eps = conditioned_inputs(t, n, seed + n, scales, params=params)
        check_columns(eval_g(t, batch, eps), t, batch, eps, (case, shape_id(shape)), errors, params)
    print(f"{case} {shape_id(shape)}: largest |K - f64| / max|R| so far: " + "  ".join(f"{k} {errors[k]:.3g}" for k in COLUMNS))


# ---- 1. parity with the float64 reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_parity_on_fresh_weights(shape):
    hp, hq, O, A = shape
    t = trainer(hp, hq, O, A)
    assert t._hidden("policy") == list(hp) and t._hidden("qf1") == list(hq or hp)
    sweep_rows(t, shape, O + A, "fresh")


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_parity_behind_twenty_steps(shape):
    hp, hq, O, A = shape
    t = fresh(hp, hq, O, A)
    before = t.state_dict()["params"]
    t.train_loop(filled_buffer(600, O, A, 3), 20, batch_size=32)
    p = t.state_dict()["params"]
    assert not np.array_equal(p["target_policy"], p["policy"])       # the target chain reads a net of its own ...
    assert not np.array_equal(p["target_policy"], before["target_policy"]) and not np.array_equal(p["policy"], before["policy"])
    sweep_rows(t, shape, O + A + 1, "20 steps")


# ---- 2. bit for bit against what exists ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hp,hq,O,A", [((512, 512), None, 42, 7), ((300, 7, 129), None, 379, 6),
                                       ((64, 64, 64), (512, 512), 42, 7), ((257,), None, 48, 16)])
def test_bitwise_against_the_existing_entries(hp, hq, O, A):
    t = fresh(hp, hq, O, A, seed=6, reward_scale=2.5, discount=0.98, target_policy_noise=SIGMA, target_policy_noise_clip=CLIP)
    t.train_loop(filled_buffer(600, O, A, 4), 12, batch_size=32)
    clipped = np.zeros(0, bool)
    for n in (1, 17, 33, 1000):
        batch, eps = inputs(n, O, A, 100 + n)
        obs, act, rew, term, nobs = batch
        c = eval_g(t, batch, eps)
        q = t.q_values(obs, act, general="device")
        assert bits(c["q1"], q[0]) and bits(c["q2"], q[1]), n
        assert bits(c["a_pi"], t.policy_act_general(obs, True, None)), n
        assert bits(c["q_pi"], t.q_values(obs, c["a_pi"], ("qf1",), general="device")[0]), n
        smooth = td3_smooth(c["a_target"], eps, SIGMA, CLIP)
        assert smooth.dtype == np.float32 and bits(c["a_smooth"], smooth), n
        tq = t.q_values(nobs, c["a_smooth"], TARGETS, general="device")
        assert bits(c["tq1"], tq[0]) and bits(c["tq2"], tq[1]), n
        r, d = rew.reshape(-1), term.reshape(-1).astype(np.float32)
        y = td3_eval_target(r, d, c["tq1"], c["tq2"], 2.5, 0.98)
        assert y.dtype == np.float32 and bits(c["y"], y), n
        assert bits(c["y"][d == 1], (np.float32(2.5) * r)[d == 1]), n
        clipped = np.concatenate([clipped, (np.abs(eps * np.float32(SIGMA)) > np.float32(CLIP)).ravel()])
        # the optional arrays may be left out: a_pi and a_smooth still reach the critics
        few = eval_g(t, batch, eps, arrays=("a_target",))
        assert bits(few["a_target"], c["a_target"]) and same(few, c, ROW_COLUMNS), n
    assert np.any(d == 1) and np.any(d == 0)
    assert np.any(clipped) and np.any(~clipped)                      # some draws clip and some do not


def test_a_target_policy_holding_the_policys_parameters_acts_as_the_policy():
    O, A = 42, 7
    t = fresh((300, 7, 129), O=O, A=A, seed=9)
    state = t.state_dict()
    state["params"]["target_policy"] = state["params"]["policy"].copy()
    t.load_state_dict(state)
    batch, eps = inputs(40, O, A, 3)
    swapped = (batch[4], batch[1], batch[2], batch[3], batch[0])     # a_target(obs) against a_pi(obs): s and s' change places
    c, s = eval_g(t, batch, eps), eval_g(t, swapped, eps)
    assert bits(s["a_target"], c["a_pi"]) and bits(c["a_target"], s["a_pi"])
    assert bits(c["a_target"], t.policy_act_general(batch[4], True, None))
    assert not bits(c["a_target"], c["a_pi"])                        # (s' is not s)


# ---- 3. row and group independence --------------------------------------------------------------------------------------
def test_rows_are_independent_bitwise():
    t = trainer((512, 512))
    batch, eps = inputs(1024, 42, 7, 2)
    full = eval_g(t, batch, eps)
    for r in (0, 15, 16, 17, 1023):
        one = eval_g(t, tuple(x[r:r + 1].copy() for x in batch), eps[r:r + 1].copy())
        for k in COLUMNS:
            assert bits(one[k][0], full[k][r]), (r, k)


def mixed_members():
    """Sixteen general-step TD3 members: depths 1 to 7, a policy deeper than its critics, fused-shape critics, mixed dims,
    smoothing and row counts (0, 1, 15, 16, 17 and 1024 among them); the deepest policy is not the first."""
    extra = [((512, 512), None, 42, 7), ((300, 7, 129), None, 379, 6), ((64, 96, 48), None, 123, 6), ((64, 64, 64), (512, 512), 42, 7)]
    rows = [17, 1, 0, 64, 16, 33, 5, 1024, 300, 2, 15, 7, 48, 1, 100, 1000]
    members = [(trainer(*shape), n) for shape, n in zip(SHAPES, rows)]
    members += [(fresh(hp, hq, O, A, seed=30 + i, target_policy_noise=0.1 + 0.05 * i), n)
                for i, ((hp, hq, O, A), n) in enumerate(zip(extra, rows[len(SHAPES):]))]
    depths = [len(t._hidden("policy")) for t, _ in members]
    assert len(members) == 16 and depths[0] < max(depths)
    return members


def test_grouped_equals_solo_bitwise():
    members = mixed_members()
    made = []
    for i, (t, n) in enumerate(members):
        batch, eps = inputs(max(n, 1), t.obs_dim, t.act_dim, 300 + i)
        made.append((batch, eps) + make_io(t, batch, eps, fill=-5.0))
    ts, n_rows = [t for t, _ in members], [n for _, n in members]
    _lib.check(many_g(ts, n_rows, [m[2] for m in made]), "td3_evaluate_general_many")
    solo = [None if n == 0 else eval_g(t, m[0], m[1]) for (t, n), m in zip(members, made)]
    for i, ((t, n), (batch, eps, _, out, _)) in enumerate(zip(members, made)):
        if n == 0:
            assert all(np.all(v == -5.0) for v in out.values()), i    # sits out: untouched
            continue
        assert same(as_columns(out), solo[i]), i
    # a member that sits out in front: trainers[0] owns the call's stream and staging
    order = [2] + [i for i in range(len(members)) if i != 2]
    again = [make_io(members[i][0], made[i][0], made[i][1], fill=-5.0) for i in order]
    _lib.check(many_g([ts[i] for i in order], [n_rows[i] for i in order], [m[0] for m in again]), "td3_evaluate_general_many")
    for k, i in enumerate(order):
        assert n_rows[i] == 0 or same(as_columns(again[k][1]), solo[i]), i
    # the Python form: each member's own evaluate_td3(general="device"), None for the member that sits out
    batches = [batch_dict(m[0]) if n else None for (_, n), m in zip(members, made)]
    got = td3_evaluate_many(ts, batches, eps=[m[1] for m in made], rows=True, general="device")
    for i, ((t, n), m) in enumerate(zip(members, made)):
        if n == 0:
            assert got[i] is None
            continue
        stats, cols = t.evaluate_td3(batches[i], eps=m[1], rows=True, general="device")
        assert got[i][0] == stats and same(got[i][1], cols) and same(cols, solo[i]), i


def test_python_windows_above_1024_rows_and_the_statistics():
    O, A = 42, 7
    gen = fresh((512, 512), O=O, A=A, seed=3)
    gen.train_loop(filled_buffer(600, O, A, 5), 10, batch_size=32)
    batch, eps = inputs(2500, O, A, 9)
    stats, cols = gen.evaluate_td3(batch_dict(batch), eps=eps, rows=True, general="device")
    assert stats == td3_eval_statistics(np.stack([cols[k] for k in ROW_COLUMNS]), cols["a_pi"])
    assert list(stats.keys())[:-8] == list(gen.get_diagnostics().keys())
    assert stats["Policy Loss"] == -float(np.mean(cols["q_pi"].astype(np.float64)))
    for lo in (0, 1024, 2048):                                       # any n, in calls of at most 1024 rows
        part = eval_g(gen, tuple(x[lo:lo + 1024] for x in batch), eps[lo:lo + 1024])
        assert all(bits(cols[k][lo:lo + 1024], part[k]) for k in COLUMNS), lo


# ---- 4. routing -------------------------------------------------------------------------------------------------------------
def test_routing():
    O, A = 42, 7
    gen = fresh((512, 512), O=O, A=A, seed=3)
    gen.train_loop(filled_buffer(600, O, A, 5), 10, batch_size=32)
    small, seps = inputs(33, O, A, 10)
    # the default stays the host path, bit for bit what it returns today, and differs from the device's somewhere
    host = gen.evaluate_td3(batch_dict(small), eps=seps, rows=True)
    today = gen._evaluate_td3_host(gen._td3_eval_inputs(batch_dict(small), seps, None))
    assert same(host[1], today) and host[0] == td3_eval_statistics(np.stack([today[k] for k in ROW_COLUMNS]), today["a_pi"])
    assert host[0] == gen.evaluate_td3(batch_dict(small), eps=seps, general="host")
    dev = gen.evaluate_td3(batch_dict(small), eps=seps, rows=True, general="device")
    assert same(dev[1], eval_g(gen, small, seps)) and not same(dev[1], host[1])
    check_columns(host[1], gen, small, seps, "host path")
    check_columns(dev[1], gen, small, seps, "device path")
    # a fused-shape trainer takes td3_evaluate under either value; a group call serves both kinds
    fused = make_td3_pair(O, A, 32, seed=4)[1]
    f = fused.evaluate_td3(batch_dict(small), eps=seps, rows=True)
    assert same(fused.evaluate_td3(batch_dict(small), eps=seps, rows=True, general="device")[1], f[1])
    got = td3_evaluate_many([fused, gen], [batch_dict(small)] * 2, eps=[seps] * 2, rows=True, general="device")
    assert got[0][0] == f[0] and same(got[0][1], f[1]) and got[1][0] == dev[0] and same(got[1][1], dev[1])
    group = ArchTD3TrainerGroup([fused, gen])
    assert group.td3_evaluate_many([batch_dict(small)] * 2, eps=[seps] * 2, general="device") == [f[0], dev[0]]
    assert group.td3_evaluate_many([batch_dict(small)] * 2, eps=[seps] * 2) == [f[0], host[0]]
    # a member with _evaluate_on_host goes to the host under either value
    for t, mine in ((gen, host), (fused, None)):
        t._evaluate_on_host = True
        try:
            h = t.evaluate_td3(batch_dict(small), eps=seps, rows=True)
            assert same(t.evaluate_td3(batch_dict(small), eps=seps, rows=True, general="device")[1], h[1])
            assert same(h[1], t._evaluate_td3_host(t._td3_eval_inputs(batch_dict(small), seps, None)))
            assert mine is None or same(h[1], mine[1])
        finally:
            t._evaluate_on_host = False
    with pytest.raises(RuntimeError, match="general"):
        gen.evaluate_td3(batch_dict(small), eps=seps, general="gpu")


# ---- 5. nothing disturbed -------------------------------------------------------------------------------------------------
def test_evaluate_disturbs_nothing():
    O, A, B = 42, 7, 64
    a, b = fresh((512, 512), O=O, A=A, seed=12, B=B, noise_seed=5), fresh((512, 512), O=O, A=A, seed=12, B=B, noise_seed=5)
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    a.train_loop(ba, 5, batch_size=B); b.train_loop(bb, 5, batch_size=B)
    before, diag = td3_state(a, ba), dict(a.get_diagnostics())
    counters = (a._num_train_steps, a._need_to_update_eval_statistics)
    batch, eps = inputs(100, O, A, 4)
    a.evaluate_td3(batch_dict(batch), eps=eps, general="device")
    a.evaluate_td3(batch_dict(batch), general="device")
    io, out, _keep = make_io(a, batch, eps, arrays=())               # null a_* outputs are accepted
    assert _lib.load().td3_evaluate_general(a._h, 100, C.byref(io)) == 0
    full = eval_g(a, batch, eps)
    assert bits(out["rows"], np.stack([full[k] for k in ROW_COLUMNS]))
    for x, y in zip(td3_state(a, ba), before):
        assert np.array_equal(x, y)
    assert dict(a.get_diagnostics()) == diag and (a._num_train_steps, a._need_to_update_eval_statistics) == counters
    for t in (a, b):
        t.end_epoch(0)
    # a loop behind an evaluation == the loop without it: the device noise stream (the smoothing draws) is unmoved
    fa, la = a.train_loop(ba, 10, batch_size=B)
    fb, lb = b.train_loop(bb, 10, batch_size=B)
    assert np.array_equal(fa, fb) and np.array_equal(la, lb) and a.get_diagnostics() == b.get_diagnostics()
    for _ in range(3):                                                # the stepwise path, on device batches
        a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
        a.evaluate_td3(batch_dict(batch), eps=eps, general="device")
    for x, y in zip(td3_state(a, ba), td3_state(b, bb)):
        assert np.array_equal(x, y)


def test_the_shared_scratch_does_not_leak():
    O, A = 42, 7
    t = fresh((300, 7, 129), O=O, A=A, seed=7)
    batch, eps = inputs(200, O, A, 9)
    obs, act = batch[0], batch[1]
    first, q1 = t.policy_act_general(obs, True, None), t.q_values(obs, act, nets=TARGETS + ("qf1", "qf2"), general="device")
    big, beps = inputs(1000, O, A, 10)                                # (the evaluation grows the scratch and fills both buffers)
    cols = eval_g(t, big, beps)
    assert bits(t.policy_act_general(obs, True, None), first)
    assert bits(t.q_values(obs, act, nets=TARGETS + ("qf1", "qf2"), general="device"), q1)
    assert same(eval_g(t, big, beps), cols)
    check_columns(cols, t, big, beps, "behind acting and Q calls")


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    a, b = fresh((512, 512), O=O, A=A, seed=1), trainer((64,) * 7, None, O, A)
    fused = make_td3_pair(O, A, 32, seed=4)[1]
    sac = make_pair(O, A, 32, seed=4, hidden=(512, 512), hidden_q=(512, 512))[1]
    conf = fresh((512, 512), O=O, A=A, seed=6)
    _lib.check(lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    buf = filled_buffer(500, O, A, 2)
    a.train_loop(buf, 3, batch_size=32)
    batch, eps = inputs(8, O, A, 1)
    want, state = eval_g(a, batch, eps), td3_state(a, buf)
    io1, out1, keep1 = make_io(a, batch, eps, fill=3.0)
    io2, out2, keep2 = make_io(b, batch, eps, fill=3.0)

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert all(np.all(v == 3.0) for v in list(out1.values()) + list(out2.values())), what
        for x, y in zip(td3_state(a, buf), state):
            assert np.array_equal(x, y), what
        assert same(eval_g(a, batch, eps), want), what                # a valid call still gives the right values

    def without(io, field):
        c = _lib.Td3EvalIO.from_buffer_copy(io)
        setattr(c, field, None)
        return c

    refused(many_g([a, None], [8, 8], [io1, io2]), "null")
    refused(many_g([a, a], [8, 8], [io1, io2]), "again")
    refused(many_g([a, fused], [8, 8], [io1, io2]), "td3_evaluate is its")
    refused(many_g([a, sac], [8, 8], [io1, io2]), "SAC trainer")
    refused(many_g([a, conf], [8, 8], [io1, io2]), "confined")
    refused(many_g([a] * 17, [8] * 17, [io1] * 17), "1..16 trainers")
    refused(many_g([a, b], [8, 1025], [io1, io2]), "rows")
    refused(many_g([a, b], [8, -1], [io1, io2]), "rows")
    refused(many_g([a, b], [0, 0], [io1, io2]), "no trainer has rows")
    for field in ("obs", "act", "rew", "term", "next_obs", "eps", "rows"):
        refused(many_g([a, b], [8, 8], [io1, without(io2, field)]), "null")
    refused(lib.td3_evaluate_general(a._h, 0, C.byref(io1)), "rows")
    refused(lib.td3_evaluate_general(a._h, 1025, C.byref(io1)), "rows")
    refused(lib.td3_evaluate_general(a._h, 8, None), "bad arguments")
    refused(lib.td3_evaluate_general(None, 8, C.byref(io1)), "bad arguments")
    refused(lib.td3_evaluate_general(fused._h, 8, C.byref(io1)), "td3_evaluate is its")
    refused(lib.td3_evaluate_general(sac._h, 8, C.byref(io1)), "SAC trainer")
    # the fused shapes' entries keep refusing the general-step trainer with their texts
    refused(lib.td3_evaluate(a._h, 8, C.byref(io1)), "general step")
    refused(lib.td3_evaluate(a._h, 8, C.byref(io1)), "forward on the host")
    # a member that sits out is not looked at
    assert many_g([a, b], [8, 0], [io1, _lib.Td3EvalIO()]) == 0 and same(as_columns(out1), want)
    # a confined member is served again once its mask is back to the whole chip
    _lib.check(lib.sac_trainer_set_xcd_mask(conf._h, 0xff), "sac_trainer_set_xcd_mask")
    check_columns(eval_g(conf, batch, eps), conf, batch, eps, "unconfined again")


# ---- 7. behind every path that moves the nets ---------------------------------------------------------------------------
def test_evaluate_follows_the_live_weights(tmp_path):
    O, A, B = 42, 7, 64
    hp = (64, 96, 48)
    hip, other = fresh(hp, O=O, A=A, seed=9, B=B), fresh(hp, O=O, A=A, seed=10, B=B)
    buf, obuf = filled_buffer(2000, O, A, 3), filled_buffer(2000, O, A, 4)
    batch, eps = inputs(40, O, A, 6)
    other.train_loop(obuf, 7, batch_size=B)
    save_checkpoint(str(tmp_path), other, obuf, dict(epoch=0))
    o, ac, rew, term, nobs = synth_transitions(B, O, A, seed=50)
    donor = fresh(hp, O=O, A=A, seed=11, B=B).state_dict()
    steps = [("initial", lambda: None),
             ("train", lambda: [hip.train(dict(observations=o, actions=ac, rewards=rew, terminals=term, next_observations=nobs))
                                for _ in range(2)]),
             ("train_loop", lambda: hip.train_loop(buf, 8, batch_size=B)),
             ("group loop", lambda: MlpTD3TrainerGroup([hip]).train_loop([buf], 6, batch_sizes=[B])),
             ("load_state_dict", lambda: hip.load_state_dict(donor)),
             ("checkpoint load", lambda: load_checkpoint(str(tmp_path), hip, buf))]
    last = None
    for what, move in steps:
        move()
        _, now = hip.evaluate_td3(batch_dict(batch), eps=eps, rows=True, general="device")
        check_columns(now, hip, batch, eps, what)
        if last is not None:
            changed = [k for k in COLUMNS if not bits(now[k], last[k])]
            assert set(changed) == set(COLUMNS), (what, changed)
        last = now
    assert same(last, other.evaluate_td3(batch_dict(batch), eps=eps, rows=True, general="device")[1])      # the loaded state, exactly


# ---- 8. non-finite ----------------------------------------------------------------------------------------------------------
CHAIN_Q, CHAIN_P, CHAIN_N = ("q1", "q2"), ("q_pi", "a_pi"), ("tq1", "tq2", "y", "a_target", "a_smooth")


@pytest.mark.parametrize("hp,O,A", [((512, 512), 42, 7), ((300, 7, 129), 379, 6)])
def test_a_nan_stays_nan_and_alone(hp, O, A):
    t = trainer(hp, None, O, A)
    batch, eps = inputs(33, O, A, 5)
    clean = eval_g(t, batch, eps)
    assert all(np.all(np.isfinite(clean[k])) for k in COLUMNS)
    keep = np.arange(33) != 3
    for which, hit, spared in ((0, CHAIN_Q + CHAIN_P, CHAIN_N), (4, CHAIN_N, CHAIN_Q + CHAIN_P)):
        b = [x.copy() for x in batch]
        b[which][3, 2] = np.nan
        got = eval_g(t, tuple(b), eps)
        for k in hit:
            assert np.all(np.isnan(got[k][3])), (which, k)
            assert bits(got[k][keep], clean[k][keep]), (which, k)
        for k in spared:
            assert bits(got[k], clean[k]), (which, k)
    # a NaN draw: a NaN a_smooth element there and nowhere else; that row's targets follow, a_target and the rest do not
    e = eps.copy()
    e[5, 2] = np.nan
    got = eval_g(t, batch, e)
    at = np.zeros_like(e, bool)
    at[5, 2] = True
    assert np.all(np.isnan(got["a_smooth"][at])) and bits(got["a_smooth"][~at], clean["a_smooth"][~at])
    assert bits(got["a_target"], clean["a_target"]) and all(bits(got[k], clean[k]) for k in CHAIN_Q + CHAIN_P)
    rest = np.arange(33) != 5
    for k in ("tq1", "tq2", "y"):
        assert np.isnan(got[k][5]) and bits(got[k][rest], clean[k][rest]), k


# ---- 9. driver --------------------------------------------------------------------------------------------------------------
def test_hidden_sweep_td3_validation_on_the_device(monkeypatch):
    from robosuite_benchmark_amd import driver
    from tests.test_gpu_td3_evaluate import small_td3_variant
    vs = []
    for hidden in ((128, 64), (64, 96, 48)):                          # the first has the fused kernels' shapes
        v = small_td3_variant()
        v["policy_kwargs"]["hidden_sizes"] = list(hidden)
        v["qf_kwargs"]["hidden_sizes"] = list(hidden)
        vs.append(v)
    runs = [(v, 17 + i) for i, v in enumerate(vs)]
    seen, own, real = [], [], driver.td3_evaluate_many

    def recording(trainers, batches, eps=None, **kw):
        got = real(trainers, batches, eps=eps, **kw)
        seen.append(kw)
        if kw.get("general", "host") == "device":                     # each member's own evaluate_td3 at this point
            assert [runs_general_step(t) for t in trainers] == [False, True]
            mine = [t.evaluate_td3(b, eps=e, general="device") for t, b, e in zip(trainers, batches, eps)]
            assert mine == got
            own.append(mine)
        return got

    monkeypatch.setattr(driver, "td3_evaluate_many", recording)
    kw = dict(num_epochs=2, quiet=True, hidden_sweep=True, td3_validation=True)
    dev = driver.experiment_sweep(copy.deepcopy(runs), eval_general="device", **kw)
    assert seen == [dict(general="device")] * 2
    host = driver.experiment_sweep(copy.deepcopy(runs), eval_general="host", **kw)
    assert seen[2:] == [{}] * 2                                       # (the default call is what it was)
    differs = False
    for i, (rows_d, rows_h) in enumerate(zip(dev, host)):
        assert len(rows_d) == len(rows_h) == 2
        for epoch, (rd, rh) in enumerate(zip(rows_d, rows_h)):
            assert list(rd.keys()) == list(rh.keys()) and "validation/TD Error 2 Min" in rd
            for k in rh:
                if k.startswith("time/"):
                    continue
                if not k.startswith("validation/"):
                    assert rd[k] == rh[k], (i, k)
                elif k != "validation/Num Transitions":
                    assert rd[k] == own[epoch][i][k[len("validation/"):]], (i, k)
                    assert i == 1 or rd[k] == rh[k], (i, k)           # (run 0 has the fused kernels' shapes)
                    differs |= rd[k] != rh[k]
            assert rd["validation/Num Transitions"] == rh["validation/Num Transitions"] > 0
    assert differs                                                    # the general-step run really was evaluated elsewhere


def test_zz_report_the_largest_errors():
    """(prints the largest |K - f64| / max|R| seen by the parity tests, per shape and column: run with -s)"""
    for case in sorted(EVAL_ERRORS):
        print(f"general evaluate_td3 {case}: " + "  ".join(f"{k} {v:.3g}" for k, v in EVAL_ERRORS[case].items()))
    worst = {k: max((e.get(k, 0.0) for e in EVAL_ERRORS.values()), default=0.0) for k in COLUMNS}
    print("general evaluate_td3, largest per column: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
