"""GPU: acting on the device for general-step policies -- sac_policy_act_general / sac_policy_act_general_many
(k_act_layer, csrc/sac_act_general.h), the Python entries over them (SACTrainer.policy_act_general, policy.acting =
"device_all", act_many / GroupActor with general="device") and the drivers' acting="device_all".

Reference: oracle.sac_step_torch.PolicyNet.  Bound (helpers.check_act): max|K - f64| <= max(2e-5, 8 x max|fp32 oracle -
f64|), atol 2e-5 against the fp32 oracle, which check_act first asserts to be well conditioned (within 2.5e-6 of float64).
Row independence, grouped == solo, refusals and routing are bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from robosuite_benchmark_amd import ArchSACTrainerGroup, GroupActor, MlpSACTrainerGroup, _lib
from robosuite_benchmark_amd.group import act_many, runs_general_step
from tests import edge_states as ES
from tests.helpers import (ACT_ERRORS, act_c, act_reference, check_act, draws, filled_buffer, flat_of, is_td3,
                           layers_from_flat, make_pair, make_td3_pair)
from tests.test_gpu_device_acting import assert_rows, small_variant

pytestmark = pytest.mark.gpu

# policy hidden sizes, O, A: K and N on both sides of the 16- and 64-wide tile edges and of the 128-wide reduction chunk,
# K not a multiple of 4, one column tile and many, depth 1 and 7, head widths 2 and 32
SHAPES = [((512, 512), 42, 7), ((256, 256, 256), 42, 7), ((1024,), 42, 7), ((4096,), 42, 7), ((1024, 1024), 42, 7),
          ((300, 7, 129), 379, 6), ((64,) * 7, 42, 7), ((1,), 17, 5), ((257,), 42, 16), ((64, 96, 48), 42, 1)]
TD3_SHAPES = [((512, 512), 42, 7), ((300, 7, 129), 379, 6), ((1,), 17, 5)]
BIG_ROWS = {(512, 512), (300, 7, 129)}              # these run 1024 rows too
CASES = [("sac", *s) for s in SHAPES] + [("td3", *s) for s in TD3_SHAPES]


def shape_id(case):
    algo, hidden, O, A = case
    return f"{algo}-h{'x'.join(map(str, hidden))}-O{O}-A{A}"


_TRAINERS = {}


def trainer(algo, hidden, O, A, seed=5, B=32):
    """A general-step trainer of one shape, weights as created (shared by the tests that do not change them)."""
    key = (algo, tuple(hidden), O, A, seed, B)
    if key not in _TRAINERS:
        _TRAINERS[key] = (make_pair if algo == "sac" else make_td3_pair)(O, A, B, seed=seed, hidden=tuple(hidden))[1]
        assert runs_general_step(_TRAINERS[key])
    return _TRAINERS[key]


def fresh(algo, hidden, O=42, A=7, seed=5, B=32):
    return (make_pair if algo == "sac" else make_td3_pair)(O, A, B, seed=seed, hidden=tuple(hidden))[1]


def policy_layers(t):
    """The policy the device holds NOW, as the oracle's layer list (any depth)."""
    dims = [t.obs_dim] + t._hidden("policy")
    shapes = [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)] + [(t.act_dim, dims[-1])] * (1 if is_td3(t) else 2)
    return layers_from_flat(t.state_dict()["params"]["policy"], shapes)


def act_g(t, obs, deterministic, eps, sentinel=7.0, extra=0):
    """sac_policy_act_general through the C ABI (extra: rows behind the call's, which must keep the sentinel)."""
    n = obs.shape[0]
    out = np.full((n + extra, t.act_dim), sentinel, np.float32)
    e = None if (deterministic or is_td3(t)) else eps
    _lib.check(_lib.load().sac_policy_act_general(t._h, n, _lib.ptr(obs), int(deterministic), _lib.ptr(e), _lib.ptr(out)),
               "sac_policy_act_general")
    assert np.all(out[n:] == sentinel)
    return out[:n]


def many_g(ts, n_rows, obs, det, eps, outs):
    R = len(ts)
    vp = lambda arrs: (C.c_void_p * R)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    return _lib.load().sac_policy_act_general_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                                   (C.c_int32 * R)(*n_rows), vp(obs), (C.c_int32 * R)(*[int(d) for d in det]),
                                                   None if eps is None else vp(eps), vp(outs))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. against the float64 oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=shape_id)
def test_parity_with_the_oracle(case):
    algo, hidden, O, A = case
    t = trainer(algo, hidden, O, A)
    layers = policy_layers(t)
    rs = np.random.RandomState(O + A + len(hidden))
    for n in (1, 16, 17) + ((1024,) if tuple(hidden) in BIG_ROWS else ()):
        obs, eps = draws(rs, n, O, A)
        for det in (True, False):
            got = act_g(t, obs, det, eps, extra=2)
            check_act(t, got, layers, obs, det, eps, (shape_id(case), n, "deterministic" if det else "stochastic"),
                      tag=("general", shape_id(case)))
    if algo == "td3":                                # TD3 is deterministic whatever the flag says, and needs no eps
        assert same_bits(act_g(t, obs, True, None), act_g(t, obs, False, None))


# ---- 2. row independence, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("sac", (512, 512), 42, 7), ("sac", (300, 7, 129), 379, 6), ("td3", (300, 7, 129), 379, 6),
                                  ("sac", (64,) * 7, 42, 7), ("sac", (257,), 42, 16)], ids=shape_id)
def test_rows_are_independent_bitwise(case):
    algo, hidden, O, A = case
    t = trainer(algo, hidden, O, A)
    rs = np.random.RandomState(2)
    obs, eps = draws(rs, 17, O, A)
    for det in (True, False):
        full = act_g(t, obs, det, eps)
        for r in (0, 15, 16):
            one = act_g(t, obs[r:r + 1].copy(), det, eps[r:r + 1].copy())
            assert same_bits(one[0], full[r]), (r, det)
    if tuple(hidden) in BIG_ROWS:
        obs, eps = draws(rs, 1024, O, A)
        full = act_g(t, obs, False, eps)
        blocks = [act_g(t, obs[i:i + 100].copy(), False, eps[i:i + 100].copy()) for i in range(0, 1024, 100)]
        assert same_bits(np.concatenate(blocks), full)
        # Python: any number of rows, in calls of 1024, equal to the C call
        o2, e2 = draws(rs, 1500, O, A)
        got = t.policy_act_general(o2, False, None if is_td3(t) else e2)
        want = np.concatenate([act_g(t, o2[:1024].copy(), False, e2[:1024].copy()), act_g(t, o2[1024:].copy(), False, e2[1024:].copy())])
        assert same_bits(got, want)
    obs1, eps1 = draws(rs, 1, O, A)
    rep = act_g(t, np.repeat(obs1, 37, 0), False, np.repeat(eps1, 37, 0))
    assert same_bits(rep, np.repeat(rep[:1], 37, 0))
    assert same_bits(t.policy_act_general(obs1, True, None), act_g(t, obs1, True, None))


def test_grouped_equals_solo_bitwise():
    ts = [trainer("sac", (512, 512), 42, 7), trainer("td3", (300, 7, 129), 379, 6), trainer("sac", (64,) * 7, 42, 7),
          trainer("sac", (1024,), 42, 7)]
    rows, det = [3, 17, 0, 1], [False, False, False, True]
    rs = np.random.RandomState(4)
    obs, eps, outs = [], [], []
    for t, n, d in zip(ts, rows, det):
        o, e = draws(rs, max(n, 1), t.obs_dim, t.act_dim)
        obs.append(o[:n].copy() if n else o)
        eps.append(None if (d or is_td3(t)) else e[:n].copy())
        outs.append(np.full((n + 3, t.act_dim), -5.0, np.float32))            # (three sentinel rows behind the call's)
    _lib.check(many_g(ts, rows, obs, det, eps, outs), "sac_policy_act_general_many")
    for i, (t, n, d) in enumerate(zip(ts, rows, det)):
        assert np.all(outs[i][n:] == -5.0), i                                 # rows beyond n; the member that sits out
        if n:
            assert same_bits(outs[i][:n], act_g(t, obs[i], d, eps[i])), i
            check_act(t, outs[i][:n], policy_layers(t), obs[i], d, eps[i], ("grouped", i), tag=("general", "grouped"))
    # the sitting-out member in front: trainers[0] owns the call's stream and staging
    order = [2, 0, 1, 3]
    outs2 = [np.full_like(o, -5.0) for o in outs]
    _lib.check(many_g([ts[i] for i in order], [rows[i] for i in order], [obs[i] for i in order], [det[i] for i in order],
                      [eps[i] for i in order], [outs2[i] for i in order]), "sac_policy_act_general_many")
    for a, b in zip(outs, outs2):
        assert same_bits(a, b)
    # act_many(general="device"): the same bits; the default still serves them through policy_act
    got = act_many(ts, [o if n else None for o, n in zip(obs, rows)], det, eps, general="device")
    host = act_many(ts, [o if n else None for o, n in zip(obs, rows)], det, eps)
    for i, (t, n, d) in enumerate(zip(ts, rows, det)):
        assert got[i].shape == (n, t.act_dim) and same_bits(got[i], outs[i][:n]), i
        if n:
            assert same_bits(host[i], t.policy_act(obs[i], d, eps[i])), i
    with pytest.raises(RuntimeError, match="general"):
        act_many(ts[:1], [obs[0]], [False], [eps[0]], general="gpu")


# ---- 3. edges ---------------------------------------------------------------------------------------------------------
EDGE_CASES = [c for c in ES.acting_cases() if tuple(c[4]) in ES.ACT_GENERAL_HIDDEN]


@pytest.mark.parametrize("case", EDGE_CASES, ids=ES.acting_case_id)
def test_edge_matrix(case):
    edge, algo, O, A, hidden = case
    t = fresh(algo, hidden, O, A)
    for n in ES.ACT_ROWS:
        layers, obs, eps, meta = ES.build_acting(edge, algo, O, A, hidden, n, seed=11)
        twin_out = {}
        if edge == "clamp":                          # the twin whose clamped columns sit exactly on the bound
            t._set_params("policy", flat_of(ES.clamp_twin(layers, meta)))
            twin_out = {det: act_g(t, obs, det, eps) for det in (True, False)}
        t._set_params("policy", flat_of(layers))
        for det in (True, False):
            got = act_g(t, obs, det, eps)
            where = (ES.acting_case_id(case), n, "general", "deterministic" if det else "stochastic")
            check_act(t, got, layers, obs, det, eps, where, tag=("general edge", edge))
            if edge == "clamp":
                assert same_bits(got, twin_out[det]), where
            elif edge == "tanh":
                for c, sign in meta["saturated_cols"].items():
                    assert np.all(got[:, c] == sign), (where, c)
                if meta["stoch_col"] is not None and not det:
                    assert np.all(got[meta["stoch_rows"], meta["stoch_col"]] == meta["stoch_signs"]), where
            elif edge == "relu":
                zr = meta["zero_rows"]
                assert same_bits(got[zr], np.repeat(got[:1], zr.size, 0)), where


@pytest.mark.parametrize("algo,O,A,hidden", [("sac", 42, 7, (512, 512)), ("sac", 17, 7, (64, 96, 48)), ("td3", 42, 7, (512, 512))])
def test_a_non_finite_row_stays_in_its_row(algo, O, A, hidden):
    t = fresh(algo, hidden, O, A)
    layers = ES.build_acting("relu", algo, O, A, hidden, 1, seed=11)[0]
    t._set_params("policy", flat_of(layers))
    n = 33
    obs, eps = draws(np.random.RandomState(7), n, O, A)
    for det in (True, False):
        clean = act_g(t, obs, det, eps)
        for row, k in ((0, 0), (16, O // 2), (32, O - 1), (5, O - 1)):
            for bad in (np.nan, np.inf, -np.inf):
                o = obs.copy()
                o[row, k] = bad
                got = act_g(t, o, det, eps)
                where = (det, row, k, bad)
                others = np.arange(n) != row
                assert same_bits(got[others], clean[others]), where
                want = act_reference(layers, is_td3(t), o[row:row + 1], det, eps[row:row + 1], torch.float32)[0]
                assert np.any(np.isnan(want)) or np.all(np.abs(want) == 1.0), where
                assert np.array_equal(np.isnan(got[row]), np.isnan(want)), (where, got[row], want)
                ok = ~np.isnan(want)
                assert np.allclose(got[row][ok], want[ok], atol=2e-5), (where, got[row], want)


# ---- 4. live weights --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_acting_follows_the_live_weights(algo):
    O, A, B = 42, 7, 48
    obs, eps = draws(np.random.RandomState(6), 40, O, A)

    def moved(t, before, where):
        now = act_g(t, obs, False, eps)              # FIRST, without a sync: the call drains the trainer itself
        layers = policy_layers(t)                    # ... and only then the parameters are read
        check_act(t, now, layers, obs, False, eps, (where, "general"), tag=("general", "live"))
        check_act(t, act_g(t, obs, True, None), layers, obs, True, None, (where, "general, deterministic"), tag=("general", "live"))
        assert not np.array_equal(now, before), where
        host = t.policy_act(obs, False, None if is_td3(t) else eps)           # the mirror was neither used nor spoiled
        check_act(t, host, layers, obs, False, eps, (where, "host"), tag=("general", "live host"))
        assert same_bits(act_g(t, obs, False, eps), now), where
        return now

    t, u = fresh(algo, (512, 512), O, A, seed=9, B=B), fresh(algo, (512, 512), O, A, seed=10, B=B)
    buf = filled_buffer(2000, O, A, 3)
    t.policy_act(obs, False, None if is_td3(t) else eps)                      # (the host mirror is warm)
    last = act_g(t, obs, False, eps)
    check_act(t, last, policy_layers(t), obs, False, eps, "initial", tag=("general", "live"))
    t.train_loop(buf, 5, batch_size=B)
    last = moved(t, last, "train_loop")
    t._set_params("policy", u.state_dict()["params"]["policy"])
    last = moved(t, last, "_set_params")
    u.train_loop(buf, 5, batch_size=B)
    t.load_state_dict(u.state_dict())
    moved(t, last, "load_state_dict")


def test_acting_follows_the_live_weights_behind_trainer_groups():
    O, A, B = 42, 7, 48
    obs, eps = draws(np.random.RandomState(6), 40, O, A)
    for kind, hiddens in ((MlpSACTrainerGroup, [(512, 512), (512, 512)]),
                          (ArchSACTrainerGroup, [(256, 256), (512, 512), (64, 96, 48)])):
        ts = [fresh("sac", h, O, A, seed=30 + i, B=B) for i, h in enumerate(hiddens)]
        bufs = [filled_buffer(1500, O, A, 40 + i) for i in range(len(ts))]
        gen = [t for t in ts if runs_general_step(t)]
        before = [act_g(t, obs, False, eps) for t in gen]
        kind(ts).train_loop(bufs, 5)
        for t, b in zip(gen, before):
            now = act_g(t, obs, False, eps)
            layers = policy_layers(t)
            check_act(t, now, layers, obs, False, eps, (kind.__name__, t._hidden("policy")), tag=("general", "live"))
            assert not np.array_equal(now, b)
            check_act(t, t.policy_act(obs, False, eps), layers, obs, False, eps, (kind.__name__, "host"), tag=("general", "live host"))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    a, b = trainer("sac", (512, 512), O, A), trainer("sac", (1024,), O, A)
    td3 = trainer("td3", (512, 512), O, A)
    fused = make_pair(O, A, 32, seed=1)[1]
    conf = fresh("sac", (512, 512), O, A, seed=6)
    _lib.check(lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    obs, eps = draws(np.random.RandomState(1), 8, O, A)
    want = act_g(a, obs, False, eps)
    out, out2 = np.full((8, A), 3.0, np.float32), np.full((8, A), 3.0, np.float32)

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert np.all(out == 3.0) and np.all(out2 == 3.0), what
        ok = np.empty((8, A), np.float32)                            # a valid call still gives the right actions
        assert many_g([a], [8], [obs], [0], [eps], [ok]) == 0 and same_bits(ok, want), what

    two = ([obs, obs], [0, 0], [eps, eps], [out, out2])
    refused(many_g([a, fused], [8, 8], *two), "sac_policy_act_device")
    refused(lib.sac_policy_act_general(fused._h, 8, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out)), "sac_policy_act_device")
    refused(many_g([a, None], [8, 8], *two), "null")
    refused(many_g([a, a], [8, 8], *two), "again")
    refused(many_g([a] * 17, [8] * 17, [obs] * 17, [0] * 17, [eps] * 17, [out] * 17), "1..16 trainers")
    refused(many_g([a, b], [8, -1], *two), "rows")
    refused(many_g([a, b], [8, 1025], *two), "rows")
    refused(many_g([a, b], [0, 0], *two), "no trainer has rows")
    refused(many_g([a, b], [8, 8], [obs, obs], [0, 0], [eps, None], [out, out2]), "eps")
    refused(many_g([a, b], [8, 8], [obs, obs], [0, 0], None, [out, out2]), "eps")
    refused(many_g([a, conf], [8, 8], *two), "confined")
    refused(lib.sac_policy_act_general(a._h, 0, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out)), "rows")
    refused(lib.sac_policy_act_general(a._h, 1025, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out)), "rows")
    refused(lib.sac_policy_act_general(a._h, 8, _lib.ptr(obs), 0, None, _lib.ptr(out)), "eps")
    refused(lib.sac_policy_act_general(None, 8, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out)), "bad arguments")
    with pytest.raises(RuntimeError, match="sac_policy_act_device"):
        fused.policy_act_general(obs, True, None)
    # a confined member is served again once its mask is back to the whole chip
    _lib.check(lib.sac_trainer_set_xcd_mask(conf._h, 0xff), "sac_trainer_set_xcd_mask")
    got = np.full((8, A), 3.0, np.float32)
    assert many_g([a, conf], [8, 8], [obs, obs], [0, 0], [eps, eps], [out, got]) == 0
    assert same_bits(out, want) and same_bits(got, act_g(conf, obs, False, eps))
    check_act(conf, got, policy_layers(conf), obs, False, eps, "unconfined again", tag=("general", "refusals"))
    out[:] = 3.0
    # TD3 needs no eps
    assert many_g([td3], [8], [obs], [0], [None], [out2]) == 0 and not np.any(out2 == 3.0)
    out2[:] = 3.0
    # the three existing entries refuse the general-step trainer with today's text
    R = 2
    vp = lambda arrs: (C.c_void_p * R)(*[x.ctypes.data for x in arrs])  # noqa: E731
    rc = lib.sac_policy_act_many((C.c_void_p * R)(fused._h.value, a._h.value), R, (C.c_int32 * R)(8, 8), vp([obs, obs]),
                                 (C.c_int32 * R)(0, 0), vp([eps, eps]), vp([out, out2]))
    assert rc < 0 and "sac_policy_act is the acting path" in _lib.last_error() and "general step" in _lib.last_error()
    assert np.all(out == 3.0) and np.all(out2 == 3.0)
    rc = lib.sac_policy_act_device(a._h, 8, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out))
    assert rc < 0 and "general step" in _lib.last_error() and np.all(out == 3.0)
    actor = C.c_void_p()
    rc = lib.sac_actor_create(C.byref(actor), (C.c_void_p * 1)(a._h.value), 1, (C.c_int32 * 1)(4))
    assert rc < 0 and not actor and "general step" in _lib.last_error() and "sac_policy_act is the acting path" in _lib.last_error()
    with pytest.raises(RuntimeError, match="sac_policy_act is the acting path"):
        a.policy_act_device(obs, True, None)
    # the defaults of act_many and GroupActor still give the general-step member its policy_act bits
    host = a.policy_act(obs, False, eps)
    got = act_many([fused, a], [obs, obs], [False, False], [eps, eps])
    assert same_bits(got[1], host) and same_bits(got[0], act_c(fused, obs, False, eps))
    g = GroupActor([fused, a], max_rows=8)
    for i in range(2):
        g.obs[i][:], g.eps[i][:] = obs, eps
    g.act([8, 8], False)
    assert same_bits(np.array(g.act[1]), host) and same_bits(np.array(g.act[0]), got[0])
    g.close()
    # ... and a valid call after all of it is correct
    ok = act_g(a, obs, False, eps)
    assert same_bits(ok, want)
    check_act(a, ok, policy_layers(a), obs, False, eps, "after the refusals", tag=("general", "refusals"))


# ---- 6. Python routing ------------------------------------------------------------------------------------------------
def test_policy_acting_device_all_routes_get_actions():
    obs, eps = draws(np.random.RandomState(3), 12, 42, 7)
    e9 = np.random.RandomState(9).standard_normal((12, 7)).astype(np.float32)
    gen, fused = trainer("sac", (512, 512), 42, 7), make_pair(42, 7, 32, seed=2)[1]
    for t, want in ((gen, lambda: act_g(gen, obs, False, e9)), (fused, lambda: act_c(fused, obs, False, e9))):
        t.policy.acting = "host"
        t.policy._noise = np.random.RandomState(9)
        host = t.policy.get_actions(obs)
        after_host = t.policy._noise.standard_normal(4)
        t.policy.acting = "device_all"
        t.policy._noise = np.random.RandomState(9)
        dev = t.policy.get_actions(obs)
        assert np.array_equal(t.policy._noise.standard_normal(4), after_host)        # the stream is consumed as under "host"
        assert same_bits(dev, want()) and same_bits(host, t.policy_act(obs, False, e9))
        assert np.allclose(host, dev, atol=4e-5)
        t.policy.acting = "host"
    gen.policy.acting = "device_all"
    a, info = gen.policy.get_action(obs[0], deterministic=True)
    assert info == {} and same_bits(a[None], act_g(gen, obs[:1].copy(), True, None))
    gen.policy.acting = "device"                     # "device" keeps its meaning: the general step is refused
    with pytest.raises(RuntimeError, match="sac_policy_act is the acting path"):
        gen.policy.get_actions(obs)
    gen.policy.acting = "host"
    td3 = trainer("td3", (512, 512), 42, 7)
    td3.policy.acting = "device_all"
    assert same_bits(td3.policy.get_actions(obs), act_g(td3, obs, True, None))
    td3.policy.acting = "host"


def test_group_actor_with_general_on_the_device():
    ts = [make_pair(42, 7, 32, seed=21)[1], fresh("sac", (512, 512), 42, 7, seed=22), make_td3_pair(46, 7, 32, seed=23)[1],
          fresh("td3", (64, 96, 48), 89, 14, seed=24)]
    rows, det = [5, 4, 3, 6], [False, False, False, False]
    rs = np.random.RandomState(8)
    obs64 = [rs.normal(0, 0.4, (n, t.obs_dim)) for t, n in zip(ts, rows)]           # float64, as an env hands them over
    eps = [rs.normal(size=(n, t.act_dim)).astype(np.float32) for t, n in zip(ts, rows)]
    assert any(np.any(o.astype(np.float32) != o) for o in obs64)
    out = {}
    for general in ("host", "device"):
        g = GroupActor(ts, max_rows=8, general=general)
        for i, n in enumerate(rows):
            g.obs[i][:n], g.eps[i][:n] = obs64[i], eps[i]
            g.act[i][:] = -5.0
        g.act(rows, det)
        out[general] = [np.array(g.act[i]) for i in range(4)]
        if general == "device":
            keep = g
        else:
            g.close()
    for i, (t, n) in enumerate(zip(ts, rows)):
        assert np.all(out["device"][i][n:] == -5.0), i
        o32 = obs64[i].astype(np.float32)
        if runs_general_step(t):
            assert same_bits(out["device"][i][:n], t.policy_act_general(o32, False, eps[i])), i
            assert same_bits(out["host"][i][:n], t.policy_act(o32, False, None if is_td3(t) else eps[i])), i
        else:
            assert same_bits(out["device"][i], out["host"][i]), i
    # a member replaces its handle (a first loop at another batch size): the next act() is still correct
    t = ts[1]
    h0 = t._handle_gen
    t.train_loop(filled_buffer(1500, 42, 7, 3), 3, batch_size=64)
    assert t._handle_gen != h0
    keep.act(rows, det)
    o32 = obs64[1].astype(np.float32)
    assert same_bits(np.array(keep.act[1][:4]), t.policy_act_general(o32, False, eps[1]))
    check_act(t, np.array(keep.act[1][:4]), policy_layers(t), o32, False, eps[1], "after a new handle", tag=("general", "actor"))
    assert same_bits(np.array(keep.act[0]), out["device"][0])
    keep.close()
    with pytest.raises(RuntimeError, match="general"):
        GroupActor(ts, general="gpu")


# ---- 7. drivers -------------------------------------------------------------------------------------------------------
def test_hidden_sweep_with_device_all_equals_solo_experiments():
    from robosuite_benchmark_amd.driver import experiment, experiment_sweep
    vs = [small_variant("Lift-Panda-OSC-POSE-SEED17", (256, 256), batch=100),
          small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512), batch=100),
          small_variant("TwoArmLift-PandaPanda-OSC-POSE-SEED17", (128, 64), batch=100)]
    runs = [(v, 17) for v in vs]
    got = experiment_sweep(copy.deepcopy(runs), num_epochs=2, quiet=True, hidden_sweep=True, acting="device_all")
    solo = [experiment(copy.deepcopy(v), seed=s, num_epochs=2, quiet=True, acting="device_all") for v, s in runs]
    for (v, s), rows, want in zip(runs, got, solo):
        assert_rows(rows, want, v["policy_kwargs"]["hidden_sizes"])
    off = experiment_sweep(copy.deepcopy(runs), num_epochs=2, quiet=True, hidden_sweep=True, acting="device_all", sessions=False)
    for (v, s), rows, want in zip(runs, off, got):
        assert_rows(rows, want, ("sessions=False", v["policy_kwargs"]["hidden_sizes"]))
    dev = experiment_sweep(copy.deepcopy(runs), num_epochs=2, quiet=True, hidden_sweep=True, acting="device")
    for i in (0, 2):                                 # the fused-shape runs: "device_all" is "device" for them
        assert_rows(got[i], dev[i], ("device", i))
    # the general-step run really acted elsewhere: its actions differ from the host forward's in the last bits
    assert any(got[1][1][k] != dev[1][1][k] for k in dev[1][1] if k.startswith("evaluation/Actions"))


def test_experiment_group_with_device_all_resumes(tmp_path):
    from robosuite_benchmark_amd.driver import experiment_group
    v = small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512), batch=100)
    seeds = [17, 18, 19]
    want = experiment_group(copy.deepcopy(v), seeds=seeds, num_epochs=2, quiet=True, acting="device_all")
    ck = str(tmp_path / "ck")
    first = experiment_group(copy.deepcopy(v), seeds=seeds, num_epochs=1, quiet=True, acting="device_all", checkpoint_dir=ck)
    rest = experiment_group(copy.deepcopy(v), seeds=seeds, num_epochs=2, quiet=True, acting="device_all", checkpoint_dir=ck,
                            resume=True)
    for s in seeds:
        assert [r["Epoch"] for r in rest[s]] == [1]
        assert_rows(first[s] + rest[s], want[s], s)


def test_zz_report_the_largest_errors():
    """(prints, per shape, the largest |K - f64| seen by this file's checks and the fp32 oracle's own |fp32 - f64| of that
    call: run with -s)"""
    for tag in sorted(ACT_ERRORS, key=str):
        e, e32, where = ACT_ERRORS[tag]
        print(f"acting errors {tag}: largest |K - f64| {e:.3g} (|fp32 oracle - f64| {e32:.3g}) at {where}")
