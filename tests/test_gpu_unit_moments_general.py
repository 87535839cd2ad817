"""GPU: per-unit statistics of the hidden layers of general-step trainers on the device -- sac_unit_moments_general /
sac_unit_moments_general_many (k_qval_layer per layer depth and k_unit_moments on its outputs, csrc/sac_units.h,
csrc/sac_units_general.h), SACTrainer.unit_moments / group.unit_moments_many with general="device" over them.

Without a tolerance: the records are byte for byte infer.unit_moments_reference of the activations the same call
returned (tests/unit_reference.same_record: +0 is not -0; a NaN equals any NaN), independent of `activations`, of the
nets selected, of the other members, and follow the live weights.  With the project's bound (tests/helpers.check_f64:
max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5) per layer): the activations against tests/unit_reference's
float64 forward R, P its float32 forward.  Largest ratio max|K - R| / max|R| seen on an MI355X: see
test_zz_report_the_largest_errors (run with -s)."""
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import MlpSACTrainerGroup, _lib
from robosuite_benchmark_amd.group import merge_unit_moments, unit_moments_many, unit_moments_reference
from tests.helpers import check_f64, filled_buffer, full_state, is_td3, make_pair, synth_transitions
from tests.test_gpu_q_values import inputs
from tests.test_gpu_q_values_general import fresh, trainer
from tests.unit_reference import hidden_forward, same_record

pytestmark = pytest.mark.gpu
SAC_NETS = ("policy", "qf1", "qf2", "target_qf1", "target_qf2")
TD3_NETS = SAC_NETS + ("target_policy",)
ERRORS = {}


def nets_of(t):
    return TD3_NETS if is_td3(t) else SAC_NETS


def um(t, obs, act, nets=None, activations=True):
    return t.unit_moments(obs, act, nets=nets or nets_of(t), activations=activations, general="device")


def same_result(a, b, h=True):
    assert list(a) == list(b)
    for net in a:
        assert len(a[net]) == len(b[net]), net
        for l, (x, y) in enumerate(zip(a[net], b[net])):
            assert same_record(x, y), (net, l)
            if h and "h" in x and "h" in y:
                assert x["h"].shape == y["h"].shape and np.array_equal(x["h"].view(np.uint32), y["h"].view(np.uint32)), (net, l)


def check_reference(t, got, n):
    """Every record is the reference of its own activations, of the true width and n rows."""
    for net, records in got.items():
        assert [r["sum"].size for r in records] == t._hidden(net), net
        for l, r in enumerate(records):
            assert r["h"].shape == (n, t._hidden(net)[l]) and r["h"].dtype == np.float32 and r["count"] == n
            assert same_record(r, unit_moments_reference(r["h"])), (net, l, n)


def units_c(ts, n_rows, ios):
    R = len(ts)
    arr = (_lib.SacUnitsIO * R)(*ios)
    return _lib.load().sac_unit_moments_general_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                                     (C.c_int32 * R)(*n_rows), arr)


# ---- 1. records == the reference of the returned activations; two windows -----------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_records_are_the_reference_of_the_returned_activations(algo):
    O, A = 379, 6
    t = trainer(algo, (300, 7, 129), O, A)
    rs = np.random.RandomState(3)
    for n in (1, 3, 4, 5, 15, 16, 17, 64, 1024):
        obs, act = inputs(rs, n, O, A)
        got = um(t, obs, act)
        assert list(got) == list(nets_of(t))
        check_reference(t, got, n)
        # 2. the same record bytes without the activations
        same_result(um(t, obs, act, activations=False), got)
        assert all("h" not in r for rec in um(t, obs, act, activations=False).values() for r in rec)
    obs, act = inputs(rs, 1030, O, A)
    w0, w1, both = um(t, obs[:1024], act[:1024]), um(t, obs[1024:], act[1024:]), um(t, obs, act)
    check_reference(t, w0, 1024)
    check_reference(t, w1, 6)
    same_result(both, {net: [merge_unit_moments(x, y) for x, y in zip(w0[net], w1[net])] for net in w0})


# ---- 3. any subset of nets ------------------------------------------------------------------------------------------------
def test_any_subset_of_nets_gives_the_same_bytes():
    O, A = 42, 7
    t = trainer("td3", (512, 512), O, A)
    obs, act = inputs(np.random.RandomState(4), 37, O, A)
    full = um(t, obs, act)
    for mask in range(1, 64):
        nets = [n for k, n in enumerate(TD3_NETS) if mask >> k & 1][::-1]        # (in another order than the ids')
        got = um(t, obs, act, nets=nets)
        assert list(got) == nets
        same_result(got, {n: full[n] for n in nets})
    # the policy alone needs no actions
    same_result(t.unit_moments(obs, nets=("target_policy", "policy"), activations=True, general="device"),
                {n: full[n] for n in ("target_policy", "policy")})


# ---- 4. grouped == solo -----------------------------------------------------------------------------------------------------
def test_grouped_is_solo_bytewise():
    shapes = [("sac", (300, 7, 129), 379, 6, None), ("td3", (512, 512), 42, 7, None), ("sac", (1,), 17, 5, None),
              ("sac", (512, 512), 42, 7, (256, 256)), ("td3", (1,), 17, 5, None), ("sac", (64,) * 7, 42, 7, None)]
    ts = [trainer(*shapes[i % len(shapes)], seed=5 + i // len(shapes)) for i in range(16)]
    rs = np.random.RandomState(8)
    rows = [(1, 33, 16, 0, 17, 5, 64, 2)[i % 8] for i in range(16)]
    rows[7] = 0                                                                   # a member that sits out, in the middle
    io = [inputs(rs, max(n, 1), t.obs_dim, t.act_dim) for t, n in zip(ts, rows)]
    obs_l = [None if n == 0 else o[:n] for (o, _), n in zip(io, rows)]
    act_l = [None if n == 0 else a[:n] for (_, a), n in zip(io, rows)]
    nets_l = [nets_of(t)[i % 3:] for i, t in enumerate(ts)]
    got = unit_moments_many(ts, obs_l, act_l, nets_l, activations=True, general="device")
    for i, (t, n) in enumerate(zip(ts, rows)):
        if n == 0:
            assert got[i] is None
            continue
        same_result(got[i], um(t, obs_l[i], act_l[i], nets=nets_l[i]))
        check_reference(t, got[i], n)
    # a group of one family's members, through the group's own method
    members = [trainer("sac", (512, 512), 42, 7, seed=5 + i) for i in range(3)]
    o, a = inputs(rs, 20, 42, 7)
    many = MlpSACTrainerGroup(members).unit_moments_many([o] * 3, [a] * 3, activations=True, general="device")
    for t, g in zip(members, many):
        same_result(g, um(t, o, a, nets=("policy", "qf1", "qf2")))


# ---- 5. n rows == n one-row calls -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_rows_are_independent_bitwise(algo):
    O, A = 379, 6
    t = trainer(algo, (300, 7, 129), O, A)
    obs, act = inputs(np.random.RandomState(2), 17, O, A)
    whole = um(t, obs, act)
    for r in range(17):
        one = um(t, obs[r:r + 1], act[r:r + 1])
        for net in whole:
            for x, y in zip(whole[net], one[net]):
                assert np.array_equal(x["h"][r:r + 1].view(np.uint32), y["h"].view(np.uint32)), (net, r)


# ---- 7. constructed units -------------------------------------------------------------------------------------------------
def test_constructed_units_are_exact():
    O, A, n = 42, 7, 21
    t = fresh("sac", (300, 129), O, A, seed=3)
    obs, act = inputs(np.random.RandomState(6), n, O, A)
    dead, live = (0, 16, 64), (15, 63, 299)
    for net, K in (("policy", O), ("qf1", O + A)):
        flat = t.state_dict()["params"][net].copy()
        w, b = flat[:300 * K].reshape(300, K), flat[300 * K:300 * K + 300]
        for u in dead:
            w[u], b[u] = 0.0, -1.0
        for u in live:
            w[u], b[u] = 0.0, 0.75
        t._set_params(net, flat)
    got = um(t, obs, act, nets=("policy", "qf1"))
    for net in got:
        r = got[net][0]
        for u in dead:
            assert r["sum"][u] == 0 and r["sumsq"][u] == 0 and r["active"][u] == 0 and r["max"][u] == 0, (net, u)
        for u in live:
            assert r["sum"][u] == 0.75 * n and r["sumsq"][u] == 0.5625 * n and r["active"][u] == n and r["max"][u] == 0.75, (net, u)
        check_reference(t, {net: got[net]}, n)


# ---- 8. a NaN row ---------------------------------------------------------------------------------------------------------
def test_a_nan_row_stays_in_its_member():
    O, A = 42, 7
    a, b = trainer("sac", (512, 512), O, A), trainer("td3", (512, 512), O, A)
    obs, act = inputs(np.random.RandomState(5), 19, O, A)
    bad = obs.copy()
    bad[7, 3] = np.nan
    clean = [um(t, obs, act) for t in (a, b)]
    got = unit_moments_many([a, b], [bad, obs], [act, act], [nets_of(a), nets_of(b)], activations=True, general="device")
    same_result(got[1], clean[1])
    for net, records in got[0].items():
        for r in records:
            assert np.all(np.isnan(r["sum"])) and np.all(np.isnan(r["max"])) and np.all(np.isnan(r["sumsq"])), net
            assert np.all(r["active"] <= 18)
            assert same_record(r, unit_moments_reference(r["h"]))


# ---- 9. live weights --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_records_follow_the_live_weights(algo):
    O, A, B = 42, 7, 48
    obs, act = inputs(np.random.RandomState(6), 40, O, A)
    kw = dict(target_update_period=1) if algo == "sac" else dict(policy_and_target_update_period=1)
    t, u = fresh(algo, (512, 512), O, A, seed=9, B=B, **kw), fresh(algo, (512, 512), O, A, seed=10, B=B, **kw)
    twin = fresh(algo, (512, 512), O, A, seed=11, B=B, **kw)
    buf = filled_buffer(2000, O, A, 3)

    def moved(before, where):
        now = um(t, obs, act)                        # FIRST, without a sync: the call drains the trainer itself
        params = t.state_dict()["params"]
        for net in nets_of(t):
            twin._set_params(net, params[net])
        same_result(now, um(twin, obs, act))
        assert all(not np.array_equal(now[net][0]["sum"], before[net][0]["sum"]) for net in now), where
        return now

    last = um(t, obs, act)
    o, ac, rew, term, nobs = synth_transitions(B, O, A, seed=50)
    for _ in range(2):
        t.train(dict(observations=o, actions=ac, rewards=rew, terminals=term, next_observations=nobs))
    last = moved(last, "train")
    t.train_loop(buf, 5, batch_size=B)
    last = moved(last, "train_loop")
    for net in nets_of(t):
        t._set_params(net, u.state_dict()["params"][net])
    last = moved(last, "sac_set_params")
    u.train_loop(buf, 5, batch_size=B)
    t.load_state_dict(u.state_dict())
    last = moved(last, "checkpoint load")
    if algo == "sac":
        bufs = [filled_buffer(1500, O, A, 40 + i) for i in range(2)]
        MlpSACTrainerGroup([t, u]).train_loop(bufs, 5)
        moved(last, "group loop")


# ---- 10. no trace -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_unit_moments_leave_no_trace(algo):
    O, A, B = 42, 7, 64
    a, b = fresh(algo, (512, 512), O, A, seed=12, B=B, noise_seed=5), fresh(algo, (512, 512), O, A, seed=12, B=B, noise_seed=5)
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    rs = np.random.RandomState(4)
    for i in range(3):
        a.train_loop(ba, 2, batch_size=B); b.train_loop(bb, 2, batch_size=B)
        o, ac = inputs(rs, 17 + 500 * (i % 2), O, A)
        um(a, o, ac, activations=bool(i % 2))
    for i in range(3):
        da, db = a.train(ba.random_batch(B)), b.train(bb.random_batch(B))
        o, ac = inputs(rs, 33, O, A)
        unit_moments_many([a], [o], [ac], [nets_of(a)], general="device")
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y)
    assert list(a.get_diagnostics().items()) == list(b.get_diagnostics().items())


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    a, b, td3 = fresh("sac", (512, 512), O, A, seed=1), trainer("sac", (1024,), O, A), trainer("td3", (512, 512), O, A)
    fused = make_pair(O, A, 32, seed=4)[1]
    buf = filled_buffer(500, O, A, 2)
    a.train_loop(buf, 3, batch_size=32)
    obs, act = inputs(np.random.RandomState(1), 8, O, A)
    want, state = um(a, obs, act, nets=("policy", "qf1")), full_state(a, buf)
    units = 2 * 1024
    mom, mom2 = np.full(4 * units, 3.0), np.full(4 * 3 * 1024, 3.0)

    def io(m, nets=3, o=obs, ac=act, taps=None):
        return _lib.SacUnitsIO(None if o is None else o.ctypes.data, None if ac is None else ac.ctypes.data, nets, 0,
                               None if m is None else m.ctypes.data, taps)

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert np.all(mom == 3.0) and np.all(mom2 == 3.0), what
        for x, y in zip(full_state(a, buf), state):
            assert np.array_equal(x, y), what

    refused(units_c([a, fused], [8, 8], [io(mom), io(mom2)]), "sac_unit_moments_general serves the general step")
    refused(units_c([a, b], [8, 8], [io(mom, 1 << 5), io(mom2)]), "only a TD3 trainer")
    refused(units_c([a, b], [8, 8], [io(mom, 0), io(mom2)]), "nets")
    refused(units_c([a, b], [8, 8], [io(mom), io(mom2, 64)]), "nets")
    refused(units_c([a, b], [8, 8], [io(mom, 3, ac=None), io(mom2)]), "actions are null")
    refused(units_c([a, b], [8, 1025], [io(mom), io(mom2)]), "rows")
    refused(units_c([a, a], [8, 8], [io(mom), io(mom2)]), "again")
    refused(units_c([a, b], [8, 8], [io(mom, o=None), io(mom2)]), "null observations or moments")
    refused(units_c([a, b], [8, 8], [io(mom), io(None)]), "null observations or moments")
    refused(units_c([a, b], [0, 0], [io(mom), io(mom2)]), "no trainer has rows")
    one = io(mom)
    refused(lib.sac_unit_moments_general(a._h, 1025, C.byref(one)), "rows")
    refused(lib.sac_unit_moments_general(a._h, 0, C.byref(one)), "rows")
    refused(lib.sac_unit_moments_general(fused._h, 8, C.byref(one)), "serves the general step")
    # bit 5 on a TD3 handle is served; the policy alone with null actions too; a valid call still gives the right bytes
    m3 = np.empty(4 * 1024)
    assert units_c([td3], [8], [io(m3, 1 << 5, ac=None)]) == 0
    assert lib.sac_unit_moments_general(a._h, 8, C.byref(one)) == 0
    same_result({k: [dict(r, count=8.0) for r in v] for k, v in want.items()},
                {"policy": [dict(count=8.0, **{f: mom[(4 * l + j) * 512:(4 * l + j + 1) * 512] for j, f in enumerate(_lib.UNIT_FIELDS)})
                            for l in range(2)],
                 "qf1": [dict(count=8.0, **{f: mom[2048 * 2 + (4 * l + j) * 512:2048 * 2 + (4 * l + j + 1) * 512]
                                            for j, f in enumerate(_lib.UNIT_FIELDS)}) for l in range(2)]}, h=False)


# ---- the activations against the float64 forward ---------------------------------------------------------------------------
SHAPES = [("sac", (1,), 17, 5, None), ("sac", (16,), 1, 1, None), ("sac", (300, 7, 129), 379, 6, None),
          ("sac", (64,) * 7, 42, 7, None), ("sac", (4096,), 42, 7, None), ("sac", (512, 512), 42, 7, (256, 256, 256)),
          ("td3", (300, 7, 129), 379, 6, None)]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: f"{c[0]}-q{'x'.join(map(str, c[1]))}-O{c[2]}-A{c[3]}" + ("" if c[4] is None else "-deep"))
def test_activations_against_the_float64_forward(case):
    algo, hq, O, A, hp = case
    t = trainer(algo, hq, O, A, hp)
    params = t.state_dict()["params"]
    rs = np.random.RandomState(O + A + len(hq))
    for n in (17,) if max(hq) == 4096 else (1, 17, 33):
        obs, act = inputs(rs, n, O, A)
        got = um(t, obs, act)
        check_reference(t, got, n)
        for net in got:
            p32 = hidden_forward(t, params[net], net, obs, act, np.float32)
            r64 = hidden_forward(t, params[net], net, obs, act, np.float64)
            for l, r in enumerate(got[net]):
                e = check_f64(f"{case} {net} layer {l} n={n}", r["h"], p32[l], r64[l])
                ERRORS[str(case)] = max(ERRORS.get(str(case), 0.0), e)
    print(f"{case}: largest |K - f64| / max|R| = {ERRORS[str(case)]:.3g}")


def test_the_host_route_agrees_within_the_bound():
    """general="host" (the default for these trainers) is the float32 NumPy forward: its records are the reference of ITS
    activations, and the device's activations stand within the project's bound of the same float64 forward."""
    O, A = 42, 7
    t = trainer("sac", (512, 512), O, A)
    obs, act = inputs(np.random.RandomState(3), 50, O, A)
    host = t.unit_moments(obs, act, nets=SAC_NETS, activations=True)
    assert list(host) == list(SAC_NETS)
    check_reference(t, host, 50)
    params = t.state_dict()["params"]
    for net in SAC_NETS:
        p32 = hidden_forward(t, params[net], net, obs, act, np.float32)
        for l, r in enumerate(host[net]):
            assert np.array_equal(r["h"], p32[l]), (net, l)


def test_zz_report_the_largest_errors():
    for case, e in ERRORS.items():
        print(f"unit_moments general {case}: {e:.3g}")
    if ERRORS:
        print(f"unit_moments general: largest |K - f64| / max|R| over all cases = {max(ERRORS.values()):.3g}")
