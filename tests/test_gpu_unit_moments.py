"""GPU: per-unit statistics of the hidden layers for the fused kernels' shapes on the device -- sac_unit_moments /
sac_unit_moments_many (k_units and k_unit_moments, csrc/sac_units.h), SACTrainer.unit_moments /
group.unit_moments_many over them, and the drivers' unit_diagnostics.

Without a tolerance: the records are byte for byte infer.unit_moments_reference of the activations the same call
returned (tests/unit_reference.same_record), independent of `activations`, of the nets selected and of the other
members; their lengths are the TRUE widths (pad units are not units); constructed units are exact; the weights are the
live ones; the calls leave no trace.  With the project's bound (tests/helpers.check_f64, per layer): the activations
against tests/unit_reference's float64 forward, on fresh shapes and on the trained Lift weights of tests/golden."""
import ctypes as C
import os

import numpy as np
import pytest

from robosuite_benchmark_amd import ArchSACTrainerGroup, MixedSACTrainerGroup, _lib, driver
from robosuite_benchmark_amd.group import merge_unit_moments, unit_moments_many, unit_moments_reference
from robosuite_benchmark_amd.variant import default_variant
from tests.edge_states import build_acting
from tests.helpers import check_f64, filled_buffer, flat_of, full_state, make_pair, make_td3_pair, synth_transitions
from tests.test_gpu_q_values import inputs
from tests.test_gpu_q_values_general import trainer as general_trainer
from tests.test_gpu_unit_moments_general import check_reference, nets_of, same_result, um
from tests.unit_reference import hidden_forward, same_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ERRORS = {}
_TRAINERS = {}


def fresh(algo, hp=(256, 256), O=42, A=7, hq=None, seed=5, B=32, **kw):
    if algo == "td3":
        assert hq is None
        return make_td3_pair(O, A, B, seed=seed, hidden=tuple(hp), **kw)[1]
    return make_pair(O, A, B, seed=seed, hidden=tuple(hp), hidden_q=tuple(hq or hp), **kw)[1]


def trainer(algo, hp=(256, 256), O=42, A=7, hq=None, seed=5):
    """A fused-shape trainer, weights as created (shared by the tests that do not change them)."""
    key = (algo, tuple(hp), O, A, hq, seed)
    if key not in _TRAINERS:
        _TRAINERS[key] = fresh(algo, hp, O, A, hq, seed)
        assert not _TRAINERS[key].runs_general_step()
    return _TRAINERS[key]


def units_c(ts, n_rows, ios, entry="sac_unit_moments_many"):
    R = len(ts)
    return getattr(_lib.load(), entry)((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                       (C.c_int32 * R)(*n_rows), (_lib.SacUnitsIO * R)(*ios))


# ---- 1. / 2. records == the reference of the returned activations; two windows; with and without activations ---------------
@pytest.mark.parametrize("algo,hp,O,A", [("sac", (256, 256), 42, 7), ("td3", (240, 256), 42, 7), ("sac", (64, 32), 17, 5)])
def test_records_are_the_reference_of_the_returned_activations(algo, hp, O, A):
    t = trainer(algo, hp, O, A)
    rs = np.random.RandomState(3)
    for n in (1, 3, 4, 5, 15, 16, 17, 64, 1024):
        obs, act = inputs(rs, n, O, A)
        got = um(t, obs, act)
        assert list(got) == list(nets_of(t))
        check_reference(t, got, n)
        bare = um(t, obs, act, activations=False)
        same_result(bare, got)
        assert all("h" not in r for rec in bare.values() for r in rec)
        same_result(t.unit_moments(obs, act, nets=nets_of(t), activations=True, general="host"), got)    # (either `general`)
    obs, act = inputs(rs, 1030, O, A)
    w0, w1, both = um(t, obs[:1024], act[:1024]), um(t, obs[1024:], act[1024:]), um(t, obs, act)
    check_reference(t, w0, 1024)
    check_reference(t, w1, 6)
    same_result(both, {net: [merge_unit_moments(x, y) for x, y in zip(w0[net], w1[net])] for net in w0})


# ---- 3. any subset of nets ------------------------------------------------------------------------------------------------
def test_any_subset_of_nets_gives_the_same_bytes():
    O, A = 42, 7
    t = trainer("td3", (240, 256), O, A)
    obs, act = inputs(np.random.RandomState(4), 37, O, A)
    full = um(t, obs, act)
    names = nets_of(t)
    for mask in range(1, 64):
        nets = [n for k, n in enumerate(names) if mask >> k & 1][::-1]
        got = um(t, obs, act, nets=nets)
        assert list(got) == nets
        same_result(got, {n: full[n] for n in nets})
    same_result(t.unit_moments(obs, nets=("target_policy", "policy"), activations=True),
                {n: full[n] for n in ("target_policy", "policy")})


# ---- 4. grouped == solo -----------------------------------------------------------------------------------------------------
def test_grouped_is_solo_bytewise():
    shapes = [("sac", (256, 256), 42, 7, None), ("td3", (240, 256), 42, 7, None), ("sac", (64, 32), 17, 5, None),
              ("sac", (64, 32), 42, 7, (256, 256)), ("td3", (16, 16), 17, 5, None), ("sac", (16, 16), 379, 6, None)]
    ts = [trainer(*shapes[i % len(shapes)], seed=5 + i // len(shapes)) for i in range(16)]
    rs = np.random.RandomState(8)
    rows = [(1, 33, 16, 0, 17, 5, 64, 2)[i % 8] for i in range(16)]
    rows[7] = 0                                                                   # a member that sits out, in the middle
    io = [inputs(rs, max(n, 1), t.obs_dim, t.act_dim) for t, n in zip(ts, rows)]
    obs_l = [None if n == 0 else o[:n] for (o, _), n in zip(io, rows)]
    act_l = [None if n == 0 else a[:n] for (_, a), n in zip(io, rows)]
    nets_l = [nets_of(t)[i % 3:] for i, t in enumerate(ts)]
    got = unit_moments_many(ts, obs_l, act_l, nets_l, activations=True)
    for i, (t, n) in enumerate(zip(ts, rows)):
        if n == 0:
            assert got[i] is None
            continue
        same_result(got[i], um(t, obs_l[i], act_l[i], nets=nets_l[i]))
        check_reference(t, got[i], n)
    # both families in one call, and through a group's own method
    gen = general_trainer("sac", (512, 512), 42, 7)
    a, b = trainer("sac", (256, 256), 42, 7), trainer("sac", (64, 32), 42, 7, (256, 256))
    o, ac = inputs(rs, 20, 42, 7)
    for many in (unit_moments_many([a, gen, b], [o] * 3, [ac] * 3, [("policy", "qf1", "qf2")] * 3, activations=True, general="device"),
                 ArchSACTrainerGroup([a, gen, b]).unit_moments_many([o] * 3, [ac] * 3, activations=True, general="device")):
        for t, g in zip((a, gen, b), many):
            same_result(g, um(t, o, ac, nets=("policy", "qf1", "qf2")))
    c = trainer("sac", (256, 256), 42, 7, seed=6)
    bare = MixedSACTrainerGroup([a, c]).unit_moments_many([o] * 2, [ac] * 2)      # (the defaults: records alone)
    same_result(bare[1], um(c, o, ac, nets=("policy", "qf1", "qf2"), activations=False))


# ---- 5. n rows == n one-row calls -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_rows_are_independent_bitwise(algo):
    O, A = 42, 7
    t = trainer(algo, (240, 256), O, A)
    obs, act = inputs(np.random.RandomState(2), 17, O, A)
    whole = um(t, obs, act)
    for r in range(17):
        one = um(t, obs[r:r + 1], act[r:r + 1])
        for net in whole:
            for x, y in zip(whole[net], one[net]):
                assert np.array_equal(x["h"][r:r + 1].view(np.uint32), y["h"].view(np.uint32)), (net, r)


# ---- 6. record lengths are the true widths -------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp,hq", [((16, 16), None), ((64, 32), None), ((240, 256), None), ((256, 256), None),
                                   ((64, 32), (256, 256))])
def test_record_lengths_are_the_true_widths(hp, hq):
    O, A = 42, 7
    t = trainer("sac", hp, O, A, hq)
    obs, act = inputs(np.random.RandomState(7), 19, O, A)
    got = um(t, obs, act)
    for net in got:
        want = list(hp) if net == "policy" else list(hq or hp)
        assert [r["sum"].size for r in got[net]] == want and [r["h"].shape for r in got[net]] == [(19, w) for w in want]
    check_reference(t, got, 19)
    params = t.state_dict()["params"]
    for net in got:
        p32, r64 = (hidden_forward(t, params[net], net, obs, act, d) for d in (np.float32, np.float64))
        for l, r in enumerate(got[net]):
            e = check_f64(f"{hp}/{hq} {net} layer {l}", r["h"], p32[l], r64[l])
            ERRORS[f"fresh {hp}/{hq}"] = max(ERRORS.get(f"fresh {hp}/{hq}", 0.0), e)


# ---- 7. constructed units -------------------------------------------------------------------------------------------------
def test_constructed_units_are_exact():
    O, A, n = 42, 7, 21
    t = fresh("sac", (256, 256), O, A, seed=3)
    obs, act = inputs(np.random.RandomState(6), n, O, A)
    dead, live = (0, 16, 64), (15, 63, 255)
    for net, K in (("policy", O), ("qf1", O + A)):
        flat = t.state_dict()["params"][net].copy()
        for l, off in ((0, 0), (1, 256 * K + 256)):
            k = K if l == 0 else 256
            w, b = flat[off:off + 256 * k].reshape(256, k), flat[off + 256 * k:off + 256 * k + 256]
            for u in dead:
                w[u], b[u] = 0.0, -1.0
            for u in live:
                w[u], b[u] = 0.0, 0.75
        t._set_params(net, flat)
    got = um(t, obs, act, nets=("policy", "qf1"))
    for net in got:
        for r in got[net]:
            for u in dead:
                assert r["sum"][u] == 0 and r["sumsq"][u] == 0 and r["active"][u] == 0 and r["max"][u] == 0, (net, u)
            for u in live:
                assert (r["sum"][u] == 0.75 * n and r["sumsq"][u] == 0.5625 * n and r["active"][u] == n
                        and r["max"][u] == 0.75), (net, u)
        check_reference(t, {net: got[net]}, n)


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_exact_zero_relu_rows(algo):
    """edge_states' relu policy: zero observation rows meet first-layer units of bias 0 (pre-activation exactly 0: not
    active), units 8..11 are dead, units 0..5 of the second layer have a zero row and a zero bias."""
    O, A, n = 42, 7, 33
    t = fresh(algo, (100, 50), O, A, seed=3)
    layers, obs, _, meta = build_acting("relu", algo, O, A, hidden=(100, 50), n=n)
    t._set_params("policy", flat_of(layers))
    got = um(t, obs, None, nets=("policy",))["policy"]
    check_reference(t, {"policy": got}, n)
    first, second = got
    zero = meta["zero_rows"]
    assert np.all(first["h"][zero][:, meta["zero_bias_units"]] == 0)
    assert np.all(first["active"][meta["zero_bias_units"]] <= n - len(zero))
    for f in ("sum", "sumsq", "active", "max"):
        assert np.all(first[f][meta["dead_units"]] == 0) and np.all(second[f][meta["zero_units_deep"]] == 0), f
    assert np.all(first["active"][12:] > 0) and np.all(second["sum"][6:] >= 0)


# ---- 8. a NaN row ---------------------------------------------------------------------------------------------------------
def test_a_nan_row_stays_in_its_member():
    O, A = 42, 7
    a, b = trainer("sac", (256, 256), O, A), trainer("td3", (240, 256), O, A)
    obs, act = inputs(np.random.RandomState(5), 19, O, A)
    bad = obs.copy()
    bad[7, 3] = np.nan
    clean = um(b, obs, act)
    got = unit_moments_many([a, b], [bad, obs], [act, act], [nets_of(a), nets_of(b)], activations=True)
    same_result(got[1], clean)
    for net, records in got[0].items():
        for r in records:
            assert np.all(np.isnan(r["sum"])) and np.all(np.isnan(r["max"])) and np.all(np.isnan(r["sumsq"])), net
            assert np.all(r["active"] <= 18) and same_record(r, unit_moments_reference(r["h"]))


# ---- 9. live weights --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_records_follow_the_live_weights(algo):
    O, A, B = 42, 7, 48
    obs, act = inputs(np.random.RandomState(6), 40, O, A)
    kw = dict(target_update_period=1) if algo == "sac" else dict(policy_and_target_update_period=1)
    t, u, twin = (fresh(algo, (256, 256), O, A, seed=s, B=B, **kw) for s in (9, 10, 11))
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
        MixedSACTrainerGroup([t, u]).train_loop(bufs, 5, batch_sizes=[B, B])
        moved(last, "group loop")


# ---- 10. no trace -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_unit_moments_leave_no_trace(algo):
    O, A, B = 42, 7, 64
    a, b = (fresh(algo, (256, 256), O, A, seed=12, B=B, noise_seed=5) for _ in range(2))
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    rs = np.random.RandomState(4)
    for i in range(3):
        a.train_loop(ba, 2, batch_size=B); b.train_loop(bb, 2, batch_size=B)
        o, ac = inputs(rs, 17 + 500 * (i % 2), O, A)
        um(a, o, ac, activations=bool(i % 2))
    for i in range(3):
        a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
        o, ac = inputs(rs, 33, O, A)
        unit_moments_many([a], [o], [ac], [nets_of(a)])
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y)
    assert list(a.get_diagnostics().items()) == list(b.get_diagnostics().items())


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    a, b, td3 = fresh("sac", seed=1), trainer("sac", (64, 32), O, A), trainer("td3", (240, 256), O, A)
    gen = general_trainer("sac", (512, 512), O, A)
    buf = filled_buffer(500, O, A, 2)
    a.train_loop(buf, 3, batch_size=32)
    obs, act = inputs(np.random.RandomState(1), 8, O, A)
    want, state = um(a, obs, act, nets=("policy", "qf1"), activations=False), full_state(a, buf)
    mom, mom2 = np.full(4 * 1024, 3.0), np.full(4 * 1024, 3.0)

    def io(m, nets=3, o=obs, ac=act):
        return _lib.SacUnitsIO(None if o is None else o.ctypes.data, None if ac is None else ac.ctypes.data, nets, 0,
                               None if m is None else m.ctypes.data, None)

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert np.all(mom == 3.0) and np.all(mom2 == 3.0), what
        for x, y in zip(full_state(a, buf), state):
            assert np.array_equal(x, y), what

    refused(units_c([a, gen], [8, 8], [io(mom), io(mom2)]), "sac_unit_moments_general is the entry")
    refused(units_c([gen, a], [8, 8], [io(mom), io(mom2)], "sac_unit_moments_general_many"), "sac_unit_moments is its")
    refused(units_c([a, b], [8, 8], [io(mom, 1 << 5), io(mom2)]), "only a TD3 trainer")
    refused(units_c([a, b], [8, 8], [io(mom, 0), io(mom2)]), "nets")
    refused(units_c([a, b], [8, 8], [io(mom), io(mom2, 64)]), "nets")
    refused(units_c([a, b], [8, 8], [io(mom, 3, ac=None), io(mom2)]), "actions are null")
    refused(units_c([a, b], [8, 1025], [io(mom), io(mom2)]), "rows")
    refused(units_c([a, a], [8, 8], [io(mom), io(mom2)]), "again")
    refused(units_c([a, b], [8, 8], [io(mom, o=None), io(mom2)]), "null observations or moments")
    refused(units_c([a, b], [0, 0], [io(mom), io(mom2)]), "no trainer has rows")
    one = io(mom)
    refused(lib.sac_unit_moments(a._h, 1025, C.byref(one)), "rows")
    refused(lib.sac_unit_moments(a._h, 0, C.byref(one)), "rows")
    refused(lib.sac_unit_moments(gen._h, 8, C.byref(one)), "sac_unit_moments_general is the entry")
    # bit 5 on a TD3 handle is served, the policies alone with null actions; a valid call still gives the right bytes
    m3 = np.empty(4 * (240 + 256) * 2)
    assert units_c([td3], [8], [io(m3, 1 | 1 << 5, ac=None)]) == 0
    assert lib.sac_unit_moments(a._h, 8, C.byref(one)) == 0
    got = {net: [dict(count=8.0, **{f: mom[(8 * s + 4 * l + j) * 256:(8 * s + 4 * l + j + 1) * 256]
                                   for j, f in enumerate(_lib.UNIT_FIELDS)}) for l in range(2)]
           for s, net in enumerate(("policy", "qf1"))}
    same_result(got, want)


# ---- the activations against the float64 forward: the trained Lift weights -------------------------------------------------
def test_activations_on_trained_lift_weights():
    O, A = 42, 7
    blobs = np.load(os.path.join(HERE, "golden", "trained_weights_lift_seed129.npz"))
    t = fresh("sac", (256, 256), O, A, seed=2)
    names = [n for n in nets_of(t) if n in blobs.files]
    assert "policy" in names and "qf1" in names, blobs.files
    for net in names:
        t._set_params(net, np.asarray(blobs[net], np.float32))
    rs = np.random.RandomState(11)
    for n in (1, 17, 200):
        obs, act = inputs(rs, n, O, A)
        got = um(t, obs, act, nets=names)
        check_reference(t, got, n)
        for net in names:
            p32, r64 = (hidden_forward(t, blobs[net], net, obs, act, d) for d in (np.float32, np.float64))
            for l, r in enumerate(got[net]):
                e = check_f64(f"trained Lift {net} layer {l} n={n}", r["h"], p32[l], r64[l])
                ERRORS["trained Lift"] = max(ERRORS.get("trained Lift", 0.0), e)
    stats = driver.unit_statistics(um(t, obs, act, nets=("policy", "qf1", "qf2"), activations=False))
    assert len(stats) == 12 and all(np.isfinite(v) and v >= 0 for v in stats.values())


# ---- the drivers ------------------------------------------------------------------------------------------------------------
UNIT_KEYS = [f"units/{t} {f}" for t in ("Policy", "QF1", "QF2")
             for f in ("Dormant Fraction", "Dead Fraction", "Active Fraction", "Feature Norm")]


def variant(hidden=(256, 256), algo="SAC"):
    v = default_variant(agent=algo) if algo != "SAC" else default_variant()
    v["algorithm_kwargs"].update(num_epochs=2, num_eval_steps_per_epoch=40, num_expl_steps_per_train_loop=30,
                                 eval_max_path_length=20, expl_max_path_length=20, min_num_steps_before_training=40,
                                 num_trains_per_train_loop=4, batch_size=32)
    v["replay_buffer_size"] = 500
    for kw in ("policy_kwargs", "qf_kwargs"):
        v[kw]["hidden_sizes"] = list(hidden)
    return v


def check_unit_columns(rows, ref=None):
    for row in rows:
        keys = list(row)
        i = keys.index(UNIT_KEYS[0])
        assert keys[i:i + 12] == UNIT_KEYS and keys[i + 12] == "time/data storing (s)"
        for k in UNIT_KEYS:
            assert np.isfinite(row[k]) and row[k] >= 0 and (k.endswith("Feature Norm") or row[k] <= 1), (k, row[k])
    if ref is not None:
        for row, want in zip(rows, ref):
            assert [k for k in row if not k.startswith("units/")] == list(want)


def test_drivers_log_the_units_block():
    O, A = 11, 3
    kw = dict(obs_dim=O, action_dim=A, quiet=True)
    plain = driver.experiment(variant(), seed=3, **kw)
    solo = {s: driver.experiment(variant(), seed=s, unit_diagnostics=True, **kw) for s in (3, 4)}
    check_unit_columns(solo[3], plain)
    for row, want in zip(solo[3], plain):                         # nothing else moves
        assert all(k.startswith(("time/", "units/")) or row[k] == want[k] or (row[k] != row[k] and want[k] != want[k]) for k in row)
    group = driver.experiment_group(variant(), [3, 4], unit_diagnostics=True, **kw)
    for s in (3, 4):
        check_unit_columns(group[s])
        for row, want in zip(group[s], solo[s]):                  # a group's rows equal its members' solo rows
            assert [row[k] for k in UNIT_KEYS] == [want[k] for k in UNIT_KEYS], s
    td3 = driver.experiment(variant(algo="TD3"), seed=3, unit_diagnostics=True, **kw)
    check_unit_columns(td3)


def test_arch_sweep_units_host_and_device_agree():
    O, A = 11, 3
    runs = [(variant((256, 256)), 3, O, A), (variant((300, 200)), 3, O, A), (variant((64, 64, 64)), 4, O, A)]
    kw = dict(hidden_sweep=True, quiet=True, unit_diagnostics=True)
    host = driver.experiment_sweep(runs, **kw)
    dev = driver.experiment_sweep(runs, unit_general="device", **kw)
    # The bound above, propagated.  Host and device activations each stand within eps max|h| of the float64 forward per
    # layer, eps = max(8 e32, 1e-5) = 1e-5 for nets this small (e32, the float32 forward's own error, is some 1e-7), so
    # within 2 eps max|h| of each other.  Feature Norm = ||h||_F / sqrt(n) over the last layer's (n, N) block:
    # |difference| <= sqrt(n N) 2 eps max|h| / sqrt(n), and max|h| <= sqrt(n) Feature Norm, so relative
    # 2 eps sqrt(n N), n = 40 steps.  A fraction moves by 1 / units for every unit that close to its threshold (sum at
    # tau mean; an activation at 0): none is expected among some hundred units with continuous weights -- allowed: two.
    n = 40
    for (v, _, _, _), h_rows, d_rows in zip(runs, host, dev):
        check_unit_columns(h_rows)
        check_unit_columns(d_rows)
        hidden = v["qf_kwargs"]["hidden_sizes"]
        for h, d in zip(h_rows, d_rows):
            for k in UNIT_KEYS:
                if k.endswith("Feature Norm"):
                    assert abs(h[k] - d[k]) <= 2e-5 * np.sqrt(n * hidden[-1]) * abs(h[k]), (k, h[k], d[k])
                else:
                    assert abs(h[k] - d[k]) <= 2.0 / sum(hidden), (k, h[k], d[k])
    # the run of the fused shapes is served by the device under either value: the same bytes
    assert [host[0][e][k] for e in range(2) for k in UNIT_KEYS] == [dev[0][e][k] for e in range(2) for k in UNIT_KEYS]


def test_zz_report_the_largest_errors():
    for case, e in ERRORS.items():
        print(f"unit_moments fused {case}: {e:.3g}")
    if ERRORS:
        print(f"unit_moments fused: largest |K - f64| / max|R| over all cases = {max(ERRORS.values()):.3g}")
