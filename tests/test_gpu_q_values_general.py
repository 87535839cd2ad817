"""GPU: evaluating the critics of general-step trainers on the device -- sac_q_values_general /
sac_q_values_general_many (k_qval_layer, csrc/sac_qval_general.h), the Python entries over them (q_values /
q_values_many / q_many with general="device") and the drivers' q_general="device".

Reference: oracle.sac_step_torch.QNet (any depth) on the weights the device holds now (t.state_dict()["params"]), in
float32 (P) and float64 (R).  Bound: the project's per-tensor rule helpers.check_f64,
max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5).  Inputs as in test_gpu_q_values.inputs.  Row independence,
net selection, grouped == solo, routing and "disturbs nothing" are bit for bit.  The weights are as initialised (the
four nets of a trainer are four independent draws) or trained from there with the targets updated on every step.  On an
MI355X the largest error seen is 2.5e-5 of max|R|, on a one-row call whose value is 4.3e-5 (the fp32 oracle itself is
3.4e-5 off there); test_zz_report_the_largest_errors prints the figures per case (run with -s)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from robosuite_benchmark_amd import ArchSACTrainerGroup, MlpSACTrainerGroup, _lib
from robosuite_benchmark_amd.group import q_values_many, runs_general_step
from oracle.sac_step_torch import QNet
from tests.helpers import (check_f64, draws, filled_buffer, full_state, is_td3, layers_from_flat, make_pair, make_td3_pair,
                           synth_transitions)
from tests.test_gpu_q_values import inputs, q_c

pytestmark = pytest.mark.gpu
Q_NETS = ("qf1", "qf2", "target_qf1", "target_qf2")
Q_WORST = {}
Q_ERRORS = {}               # case -> largest |K - f64| / max|R| seen (printed per case; README quotes the largest)

# critic hidden sizes, O, A, policy hidden sizes (None: the critics')
SHAPES = [((512, 512), 42, 7, None), ((256, 256, 256), 42, 7, None), ((1024,), 42, 7, None), ((4096,), 42, 7, None),
          ((300, 7, 129), 379, 6, None),           # first K 385: no multiple of 4
          ((64,) * 7, 42, 7, None),                # eight launches
          ((1,), 17, 5, None),
          ((257,), 48, 16, None),                  # first K 64
          ((64, 96, 48), 122, 6, None),            # first K 128: exactly one chunk
          ((64, 96, 48), 123, 6, None),            # first K 129
          ((256, 256), 42, 7, (512, 512)),         # critics of the fused shape inside a general trainer
          ((512, 512), 42, 7, (256, 256))]
TD3_SHAPES = [((512, 512), 42, 7, None), ((300, 7, 129), 379, 6, None), ((1,), 17, 5, None)]
BIG_ROWS = {(512, 512), (300, 7, 129)}              # these run 15, 16, 1000 and 1024 rows too
CASES = [("sac", *s) for s in SHAPES] + [("td3", *s) for s in TD3_SHAPES]


def shape_id(case):
    algo, hq, O, A, hp = case
    return f"{algo}-q{'x'.join(map(str, hq))}-O{O}-A{A}" + ("" if hp is None else f"-p{'x'.join(map(str, hp))}")


def fresh(algo, hq, O=42, A=7, hp=None, seed=5, B=32, **kw):
    if algo == "td3":
        assert hp is None
        t = make_td3_pair(O, A, B, seed=seed, hidden=tuple(hq), **kw)[1]
    else:
        t = make_pair(O, A, B, seed=seed, hidden=tuple(hp or hq), hidden_q=tuple(hq), **kw)[1]
    return t


_TRAINERS = {}


def trainer(algo, hq, O=42, A=7, hp=None, seed=5):
    """A general-step trainer of one shape, weights as created (shared by the tests that do not change them)."""
    key = (algo, tuple(hq), O, A, hp, seed)
    if key not in _TRAINERS:
        _TRAINERS[key] = fresh(algo, hq, O, A, hp, seed)
        assert runs_general_step(_TRAINERS[key]) and _TRAINERS[key].fused_mode() == 3
    return _TRAINERS[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def q_g(t, obs, act, mask, sentinel=7.0, extra=0):
    """sac_q_values_general through the C ABI: (popcount(mask), n), the selected nets in ascending order (extra: values
    behind the call's, which must keep the sentinel)."""
    k, n = bin(mask).count("1"), obs.shape[0]
    out = np.full(k * n + extra, sentinel, np.float32)
    _lib.check(_lib.load().sac_q_values_general(t._h, n, _lib.ptr(obs), _lib.ptr(act), mask, _lib.ptr(out)),
               "sac_q_values_general")
    assert np.all(out[k * n:] == sentinel)
    return out[:k * n].reshape(k, n)


def many_g(ts, n_rows, obs_l, act_l, masks, out_l):
    R = len(ts)
    vp = lambda arrs: (C.c_void_p * R)(*[None if x is None else x.ctypes.data for x in arrs])  # noqa: E731
    return _lib.load().sac_q_values_general_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                                 (C.c_int32 * R)(*n_rows), vp(obs_l), vp(act_l), (C.c_uint32 * R)(*masks),
                                                 vp(out_l))


def q_params(t):
    return t.state_dict()["params"]


def reference(t, params, net, obs, act, dtype):
    """QNet on the weights the device holds NOW (params: q_params(t)), any depth."""
    dims = [t.obs_dim + t.act_dim] + list(t._hidden("qf1"))
    layers = layers_from_flat(params[net], [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)] + [(1, dims[-1])])
    with torch.no_grad():
        return QNet(layers, dtype=dtype)(torch.from_numpy(obs).to(dtype), torch.from_numpy(act).to(dtype)).numpy()[:, 0]


def check_against_oracle(t, params, got, nets, obs, act, case):
    assert got.shape == (len(nets), obs.shape[0]) and got.dtype == np.float32, (case, got.shape)
    refs = []
    for row, net in zip(got, nets):
        p32, r64 = reference(t, params, net, obs, act, torch.float32), reference(t, params, net, obs, act, torch.float64)
        e = check_f64(f"{case} {net} n={obs.shape[0]}", row, p32, r64)
        Q_ERRORS[str(case)] = max(Q_ERRORS.get(str(case), 0.0), e)
        if e >= Q_WORST.get("e", 0.0):               # the largest error overall, with the fp32 oracle's own of that call
            s = float(np.max(np.abs(r64)))
            Q_WORST.update(e=e, where=f"{case} {net} n={obs.shape[0]}", max_r=s, fp32=float(np.max(np.abs(p32 - r64))) / s)
        refs.append(r64)
    return refs


def assert_nets_differ(refs, case):
    """(a kernel that reads the wrong net must not pass: the four nets' references are four different rows)"""
    for i in range(len(refs)):
        for j in range(i):
            assert not np.allclose(refs[i], refs[j], rtol=1e-3, atol=0), (case, i, j)


# ---- 1. parity with the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=shape_id)
def test_parity_with_the_oracle(case):
    algo, hq, O, A, hp = case
    t = trainer(algo, hq, O, A, hp)
    assert t._hidden("qf1") == list(hq) and t._hidden("policy") == list(hp or hq)
    params = q_params(t)
    rs = np.random.RandomState(O + A + len(hq))
    for n in (1, 17, 33) + ((15, 16, 1000, 1024) if tuple(hq) in BIG_ROWS and hp is None else ()):
        obs, act = inputs(rs, n, O, A)
        got = q_g(t, obs, act, 15, extra=3)
        refs = check_against_oracle(t, params, got, Q_NETS, obs, act, shape_id(case))
        if n > 1:
            assert_nets_differ(refs, (shape_id(case), n))
    print(f"{shape_id(case)}: largest |K - f64| / max|R| = {Q_ERRORS[shape_id(case)]:.3g}")


# ---- 2. live weights --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_q_values_follow_the_live_weights(algo):
    O, A, B = 42, 7, 48
    obs, act = inputs(np.random.RandomState(6), 40, O, A)
    kw = dict(target_update_period=1) if algo == "sac" else dict(policy_and_target_update_period=1)
    t, u = fresh(algo, (512, 512), O, A, seed=9, B=B, **kw), fresh(algo, (512, 512), O, A, seed=10, B=B, **kw)
    buf = filled_buffer(2000, O, A, 3)

    def moved(before, where):
        now = q_g(t, obs, act, 15)                   # FIRST, without a sync: the call drains the trainer itself
        refs = check_against_oracle(t, q_params(t), now, Q_NETS, obs, act, ("live", where))
        assert_nets_differ(refs, where)
        assert all(not np.array_equal(x, y) for x, y in zip(now, before)), where
        assert same_bits(q_g(t, obs, act, 15), now), where
        return now

    last = q_g(t, obs, act, 15)
    check_against_oracle(t, q_params(t), last, Q_NETS, obs, act, ("live", "initial"))
    o, ac, rew, term, nobs = synth_transitions(B, O, A, seed=50)
    for _ in range(2):                               # (TD3 moves its targets on every second step at most)
        t.train(dict(observations=o, actions=ac, rewards=rew, terminals=term, next_observations=nobs))
    last = moved(last, "train")
    t.train_loop(buf, 5, batch_size=B)
    last = moved(last, "train_loop")
    for net in Q_NETS:
        t._set_params(net, u.state_dict()["params"][net])
    last = moved(last, "sac_set_params")
    u.train_loop(buf, 5, batch_size=B)
    t.load_state_dict(u.state_dict())
    moved(last, "checkpoint load")


def test_q_values_follow_the_live_weights_behind_trainer_groups():
    O, A, B = 42, 7, 48
    obs, act = inputs(np.random.RandomState(6), 40, O, A)
    for kind, hiddens in ((MlpSACTrainerGroup, [(512, 512), (512, 512)]),
                          (ArchSACTrainerGroup, [(256, 256), (512, 512), (64, 96, 48)])):
        ts = [fresh("sac", h, O, A, seed=30 + i, B=B, target_update_period=1) for i, h in enumerate(hiddens)]
        bufs = [filled_buffer(1500, O, A, 40 + i) for i in range(len(ts))]
        gen = [t for t in ts if runs_general_step(t)]
        before = [q_g(t, obs, act, 15) for t in gen]
        kind(ts).train_loop(bufs, 5)
        for t, b in zip(gen, before):
            now = q_g(t, obs, act, 15)
            refs = check_against_oracle(t, q_params(t), now, Q_NETS, obs, act, ("live", kind.__name__))
            assert_nets_differ(refs, kind.__name__)
            assert all(not np.array_equal(x, y) for x, y in zip(now, b)), kind.__name__


# ---- 3. row independence, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
@pytest.mark.parametrize("hq,O,A", [((512, 512), 42, 7), ((300, 7, 129), 379, 6)])
def test_rows_are_independent_bitwise(algo, hq, O, A):
    t = trainer(algo, hq, O, A)
    rs = np.random.RandomState(2)
    for n in (15, 16, 17, 33, 1000):
        obs, act = inputs(rs, n, O, A)
        full = q_g(t, obs, act, 15)
        for r in sorted({0, 1, n // 2, 15 % n, 16 % n, n - 1}):
            one = q_g(t, obs[r:r + 1].copy(), act[r:r + 1].copy(), 15)
            assert same_bits(one[:, 0], full[:, r]), (n, r)
    # ... and on neither n nor the row's place: the same (obs, act) in every row gives the same value in every row
    obs1, act1 = inputs(rs, 1, O, A)
    rep = q_g(t, np.repeat(obs1, 37, 0), np.repeat(act1, 37, 0), 15)
    assert rep.shape == (4, 37) and same_bits(rep, np.repeat(rep[:, :1], 37, 1))


# ---- 4. net selection -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,hq,O,A", [("sac", (512, 512), 42, 7), ("td3", (300, 7, 129), 379, 6)])
def test_a_subset_of_nets_gives_the_same_bits_in_any_order(algo, hq, O, A):
    t = trainer(algo, hq, O, A)
    obs, act = inputs(np.random.RandomState(3), 50, O, A)
    full = q_g(t, obs, act, 15)
    assert_nets_differ(list(full), "mask 15")
    for mask in range(1, 16):
        rows = [k for k in range(4) if mask >> k & 1]
        assert same_bits(q_g(t, obs, act, mask), full[rows]), mask
    for nets in (("qf2",), ("target_qf2", "qf1"), ("target_qf1", "qf2", "qf1"), Q_NETS[::-1], "qf2"):
        names = [nets] if isinstance(nets, str) else list(nets)
        got = t.q_values(obs, act, nets=nets, general="device")
        assert got.shape == (len(names), 50) and same_bits(got, full[[Q_NETS.index(x) for x in names]]), nets
    assert same_bits(t.q_values(obs, act, general="device"), full[:2])          # the default nets: qf1, qf2
    # any n, in calls of at most 1024 rows
    obs, act = inputs(np.random.RandomState(4), 2500, O, A)
    big = t.q_values(obs, act, nets=("qf2", "target_qf1"), general="device")
    for lo in (0, 1024, 2048):
        assert same_bits(big[:, lo:lo + 1024], q_g(t, obs[lo:lo + 1024], act[lo:lo + 1024], 2 | 4)), lo


# ---- 5. grouped == solo -----------------------------------------------------------------------------------------------
def mixed_members():
    """16 general-step members: SAC and TD3, depths 1 to 7 (later launches hold fewer jobs), mixed dims, row counts with
    0, 1, 16, 17, 1000 and 1024 among them, another net mask for almost every member."""
    shapes = [((512, 512), 42, 7), ((300, 7, 129), 379, 6), ((64,) * 7, 42, 7), ((1024,), 46, 7), ((64, 96, 48), 123, 6),
              ((33,) * 4, 89, 14), ((40,) * 5, 64, 4), ((24,) * 6, 73, 12), ((257,), 48, 16), ((1,), 17, 5)]
    rows = [1, 17, 0, 64, 5, 16, 0, 300, 1, 33, 2, 0, 1024, 7, 48, 1000]
    members = []
    for i in range(16):
        hq, O, A = shapes[i % len(shapes)]
        members.append((trainer("td3" if i % 3 == 2 else "sac", hq, O, A, seed=20 + i), rows[i], 1 + (7 * i + 2) % 15))
    return members


def test_grouped_equals_solo_bitwise():
    members = mixed_members()
    assert any(is_td3(t) for t, _, _ in members) and not all(is_td3(t) for t, _, _ in members)
    assert {len(t._hidden("qf1")) for t, _, _ in members} == set(range(1, 8))
    assert {0, 1, 16, 17, 1000, 1024} <= {n for _, n, _ in members} and len({m for _, _, m in members}) == 15
    rs = np.random.RandomState(16)
    obs, act, outs = [], [], []
    for t, n, mask in members:
        o, a = inputs(rs, n, t.obs_dim, t.act_dim)
        obs.append(o); act.append(a)
        outs.append(np.full((bin(mask).count("1"), n if n else 3), -5.0, np.float32))      # (sentinel)
    _lib.check(many_g([t for t, _, _ in members], [n for _, n, _ in members], obs, act, [m for _, _, m in members], outs),
               "sac_q_values_general_many")
    for i, (t, n, mask) in enumerate(members):
        if n == 0:
            assert np.all(outs[i] == -5.0), i                         # a member that sits out: untouched
        else:
            assert same_bits(outs[i], q_g(t, obs[i], act[i], mask)), i
            nets = [x for k, x in enumerate(Q_NETS) if mask >> k & 1]
            check_against_oracle(t, q_params(t), outs[i], nets, obs[i], act[i], "grouped")
    # a member that sits out in front: trainers[0] owns the call's stream and staging
    order = [2] + [i for i in range(16) if i != 2]
    outs2 = [np.full_like(o, -5.0) for o in outs]
    _lib.check(many_g([members[i][0] for i in order], [members[i][1] for i in order], [obs[i] for i in order],
                      [act[i] for i in order], [members[i][2] for i in order], [outs2[i] for i in order]),
               "sac_q_values_general_many")
    for a, b in zip(outs, outs2):
        assert same_bits(a, b)
    # the Python form: the same values in the order of the names, empty arrays for the members that sit out
    names = [[x for k, x in enumerate(Q_NETS) if m >> k & 1][::-1] for _, _, m in members]
    got = q_values_many([t for t, _, _ in members], [o if o.shape[0] else None for o in obs], act, names, general="device")
    for i, (t, n, _) in enumerate(members):
        assert got[i].shape == (len(names[i]), n) and (n == 0 or same_bits(got[i], outs[i][::-1])), i


# ---- 6. non-finite rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,hq,O,A", [("sac", (512, 512), 42, 7), ("sac", (300, 7, 129), 379, 6), ("td3", (512, 512), 42, 7)])
def test_a_non_finite_row_stays_in_its_row(algo, hq, O, A):
    t = trainer(algo, hq, O, A)
    n = 33
    obs, act = inputs(np.random.RandomState(5), n, O, A)
    clean = q_g(t, obs, act, 15)
    assert np.all(np.isfinite(clean))
    for which, row, k in (("obs", 3, 2), ("obs", 16, O - 1), ("act", 32, A - 1), ("act", 0, 0)):
        for bad in (np.nan, np.inf, -np.inf):
            o, a = obs.copy(), act.copy()
            (o if which == "obs" else a)[row, k] = bad
            got = q_g(t, o, a, 15)
            assert not np.any(np.isfinite(got[:, row])), (which, row, k, bad, got[:, row])
            keep = np.arange(n) != row
            assert same_bits(got[:, keep], clean[:, keep]), (which, row, k, bad)


# ---- 7. disturbs nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_q_values_disturb_nothing(algo):
    O, A, B = 42, 7, 64
    a, b = fresh(algo, (512, 512), O, A, seed=12, B=B, noise_seed=5), fresh(algo, (512, 512), O, A, seed=12, B=B, noise_seed=5)
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    rs = np.random.RandomState(4)
    a.train_loop(ba, 3, batch_size=B); b.train_loop(bb, 3, batch_size=B)
    before = full_state(a, ba)
    a.q_values(*inputs(rs, 100, O, A), nets=Q_NETS, general="device")
    for x, y in zip(full_state(a, ba), before):
        assert np.array_equal(x, y)
    for i in range(4):                                                # a loop with Q calls between its steps
        a.train_loop(ba, 2, batch_size=B); b.train_loop(bb, 2, batch_size=B)
        a.q_values(*inputs(rs, 17 + 500 * (i % 2), O, A), nets=Q_NETS[i:], general="device")
    for i in range(3):                                                # stepwise
        a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
        qo, qa = inputs(rs, 33, O, A)
        q_values_many([a], [qo], [qa], [Q_NETS], general="device")
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_the_shared_scratch_does_not_leak_into_acting(algo):
    O, A = 42, 7
    t = fresh(algo, (300, 7, 129), O, A, seed=7)
    rs = np.random.RandomState(9)
    obs, eps = draws(rs, 200, O, A)
    e = None if is_td3(t) else eps
    first = t.policy_act_general(obs, False, e)
    qo, qa = inputs(rs, 1000, O, A)                                  # (the Q call grows the scratch and fills both buffers)
    q1 = t.q_values(qo, qa, nets=Q_NETS, general="device")
    again = t.policy_act_general(obs, False, e)
    assert same_bits(first, again)
    assert same_bits(t.q_values(qo, qa, nets=Q_NETS, general="device"), q1)
    check_against_oracle(t, q_params(t), q1, Q_NETS, qo, qa, "behind acting")


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    a, b = fresh("sac", (512, 512), O, A, seed=1), trainer("sac", (1024,), O, A)
    fused = make_pair(O, A, 32, seed=4)[1]
    conf = fresh("sac", (512, 512), O, A, seed=6)
    _lib.check(lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    buf = filled_buffer(500, O, A, 2)
    a.train_loop(buf, 3, batch_size=32)
    obs, act = inputs(np.random.RandomState(1), 8, O, A)
    want, state = q_g(a, obs, act, 3), full_state(a, buf)
    out, out2 = np.full((2, 8), 3.0, np.float32), np.full((2, 8), 3.0, np.float32)

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert np.all(out == 3.0) and np.all(out2 == 3.0), what
        for x, y in zip(full_state(a, buf), state):
            assert np.array_equal(x, y), what
        ok = np.empty((2, 8), np.float32)                             # a valid call still gives the right values
        assert many_g([a], [8], [obs], [act], [3], [ok]) == 0 and same_bits(ok, want), what

    two = ([obs, obs], [act, act])
    refused(many_g([a, None], [8, 8], *two, [3, 3], [out, out2]), "null")
    refused(many_g([a, a], [8, 8], *two, [3, 3], [out, out2]), "again")
    refused(many_g([a, fused], [8, 8], *two, [3, 3], [out, out2]), "sac_q_values is its")
    refused(many_g([a, conf], [8, 8], *two, [3, 3], [out, out2]), "confined")
    refused(many_g([a] * 17, [8] * 17, [obs] * 17, [act] * 17, [3] * 17, [out] * 17), "1..16 trainers")
    refused(many_g([a, b], [8, 1025], *two, [3, 3], [out, out2]), "rows")
    refused(many_g([a, b], [8, -1], *two, [3, 3], [out, out2]), "rows")
    refused(many_g([a, b], [8, 8], *two, [3, 0], [out, out2]), "nets")
    refused(many_g([a, b], [8, 8], *two, [16, 3], [out, out2]), "nets")
    refused(many_g([a, b], [8, 8], [obs, None], [act, act], [3, 3], [out, out2]), "null observations")
    refused(many_g([a, b], [8, 8], [obs, obs], [None, act], [3, 3], [out, out2]), "null observations")
    refused(many_g([a, b], [8, 8], *two, [3, 3], [out, None]), "null observations")
    refused(many_g([a, b], [0, 0], *two, [3, 3], [out, out2]), "no trainer has rows")
    refused(lib.sac_q_values_general(a._h, 0, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "rows")
    refused(lib.sac_q_values_general(a._h, 1025, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "rows")
    refused(lib.sac_q_values_general(a._h, 8, _lib.ptr(obs), _lib.ptr(act), 0, _lib.ptr(out)), "nets")
    refused(lib.sac_q_values_general(a._h, 8, _lib.ptr(obs), _lib.ptr(act), 32, _lib.ptr(out)), "nets")
    refused(lib.sac_q_values_general(a._h, 8, None, _lib.ptr(act), 3, _lib.ptr(out)), "bad arguments")
    refused(lib.sac_q_values_general(fused._h, 8, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "sac_q_values is its")
    refused(lib.sac_q_values_general(None, 8, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "bad arguments")
    if _lib.device_count() > 1:                                       # (needs a second GPU to build the case)
        far = fresh("sac", (512, 512), O, A, seed=6, device=1)
        refused(many_g([a, far], [8, 8], *two, [3, 3], [out, out2]), "device")
    # the fused shapes' entries keep refusing the general-step trainer with their text
    refused(lib.sac_q_values(a._h, 8, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "forward on the host")
    # a member that sits out is not looked at: its mask and its arrays may be anything
    assert many_g([a, b], [8, 0], [obs, None], [act, None], [3, 99], [out, None]) == 0 and same_bits(out, want)
    # a confined member is served again once its mask is back to the whole chip
    _lib.check(lib.sac_trainer_set_xcd_mask(conf._h, 0xff), "sac_trainer_set_xcd_mask")
    check_against_oracle(conf, q_params(conf), q_g(conf, obs, act, 15), Q_NETS, obs, act, "unconfined again")


# ---- 9. routing -------------------------------------------------------------------------------------------------------
def test_routing():
    O, A = 42, 7
    gen, gen2 = trainer("sac", (512, 512), O, A), trainer("td3", (512, 512), O, A)
    fused, fused2 = make_pair(O, A, 32, seed=1)[1], make_pair(O, A, 32, seed=2, hidden=(128, 64))[1]
    obs, act = inputs(np.random.RandomState(1), 40, O, A)
    nets = ("qf2", "target_qf1")
    # the default on a general-step trainer: the host path, bit for bit
    host = gen._q_values_host(obs, act, list(nets))
    assert same_bits(gen.q_values(obs, act, nets=nets), host) and same_bits(gen.q_values(obs, act, nets=nets, general="host"), host)
    dev = gen.q_values(obs, act, nets=nets, general="device")
    assert same_bits(dev, q_g(gen, obs, act, 2 | 4))
    # a fused-shape trainer takes sac_q_values under either value
    assert same_bits(fused.q_values(obs, act, nets=nets, general="device"), fused.q_values(obs, act, nets=nets))
    assert same_bits(fused.q_values(obs, act, nets=nets), q_c(fused, obs, act, 2 | 4))
    # q_values_many over fused-shape members, general-step members and members that sit out
    ts = [fused, gen, fused2, gen2, trainer("sac", (64,) * 7, O, A)]
    big_o, big_a = inputs(np.random.RandomState(2), 1100, O, A)
    obs_l, act_l = [obs, big_o, None, obs[:7], None], [act, big_a, None, act[:7], None]
    nets_l = [nets, Q_NETS[::-1], nets, "qf1", nets]
    for got in (q_values_many(ts, obs_l, act_l, nets_l, general="device"),
                ArchSACTrainerGroup([fused, gen, fused2]).q_many(obs_l[:3], act_l[:3], nets_l[:3], general="device") + [None] * 2):
        for i, (t, o, a, ns) in enumerate(zip(ts, obs_l, act_l, nets_l)):
            if got[i] is None:
                continue
            k = 1 if isinstance(ns, str) else len(ns)
            if o is None:
                assert got[i].shape == (k, 0), i
            else:
                assert same_bits(got[i], t.q_values(o, a, nets=ns, general="device")), i
    # the default of q_values_many keeps the general-step members on the host
    default = q_values_many(ts, obs_l, act_l, nets_l)
    assert same_bits(default[1], gen._q_values_host(big_o, big_a, list(Q_NETS[::-1])))
    assert same_bits(default[0], fused.q_values(obs, act, nets=nets))
    with pytest.raises(RuntimeError, match="general"):
        q_values_many(ts, obs_l, act_l, nets_l, general="gpu")


# ---- 10. drivers ------------------------------------------------------------------------------------------------------
Q_COLUMNS = [f"evaluation/{name} {s}" for name in ("Q1 Estimates", "Q2 Estimates", "Returns To Go", "Q Bias")
             for s in ("Mean", "Std", "Max", "Min")]


def test_hidden_sweep_q_diagnostics_on_the_device(monkeypatch):
    from robosuite_benchmark_amd import driver
    from tests.test_gpu_device_acting import small_variant
    vs = [small_variant("Lift-Panda-OSC-POSE-SEED17", (256, 256), batch=100),
          small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512), batch=100),
          small_variant("Lift-Panda-OSC-POSE-SEED17", (64, 96, 48), batch=100)]
    runs = [(v, 17 + i) for i, v in enumerate(vs)]
    seen, real = [], driver.q_values_many

    def recording(trainers, obs_l, act_l, nets_l, **kw):
        got = real(trainers, obs_l, act_l, nets_l, **kw)
        seen.append(kw)
        for t, o, a, ns, q in zip(trainers, obs_l, act_l, nets_l, got):          # the Q values behind the columns
            check_against_oracle(t, q_params(t), q, list(ns), _lib.f32(o), _lib.f32(a), ("sweep", kw.get("general", "host")))
        return got

    monkeypatch.setattr(driver, "q_values_many", recording)
    kw = dict(num_epochs=2, quiet=True, hidden_sweep=True, q_diagnostics=True)
    dev = driver.experiment_sweep(copy.deepcopy(runs), q_general="device", **kw)
    assert seen == [dict(general="device")] * 2
    host = driver.experiment_sweep(copy.deepcopy(runs), q_general="host", **kw)
    assert seen[2:] == [{}] * 2                                       # (the default call is what it was)
    monkeypatch.undo()
    for (v, s), rows in zip(runs, dev):
        want = driver.experiment(copy.deepcopy(v), seed=s, num_epochs=2, quiet=True, q_diagnostics=True, q_general="device")
        assert len(rows) == len(want) == 2
        for rg, rw in zip(rows, want):
            assert list(rg.keys()) == list(rw.keys()) and all(k in rg for k in Q_COLUMNS)
            for k in rw:
                if not k.startswith("time/"):
                    assert rg[k] == rw[k], (s, k)
    differs = False
    for i, (rows_d, rows_h) in enumerate(zip(dev, host)):
        for rd, rh in zip(rows_d, rows_h):
            assert list(rd.keys()) == list(rh.keys())
            for k in rh:
                if k.startswith("time/"):
                    continue
                if k not in Q_COLUMNS or "Returns To Go" in k or i == 0:      # (run 0 has the fused kernels' shapes)
                    assert rd[k] == rh[k], (i, k)
                else:                                                 # (the Q values behind these: checked in `recording`)
                    differs |= rd[k] != rh[k]
    assert differs                                                    # the general-step runs really were evaluated elsewhere


def test_zz_report_the_largest_errors():
    """(prints the largest |K - f64| / max|R| seen by this file's checks, per case: run with -s)"""
    for case in sorted(Q_ERRORS):
        print(f"general q_values {case}: largest |K - f64| / max|R| = {Q_ERRORS[case]:.3g}")
    if Q_WORST:
        print("general q_values: largest overall = {e:.3g} at {where} (max|R| {max_r:.3g}; the fp32 oracle's own {fp32:.3g})"
              .format(**Q_WORST))
