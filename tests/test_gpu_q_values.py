"""GPU: evaluating the critics on the device -- sac_q_values / sac_q_values_many (k_qval, csrc/sac_qval.h), the Python
entry points over them (SACTrainer.q_values, FlattenMlp.__call__, group.q_values_many / q_many) and the epoch drivers'
q_diagnostics=True.

Reference: oracle.sac_step_torch.QNet on the weights the device holds now, in float32 (P) and float64 (R).  Bound: the
project's per-tensor rule helpers.check_f64, max|K - R| / max|R| <= max(8 max|P - R| / max|R|, 1e-5).  On the trained
Lift weights of tests/golden, observations N(0, 0.4) and actions tanh(N(0, 1)), the fp32 oracle itself is 0.7e-7 to
2.2e-7 of max|R| away from float64 (max|q| 54 to 1440 there), so the floor is the bound; it was set from those numbers
on the CPU, not from anything the kernel gives.  Row independence, grouped == solo and "disturbs nothing" are bit for
bit."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from robosuite_benchmark_amd import ArchSACTrainerGroup, FlattenMlp, _lib
from robosuite_benchmark_amd.group import q_values_many
from oracle.sac_step_torch import QNet
from tests.helpers import (check_f64, draws, filled_buffer, full_state, layers_from_flat, make_pair, make_pair_from_flat,
                           make_td3_pair, synth_transitions)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 15, 16, 17, 1000, 1024)
Q_NETS = ("qf1", "qf2", "target_qf1", "target_qf2")
Q_ERRORS = {}               # case -> largest |K - f64| / max|R| seen (printed per case; README quotes the largest)


def trained_flats():
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_weights_lift_seed129.npz"))
    return {k: z[k] for k in z.files}


def inputs(rs, n, O, A):
    obs, eps = draws(rs, n, O, A)
    return obs, np.tanh(eps)


def mask_of(nets):
    return sum(_lib.Q_NET_BITS[n] for n in nets)


def q_c(t, obs, act, mask):
    """sac_q_values through the C ABI: (popcount(mask), n), the selected nets in ascending order."""
    out = np.full((bin(mask).count("1"), obs.shape[0]), 7.0, np.float32)
    _lib.check(_lib.load().sac_q_values(t._h, obs.shape[0], _lib.ptr(obs), _lib.ptr(act), mask, _lib.ptr(out)),
               "sac_q_values")
    return out


def q_params(t):
    return t.state_dict()["params"]


def reference(t, params, net, obs, act, dtype):
    """QNet on the weights the device holds NOW (params: q_params(t))."""
    hs, K = t._hidden("qf1"), t.obs_dim + t.act_dim
    layers = layers_from_flat(params[net], [(hs[0], K), (hs[1], hs[0]), (1, hs[1])])
    with torch.no_grad():
        return QNet(layers, dtype=dtype)(torch.from_numpy(obs).to(dtype), torch.from_numpy(act).to(dtype)).numpy()[:, 0]


def check_against_oracle(t, params, got, nets, obs, act, case):
    assert got.shape == (len(nets), obs.shape[0]) and got.dtype == np.float32, (case, got.shape)
    for row, net in zip(got, nets):
        e = check_f64(f"{case} {net} n={obs.shape[0]}", row, reference(t, params, net, obs, act, torch.float32),
                      reference(t, params, net, obs, act, torch.float64))
        Q_ERRORS[str(case)] = max(Q_ERRORS.get(str(case), 0.0), e)


def sweep_rows(t, seed, case, nets=Q_NETS):
    rs, params = np.random.RandomState(seed), q_params(t)
    for n in ROWS:
        obs, act = inputs(rs, n, t.obs_dim, t.act_dim)
        check_against_oracle(t, params, q_c(t, obs, act, mask_of(nets)), nets, obs, act, case)
    print(f"{case}: largest |K - f64| / max|R| = {Q_ERRORS[str(case)]:.3g}")


# ---- 1. parity with the oracle ----------------------------------------------------------------------------------------
def test_parity_on_trained_weights():
    _, hip = make_pair_from_flat(trained_flats(), 42, 7, 64)       # (the fixture has no targets)
    sweep_rows(hip, 1, "trained Lift", nets=("qf1", "qf2"))


@pytest.mark.parametrize("O,A,hidden", [(16, 1, (256, 256)), (17, 7, (256, 256)), (42, 7, (256, 256)), (48, 16, (256, 256)),
                                        (177, 6, (256, 256)), (379, 6, (256, 256)), (496, 7, (256, 256)), (42, 7, (128, 64))])
def test_parity_on_fresh_weights(O, A, hidden):
    _, hip = make_pair(O, A, 32, seed=5, hidden=hidden)
    sweep_rows(hip, O + A, (O, A, hidden))


def test_parity_td3():
    _, hip = make_td3_pair(42, 7, 32, seed=4)
    sweep_rows(hip, 3, "td3")


# ---- 2. against the step itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,A", [(42, 7), (379, 6)])                # (379: the step splits its first layer)
def test_q_values_agree_with_the_step(O, A):
    B = 32
    _, hip = make_pair(O, A, B, seed=7)
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=11)
    params = q_params(hip)
    before = hip.q_values(obs, act)                                   # qf1, qf2 on the weights the step starts from
    hip.train(dict(observations=obs, actions=act, rewards=rew, terminals=term, next_observations=nobs))
    for row, net, name in zip(before, ("qf1", "qf2"), ("q1", "q2")):
        step = hip.debug_fetch(name, B)
        p32, r64 = reference(hip, params, net, obs, act, torch.float32), reference(hip, params, net, obs, act, torch.float64)
        e_q, e_s = check_f64(f"q_values {net}", row, p32, r64), check_f64(f"step {name}", step, p32, r64)
        s = float(np.max(np.abs(r64)))
        e_p, diff = float(np.max(np.abs(p32 - r64))) / s, float(np.max(np.abs(row.astype(np.float64) - step))) / s
        print(f"({O},{A}) {net}: q_values {e_q:.3g}  step {e_s:.3g}  |q_values - step| {diff:.3g}  fp32 oracle {e_p:.3g}")
        assert diff <= max(8.0 * e_p, 1e-5), (net, diff, e_p)


# ---- 3. row independence ----------------------------------------------------------------------------------------------
def test_rows_are_independent_bitwise():
    _, hip = make_pair(42, 7, 32, seed=6)
    rs = np.random.RandomState(2)
    for n in (15, 16, 17, 33, 1000):
        obs, act = inputs(rs, n, 42, 7)
        full = q_c(hip, obs, act, 15)
        for r in sorted({0, 1, n // 2, 15 % n, 16 % n, n - 1}):
            one = q_c(hip, obs[r:r + 1].copy(), act[r:r + 1].copy(), 15)
            assert np.array_equal(one[:, 0], full[:, r]), (n, r)
    # ... and on neither n nor the row's place: the same (obs, act) in every row gives the same value in every row
    obs1, act1 = inputs(rs, 1, 42, 7)
    rep = q_c(hip, np.repeat(obs1, 37, 0), np.repeat(act1, 37, 0), 15)
    assert rep.shape == (4, 37) and np.all(rep == rep[:, :1])


def test_a_subset_of_nets_gives_the_same_bits_in_any_order():
    _, hip = make_pair(42, 7, 32, seed=6)
    obs, act = inputs(np.random.RandomState(3), 50, 42, 7)
    full = q_c(hip, obs, act, 15)
    for mask in range(1, 16):
        rows = [k for k in range(4) if mask >> k & 1]
        assert np.array_equal(q_c(hip, obs, act, mask), full[rows]), mask
    for nets in (("qf2",), ("target_qf2", "qf1"), ("target_qf1", "qf2", "qf1"), Q_NETS[::-1], "qf2"):
        names = [nets] if isinstance(nets, str) else list(nets)
        got = hip.q_values(obs, act, nets=nets)
        assert got.shape == (len(names), 50) and np.array_equal(got, full[[Q_NETS.index(x) for x in names]]), nets
    assert np.array_equal(hip.q_values(obs, act), full[:2])          # the default: qf1, qf2
    # any n, in calls of at most 1024 rows
    obs, act = inputs(np.random.RandomState(4), 2500, 42, 7)
    big = hip.q_values(obs, act, nets=("qf2", "target_qf1"))
    for lo in (0, 1024, 2048):
        assert np.array_equal(big[:, lo:lo + 1024], q_c(hip, obs[lo:lo + 1024], act[lo:lo + 1024], 2 | 4)), lo


# ---- 4. non-finite rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(256, 256), (128, 64)])
def test_a_nan_row_stays_nan_and_alone(hidden):
    _, hip = make_pair(42, 7, 32, seed=8, hidden=hidden)
    obs, act = inputs(np.random.RandomState(5), 20, 42, 7)
    clean = q_c(hip, obs, act, 15)
    assert np.all(np.isfinite(clean))
    for which in ("obs", "act"):
        o, a = obs.copy(), act.copy()
        (o if which == "obs" else a)[3, 2] = np.nan
        got = q_c(hip, o, a, 15)
        assert np.all(np.isnan(got[:, 3])), which
        keep = np.arange(20) != 3
        assert np.array_equal(got[:, keep], clean[:, keep]), which


# ---- 5. grouped == solo -----------------------------------------------------------------------------------------------
def mixed_members(R):
    """Like test_gpu_device_acting.mixed_members: mixed dims, SAC and TD3, a (128, 64) member, row counts with 0, 1, 16,
    17 and 1000 among them, another net mask for every member."""
    dims = [(42, 7), (46, 7), (89, 14), (379, 6), (64, 4), (73, 12), (50, 4)]
    rows = [1, 17, 0, 64, 5, 16, 0, 300, 1, 33, 2, 0, 1000, 7, 48, 1]
    members = []
    for i in range(R):
        O, A = dims[i % len(dims)]
        if i % 3 == 2:
            t = make_td3_pair(O, A, 32, seed=20 + i)[1]
        else:
            t = make_pair(O, A, 32, seed=20 + i, hidden=(128, 64) if i % 5 == 4 else (256, 256))[1]
        members.append((t, rows[i] if R > 2 else (16, 17)[i], 1 + (7 * i + 2) % 15))
    return members


def many(ts, n_rows, obs_l, act_l, masks, out_l):
    R = len(ts)
    vp = lambda arrs: (C.c_void_p * R)(*[None if x is None else x.ctypes.data for x in arrs])  # noqa: E731
    return _lib.load().sac_q_values_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                         (C.c_int32 * R)(*n_rows), vp(obs_l), vp(act_l), (C.c_uint32 * R)(*masks), vp(out_l))


@pytest.mark.parametrize("R", [2, 7, 16])
def test_grouped_equals_solo_bitwise(R):
    members = mixed_members(R)
    assert R == 2 or (any("target_policy" in t.NETS for t, _, _ in members) and any(n == 0 for _, n, _ in members))
    assert R < 16 or {0, 1, 16, 17, 1000} <= {n for _, n, _ in members}
    assert len({m for _, _, m in members}) == min(R, 15)              # (there are fifteen masks)
    rs = np.random.RandomState(R)
    obs, act, outs = [], [], []
    for t, n, mask in members:
        o, a = inputs(rs, n, t.obs_dim, t.act_dim)
        obs.append(o); act.append(a)
        outs.append(np.full((bin(mask).count("1"), n if n else 3), -5.0, np.float32))      # (sentinel)
    _lib.check(many([t for t, _, _ in members], [n for _, n, _ in members], obs, act, [m for _, _, m in members], outs),
               "sac_q_values_many")
    for i, (t, n, mask) in enumerate(members):
        if n == 0:
            assert np.all(outs[i] == -5.0), i                         # a member that sits out: untouched
        else:
            assert np.array_equal(outs[i], q_c(t, obs[i], act[i], mask)), i
            nets = [x for k, x in enumerate(Q_NETS) if mask >> k & 1]
            check_against_oracle(t, q_params(t), outs[i], nets, obs[i], act[i], ("grouped", R))
    # the Python form: the same values in the order of the names, empty arrays for the members that sit out
    names = [[x for k, x in enumerate(Q_NETS) if m >> k & 1][::-1] for _, _, m in members]
    got = q_values_many([t for t, _, _ in members], [o if o.shape[0] else None for o in obs], act, names)
    for i, (t, n, _) in enumerate(members):
        assert got[i].shape == (len(names[i]), n) and (n == 0 or np.array_equal(got[i], outs[i][::-1])), i


def test_a_general_step_member_takes_the_host_path():
    O, A = 42, 7
    a, b = make_pair(O, A, 32, seed=1)[1], make_pair(O, A, 32, seed=2, hidden=(128, 64))[1]
    gen = make_pair(O, A, 32, seed=4, hidden=(512, 512))[1]
    assert gen.fused_mode() == 3
    obs, act = inputs(np.random.RandomState(1), 40, O, A)
    outs = [np.full((2, 40), -5.0, np.float32) for _ in range(3)]
    assert many([a, gen, b], [40] * 3, [obs] * 3, [act] * 3, [3] * 3, outs) < 0
    assert "general step" in _lib.last_error() and "host" in _lib.last_error()
    assert all(np.all(o == -5.0) for o in outs)
    solo = [t.q_values(obs, act, nets=("qf2", "target_qf1")) for t in (a, gen, b)]
    got = ArchSACTrainerGroup([a, gen, b]).q_many([obs] * 3, [act] * 3, [("qf2", "target_qf1")] * 3)
    for g, s in zip(got, solo):
        assert np.array_equal(g, s)
    assert np.array_equal(solo[0], q_c(a, obs, act, 2 | 4))
    # the host path is the float32 forward on the live weights: against the oracle, and against the holder's own forward
    check_against_oracle(gen, q_params(gen), solo[1], ("qf2", "target_qf1"), obs, act, "general step, host path")
    assert np.allclose(solo[1][0], gen.qf2.forward_np(obs, act)[:, 0], rtol=1e-5, atol=1e-6)
    default = ArchSACTrainerGroup([a, gen, b]).q_many([obs] * 3, [act] * 3)
    assert np.array_equal(default[0], a.q_values(obs, act)) and np.array_equal(default[1], gen.q_values(obs, act))


# ---- 6. live weights; nothing disturbed ---------------------------------------------------------------------------------
def test_q_values_follow_the_live_weights():
    O, A, B = 42, 7, 64
    obs, act = inputs(np.random.RandomState(6), 40, O, A)
    _, hip = make_pair(O, A, B, seed=9)
    buf = filled_buffer(2000, O, A, 3)
    last = hip.q_values(obs, act, nets=Q_NETS)
    check_against_oracle(hip, q_params(hip), last, Q_NETS, obs, act, "initial")
    for what in ("train_loop", "device batches"):
        if what == "train_loop":
            hip.train_loop(buf, 8, batch_size=B)
        else:
            for _ in range(6):                                        # stepwise, nothing synchronised
                hip.train(buf.random_batch(B))
        now = hip.q_values(obs, act, nets=Q_NETS)
        check_against_oracle(hip, q_params(hip), now, Q_NETS, obs, act, what)
        assert all(not np.array_equal(x, y) for x, y in zip(now, last)), what
        last = now


def test_q_values_disturb_nothing():
    O, A, B = 42, 7, 64
    (_, a), (_, b) = make_pair(O, A, B, seed=12, noise_seed=5), make_pair(O, A, B, seed=12, noise_seed=5)
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    rs = np.random.RandomState(4)
    a.train_loop(ba, 5, batch_size=B); b.train_loop(bb, 5, batch_size=B)
    before = full_state(a, ba)
    obs, act = inputs(rs, 100, O, A)
    a.q_values(obs, act, nets=Q_NETS)
    for x, y in zip(full_state(a, ba), before):
        assert np.array_equal(x, y)
    for _ in range(6):                                                # the fused stepwise path, on device batches
        a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
        a.q_values(*inputs(rs, 17, O, A))
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y)
    for i in range(6):                                                # host batches
        o, ac, rew, term, nobs = synth_transitions(B, O, A, seed=50 + i)
        for t in (a, b):
            t.train(dict(observations=o, actions=ac, rewards=rew, terminals=term, next_observations=nobs))
        a.q_values(*inputs(rs, 33, O, A), nets=("target_qf2",))
        q_values_many([a], [obs], [act], [Q_NETS])
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    (_, a), (_, b) = make_pair(O, A, 32, seed=1), make_pair(O, A, 32, seed=2)
    _, gen = make_pair(O, A, 32, seed=4, hidden=(512, 512))
    _, conf = make_pair(O, A, 32, seed=5)
    _lib.check(lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    buf = filled_buffer(500, O, A, 2)
    a.train_loop(buf, 3, batch_size=32)
    obs, act = inputs(np.random.RandomState(1), 8, O, A)
    want, state = q_c(a, obs, act, 3), full_state(a, buf)
    out, out2 = np.full((2, 8), 3.0, np.float32), np.full((2, 8), 3.0, np.float32)

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert np.all(out == 3.0) and np.all(out2 == 3.0), what
        for x, y in zip(full_state(a, buf), state):
            assert np.array_equal(x, y), what
        ok = np.empty((2, 8), np.float32)                             # a valid call still gives the right values
        assert many([a], [8], [obs], [act], [3], [ok]) == 0 and np.array_equal(ok, want), what

    two = ([obs, obs], [act, act])
    refused(many([a, None], [8, 8], *two, [3, 3], [out, out2]), "null")
    refused(many([a, a], [8, 8], *two, [3, 3], [out, out2]), "again")
    refused(many([a, gen], [8, 8], *two, [3, 3], [out, out2]), "forward on the host")
    refused(many([a, conf], [8, 8], *two, [3, 3], [out, out2]), "confined")
    refused(many([a, b], [8, 1025], *two, [3, 3], [out, out2]), "rows")
    refused(many([a, b], [8, -1], *two, [3, 3], [out, out2]), "rows")
    refused(many([a, b], [8, 8], *two, [3, 0], [out, out2]), "nets")
    refused(many([a, b], [8, 8], *two, [16, 3], [out, out2]), "nets")
    refused(many([a, b], [8, 8], [obs, None], [act, act], [3, 3], [out, out2]), "null observations")
    refused(many([a, b], [8, 8], [obs, obs], [None, act], [3, 3], [out, out2]), "null observations")
    refused(many([a, b], [8, 8], *two, [3, 3], [out, None]), "null observations")
    refused(many([a, b], [0, 0], *two, [3, 3], [out, out2]), "no trainer has rows")
    refused(lib.sac_q_values(a._h, 0, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "rows")
    refused(lib.sac_q_values(a._h, 1025, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "rows")
    refused(lib.sac_q_values(a._h, 8, _lib.ptr(obs), _lib.ptr(act), 0, _lib.ptr(out)), "nets")
    refused(lib.sac_q_values(a._h, 8, _lib.ptr(obs), _lib.ptr(act), 32, _lib.ptr(out)), "nets")
    refused(lib.sac_q_values(a._h, 8, None, _lib.ptr(act), 3, _lib.ptr(out)), "bad arguments")
    refused(lib.sac_q_values(gen._h, 8, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "general step")
    refused(lib.sac_q_values(None, 8, _lib.ptr(obs), _lib.ptr(act), 3, _lib.ptr(out)), "bad arguments")
    if _lib.device_count() > 1:                                       # (needs a second GPU to build the case)
        _, far = make_pair(O, A, 32, seed=6, device=1)
        refused(many([a, far], [8, 8], *two, [3, 3], [out, out2]), "device")
    # a member that sits out is not looked at: its mask and its arrays may be anything
    assert many([a, b], [8, 0], [obs, None], [act, None], [3, 99], [out, None]) == 0 and np.array_equal(out, want)


# ---- 8. holders -------------------------------------------------------------------------------------------------------
def test_holders_answer_from_the_live_weights():
    O, A, B = 42, 7, 64
    _, hip = make_pair(O, A, B, seed=3)
    obs, act = inputs(np.random.RandomState(2), 30, O, A)
    initial = hip.qf1.forward_np(obs, act)
    hip.train_loop(filled_buffer(1000, O, A, 5), 10, batch_size=B)
    for name in Q_NETS:
        got = getattr(hip, name)(obs, act)
        assert got.shape == (30, 1) and got.dtype == np.float32
        assert np.array_equal(got, hip.q_values(obs, act, nets=(name,)).reshape(30, 1)), name
    assert np.array_equal(hip.qf1.forward_np(obs, act), initial)      # forward_np: still the initial host weights
    assert not np.allclose(hip.qf1(obs, act), initial, rtol=1e-4, atol=1e-6)
    free = FlattenMlp([32, 16], 1, O + A, rs=np.random.RandomState(1))
    assert np.array_equal(free(obs, act), free.forward_np(obs, act)) and free(obs, act).shape == (30, 1)


# ---- 9. drivers -------------------------------------------------------------------------------------------------------
Q_COLUMNS = [f"evaluation/{name} {s}" for name in ("Q1 Estimates", "Q2 Estimates", "Returns To Go", "Q Bias")
             for s in ("Mean", "Std", "Max", "Min")]


def small_variant():
    from robosuite_benchmark_amd import variant
    v = variant.load_variant(os.path.join(ROOT, "tests", "golden", "Lift-Panda-OSC-POSE-SEED17.variant.json"))
    v["algorithm_kwargs"].update(min_num_steps_before_training=150, num_eval_steps_per_epoch=130,
                                 num_expl_steps_per_train_loop=170, num_trains_per_train_loop=40,
                                 eval_max_path_length=50, expl_max_path_length=60)
    v["replay_buffer_size"] = 3000
    return v


def test_experiment_q_diagnostics(monkeypatch):
    from robosuite_benchmark_amd import driver
    from robosuite_benchmark_amd.sac import SACTrainer
    v = small_variant()
    plain = driver.experiment(copy.deepcopy(v), seed=17, num_epochs=2, quiet=True)
    assert driver.experiment(copy.deepcopy(v), seed=17, num_epochs=2, quiet=True, q_diagnostics=False)[0].keys() == plain[0].keys()
    seen, q_values, q_info = [], SACTrainer.q_values, driver.q_bias_information

    def recording_q_values(self, obs, act, nets=("qf1", "qf2")):
        got = q_values(self, obs, act, nets=nets)
        check_against_oracle(self, q_params(self), got, list(nets), obs, act, "experiment")
        seen.append(dict(trainer=self, obs=obs.copy(), act=act.copy(), nets=tuple(nets), q=got.copy()))
        return got

    def recording_q_info(paths, q1, q2, discount, reward_scale):
        seen[-1].update(paths=copy.deepcopy(paths), q1=np.array(q1), q2=np.array(q2), discount=discount,
                        reward_scale=reward_scale)
        return q_info(paths, q1, q2, discount, reward_scale)

    monkeypatch.setattr(SACTrainer, "q_values", recording_q_values)
    monkeypatch.setattr(driver, "q_bias_information", recording_q_info)
    rows = driver.experiment(copy.deepcopy(v), seed=17, num_epochs=2, quiet=True, q_diagnostics=True)
    assert len(rows) == len(plain) == len(seen) == 2
    header = list(plain[0].keys())
    at = header.index("time/data storing (s)")
    assert all(k.startswith("evaluation/") for k in header[at - 3:at]) and all(k.startswith("time/") or k == "Epoch" for k in header[at:])
    for row, want, s in zip(rows, plain, seen):
        assert list(row.keys()) == header[:at] + Q_COLUMNS + header[at:]
        for k in want:
            if not k.startswith("time/"):
                assert row[k] == want[k], k
        # the epoch's own evaluation paths, every step of them, through trainer.q_values on qf1 and qf2
        assert s["nets"] == ("qf1", "qf2") and len(s["paths"]) == int(row["evaluation/Num Paths"])
        assert np.array_equal(s["obs"], np.concatenate([p["observations"] for p in s["paths"]]).astype(np.float32))
        assert np.array_equal(s["act"], np.concatenate([p["actions"] for p in s["paths"]]).astype(np.float32))
        assert np.array_equal(s["q"][0], s["q1"]) and np.array_equal(s["q"][1], s["q2"])
        assert s["discount"] == s["trainer"].discount == v["trainer_kwargs"].get("discount", 0.99)
        assert s["reward_scale"] == s["trainer"].reward_scale
        info = q_info(s["paths"], s["q"][0], s["q"][1], s["trainer"].discount, s["trainer"].reward_scale)
        assert list(info.keys()) == Q_COLUMNS and all(row[k] == info[k] for k in Q_COLUMNS)
        assert row["evaluation/Q1 Estimates Mean"] == float(np.mean(s["q"][0].astype(np.float64)))
    assert rows[0]["evaluation/Q1 Estimates Mean"] != rows[1]["evaluation/Q1 Estimates Mean"]     # the critics moved


def test_experiment_group_q_diagnostics_equals_solo():
    from robosuite_benchmark_amd.driver import experiment, experiment_group
    v = small_variant()
    got = experiment_group(copy.deepcopy(v), seeds=[17, 18, 19], num_epochs=2, quiet=True, q_diagnostics=True)
    for s in (17, 18, 19):
        want = experiment(copy.deepcopy(v), seed=s, num_epochs=2, quiet=True, q_diagnostics=True)
        assert len(got[s]) == len(want) == 2
        for rg, rw in zip(got[s], want):
            assert list(rg.keys()) == list(rw.keys()) and all(k in rg for k in Q_COLUMNS), s
            for k in rw:
                if not k.startswith("time/"):
                    assert rg[k] == rw[k], (s, k)
    lock = experiment_group(copy.deepcopy(v), seeds=[17, 18], num_epochs=2, quiet=True, q_diagnostics=True, acting="device")
    want = experiment(copy.deepcopy(v), seed=18, num_epochs=2, quiet=True, q_diagnostics=True, acting="device")
    for rg, rw in zip(lock[18], want):
        assert all(rg[k] == rw[k] for k in rw if not k.startswith("time/"))
