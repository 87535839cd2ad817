"""GPU: acting on the device -- sac_policy_act_device / sac_policy_act_many (k_act, csrc/sac_act.h), the Python entry
points over them (SACTrainer.policy_act_device, group.act_many, policy.acting = "device") and the lockstep collection
of the group drivers (acting="device").

Reference: oracle.sac_step_torch.PolicyNet.  Bounds: atol 2e-5 on actions against the fp32 PolicyNet (what
test_gpu_trained_weights.py holds sac_policy_act to), and against the float64 PolicyNet an error of at most
max(2e-5, 8 x the fp32 oracle's own error) (the rule of helpers.check_step_f64).  Row independence and grouped == solo
are bit for bit."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from robosuite_benchmark_amd import MixedSACTrainerGroup, SACTrainerGroup, _lib
from robosuite_benchmark_amd.group import act_many
from tests.helpers import (act_c, act_reference, draws, filled_buffer, full_state, is_td3, layers_from_flat, make_pair,
                           make_pair_from_flat, make_td3_pair)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 5, 16, 17, 64, 1000)


def trained_flats():
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_weights_lift_seed129.npz"))
    return {k: z[k] for k in z.files}


def policy_layers(t):
    """The policy the device holds NOW, as the oracle's layer list."""
    hs, O, A = t._hidden("policy"), t.obs_dim, t.act_dim
    shapes = [(hs[0], O), (hs[1], hs[0]), (A, hs[1])] + ([] if is_td3(t) else [(A, hs[1])])
    return layers_from_flat(t.state_dict()["params"]["policy"], shapes)


def reference(t, obs, deterministic, eps, dtype):
    return act_reference(policy_layers(t), is_td3(t), obs, deterministic, eps, dtype)


def check_against_oracle(t, got, obs, deterministic, eps, where):
    w32, w64 = reference(t, obs, deterministic, eps, torch.float32), reference(t, obs, deterministic, eps, torch.float64)
    e_k32, e_k64 = float(np.max(np.abs(got - w32))), float(np.max(np.abs(got.astype(np.float64) - w64)))
    e_32 = float(np.max(np.abs(w32.astype(np.float64) - w64)))
    print(f"{where}: |device - fp32 oracle| {e_k32:.3g}  |device - f64| {e_k64:.3g}  |fp32 oracle - f64| {e_32:.3g}")
    assert np.allclose(got, w32, atol=2e-5), (where, e_k32)
    assert e_k64 <= max(2e-5, 8.0 * e_32), (where, e_k64, e_32)


def sweep_rows(t, seed, where):
    rs = np.random.RandomState(seed)
    for n in ROWS:
        obs, eps = draws(rs, n, t.obs_dim, t.act_dim)
        check_against_oracle(t, act_c(t, obs, True, None), obs, True, None, (where, n, "deterministic"))
        check_against_oracle(t, act_c(t, obs, False, None if is_td3(t) else eps), obs, False, eps, (where, n, "stochastic"))


# ---- 1. parity with the oracle ----------------------------------------------------------------------------------------
def test_parity_on_trained_weights():
    _, hip = make_pair_from_flat(trained_flats(), 42, 7, 64)
    sweep_rows(hip, 1, "trained Lift")


@pytest.mark.parametrize("O,A,hidden", [(42, 7, (256, 256)), (46, 7, (256, 256)), (89, 14, (256, 256)),
                                        (379, 6, (256, 256)), (496, 7, (256, 256)), (42, 7, (128, 64))])
def test_parity_on_fresh_weights(O, A, hidden):
    _, hip = make_pair(O, A, 32, seed=5, hidden=hidden)
    sweep_rows(hip, O + A, (O, A, hidden))


def test_parity_td3():
    _, hip = make_td3_pair(42, 7, 32, seed=4)
    sweep_rows(hip, 3, "td3")
    obs, _ = draws(np.random.RandomState(8), 20, 42, 7)
    assert np.array_equal(hip.policy_act_device(obs, False, None), hip.policy_act_device(obs, True, None))


# ---- 2. row independence ----------------------------------------------------------------------------------------------
def test_rows_are_independent_bitwise():
    _, hip = make_pair_from_flat(trained_flats(), 42, 7, 64)
    rs = np.random.RandomState(2)
    for n in (15, 16, 17, 33, 1000):
        obs, eps = draws(rs, n, 42, 7)
        for det in (True, False):
            full = act_c(hip, obs, det, None if det else eps)
            for r in sorted({0, 1, n // 2, 15 % n, 16 % n, n - 1}):
                one = act_c(hip, obs[r:r + 1].copy(), det, None if det else eps[r:r + 1].copy())
                assert np.array_equal(one[0], full[r]), (n, r, det)
    # ... and on neither n nor the row's place: the same observation in every row gives the same action in every row
    obs1, eps1 = draws(rs, 1, 42, 7)
    rep = act_c(hip, np.repeat(obs1, 37, 0), False, np.repeat(eps1, 37, 0))
    assert np.all(rep == rep[0])


# ---- 3. grouped == solo -----------------------------------------------------------------------------------------------
def mixed_members(R):
    dims = [(42, 7), (46, 7), (89, 14), (379, 6), (64, 4), (73, 12), (50, 4)]
    rows = [1, 17, 0, 64, 5, 16, 0, 300, 1, 33, 2, 0, 1000, 7, 48, 1]
    members = []
    for i in range(R):
        O, A = dims[i % len(dims)]
        if i % 3 == 2:
            t = make_td3_pair(O, A, 32, seed=20 + i)[1]
        else:
            t = make_pair(O, A, 32, seed=20 + i, hidden=(128, 64) if i % 5 == 4 else (256, 256))[1]
        members.append((t, rows[i] if R > 2 else (5, 17)[i], i % 2 == 0))
    return members


@pytest.mark.parametrize("R", [2, 7, 16])
def test_grouped_equals_solo_bitwise(R):
    members = mixed_members(R)
    assert R == 2 or (any(is_td3(t) for t, _, _ in members) and any(n == 0 for _, n, _ in members))
    rs = np.random.RandomState(R)
    obs, eps, outs = [], [], []
    for t, n, det in members:
        o, e = draws(rs, n, t.obs_dim, t.act_dim)
        obs.append(o); eps.append(None if (det or is_td3(t)) else e)
        outs.append(np.full((n if n else 3, t.act_dim), -5.0, np.float32))          # (sentinel)
    vp = lambda arrs: (C.c_void_p * R)(*[None if a is None else a.ctypes.data for a in arrs])  # noqa: E731
    rc = _lib.load().sac_policy_act_many((C.c_void_p * R)(*[t._h.value for t, _, _ in members]), R,
                                         (C.c_int32 * R)(*[n for _, n, _ in members]), vp(obs),
                                         (C.c_int32 * R)(*[int(det) for _, _, det in members]), vp(eps), vp(outs))
    _lib.check(rc, "sac_policy_act_many")
    for i, (t, n, det) in enumerate(members):
        if n == 0:
            assert np.all(outs[i] == -5.0), i                       # a member that sits out: untouched
        else:
            assert np.array_equal(outs[i], act_c(t, obs[i], det, eps[i])), i
            check_against_oracle(t, outs[i], obs[i], det, eps[i], ("grouped", R, i))
    # the Python form: the same actions, empty arrays for the members that sit out
    got = act_many([t for t, _, _ in members], [o if o.shape[0] else None for o in obs], [d for _, _, d in members], eps)
    for i, (t, n, _) in enumerate(members):
        assert got[i].shape == (n, t.act_dim) and (n == 0 or np.array_equal(got[i], outs[i])), i


# ---- 4. live weights --------------------------------------------------------------------------------------------------
def test_acting_follows_the_live_weights():
    O, A, B = 42, 7, 64
    rs = np.random.RandomState(6)
    obs, eps = draws(rs, 40, O, A)

    def moved(ts, before, where):
        for t, b in zip(ts, before):
            now = act_c(t, obs, False, eps)
            check_against_oracle(t, now, obs, False, eps, where)
            check_against_oracle(t, act_c(t, obs, True, None), obs, True, None, where)
            assert not np.array_equal(now, b), where
        return [act_c(t, obs, False, eps) for t in ts]

    _, hip = make_pair(O, A, B, seed=9)
    buf = filled_buffer(2000, O, A, 3)
    last = [act_c(hip, obs, False, eps)]
    check_against_oracle(hip, last[0], obs, False, eps, "initial")
    hip.train_loop(buf, 30, batch_size=B)
    last = moved([hip], last, "train_loop")
    for _ in range(20):                                             # stepwise, on device batches, nothing synchronised
        hip.train(buf.random_batch(B))
    last = moved([hip], last, "device batches")
    from tests.helpers import flat_of
    from oracle.sac_step_torch import init_sac_params
    hip._set_params("policy", flat_of(init_sac_params(O, A, seed=77)["policy"]))
    moved([hip], last, "set_params")
    # trainer groups: uniform and mixed
    ts = [make_pair(O, A, B, seed=30 + i)[1] for i in range(3)]
    bufs = [filled_buffer(1500, O, A, 40 + i) for i in range(3)]
    last = [act_c(t, obs, False, eps) for t in ts]
    SACTrainerGroup(ts).train_loop(bufs, 25, batch_size=B)
    moved(ts, last, "SACTrainerGroup")
    a, b = make_pair(O, A, 48, seed=50)[1], make_pair(46, 7, 100, seed=51)[1]
    ba, bb = filled_buffer(900, O, A, 1), filled_buffer(900, 46, 7, 2)
    obs_b, eps_b = draws(rs, 9, 46, 7)
    before_a, before_b = act_c(a, obs, False, eps), act_c(b, obs_b, False, eps_b)
    MixedSACTrainerGroup([a, b]).train_loop([ba, bb], 25, batch_sizes=[48, 100])
    moved([a], [before_a], "MixedSACTrainerGroup")
    now_b = act_c(b, obs_b, False, eps_b)
    check_against_oracle(b, now_b, obs_b, False, eps_b, "MixedSACTrainerGroup b")
    assert not np.array_equal(now_b, before_b)


# ---- 5. acting disturbs nothing ---------------------------------------------------------------------------------------
def test_acting_disturbs_nothing():
    O, A, B = 42, 7, 64
    (_, a), (_, b) = make_pair(O, A, B, seed=12, noise_seed=5), make_pair(O, A, B, seed=12, noise_seed=5)
    ba, bb = filled_buffer(2000, O, A, 8), filled_buffer(2000, O, A, 8)
    rs = np.random.RandomState(4)
    for block in range(4):
        a.train_loop(ba, 20, batch_size=B); b.train_loop(bb, 20, batch_size=B)
        for _ in range(6):
            a.train(ba.random_batch(B)); b.train(bb.random_batch(B))
            obs, eps = draws(rs, 1 + 16 * block, O, A)               # a acts in the middle of its device-batch steps
            a.policy_act_device(obs, False, eps)
        obs, eps = draws(rs, 100, O, A)
        a.policy_act_device(obs, True, None)
        act_many([a], [obs], [False], [eps])
    for x, y in zip(full_state(a, ba), full_state(b, bb)):
        assert np.array_equal(x, y)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    lib = _lib.load()
    O, A = 42, 7
    (_, a), (_, b) = make_pair(O, A, 32, seed=1), make_pair(O, A, 32, seed=2)
    _, td3 = make_td3_pair(O, A, 32, seed=3)
    _, gen = make_pair(O, A, 32, seed=4, hidden=(512, 512))
    _, conf = make_pair(O, A, 32, seed=5)
    _lib.check(lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    obs, eps = draws(np.random.RandomState(1), 8, O, A)
    want = act_c(a, obs, False, eps)
    out = np.full((8, A), 3.0, np.float32)

    def many(ts, n_rows, obs_l, det, eps_l, out_l):
        R = len(ts)
        vp = lambda arrs: (C.c_void_p * R)(*[None if x is None else x.ctypes.data for x in arrs])  # noqa: E731
        return lib.sac_policy_act_many((C.c_void_p * R)(*[None if t is None else t._h.value for t in ts]), R,
                                       (C.c_int32 * R)(*n_rows), vp(obs_l), (C.c_int32 * R)(*det), vp(eps_l), vp(out_l))

    def refused(rc, what):
        assert rc < 0 and what in _lib.last_error(), (rc, what, _lib.last_error())
        assert np.all(out == 3.0), what
        ok = np.empty((8, A), np.float32)                            # a valid call still gives the right actions
        assert many([a], [8], [obs], [0], [eps], [ok]) == 0 and np.array_equal(ok, want), what

    out2 = np.full((8, A), 3.0, np.float32)
    refused(many([a, None], [8, 8], [obs, obs], [0, 0], [eps, eps], [out, out2]), "null")
    refused(many([a, a], [8, 8], [obs, obs], [0, 0], [eps, eps], [out, out2]), "again")
    refused(many([a, b], [8, 1025], [obs, obs], [0, 0], [eps, eps], [out, out2]), "rows")
    refused(many([a, b], [8, -1], [obs, obs], [0, 0], [eps, eps], [out, out2]), "rows")
    refused(many([a, b], [0, 0], [obs, obs], [0, 0], [eps, eps], [out, out2]), "no trainer has rows")
    refused(many([a, b], [8, 8], [obs, obs], [0, 0], [eps, None], [out, out2]), "eps")
    refused(many([a, gen], [8, 8], [obs, obs], [0, 0], [eps, eps], [out, out2]), "sac_policy_act is the acting path")
    refused(many([a, conf], [8, 8], [obs, obs], [0, 0], [eps, eps], [out, out2]), "confined")
    refused(lib.sac_policy_act_device(a._h, 0, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out)), "rows")
    refused(lib.sac_policy_act_device(a._h, 1025, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out)), "rows")
    refused(lib.sac_policy_act_device(a._h, 8, _lib.ptr(obs), 0, None, _lib.ptr(out)), "eps")
    refused(lib.sac_policy_act_device(gen._h, 8, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out)), "general step")
    refused(lib.sac_policy_act_device(None, 8, _lib.ptr(obs), 0, _lib.ptr(eps), _lib.ptr(out)), "bad arguments")
    assert np.all(out2 == 3.0)
    if _lib.device_count() > 1:                                      # (needs a second GPU to build the case)
        _, far = make_pair(O, A, 32, seed=6, device=1)
        refused(many([a, far], [8, 8], [obs, obs], [0, 0], [eps, eps], [out, out2]), "device")
    # TD3 needs no eps, and Python's policy_act_device raises for the general step instead of acting on the host
    assert many([td3], [8], [obs], [0], [None], [out2]) == 0 and not np.all(out2 == 3.0)
    with pytest.raises(RuntimeError, match="sac_policy_act is the acting path"):
        gen.policy_act_device(obs, True, None)
    # ... while act_many serves it through its host path, next to a device member
    got = act_many([a, gen], [obs, obs], [False, True], [eps, None])
    assert np.array_equal(got[0], want) and np.array_equal(got[1], gen.policy_act(obs, True, None))


def test_policy_acting_attribute_routes_get_actions():
    _, hip = make_pair_from_flat(trained_flats(), 42, 7, 64)
    obs, eps = draws(np.random.RandomState(3), 12, 42, 7)
    assert hip.policy.acting == "host"
    hip.policy._noise = np.random.RandomState(9)
    host = hip.policy.get_actions(obs)
    hip.policy.acting = "device"
    hip.policy._noise = np.random.RandomState(9)
    dev = hip.policy.get_actions(obs)
    e9 = np.random.RandomState(9).standard_normal((12, 7)).astype(np.float32)
    assert np.array_equal(dev, act_c(hip, obs, False, e9))                       # the same draws of the same stream
    assert np.array_equal(host, hip.policy_act(obs, False, e9)) and np.allclose(host, dev, atol=4e-5)
    a, info = hip.policy.get_action(obs[0], deterministic=True)
    assert info == {} and np.array_equal(a, act_c(hip, obs[:1].copy(), True, None)[0])
    hip.policy.acting = "gpu"
    with pytest.raises(ValueError, match="acting"):
        hip.policy.get_actions(obs)


# ---- 7. drivers -------------------------------------------------------------------------------------------------------
def small_variant(name, hidden=None, batch=None, td3=False):
    from robosuite_benchmark_amd import variant
    v = variant.load_variant(os.path.join(ROOT, "tests", "golden", name + ".variant.json"))
    v["algorithm_kwargs"].update(min_num_steps_before_training=150, num_eval_steps_per_epoch=130,
                                 num_expl_steps_per_train_loop=170, num_trains_per_train_loop=40,
                                 eval_max_path_length=50, expl_max_path_length=60)
    v["replay_buffer_size"] = 3000
    if batch:
        v["algorithm_kwargs"]["batch_size"] = batch
    if hidden:
        v["policy_kwargs"]["hidden_sizes"] = list(hidden)
        v["qf_kwargs"]["hidden_sizes"] = list(hidden)
    return v


def assert_rows(got, want, where):
    assert len(got) == len(want) == 2, where
    for rg, rw in zip(got, want):
        assert list(rg.keys()) == list(rw.keys()), where
        for k in rw:
            if not k.startswith("time/"):
                assert rg[k] == rw[k], (where, k)


def test_experiment_group_on_the_device_equals_solo_experiments():
    from robosuite_benchmark_amd.driver import experiment, experiment_group
    v = small_variant("Lift-Panda-OSC-POSE-SEED17")
    got = experiment_group(copy.deepcopy(v), seeds=[17, 18, 19], num_epochs=2, quiet=True, acting="device")
    for s in (17, 18, 19):
        assert_rows(got[s], experiment(copy.deepcopy(v), seed=s, num_epochs=2, quiet=True, acting="device"), s)
    # "host" is the default
    host = experiment(copy.deepcopy(v), seed=17, num_epochs=2, quiet=True, acting="host")
    assert_rows(host, experiment(copy.deepcopy(v), seed=17, num_epochs=2, quiet=True), "host")
    assert any(host[1][k] != got[17][1][k] for k in host[1] if k.startswith("evaluation/Actions"))
    ghost = experiment_group(copy.deepcopy(v), seeds=[17, 18], num_epochs=2, quiet=True, acting="host")
    gdef = experiment_group(copy.deepcopy(v), seeds=[17, 18], num_epochs=2, quiet=True)
    for s in (17, 18):
        assert_rows(ghost[s], gdef[s], ("group host", s))
    assert_rows(ghost[17], host, "group host == solo host")
    with pytest.raises(ValueError, match="acting"):
        experiment_group(copy.deepcopy(v), seeds=[17], num_epochs=1, quiet=True, acting="gpu")


def test_experiment_sweep_on_the_device_equals_solo_experiments():
    from robosuite_benchmark_amd.driver import experiment, experiment_sweep
    vs = [small_variant("Lift-Panda-OSC-POSE-SEED17"), small_variant("TwoArmLift-PandaPanda-OSC-POSE-SEED17", batch=100)]
    runs = [(v, s) for v in vs for s in (17, 18)]
    got = experiment_sweep(copy.deepcopy(runs), num_epochs=2, quiet=True, acting="device")
    for (v, s), rows in zip(runs, got):
        assert_rows(rows, experiment(copy.deepcopy(v), seed=s, num_epochs=2, quiet=True, acting="device"),
                    (v["expl_environment_kwargs"]["env_name"], s))


def test_hidden_sweep_on_the_device_with_a_general_step_member():
    from robosuite_benchmark_amd.driver import experiment, experiment_sweep
    vs = [small_variant("Lift-Panda-OSC-POSE-SEED17", (256, 256), batch=100),
          small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512), batch=100),          # the general step: acts on the host
          small_variant("TwoArmLift-PandaPanda-OSC-POSE-SEED17", (128, 64), batch=100)]
    runs = [(v, 17) for v in vs]
    got = experiment_sweep(copy.deepcopy(runs), num_epochs=2, quiet=True, hidden_sweep=True, acting="device")
    for (v, s), rows in zip(runs, got):
        assert_rows(rows, experiment(copy.deepcopy(v), seed=s, num_epochs=2, quiet=True, acting="device"),
                    v["policy_kwargs"]["hidden_sizes"])


def test_td3_group_on_the_device_equals_solo_experiments():
    from robosuite_benchmark_amd.driver import experiment, experiment_group
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=17, batch_size=64, agent="TD3")
    v["algorithm_kwargs"].update(min_num_steps_before_training=150, num_eval_steps_per_epoch=130,
                                 num_expl_steps_per_train_loop=170, num_trains_per_train_loop=40,
                                 eval_max_path_length=50, expl_max_path_length=60)
    v["replay_buffer_size"] = 3000
    got = experiment_group(copy.deepcopy(v), seeds=[5, 6], num_epochs=2, quiet=True, acting="device")
    for s in (5, 6):
        assert_rows(got[s], experiment(copy.deepcopy(v), seed=s, num_epochs=2, quiet=True, acting="device"), ("td3", s))
