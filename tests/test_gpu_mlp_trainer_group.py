"""GPU: MLP trainer groups (sac_group_create_mlp / td3_group_create_mlp, MlpSACTrainerGroup / MlpTD3TrainerGroup) --
runs of the general step (hidden sizes other than two layers of at most 256 units) trained with grouped launches.
Every member must equal, bit for bit, a solo twin (same initial weights and config, a buffer with the same rows and
seed) that ran train_loop for the same steps on its own batch size."""
import ctypes as C
import os

import numpy as np
import pytest

from robosuite_benchmark_amd import EnvReplayBuffer, MlpSACTrainerGroup, MlpTD3TrainerGroup, _lib
from tests.helpers import make_pair, make_td3_pair, synth_transitions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAC_NETS = ("policy", "qf1", "qf2", "target_qf1", "target_qf2")
TD3_NETS = SAC_NETS + ("target_policy",)


def sac_trainer(O, A, B, seed, hidden, **kw):
    return make_pair(O, A, B, seed=seed, noise_seed=1000 + seed, hidden=hidden, **kw)[1]


def td3_trainer(O, A, B, seed, hidden, **kw):
    return make_td3_pair(O, A, B, seed=seed, noise_seed=1000 + seed, hidden=hidden, **kw)[1]


def buffer(n, O, A, data_seed, rng_seed=None):
    obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=data_seed, term_frac=0.1)
    buf = EnvReplayBuffer(n, obs_dim=O, action_dim=A)
    buf.add_block(obs, act, rew, nobs, term)
    if rng_seed is not None:
        buf.seed(rng_seed)
    return buf


def opt_state(t, name, ids):
    n = t._get_params(name).size
    m, v = np.empty(n, np.float32), np.empty(n, np.float32)
    _lib.check(t._lib.sac_get_opt_state(t._h, ids[name], _lib.ptr(m), _lib.ptr(v), n), "sac_get_opt_state")
    return m, v


def scalars(t):
    sc = np.zeros(6, np.float64)
    _lib.check(t._lib.sac_get_scalars(t._h, _lib.ptr(sc)), "sac_get_scalars")
    return sc


def assert_twins(t, twin, buf, buf_twin, nets, ids, where=""):
    for name in nets:
        assert np.array_equal(t._get_params(name), twin._get_params(name)), (where, name)
    for name in ("policy", "qf1", "qf2"):
        for a, b in zip(opt_state(t, name, ids), opt_state(twin, name, ids)):
            assert np.array_equal(a, b), (where, "adam", name)
    assert np.array_equal(scalars(t), scalars(twin)), (where, scalars(t), scalars(twin))
    (k1, p1), (k2, p2) = buf.rng_state(), buf_twin.rng_state()
    assert p1 == p2 and np.array_equal(k1, k2), (where, "generator")


def run_and_compare(group, members, twins, bufs, tbufs, batches, steps, nets, ids):
    first, last = group.train_loop(bufs, steps, batch_sizes=batches)
    for r, (tw, tb, B) in enumerate(zip(twins, tbufs, batches)):
        f, l = tw.train_loop(tb, steps, batch_size=B)
        assert np.array_equal(first[r], f), (r, steps, "diag_first")
        assert np.array_equal(last[r], l), (r, steps, "diag_last")
    for r in range(len(members)):
        assert_twins(members[r], twins[r], bufs[r], tbufs[r], nets, ids, where=(r, steps))


def sac_set(shapes, hidden, seed0=3):
    """shapes: (obs_dim, act_dim, batch) per member; every member with other hyperparameters"""
    members, twins, bufs, tbufs = [], [], [], []
    for i, (O, A, B) in enumerate(shapes):
        kw = dict(reward_scale=1.0 + i, policy_lr=1e-3 / (1 + i), target_update_period=1 + i % 3)
        members.append(sac_trainer(O, A, B, seed0 + i, hidden, **kw))
        twins.append(sac_trainer(O, A, B, seed0 + i, hidden, **kw))
        bufs.append(buffer(3000 + 777 * i, O, A, 50 + i, 70 + i))
        tbufs.append(buffer(3000 + 777 * i, O, A, 50 + i, 70 + i))
    return members, twins, bufs, tbufs


@pytest.mark.parametrize("hidden,shapes,steps", [
    ((512, 512), [(42, 7, 256)] * 3, (600, 7)),                 # three seeds of Lift; 600 steps cross the chunk boundary
    ((256, 256, 256), [(42, 7, 128)] * 2, (300, 5)),
    ((1024, 1024), [(42, 7, 128)] * 2, (40, 3)),
])
def test_mlp_sac_group_equals_solo_runs_bitwise(hidden, shapes, steps):
    members, twins, bufs, tbufs = sac_set(shapes, hidden)
    batches = [B for _, _, B in shapes]
    group = MlpSACTrainerGroup(members)
    for n in steps:
        run_and_compare(group, members, twins, bufs, tbufs, batches, n, SAC_NETS, _lib.NET_IDS)
    # a member is still an ordinary trainer: a solo train_loop on it and its twin
    members[0].train_loop(bufs[0], 9, batch_size=batches[0])
    twins[0].train_loop(tbufs[0], 9, batch_size=batches[0])
    assert_twins(members[0], twins[0], bufs[0], tbufs[0], SAC_NETS, _lib.NET_IDS, where="solo after group")


def test_mlp_sac_group_of_mixed_dims_and_both_action_classes():
    # Lift, Wipe, TwoArmLift, and one action / sixteen actions: both template classes of the elementwise kernels
    shapes = [(42, 7, 256), (379, 6, 64), (89, 14, 100), (30, 1, 96), (50, 16, 128)]
    members, twins, bufs, tbufs = sac_set(shapes, (512, 512), seed0=11)
    batches = [B for _, _, B in shapes]
    group = MlpSACTrainerGroup(members)
    for n in (600, 4):
        run_and_compare(group, members, twins, bufs, tbufs, batches, n, SAC_NETS, _lib.NET_IDS)


def test_mlp_td3_group_keeps_each_members_update_plan():
    shapes = [(42, 7, 256, 1), (42, 7, 256, 2), (379, 6, 64, 3), (30, 12, 128, 2)]
    members, twins, bufs, tbufs = [], [], [], []
    for i, (O, A, B, period) in enumerate(shapes):
        kw = dict(policy_and_target_update_period=period, reward_scale=1.0 + 0.5 * i)
        members.append(td3_trainer(O, A, B, 20 + i, (512, 512), **kw))
        twins.append(td3_trainer(O, A, B, 20 + i, (512, 512), **kw))
        bufs.append(buffer(2500 + 501 * i, O, A, 30 + i, 40 + i))
        tbufs.append(buffer(2500 + 501 * i, O, A, 30 + i, 40 + i))
    batches = [B for _, _, B, _ in shapes]
    group = MlpTD3TrainerGroup(members)
    for n in (600, 7):
        run_and_compare(group, members, twins, bufs, tbufs, batches, n, TD3_NETS, _lib.TD3_NET_IDS)


def test_one_member_group():
    members, twins, bufs, tbufs = sac_set([(42, 7, 256)], (512, 512), seed0=5)
    group = MlpSACTrainerGroup(members)
    run_and_compare(group, members, twins, bufs, tbufs, [256], 20, SAC_NETS, _lib.NET_IDS)


def test_buffers_on_the_numpy_stream_continue_it_with_each_members_batch():
    shapes = [(42, 7, 256), (379, 6, 64), (46, 8, 100)]

    def bound_set():
        members, bufs = [], []
        for i, (O, A, B) in enumerate(shapes):
            members.append(sac_trainer(O, A, B, 81 + i, (512, 512)))
            bufs.append(buffer(1500 + 400 * i, O, A, 90 + i))          # bound to np.random (the default)
        return members, bufs

    members, bufs = bound_set()
    twins, tbufs = bound_set()
    batches = [B for _, _, B in shapes]
    group = MlpSACTrainerGroup(members)
    for steps in (30, 300):
        np.random.seed(1234 + steps)
        first, last = group.train_loop(bufs, steps, batch_sizes=batches)
        after_group = np.random.get_state()
        np.random.seed(1234 + steps)
        for r, (tw, tb, B) in enumerate(zip(twins, tbufs, batches)):
            f, l = tw.train_loop(tb, steps, batch_size=B)
            assert np.array_equal(first[r], f) and np.array_equal(last[r], l), (steps, r)
        after_solo = np.random.get_state()
        assert np.array_equal(after_group[1], after_solo[1]) and after_group[2] == after_solo[2], steps
        for r in range(len(shapes)):
            for name in SAC_NETS:
                assert np.array_equal(members[r]._get_params(name), twins[r]._get_params(name)), (steps, r, name)
            assert np.array_equal(scalars(members[r]), scalars(twins[r])), (steps, r)


def c_group(trainers, td3=False):
    lib = _lib.load()
    arr = (C.c_void_p * len(trainers))(*[t._h.value for t in trainers])
    g = C.c_void_p()
    if getattr(lib, "td3_group_create_mlp" if td3 else "sac_group_create_mlp")(C.byref(g), arr, len(trainers)) < 0:
        raise RuntimeError(_lib.last_error())
    return g


def test_mlp_refusals_leave_members_unchanged():
    (O1, A1, B1), (O2, A2, B2) = (42, 7, 128), (86, 14, 64)
    a, b = sac_trainer(O1, A1, B1, 61, (512, 512)), sac_trainer(O2, A2, B2, 62, (512, 512))
    before = {id(t): [t._get_params(n) for n in SAC_NETS] for t in (a, b)}
    fused = sac_trainer(O1, A1, B1, 60, (256, 256))
    with pytest.raises(RuntimeError, match="shapes of the fused kernels"):
        c_group([a, fused])
    td3 = td3_trainer(O1, A1, B1, 60, (512, 512))
    with pytest.raises(RuntimeError, match="TD3 trainer"):
        c_group([a, td3])
    with pytest.raises(RuntimeError, match="SAC trainer"):
        c_group([td3, a], td3=True)
    other = sac_trainer(O1, A1, B1, 63, (512, 256))
    with pytest.raises(RuntimeError, match="other hidden sizes"):
        c_group([a, other])
    with pytest.raises(RuntimeError, match="same trainer"):
        c_group([a, b, a])
    with pytest.raises(RuntimeError, match="1..16"):
        c_group([a] * 17)
    conf = sac_trainer(O2, A2, B2, 64, (512, 512))
    _lib.check(conf._lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    with pytest.raises(RuntimeError, match="confined"):
        c_group([a, conf])
    # the existing kinds keep refusing general-step members
    lib = _lib.load()
    for name in ("sac_group_create", "sac_group_create_mixed"):
        arr = (C.c_void_p * 1)(a._h.value)
        g = C.c_void_p()
        assert getattr(lib, name)(C.byref(g), arr, 1) < 0 and "general step" in _lib.last_error()
    b1, b2 = buffer(800, O1, A1, 1, 1), buffer(800, O2, A2, 2, 2)
    g = c_group([a, b])
    try:
        for bs, what in (([b1, b1], "same buffer"), ([b2, b1], "has dims"),
                         ([b1, EnvReplayBuffer(100, obs_dim=O2, action_dim=A2)], "empty")):
            arr = (C.c_void_p * 2)(*[x._h.value for x in bs])
            assert lib.sac_group_train_loop(g, arr, 5, None, None) < 0
            assert what in _lib.last_error(), (what, _lib.last_error())
    finally:
        lib.sac_group_destroy(g)
    for t in (a, b):
        for n, p in zip(SAC_NETS, before[id(t)]):
            assert np.array_equal(t._get_params(n), p), n
        assert scalars(t)[4] == 0
    MlpSACTrainerGroup([a, b]).train_loop([b1, b2], 5)
    assert scalars(a)[4] == 5 and scalars(b)[4] == 5


def _small_variant(name, hidden, batch=None):
    from robosuite_benchmark_amd import variant
    v = variant.load_variant(os.path.join(ROOT, "tests", "golden", name + ".variant.json"))
    v["algorithm_kwargs"].update(min_num_steps_before_training=600, num_eval_steps_per_epoch=300,
                                 num_expl_steps_per_train_loop=400, num_trains_per_train_loop=150,
                                 eval_max_path_length=100, expl_max_path_length=100)
    if batch:
        v["algorithm_kwargs"]["batch_size"] = batch
    v["replay_buffer_size"] = 5000
    v["policy_kwargs"]["hidden_sizes"] = list(hidden)
    v["qf_kwargs"]["hidden_sizes"] = list(hidden)
    return v


def _assert_rows(got, want, where):
    assert len(got) == len(want), where
    for rg, rw in zip(got, want):
        assert list(rg.keys()) == list(rw.keys())
        for k in rw:
            if not k.startswith("time/"):
                assert rg[k] == rw[k], (where, k)


def test_experiment_group_on_a_general_variant_equals_solo_experiments():
    from robosuite_benchmark_amd.driver import experiment, experiment_group
    v = _small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512))
    got = experiment_group(v, [17, 18], num_epochs=2, quiet=True)
    for s in (17, 18):
        _assert_rows(got[s], experiment(v, seed=s, num_epochs=2, quiet=True), s)


def test_experiment_sweep_on_a_general_variant_equals_solo_experiments():
    from robosuite_benchmark_amd.driver import experiment, experiment_sweep
    vs = [_small_variant("Lift-Panda-OSC-POSE-SEED17", (256, 256, 256)),
          _small_variant("TwoArmLift-PandaPanda-OSC-POSE-SEED17", (256, 256, 256), batch=100)]
    runs = [(v, 17) for v in vs]
    got = experiment_sweep(runs, num_epochs=2, quiet=True)
    for (v, s), rows in zip(runs, got):
        _assert_rows(rows, experiment(v, seed=s, num_epochs=2, quiet=True), v["expl_environment_kwargs"]["env_name"])


def test_experiment_group_checkpoint_resume_equals_straight_run(tmp_path):
    from robosuite_benchmark_amd.driver import experiment_group
    v = _small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512))
    straight = experiment_group(v, [17, 18], num_epochs=4, quiet=True)
    ck = str(tmp_path / "ck")
    experiment_group(v, [17, 18], num_epochs=2, quiet=True, checkpoint_dir=ck)
    resumed = experiment_group(v, [17, 18], num_epochs=4, quiet=True, checkpoint_dir=ck, resume=True)
    for s in (17, 18):
        _assert_rows(resumed[s], straight[s][2:], s)
