"""GPU: mixed trainer groups (sac_group_create_mixed / td3_group_create_mixed, MixedSACTrainerGroup /
MixedTD3TrainerGroup) -- runs of different tasks (obs_dim, act_dim and batch per member) trained with grouped launches.
Every member must equal, bit for bit, a solo twin (same initial weights and config, a buffer with the same rows and
seed) that ran train_loop for the same steps on its own batch size."""
import ctypes as C
import os

import numpy as np
import pytest

from robosuite_benchmark_amd import EnvReplayBuffer, MixedSACTrainerGroup, MixedTD3TrainerGroup, _lib
from tests.helpers import make_pair, make_td3_pair, synth_transitions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAC_NETS = ("policy", "qf1", "qf2", "target_qf1", "target_qf2")
TD3_NETS = SAC_NETS + ("target_policy",)

# (obs_dim, act_dim, batch): the three SAC variant classes of the task sweep (<1 head tile, narrow>, <2, narrow>,
# <1, wide>), unequal batches and a batch that is not a multiple of 16
SAC_MEMBERS = [(42, 7, 256), (46, 8, 128), (86, 14, 256), (379, 6, 64), (55, 7, 100)]
# (obs_dim, act_dim, batch, policy_and_target_update_period)
TD3_MEMBERS = [(42, 7, 256, 2), (379, 6, 64, 3), (73, 12, 128, 1)]


def sac_trainer(O, A, B, seed, **kw):
    return make_pair(O, A, B, seed=seed, noise_seed=1000 + seed, **kw)[1]


def td3_trainer(O, A, B, seed, **kw):
    return make_td3_pair(O, A, B, seed=seed, noise_seed=1000 + seed, **kw)[1]


def buffer(n, O, A, data_seed, rng_seed=None, term_frac=0.1):
    obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=data_seed, term_frac=term_frac)
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


def group_and_twins_step(group, members, twins, bufs, tbufs, batches, steps, nets, ids):
    first, last = group.train_loop(bufs, steps, batch_sizes=batches)
    for r, (tw, tb, B) in enumerate(zip(twins, tbufs, batches)):
        f, l = tw.train_loop(tb, steps, batch_size=B)
        assert np.array_equal(first[r], f), (r, steps, "diag_first")
        assert np.array_equal(last[r], l), (r, steps, "diag_last")
    for r in range(len(members)):
        assert_twins(members[r], twins[r], bufs[r], tbufs[r], nets, ids, where=(r, steps))


def sac_set(shapes, seed0=3, rows0=3000):
    members, twins, bufs, tbufs = [], [], [], []
    for i, (O, A, B) in enumerate(shapes):
        kw = dict(reward_scale=1.0 + i, policy_lr=1e-3 / (1 + i))
        members.append(sac_trainer(O, A, B, seed0 + i, **kw))
        twins.append(sac_trainer(O, A, B, seed0 + i, **kw))
        bufs.append(buffer(rows0 + 777 * i, O, A, 50 + i, 70 + i))
        tbufs.append(buffer(rows0 + 777 * i, O, A, 50 + i, 70 + i))
    return members, twins, bufs, tbufs


def test_mixed_sac_group_equals_solo_runs_bitwise():
    members, twins, bufs, tbufs = sac_set(SAC_MEMBERS)
    batches = [B for _, _, B in SAC_MEMBERS]
    group = MixedSACTrainerGroup(members)
    # 600 steps: two whole LOOP_CH = 256 chunks and a partial one; then a short call
    for steps in (600, 7):
        group_and_twins_step(group, members, twins, bufs, tbufs, batches, steps, SAC_NETS, _lib.NET_IDS)
    # a member is still an ordinary trainer: a solo stepwise train on it and its twin
    O, A, B = SAC_MEMBERS[3]
    batch = bufs[3].random_batch(B)
    tbatch = tbufs[3].random_batch(B)
    members[3].train(batch)
    twins[3].train(tbatch)
    assert_twins(members[3], twins[3], bufs[3], tbufs[3], SAC_NETS, _lib.NET_IDS, where="stepwise")


def test_mixed_td3_group_equals_solo_runs_bitwise():
    members, twins, bufs, tbufs = [], [], [], []
    for i, (O, A, B, period) in enumerate(TD3_MEMBERS):
        kw = dict(policy_and_target_update_period=period, reward_scale=1.0 + 0.5 * i)
        members.append(td3_trainer(O, A, B, 20 + i, **kw))
        twins.append(td3_trainer(O, A, B, 20 + i, **kw))
        bufs.append(buffer(2500 + 501 * i, O, A, 30 + i, 40 + i))
        tbufs.append(buffer(2500 + 501 * i, O, A, 30 + i, 40 + i))
    batches = [B for _, _, B, _ in TD3_MEMBERS]
    group = MixedTD3TrainerGroup(members)
    for steps in (600, 7):
        group_and_twins_step(group, members, twins, bufs, tbufs, batches, steps, TD3_NETS, _lib.TD3_NET_IDS)


def test_buffers_on_the_numpy_stream_continue_it_with_each_members_batch():
    """Default buffers all sample np.random: the group continues it buffer after buffer, each by its own member's
    batch size, as solo train_loop calls in member order do -- results and np.random's state afterwards."""
    shapes = [(42, 7, 256), (379, 6, 64), (46, 8, 100), (86, 14, 128)]

    def bound_set():
        members, bufs = [], []
        for i, (O, A, B) in enumerate(shapes):
            members.append(sac_trainer(O, A, B, 81 + i))
            bufs.append(buffer(1500 + 400 * i, O, A, 90 + i))          # bound to np.random (the default)
        return members, bufs

    members, bufs = bound_set()
    twins, tbufs = bound_set()
    batches = [B for _, _, B in shapes]
    group = MixedSACTrainerGroup(members)
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


def test_member_order_does_not_change_results():
    order = [4, 2, 0, 3, 1]
    a, _, abufs, _ = sac_set(SAC_MEMBERS)
    b, _, bbufs, _ = sac_set(SAC_MEMBERS)
    batches = [B for _, _, B in SAC_MEMBERS]
    MixedSACTrainerGroup(a).train_loop(abufs, 300, batch_sizes=batches)
    fb, lb = MixedSACTrainerGroup([b[i] for i in order]).train_loop([bbufs[i] for i in order], 300,
                                                                    batch_sizes=[batches[i] for i in order])
    for i in range(len(SAC_MEMBERS)):
        assert_twins(a[i], b[i], abufs[i], bbufs[i], SAC_NETS, _lib.NET_IDS, where=("order", i))


def c_group(trainers):
    lib = _lib.load()
    arr = (C.c_void_p * len(trainers))(*[t._h.value for t in trainers])
    g = C.c_void_p()
    if lib.sac_group_create_mixed(C.byref(g), arr, len(trainers)) < 0:
        raise RuntimeError(_lib.last_error())
    return g


def test_mixed_refusals_leave_members_unchanged():
    from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy
    (O1, A1, B1), (O2, A2, B2) = (42, 7, 128), (86, 14, 64)
    a, b = sac_trainer(O1, A1, B1, 61), sac_trainer(O2, A2, B2, 62)
    before = {id(t): [t._get_params(n) for n in SAC_NETS] for t in (a, b)}
    td3 = td3_trainer(O1, A1, B1, 60)
    with pytest.raises(RuntimeError, match="SAC trainers only"):
        MixedSACTrainerGroup([a, td3])
    with pytest.raises(RuntimeError, match="TD3 trainer"):
        c_group([a, td3])
    pol = TanhGaussianPolicy([256, 256, 256], O1, A1)
    qs = [FlattenMlp([256, 256, 256], 1, O1 + A1) for _ in range(4)]
    gen = SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], batch_size=B1)
    with pytest.raises(RuntimeError, match="general step"):
        MixedSACTrainerGroup([gen]).train_loop([buffer(500, O1, A1, 1, 1)], 5)
    with pytest.raises(RuntimeError, match="general step"):
        c_group([gen])
    big = sac_trainer(O1, A1, 512, 63)
    with pytest.raises(RuntimeError, match="at most 256 rows"):
        MixedSACTrainerGroup([a, big]).train_loop([buffer(800, O1, A1, 1, 1), buffer(800, O1, A1, 2, 2)], 5)
    with pytest.raises(RuntimeError, match="at most 256 rows"):
        c_group([a, big])
    with pytest.raises(RuntimeError, match="at most 256 rows"):
        MixedSACTrainerGroup([a, b]).train_loop([buffer(800, O1, A1, 1, 1), buffer(800, O2, A2, 2, 2)], 5,
                                                batch_sizes=[B1, 512])
    conf = sac_trainer(O2, A2, B2, 64)
    _lib.check(conf._lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    with pytest.raises(RuntimeError, match="confined"):
        c_group([a, conf])
    with pytest.raises(RuntimeError, match="same trainer"):
        c_group([a, b, a])
    group = MixedSACTrainerGroup([a, b])
    b1, b2 = buffer(800, O1, A1, 1, 1), buffer(800, O2, A2, 2, 2)
    with pytest.raises(RuntimeError, match="same buffer"):
        group.train_loop([b1, b1], 5)
    with pytest.raises(RuntimeError, match="has dims"):
        group.train_loop([b1, buffer(800, O1, A1, 3, 3)], 5)              # member 0's dims in member 1's place
    with pytest.raises(RuntimeError, match="empty"):
        group.train_loop([b1, EnvReplayBuffer(100, obs_dim=O2, action_dim=A2)], 5)
    g = c_group([a, b])
    lib = _lib.load()
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
    assert (a._batch, b._batch) == (B1, B2)
    group.train_loop([b1, b2], 5)
    assert scalars(a)[4] == 5 and scalars(b)[4] == 5
    # confined after the group was made: refused at the call, nothing changed, and the group works once it is lifted
    after = {id(t): [t._get_params(n) for n in SAC_NETS] for t in (a, b)}
    _lib.check(b._lib.sac_trainer_set_xcd(b._h, 1), "sac_trainer_set_xcd")
    with pytest.raises(RuntimeError, match="confined"):
        group.train_loop([b1, b2], 5)
    for t in (a, b):
        for n, p in zip(SAC_NETS, after[id(t)]):
            assert np.array_equal(t._get_params(n), p), n
        assert scalars(t)[4] == 5


def test_experiment_sweep_rows_equal_solo_experiments(tmp_path):
    from robosuite_benchmark_amd import variant
    from robosuite_benchmark_amd.driver import experiment, experiment_sweep
    vs = []
    for name in ("Lift-Panda-OSC-POSE-SEED17", "TwoArmLift-PandaPanda-OSC-POSE-SEED17", "LiftModded-Jaco-OSC-POSITION-SEED251"):
        v = variant.load_variant(os.path.join(ROOT, "tests", "golden", name + ".variant.json"))
        v["algorithm_kwargs"].update(min_num_steps_before_training=600, num_eval_steps_per_epoch=300,
                                     num_expl_steps_per_train_loop=400, num_trains_per_train_loop=150,
                                     eval_max_path_length=100, expl_max_path_length=100)
        v["replay_buffer_size"] = 5000
        vs.append(v)
    vs[1]["algorithm_kwargs"]["batch_size"] = 256                     # unequal batches
    runs = [(v, s) for v in vs for s in (17, 18)]
    got = experiment_sweep(runs, num_epochs=2, log_dir=str(tmp_path), quiet=True)
    assert len(got) == len(runs)
    for (v, s), rows in zip(runs, got):
        want = experiment(v, seed=s, num_epochs=2, quiet=True)
        assert len(rows) == len(want) == 2
        for rg, rw in zip(rows, want):
            assert list(rg.keys()) == list(rw.keys())
            for k in rw:
                if not k.startswith("time/"):
                    assert rg[k] == rw[k], (v["expl_environment_kwargs"]["env_name"], s, k)
        env = v["expl_environment_kwargs"]
        assert os.path.exists(tmp_path / f"{env['env_name']}-{''.join(env['robots'])}-s{s}" / "progress.csv")
