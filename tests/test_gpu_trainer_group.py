"""GPU: trainer groups (sac_group_* / SACTrainerGroup) -- R SAC runs of one shape trained with grouped launches.
Every member must equal, bit for bit, a solo twin (same initial weights and config, a buffer with the same rows and
seed) that ran sac_train_loop for the same steps."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from robosuite_benchmark_amd import EnvReplayBuffer, SACTrainerGroup, _lib
from tests.helpers import make_pair, synth_transitions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ("policy", "qf1", "qf2", "target_qf1", "target_qf2")


def trainer(O, A, B, seed, **kw):
    return make_pair(O, A, B, seed=seed, noise_seed=1000 + seed, **kw)[1]


def buffer(n, O, A, data_seed, rng_seed, term_frac=0.1):
    obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=data_seed, term_frac=term_frac)
    buf = EnvReplayBuffer(n, obs_dim=O, action_dim=A)
    buf.add_block(obs, act, rew, nobs, term)
    buf.seed(rng_seed)
    return buf


def opt_state(t, name):
    n = t._get_params(name).size
    m, v = np.empty(n, np.float32), np.empty(n, np.float32)
    _lib.check(t._lib.sac_get_opt_state(t._h, _lib.NET_IDS[name], _lib.ptr(m), _lib.ptr(v), n), "sac_get_opt_state")
    return m, v


def scalars(t):
    sc = np.zeros(6, np.float64)
    _lib.check(t._lib.sac_get_scalars(t._h, _lib.ptr(sc)), "sac_get_scalars")
    return sc


def assert_twins(t, twin, buf, buf_twin, where=""):
    for name in NETS:
        assert np.array_equal(t._get_params(name), twin._get_params(name)), (where, name)
    for name in ("policy", "qf1", "qf2"):
        for a, b in zip(opt_state(t, name), opt_state(twin, name)):
            assert np.array_equal(a, b), (where, "adam", name)
    assert np.array_equal(scalars(t), scalars(twin)), where
    (k1, p1), (k2, p2) = buf.rng_state(), buf_twin.rng_state()
    assert p1 == p2 and np.array_equal(k1, k2), (where, "generator")


def make_set(O, A, B, specs, **common):
    """specs: per member (seed, buffer rows, extra trainer kwargs) -> members, twins, buffers, twin buffers."""
    members, twins, bufs, tbufs = [], [], [], []
    for i, (seed, n, kw) in enumerate(specs):
        members.append(trainer(O, A, B, seed, **common, **kw))
        twins.append(trainer(O, A, B, seed, **common, **kw))
        bufs.append(buffer(n, O, A, 50 + i, 70 + i))
        tbufs.append(buffer(n, O, A, 50 + i, 70 + i))
    return members, twins, bufs, tbufs


def group_and_twins_step(group, members, twins, bufs, tbufs, B, steps):
    first, last = group.train_loop(bufs, steps, batch_size=B)
    for r, (tw, tb) in enumerate(zip(twins, tbufs)):
        f, l = tw.train_loop(tb, steps, batch_size=B)
        assert np.array_equal(first[r], f), (r, "diag_first")
        assert np.array_equal(last[r], l), (r, "diag_last")
    for r in range(len(members)):
        assert_twins(members[r], twins[r], bufs[r], tbufs[r], where=(r, steps))


def test_group_equals_solo_runs_bitwise():
    O, A, B = 42, 7, 256
    specs = [(3, 3000, dict(reward_scale=1.0, policy_lr=1e-3, target_entropy=None)),
             (4, 5000, dict(reward_scale=5.0, policy_lr=3e-4, target_entropy=-3.0)),
             (5, 7777, dict(reward_scale=0.5, policy_lr=2e-3, target_entropy=-10.0))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    group = SACTrainerGroup(members)
    for steps in (37, 1000):
        group_and_twins_step(group, members, twins, bufs, tbufs, B, steps)


@pytest.mark.parametrize("O,A,B", [(42, 7, 128), (379, 6, 256), (112, 7, 64), (89, 14, 256), (42, 7, 5)])
def test_group_shape_matrix(O, A, B):
    specs = [(11, 900, dict(discount=0.98)), (12, 1300, dict(soft_target_tau=0.01, qf_lr=1e-3))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    group = SACTrainerGroup(members)
    group_and_twins_step(group, members, twins, bufs, tbufs, B, 300)


def test_group_of_one_and_of_sixteen():
    O, A, B = 42, 7, 128
    members, twins, bufs, tbufs = make_set(O, A, B, [(21, 2000, {})])
    group_and_twins_step(SACTrainerGroup(members), members, twins, bufs, tbufs, B, 260)
    specs = [(30 + i, 200 + 37 * i, dict(reward_scale=1.0 + 0.25 * i)) for i in range(16)]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    group_and_twins_step(SACTrainerGroup(members), members, twins, bufs, tbufs, B, 40)


def test_group_interleaves_with_solo_entry_points():
    O, A, B = 42, 7, 256
    specs = [(41, 4000, {}), (42, 3000, dict(reward_scale=2.0))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    group = SACTrainerGroup(members)
    group_and_twins_step(group, members, twins, bufs, tbufs, B, 20)
    for t, tw, b, tb in zip(members, twins, bufs, tbufs):
        t.train_loop(b, 15, batch_size=B)
        tw.train_loop(tb, 15, batch_size=B)
        for _ in range(3):
            t.train(b.random_batch(B))
            tw.train(tb.random_batch(B))
        assert_twins(t, tw, b, tb, where="solo")
    group_and_twins_step(group, members, twins, bufs, tbufs, B, 25)
    t, tw = members[0], twins[0]
    snap, snap_tw = t.get_snapshot(), tw.get_snapshot()
    for name in NETS:
        assert np.array_equal(snap[name].flat(), snap_tw[name].flat()), name
    assert np.array_equal(snap["policy"].flat(), t._get_params("policy"))
    back = pickle.loads(pickle.dumps(t))
    assert np.array_equal(back._saved_state["params"]["policy"], tw._get_params("policy"))
    obs = np.random.RandomState(5).normal(size=(3, O)).astype(np.float32)
    assert np.array_equal(t.policy_act(obs, True, None), tw.policy_act(obs, True, None))


def test_fused_members_stay_fused():
    O, A, B = 42, 7, 128
    specs = [(51, 2500, {}), (52, 2600, dict(policy_lr=5e-4))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    assert all(t.is_fused() for t in members + twins)
    group = SACTrainerGroup(members)
    group_and_twins_step(group, members, twins, bufs, tbufs, B, 120)
    assert all(t.is_fused() for t in members)
    for t, tw, b, tb in zip(members, twins, bufs, tbufs):
        f, l = t.train_loop(b, 30, batch_size=B)
        f2, l2 = tw.train_loop(tb, 30, batch_size=B)
        assert np.array_equal(f, f2) and np.array_equal(l, l2)
        assert_twins(t, tw, b, tb, where="solo after group")
    # and members on the four-launch step from the start equal four-launch twins
    os.environ["SAC_FUSED"] = "0"
    try:
        members, twins, bufs, tbufs = make_set(O, A, B, specs)
    finally:
        del os.environ["SAC_FUSED"]
    assert not any(t.is_fused() for t in members + twins)
    group_and_twins_step(SACTrainerGroup(members), members, twins, bufs, tbufs, B, 120)


def c_group(trainers):
    lib = _lib.load()
    arr = (C.c_void_p * len(trainers))(*[t._h.value for t in trainers])
    g = C.c_void_p()
    rc = lib.sac_group_create(C.byref(g), arr, len(trainers))
    if rc < 0:
        raise RuntimeError(_lib.last_error())
    return g


def test_refusals_leave_members_unchanged():
    from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy, TD3Trainer, TanhMlpPolicy
    O, A, B = 42, 7, 128
    a, b = trainer(O, A, B, 61), trainer(O, A, B, 62)
    before = {id(t): [t._get_params(n) for n in NETS] for t in (a, b)}
    # TD3 members (host metadata and the C ABI)
    td3 = TD3Trainer(policy=TanhMlpPolicy([256, 256], A, O), qf1=FlattenMlp([256, 256], 1, O + A),
                     qf2=FlattenMlp([256, 256], 1, O + A), target_qf1=FlattenMlp([256, 256], 1, O + A),
                     target_qf2=FlattenMlp([256, 256], 1, O + A), target_policy=TanhMlpPolicy([256, 256], A, O),
                     batch_size=B)
    with pytest.raises(RuntimeError, match="SAC trainers only"):
        SACTrainerGroup([a, td3])
    with pytest.raises(RuntimeError, match="TD3 trainer"):
        c_group([a, td3])
    # general-step members
    pol = TanhGaussianPolicy([256, 256, 256], O, A)
    qs = [FlattenMlp([256, 256, 256], 1, O + A) for _ in range(4)]
    gen = SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], batch_size=B)
    with pytest.raises(RuntimeError, match="general step"):
        SACTrainerGroup([gen]).train_loop([buffer(500, O, A, 1, 1)], 5)
    with pytest.raises(RuntimeError, match="general step"):
        c_group([gen])
    # batches above 256 rows
    big = trainer(O, A, 512, 63)
    with pytest.raises(RuntimeError, match="at most 256 rows"):
        SACTrainerGroup([big]).train_loop([buffer(1000, O, A, 1, 1)], 5)
    with pytest.raises(RuntimeError, match="at most 256 rows"):
        c_group([big])
    # a member confined to an XCD
    conf = trainer(O, A, B, 64)
    _lib.check(conf._lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    with pytest.raises(RuntimeError, match="confined"):
        c_group([a, conf])
    # the same trainer twice
    with pytest.raises(RuntimeError, match="twice"):
        SACTrainerGroup([a, a])
    with pytest.raises(RuntimeError, match="same trainer"):
        c_group([a, a])
    group = SACTrainerGroup([a, b])
    b1, b2 = buffer(800, O, A, 1, 1), buffer(800, O, A, 2, 2)
    # the same buffer twice
    with pytest.raises(RuntimeError, match="same buffer"):
        group.train_loop([b1, b1], 5, batch_size=B)
    # a buffer of other dims
    with pytest.raises(RuntimeError, match="has dims"):
        group.train_loop([b1, buffer(800, O + 1, A, 3, 3)], 5, batch_size=B)
    # an empty buffer
    with pytest.raises(RuntimeError, match="empty"):
        group.train_loop([b1, EnvReplayBuffer(100, obs_dim=O, action_dim=A)], 5, batch_size=B)
    # the same refusals at the C ABI
    g = c_group([a, b])
    lib = _lib.load()
    try:
        for bs, what in (([b1, b1], "same buffer"), ([b1, buffer(800, O + 1, A, 3, 3)], "has dims"),
                         ([b1, EnvReplayBuffer(100, obs_dim=O, action_dim=A)], "empty")):
            arr = (C.c_void_p * 2)(*[x._h.value for x in bs])
            assert lib.sac_group_train_loop(g, arr, 5, None, None) < 0
            assert what in _lib.last_error(), (what, _lib.last_error())
    finally:
        lib.sac_group_destroy(g)
    # a refused call leaves the members' handles alone (no re-creation for the call's batch size)
    ha = a._h.value
    with pytest.raises(RuntimeError, match="same buffer"):
        group.train_loop([b1, b1], 5, batch_size=64)
    assert a._h.value == ha and a._batch == B
    for t in (a, b):
        for n, p in zip(NETS, before[id(t)]):
            assert np.array_equal(t._get_params(n), p), n
        assert scalars(t)[4] == 0
    # (and the group still works after all that)
    group.train_loop([b1, b2], 5, batch_size=B)
    assert scalars(a)[4] == 5 and scalars(b)[4] == 5
    # a member confined AFTER the group was made is refused at the call
    after = {id(t): [t._get_params(n) for n in NETS] for t in (a, b)}
    _lib.check(b._lib.sac_trainer_set_xcd(b._h, 1), "sac_trainer_set_xcd")
    with pytest.raises(RuntimeError, match="confined"):
        group.train_loop([b1, b2], 5, batch_size=B)
    for t in (a, b):
        for n, p in zip(NETS, after[id(t)]):
            assert np.array_equal(t._get_params(n), p), n
        assert scalars(t)[4] == 5


def test_buffers_on_the_numpy_stream_continue_it_in_member_order():
    """Default buffers all sample np.random (bound to its state words): the group continues it buffer after buffer,
    as solo train_loop calls in member order do -- indices, results and np.random's state afterwards."""
    O, A, B = 42, 7, 128
    specs = [(81, 1500, {}), (82, 2300, dict(reward_scale=3.0)), (83, 900, {})]

    def bound_set():
        members, bufs = [], []
        for i, (seed, n, kw) in enumerate(specs):
            members.append(trainer(O, A, B, seed, **kw))
            obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=90 + i, term_frac=0.1)
            buf = EnvReplayBuffer(n, obs_dim=O, action_dim=A)          # bound to np.random (the default)
            buf.add_block(obs, act, rew, nobs, term)
            bufs.append(buf)
        return members, bufs

    members, bufs = bound_set()
    twins, tbufs = bound_set()
    group = SACTrainerGroup(members)
    for steps in (30, 300):
        np.random.seed(1234 + steps)
        first, last = group.train_loop(bufs, steps, batch_size=B)
        after_group = np.random.get_state()
        np.random.seed(1234 + steps)
        for r, (tw, tb) in enumerate(zip(twins, tbufs)):
            f, l = tw.train_loop(tb, steps, batch_size=B)
            assert np.array_equal(first[r], f) and np.array_equal(last[r], l), r
        after_solo = np.random.get_state()
        assert np.array_equal(after_group[1], after_solo[1]) and after_group[2] == after_solo[2]
        for r in range(len(specs)):
            for name in NETS:
                assert np.array_equal(members[r]._get_params(name), twins[r]._get_params(name)), (steps, r, name)
            assert np.array_equal(scalars(members[r]), scalars(twins[r])), (steps, r)


def test_experiment_group_rows_equal_solo_experiments(tmp_path):
    from robosuite_benchmark_amd import variant
    from robosuite_benchmark_amd.driver import experiment, experiment_group
    v = variant.load_variant(os.path.join(ROOT, "tests", "golden", "Lift-Panda-OSC-POSE-SEED17.variant.json"))
    ak = v["algorithm_kwargs"]
    ak.update(min_num_steps_before_training=600, num_eval_steps_per_epoch=300, num_expl_steps_per_train_loop=400,
              num_trains_per_train_loop=150, eval_max_path_length=100, expl_max_path_length=100)
    v["replay_buffer_size"] = 5000
    got = experiment_group(v, seeds=[17, 18], num_epochs=2, log_dir=str(tmp_path), quiet=True)
    for s in (17, 18):
        want = experiment(v, seed=s, num_epochs=2, quiet=True)
        assert len(got[s]) == len(want) == 2
        for rg, rw in zip(got[s], want):
            assert list(rg.keys()) == list(rw.keys())
            for k in rw:
                if not k.startswith("time/"):
                    assert rg[k] == rw[k], (s, k)
        assert os.path.exists(tmp_path / f"s{s}" / "progress.csv")
    with pytest.raises(RuntimeError, match="resume"):
        experiment_group(v, seeds=[17], num_epochs=1, resume=True)
