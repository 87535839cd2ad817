"""GPU: TD3 trainer groups (td3_group_create / TD3TrainerGroup) -- R TD3 runs of one shape trained with grouped launches.
Every member must equal, bit for bit, a solo twin (same initial weights and config, a buffer with the same rows and
seed) that ran TD3Trainer.train_loop for the same steps -- whatever phase of the delayed policy update each is in."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from robosuite_benchmark_amd import EnvReplayBuffer, TD3TrainerGroup, _lib
from robosuite_benchmark_amd.checkpoint import load_checkpoint, save_checkpoint
from tests.helpers import make_pair, make_td3_pair, synth_transitions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ("policy", "qf1", "qf2", "target_qf1", "target_qf2", "target_policy")


def trainer(O, A, B, seed, **kw):
    return make_td3_pair(O, A, B, seed=seed, noise_seed=1000 + seed, **kw)[1]


def buffer(n, O, A, data_seed, rng_seed, term_frac=0.1):
    obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=data_seed, term_frac=term_frac)
    buf = EnvReplayBuffer(n, obs_dim=O, action_dim=A)
    buf.add_block(obs, act, rew, nobs, term)
    buf.seed(rng_seed)
    return buf


def opt_state(t, name):
    n = t._get_params(name).size
    m, v = np.empty(n, np.float32), np.empty(n, np.float32)
    _lib.check(t._lib.sac_get_opt_state(t._h, _lib.TD3_NET_IDS[name], _lib.ptr(m), _lib.ptr(v), n), "sac_get_opt_state")
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
    assert np.array_equal(scalars(t), scalars(twin)), (where, scalars(t), scalars(twin))
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
        assert np.array_equal(first[r], f), (r, steps, "diag_first")
        assert np.array_equal(last[r], l), (r, steps, "diag_last")
    for r in range(len(members)):
        assert_twins(members[r], twins[r], bufs[r], tbufs[r], where=(r, steps))
    return first, last


def test_group_equals_solo_runs_bitwise():
    O, A, B = 42, 7, 256
    specs = [(3, 3000, dict(policy_and_target_update_period=1, tau=0.005, reward_scale=1.0)),
             (4, 5000, dict(policy_and_target_update_period=2, tau=0.01, policy_learning_rate=3e-4, qf_learning_rate=1e-3,
                            target_policy_noise=0.1, target_policy_noise_clip=0.3, reward_scale=5.0)),
             (5, 7777, dict(policy_and_target_update_period=3, tau=0.02, policy_learning_rate=2e-3,
                            target_policy_noise=0.3, target_policy_noise_clip=0.6, reward_scale=0.5))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    group = TD3TrainerGroup(members)
    for steps in (37, 1000):
        group_and_twins_step(group, members, twins, bufs, tbufs, B, steps)
    # 1037 steps: the members' policy steps are every step, every second and every third step number
    assert [scalars(t)[0] for t in members] == [1037, 519, 346]


def test_members_out_of_phase():
    """A member that took an odd number of solo steps joins the group: its call starts on a critic-only step (the actor
    pass runs for the first step's statistics only), while the others start on policy steps."""
    O, A, B = 42, 7, 128
    specs = [(6, 2000, dict(policy_and_target_update_period=2)), (7, 2500, dict(policy_and_target_update_period=2)),
             (8, 1800, dict(policy_and_target_update_period=3))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    for t, tw, b, tb in ((members[0], twins[0], bufs[0], tbufs[0]), (members[2], twins[2], bufs[2], tbufs[2])):
        t.train_loop(b, 3, batch_size=B)
        tw.train_loop(tb, 3, batch_size=B)
    members[2].train(bufs[2].random_batch(B))
    twins[2].train(tbufs[2].random_batch(B))
    group = TD3TrainerGroup(members)
    first, _ = group_and_twins_step(group, members, twins, bufs, tbufs, B, 5)
    assert [scalars(t)[4] for t in members] == [8, 5, 9]
    i = _lib.TD3_DIAG_NAMES.index("Policy Loss")
    assert np.all(np.isfinite(first[:, i])) and np.all(first[:, i] != 0)
    # a call whose first step is a policy step for no member (step numbers 9, 5, 10 against periods 2, 2, 3)
    for r in (0, 2):
        members[r].train(bufs[r].random_batch(B))
        twins[r].train(tbufs[r].random_batch(B))
    assert [int(scalars(t)[4]) % p for t, p in zip(members, (2, 2, 3))] == [1, 1, 1]
    for steps in (1, 2, 300):
        group_and_twins_step(group, members, twins, bufs, tbufs, B, steps)


@pytest.mark.parametrize("O,A,B", [(42, 7, 128), (42, 7, 256), (89, 14, 256), (379, 6, 256), (112, 7, 64), (42, 7, 5)])
def test_group_shape_matrix(O, A, B):
    specs = [(11, 900, dict(discount=0.98)), (12, 1300, dict(tau=0.01, qf_learning_rate=1e-3, policy_and_target_update_period=3))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    group = TD3TrainerGroup(members)
    group_and_twins_step(group, members, twins, bufs, tbufs, B, 300)


def test_group_of_one_and_of_sixteen():
    O, A, B = 42, 7, 128
    members, twins, bufs, tbufs = make_set(O, A, B, [(21, 2000, {})])
    group_and_twins_step(TD3TrainerGroup(members), members, twins, bufs, tbufs, B, 260)
    specs = [(30 + i, 200 + 37 * i, dict(reward_scale=1.0 + 0.25 * i, policy_and_target_update_period=1 + i % 4))
             for i in range(16)]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    group_and_twins_step(TD3TrainerGroup(members), members, twins, bufs, tbufs, B, 40)


def test_fused_members_stay_fused():
    O, A, B = 42, 7, 128
    specs = [(51, 2500, {}), (52, 2600, dict(policy_learning_rate=5e-4, policy_and_target_update_period=3))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    assert all(t.is_fused() for t in members + twins)
    group = TD3TrainerGroup(members)
    group_and_twins_step(group, members, twins, bufs, tbufs, B, 121)
    assert all(t.is_fused() for t in members)
    for t, tw, b, tb in zip(members, twins, bufs, tbufs):
        f, l = t.train_loop(b, 31, batch_size=B)
        f2, l2 = tw.train_loop(tb, 31, batch_size=B)
        assert np.array_equal(f, f2) and np.array_equal(l, l2)
        assert_twins(t, tw, b, tb, where="solo after group")
    # and members on the four-launch step from the start equal four-launch twins
    os.environ["SAC_FUSED"] = "0"
    try:
        members, twins, bufs, tbufs = make_set(O, A, B, specs)
    finally:
        del os.environ["SAC_FUSED"]
    assert not any(t.is_fused() for t in members + twins)
    group_and_twins_step(TD3TrainerGroup(members), members, twins, bufs, tbufs, B, 121)


def test_group_interleaves_with_solo_entry_points(tmp_path):
    O, A, B = 42, 7, 256
    specs = [(41, 4000, {}), (42, 3000, dict(reward_scale=2.0, policy_and_target_update_period=3))]
    members, twins, bufs, tbufs = make_set(O, A, B, specs)
    group = TD3TrainerGroup(members)
    group_and_twins_step(group, members, twins, bufs, tbufs, B, 20)
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=99, term_frac=0.1)
    host = dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs)
    for t, tw, b, tb in zip(members, twins, bufs, tbufs):
        t.train_loop(b, 15, batch_size=B)
        tw.train_loop(tb, 15, batch_size=B)
        for _ in range(3):                                    # device batches (random_batch leaves them on the device)
            t.train(b.random_batch(B))
            tw.train(tb.random_batch(B))
        t.train(host)
        tw.train(host)
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
    # a member checkpoint saved after group steps resumes bit for bit
    ck = str(tmp_path / "ck")
    save_checkpoint(ck, members[1], bufs[1])
    # (into a trainer of the same config and noise seed, other initial weights: the checkpoint brings the state)
    resumed = make_td3_pair(O, A, B, seed=77, noise_seed=1042, **specs[1][2])[1]
    rbuf = EnvReplayBuffer(3000, obs_dim=O, action_dim=A)
    load_checkpoint(ck, resumed, rbuf)
    f, l = resumed.train_loop(rbuf, 33, batch_size=B)
    f2, l2 = twins[1].train_loop(tbufs[1], 33, batch_size=B)
    assert np.array_equal(f, f2) and np.array_equal(l, l2)
    assert_twins(resumed, twins[1], rbuf, tbufs[1], where="resumed")


def c_group(trainers, create="td3_group_create"):
    lib = _lib.load()
    arr = (C.c_void_p * len(trainers))(*[t._h.value for t in trainers])
    g = C.c_void_p()
    rc = getattr(lib, create)(C.byref(g), arr, len(trainers))
    if rc < 0:
        raise RuntimeError(_lib.last_error())
    return g


def test_refusals_leave_members_unchanged():
    from robosuite_benchmark_amd import FlattenMlp, TanhMlpPolicy, TD3Trainer
    O, A, B = 42, 7, 128
    a, b = trainer(O, A, B, 61), trainer(O, A, B, 62)
    before = {id(t): [t._get_params(n) for n in NETS] for t in (a, b)}
    # SAC members and mixed groups (host metadata and the C ABI); sac_group_create still refuses TD3 members
    sac = make_pair(O, A, B, seed=60)[1]
    for ms in ([sac], [a, sac], [sac, a]):
        with pytest.raises(RuntimeError, match="TD3 groups hold TD3 trainers only"):
            TD3TrainerGroup(ms)
        with pytest.raises(RuntimeError, match="is a SAC trainer"):
            c_group(ms)
    with pytest.raises(RuntimeError, match="TD3 trainer"):
        c_group([a], create="sac_group_create")
    # general-step members
    pols = [TanhMlpPolicy([256, 256, 256], A, O) for _ in range(2)]
    qs = [FlattenMlp([256, 256, 256], 1, O + A) for _ in range(4)]
    gen = TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1],
                     batch_size=B)
    with pytest.raises(RuntimeError, match="general step"):
        TD3TrainerGroup([gen]).train_loop([buffer(500, O, A, 1, 1)], 5)
    with pytest.raises(RuntimeError, match="general step"):
        c_group([gen])
    # batches above 256 rows
    big = trainer(O, A, 512, 63)
    with pytest.raises(RuntimeError, match="at most 256 rows"):
        TD3TrainerGroup([big]).train_loop([buffer(1000, O, A, 1, 1)], 5)
    with pytest.raises(RuntimeError, match="at most 256 rows"):
        c_group([big])
    # a member confined to an XCD
    conf = trainer(O, A, B, 64)
    _lib.check(conf._lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    with pytest.raises(RuntimeError, match="confined"):
        c_group([a, conf])
    # the same trainer twice
    with pytest.raises(RuntimeError, match="twice"):
        TD3TrainerGroup([a, a])
    with pytest.raises(RuntimeError, match="same trainer"):
        c_group([a, a])
    group = TD3TrainerGroup([a, b])
    b1, b2 = buffer(800, O, A, 1, 1), buffer(800, O, A, 2, 2)
    with pytest.raises(RuntimeError, match="same buffer"):
        group.train_loop([b1, b1], 5, batch_size=B)
    with pytest.raises(RuntimeError, match="has dims"):
        group.train_loop([b1, buffer(800, O + 1, A, 3, 3)], 5, batch_size=B)
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
    ha = a._h.value
    with pytest.raises(RuntimeError, match="same buffer"):
        group.train_loop([b1, b1], 5, batch_size=64)
    assert a._h.value == ha and a._batch == B
    for t in (a, b):
        for n, p in zip(NETS, before[id(t)]):
            assert np.array_equal(t._get_params(n), p), n
        assert scalars(t)[4] == 0 and scalars(t)[0] == 0
    # (and the group still works after all that)
    group.train_loop([b1, b2], 5, batch_size=B)
    assert [tuple(scalars(t)[[0, 3, 4]]) for t in (a, b)] == [(3, 5, 5)] * 2
    after = {id(t): [t._get_params(n) for n in NETS] for t in (a, b)}
    _lib.check(b._lib.sac_trainer_set_xcd(b._h, 1), "sac_trainer_set_xcd")
    with pytest.raises(RuntimeError, match="confined"):
        group.train_loop([b1, b2], 5, batch_size=B)
    for t in (a, b):
        for n, p in zip(NETS, after[id(t)]):
            assert np.array_equal(t._get_params(n), p), n
        assert scalars(t)[4] == 5


def test_buffers_on_the_numpy_stream_continue_it_in_member_order():
    O, A, B = 42, 7, 128
    specs = [(81, 1500, {}), (82, 2300, dict(reward_scale=3.0, policy_and_target_update_period=3)), (83, 900, {})]

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
    group = TD3TrainerGroup(members)
    for steps in (30, 301):
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


def td3_variant():
    from robosuite_benchmark_amd.variant import default_variant
    v = default_variant(env="Lift", seed=3, batch_size=128, agent="TD3")
    v["algorithm_kwargs"].update(num_epochs=3, num_trains_per_train_loop=41, num_expl_steps_per_train_loop=100,
                                 num_eval_steps_per_epoch=100, min_num_steps_before_training=200,
                                 expl_max_path_length=50, eval_max_path_length=50)
    v["replay_buffer_size"] = 5000
    return v


def test_experiment_group_on_a_td3_variant(tmp_path):
    from robosuite_benchmark_amd.driver import experiment, experiment_group
    v = td3_variant()
    got = experiment_group(v, seeds=[3, 4], log_dir=str(tmp_path), quiet=True)
    for s in (3, 4):
        want = experiment(v, seed=s, quiet=True)
        assert len(got[s]) == len(want) == 3
        for rg, rw in zip(got[s], want):
            assert list(rg.keys()) == list(rw.keys())
            for k in rw:
                if not k.startswith("time/"):
                    assert rg[k] == rw[k], (s, k)
        assert "trainer/Policy Loss" in got[s][-1] and "trainer/Alpha" not in got[s][-1]
        assert os.path.exists(tmp_path / f"s{s}" / "progress.csv")
    with pytest.raises(RuntimeError, match="resume"):
        experiment_group(v, seeds=[3], num_epochs=1, resume=True)


def test_train_script_seeds_with_td3(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--seeds", "3", "4", "--agent", "TD3",
                          "--epochs", "1", "--log_dir", str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    for s in (3, 4):
        p = tmp_path / f"s{s}" / "progress.csv"
        assert p.exists()
        lines = p.read_text().splitlines()
        assert len(lines) == 2 and "trainer/Policy Loss" in lines[0]
