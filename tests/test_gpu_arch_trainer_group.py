"""GPU: arch trainer groups (sac_group_create_arch / td3_group_create_arch, ArchSACTrainerGroup / ArchTD3TrainerGroup)
-- runs of DIFFERENT hidden sizes trained with grouped launches over a merged schedule.  Every member must equal, bit
for bit, a solo twin (same initial weights and config, a buffer with the same rows and seed) that ran train_loop for
the same steps on its own batch size: params of every net, Adam moments, scalars, diagnostics, buffer generator."""
import ctypes as C

import numpy as np
import pytest

from robosuite_benchmark_amd import ArchSACTrainerGroup, ArchTD3TrainerGroup, EnvReplayBuffer, _lib
from tests.helpers import make_pair, make_td3_pair
from tests.test_gpu_mlp_trainer_group import (SAC_NETS, TD3_NETS, _assert_rows, _small_variant, assert_twins, buffer,
                                              run_and_compare, scalars)

pytestmark = pytest.mark.gpu


def sac_trainer(O, A, B, seed, hidden, hidden_q=None, **kw):
    return make_pair(O, A, B, seed=seed, noise_seed=1000 + seed, hidden=hidden, hidden_q=hidden_q, **kw)[1]


def td3_trainer(O, A, B, seed, hidden, **kw):
    return make_td3_pair(O, A, B, seed=seed, noise_seed=1000 + seed, hidden=hidden, **kw)[1]


def sac_set(specs, seed0=3, bound=False):
    """specs: (obs_dim, act_dim, batch, policy hidden, Q hidden) per member; every member with other hyperparameters.
    bound: buffers left on np.random (their default) instead of a private seed."""
    members, twins, bufs, tbufs = [], [], [], []
    for i, (O, A, B, hp, hq) in enumerate(specs):
        kw = dict(reward_scale=1.0 + i, policy_lr=1e-3 / (1 + i), target_update_period=1 + i % 3)
        members.append(sac_trainer(O, A, B, seed0 + i, hp, hq, **kw))
        twins.append(sac_trainer(O, A, B, seed0 + i, hp, hq, **kw))
        rng = None if bound else 70 + i
        bufs.append(buffer(2000 + 577 * i, O, A, 50 + i, rng))
        tbufs.append(buffer(2000 + 577 * i, O, A, 50 + i, rng))
    return members, twins, bufs, tbufs


def c_group(trainers, td3=False, kind="arch"):
    lib = _lib.load()
    arr = (C.c_void_p * len(trainers))(*[t._h.value for t in trainers])
    g = C.c_void_p()
    if getattr(lib, f"{'td3' if td3 else 'sac'}_group_create_{kind}")(C.byref(g), arr, len(trainers)) < 0:
        raise RuntimeError(_lib.last_error())
    return g


# Lift at [512,512]; Wipe at [256,256,256]; TwoArmLift (14 actions) at [1024] (Lp = Lq = 1: empty backward sub-runs);
# one action at [128,128,128,128]; sixteen actions with policy [512,512] and Q [256,256,256]
SAC_SPECS = [(42, 7, 256, (512, 512), None), (379, 6, 64, (256, 256, 256), None), (89, 14, 100, (1024,), None),
             (30, 1, 128, (128, 128, 128, 128), None), (50, 16, 200, (512, 512), (256, 256, 256))]


def test_arch_sac_group_equals_solo_runs_bitwise():
    members, twins, bufs, tbufs = sac_set(SAC_SPECS)
    batches = [s[2] for s in SAC_SPECS]
    group = ArchSACTrainerGroup(members)
    assert [idx for idx, _ in group.subgroups] == [[0, 1, 2, 3, 4]]
    for n in (600, 7):                                  # (600 steps cross the 256-step chunk)
        run_and_compare(group, members, twins, bufs, tbufs, batches, n, SAC_NETS, _lib.NET_IDS)
    members[2].train_loop(bufs[2], 9, batch_size=batches[2])
    twins[2].train_loop(tbufs[2], 9, batch_size=batches[2])
    assert_twins(members[2], twins[2], bufs[2], tbufs[2], SAC_NETS, _lib.NET_IDS, where="solo after group")


def test_arch_td3_group_keeps_each_members_update_plan():
    shapes = [(42, 7, 256, (512, 512), 1), (42, 7, 128, (256, 256, 256), 2), (379, 6, 64, (1024,), 3),
              (30, 12, 200, (128, 128, 128, 128), 2)]
    members, twins, bufs, tbufs = [], [], [], []
    for i, (O, A, B, h, period) in enumerate(shapes):
        kw = dict(policy_and_target_update_period=period, reward_scale=1.0 + 0.5 * i)
        members.append(td3_trainer(O, A, B, 20 + i, h, **kw))
        twins.append(td3_trainer(O, A, B, 20 + i, h, **kw))
        bufs.append(buffer(2500 + 501 * i, O, A, 30 + i, 40 + i))
        tbufs.append(buffer(2500 + 501 * i, O, A, 30 + i, 40 + i))
    batches = [s[2] for s in shapes]
    group = ArchTD3TrainerGroup(members)
    for n in (600, 7):
        run_and_compare(group, members, twins, bufs, tbufs, batches, n, TD3_NETS, _lib.TD3_NET_IDS)


def test_merged_schedule_is_as_long_as_its_deepest_member():
    members, _, _, _ = sac_set(SAC_SPECS)
    lib = _lib.load()
    whole = c_group(members)
    deepest = c_group([members[3]])                     # [128]*4: the largest Lp and Lq
    per_arch = [c_group([m], kind="mlp") for m in members]
    try:
        n = lib.sac_group_stage_count(whole)
        assert n == lib.sac_group_stage_count(deepest) == 2 * 4 + 2 * 4 + 3
        assert n < sum(lib.sac_group_stage_count(g) for g in per_arch)
    finally:
        for g in [whole, deepest] + per_arch:
            lib.sac_group_destroy(g)
    ts = [td3_trainer(42, 7, 128, 5 + i, h) for i, h in enumerate(((512, 512), (1024,), (256, 256, 256)))]
    whole, deepest = c_group(ts, td3=True), c_group([ts[2]], td3=True)
    per_arch = [c_group([t], td3=True, kind="mlp") for t in ts]
    try:
        n = lib.sac_group_stage_count(whole)
        assert n == lib.sac_group_stage_count(deepest)
        assert n < sum(lib.sac_group_stage_count(g) for g in per_arch)
    finally:
        for g in [whole, deepest] + per_arch:
            lib.sac_group_destroy(g)


# the paper default [256,256] on two tasks, [64,64] (fused shapes: mixed subgroups), [512,512] and [256,256,256]
COMPOSITE = [(42, 7, 256, (512, 512), None), (42, 7, 256, (256, 256), None), (89, 14, 128, (64, 64), None),
             (379, 6, 100, (256, 256, 256), None), (89, 14, 64, (256, 256), None)]


def test_composite_arch_group_equals_solo_runs_bitwise():
    members, twins, bufs, tbufs = sac_set(COMPOSITE, seed0=31)
    batches = [s[2] for s in COMPOSITE]
    group = ArchSACTrainerGroup(members)
    assert [idx for idx, _ in group.subgroups] == [[1, 4], [2], [0, 3]] and group.run_order == [1, 4, 2, 0, 3]
    for n in (600, 7):
        run_and_compare(group, members, twins, bufs, tbufs, batches, n, SAC_NETS, _lib.NET_IDS)
    for r in (1, 3):                                    # a member is still an ordinary trainer
        members[r].train_loop(bufs[r], 9, batch_size=batches[r])
        twins[r].train_loop(tbufs[r], 9, batch_size=batches[r])
        assert_twins(members[r], twins[r], bufs[r], tbufs[r], SAC_NETS, _lib.NET_IDS, where=("solo after group", r))


def test_buffers_on_the_numpy_stream_continue_it_in_run_order():
    members, twins, bufs, tbufs = sac_set(COMPOSITE, seed0=81, bound=True)
    batches = [s[2] for s in COMPOSITE]
    group = ArchSACTrainerGroup(members)
    for steps in (30, 300):
        np.random.seed(1234 + steps)
        first, last = group.train_loop(bufs, steps, batch_sizes=batches)
        after_group = np.random.get_state()
        np.random.seed(1234 + steps)
        for r in group.run_order:
            f, l = twins[r].train_loop(tbufs[r], steps, batch_size=batches[r])
            assert np.array_equal(first[r], f) and np.array_equal(last[r], l), (steps, r)
        after_solo = np.random.get_state()
        assert np.array_equal(after_group[1], after_solo[1]) and after_group[2] == after_solo[2], steps
        for r in range(len(COMPOSITE)):
            for name in SAC_NETS:
                assert np.array_equal(members[r]._get_params(name), twins[r]._get_params(name)), (steps, r, name)
            assert np.array_equal(scalars(members[r]), scalars(twins[r])), (steps, r)


def test_arch_refusals_leave_members_unchanged():
    (O1, A1, B1), (O2, A2, B2) = (42, 7, 128), (86, 14, 64)
    a, b = sac_trainer(O1, A1, B1, 61, (512, 512)), sac_trainer(O2, A2, B2, 62, (256, 256, 256))
    before = {id(t): [t._get_params(n) for n in SAC_NETS] for t in (a, b)}
    fused = sac_trainer(O1, A1, B1, 60, (256, 256))
    with pytest.raises(RuntimeError, match="shapes of the fused kernels"):
        c_group([a, fused])
    td3 = td3_trainer(O1, A1, B1, 60, (512, 512))
    with pytest.raises(RuntimeError, match="TD3 trainer"):
        c_group([a, td3])
    with pytest.raises(RuntimeError, match="SAC trainer"):
        c_group([td3, a], td3=True)
    with pytest.raises(RuntimeError, match="same trainer"):
        c_group([a, b, a])
    with pytest.raises(RuntimeError, match="1..16"):
        c_group([a] * 17)
    conf = sac_trainer(O2, A2, B2, 64, (1024,))
    _lib.check(conf._lib.sac_trainer_set_xcd(conf._h, 0), "sac_trainer_set_xcd")
    with pytest.raises(RuntimeError, match="confined"):
        c_group([a, conf])
    # an MLP group still refuses members of other hidden sizes; the existing kinds still refuse general-step members
    with pytest.raises(RuntimeError, match="other hidden sizes"):
        c_group([a, b], kind="mlp")
    lib = _lib.load()
    for name in ("sac_group_create", "sac_group_create_mixed"):
        arr = (C.c_void_p * 1)(b._h.value)
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
    ArchSACTrainerGroup([a, b]).train_loop([b1, b2], 5)
    assert scalars(a)[4] == 5 and scalars(b)[4] == 5


def _sweep_variants():
    return [_small_variant("Lift-Panda-OSC-POSE-SEED17", (256, 256), batch=100),
            _small_variant("Lift-Panda-OSC-POSE-SEED17", (512, 512), batch=100),
            _small_variant("TwoArmLift-PandaPanda-OSC-POSE-SEED17", (256, 256, 256), batch=100)]


def test_experiment_sweep_over_hidden_sizes_equals_solo_experiments(tmp_path):
    from robosuite_benchmark_amd.driver import experiment, experiment_sweep
    runs = [(v, 17) for v in _sweep_variants()]
    got = experiment_sweep(runs, num_epochs=2, quiet=True, hidden_sweep=True, log_dir=str(tmp_path))
    for (v, s), rows in zip(runs, got):
        _assert_rows(rows, experiment(v, seed=s, num_epochs=2, quiet=True), v["policy_kwargs"]["hidden_sizes"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["Lift-Panda-h256x256-s17", "Lift-Panda-h512x512-s17",
                                                         "TwoArmLift-PandaPanda-h256x256x256-s17"]


def test_experiment_sweep_over_hidden_sizes_resumes_bitwise(tmp_path):
    from robosuite_benchmark_amd.driver import experiment_sweep
    runs = [(v, 17) for v in _sweep_variants()]
    straight = experiment_sweep(runs, num_epochs=3, quiet=True, hidden_sweep=True)
    ck = str(tmp_path / "ck")
    experiment_sweep(runs, num_epochs=1, quiet=True, hidden_sweep=True, checkpoint_dir=ck)
    resumed = experiment_sweep(runs, num_epochs=3, quiet=True, hidden_sweep=True, checkpoint_dir=ck, resume=True)
    for i, (rows, want) in enumerate(zip(resumed, straight)):
        _assert_rows(rows, want[1:], i)
