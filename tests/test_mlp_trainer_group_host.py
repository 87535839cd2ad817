"""CPU: MLP trainer groups (runs of the general step: hidden sizes other than two layers of at most 256 units) take
members of different dims and batch sizes, refuse what cannot share their grouped launches from host metadata alone,
before any handle exists, naming the member and the field, and their C entry points are declared and bound."""
import pytest

import robosuite_benchmark_amd as rba
from robosuite_benchmark_amd import (FlattenMlp, MlpSACTrainerGroup, MlpTD3TrainerGroup, SACTrainer, TanhGaussianPolicy,
                                     TanhMlpPolicy, TD3Trainer)
from robosuite_benchmark_amd import _lib


def sac(O=42, A=7, hidden=(512, 512), hidden_q=None, **kw):
    hq = list(hidden_q or hidden)
    return SACTrainer(policy=TanhGaussianPolicy(list(hidden), O, A), qf1=FlattenMlp(hq, 1, O + A),
                      qf2=FlattenMlp(hq, 1, O + A), target_qf1=FlattenMlp(hq, 1, O + A), target_qf2=FlattenMlp(hq, 1, O + A),
                      **kw)


def td3(O=42, A=7, hidden=(512, 512), **kw):
    h = list(hidden)
    return TD3Trainer(policy=TanhMlpPolicy(h, A, O), qf1=FlattenMlp(h, 1, O + A), qf2=FlattenMlp(h, 1, O + A),
                      target_qf1=FlattenMlp(h, 1, O + A), target_qf2=FlattenMlp(h, 1, O + A),
                      target_policy=TanhMlpPolicy(h, A, O), **kw)


def test_mlp_groups_are_exported():
    assert rba.MlpSACTrainerGroup is MlpSACTrainerGroup and rba.MlpTD3TrainerGroup is MlpTD3TrainerGroup
    assert "MlpSACTrainerGroup" in rba.__all__ and "MlpTD3TrainerGroup" in rba.__all__


def test_general_step_members_make_a_group_without_a_gpu():
    ms = [sac(42, 7), sac(379, 6), sac(89, 14), sac(30, 1), sac(50, 16)]
    g = MlpSACTrainerGroup(ms)
    assert len(g) == 5 and all(m._h is None for m in ms)
    deep = [sac(42, 7, hidden=(256, 256, 256)) for _ in range(3)]
    assert len(MlpSACTrainerGroup(deep)) == 3
    ts = [td3(42, 7, policy_and_target_update_period=p) for p in (1, 2, 3)]
    g = MlpTD3TrainerGroup(ts)
    assert len(g) == 3 and all(t._h is None for t in ts)


def test_mlp_refusals_before_any_handle():
    with pytest.raises(RuntimeError, match=r"member 1 has the shapes of the fused kernels \(policy hidden sizes \[256, 256\]"):
        MlpSACTrainerGroup([sac(), sac(hidden=(256, 256))])
    with pytest.raises(RuntimeError, match="member 0 has the shapes of the fused kernels"):
        MlpTD3TrainerGroup([td3(hidden=(256, 128))])
    with pytest.raises(RuntimeError, match="member 1 is a TD3Trainer: groups hold SAC trainers only"):
        MlpSACTrainerGroup([sac(), td3()])
    with pytest.raises(RuntimeError, match="member 1 is a SACTrainer: TD3 groups hold TD3 trainers only"):
        MlpTD3TrainerGroup([td3(), sac()])
    with pytest.raises(RuntimeError, match=r"member 1 has policy hidden sizes \[1024, 1024\], member 0 \[512, 512\]"):
        MlpSACTrainerGroup([sac(), sac(hidden=(1024, 1024))])
    with pytest.raises(RuntimeError, match=r"member 2 has qf1 hidden sizes \[512, 256\]"):
        MlpSACTrainerGroup([sac(), sac(), sac(hidden_q=(512, 256))])
    t = sac()
    with pytest.raises(RuntimeError, match="twice"):
        MlpSACTrainerGroup([t, sac(46, 8), t])
    for n in (0, 17):
        with pytest.raises(RuntimeError, match="1..16"):
            MlpSACTrainerGroup([sac(40 + i, 7) for i in range(n)])
        with pytest.raises(RuntimeError, match="1..16"):
            MlpTD3TrainerGroup([td3(40 + i, 7) for i in range(n)])


class StubBuffer:
    """What the group checks of a replay buffer from host metadata (no device storage behind it)."""
    _h = 1

    def __init__(self, O, A, rows=100):
        self._observation_dim, self._action_dim, self._rows = O, A, rows

    def num_steps_can_sample(self):
        return self._rows


def test_mlp_train_loop_refusals_before_any_handle():
    ms = [sac(42, 7), sac(46, 8)]
    g = MlpSACTrainerGroup(ms)
    with pytest.raises(RuntimeError, match="2 trainers but 1 replay buffers"):
        g.train_loop([StubBuffer(42, 7)], 5, batch_sizes=[128, 64])
    with pytest.raises(RuntimeError, match="member 1 has no batch size"):
        g.train_loop([None, None], 5, batch_sizes=[128, None])
    with pytest.raises(RuntimeError, match="2 trainers but 1 batch sizes"):
        g.train_loop([None, None], 5, batch_sizes=[128])
    with pytest.raises(RuntimeError, match="buffer 0 has no device storage"):
        g.train_loop([None, StubBuffer(46, 8)], 5, batch_sizes=[128, 64])
    with pytest.raises(RuntimeError, match=r"buffer 1 has dims \(42,7\), its member \(46,8\)"):
        g.train_loop([StubBuffer(42, 7), StubBuffer(42, 7)], 5, batch_sizes=[128, 64])
    with pytest.raises(RuntimeError, match="buffer 1 is empty"):
        g.train_loop([StubBuffer(42, 7), StubBuffer(46, 8, rows=0)], 5, batch_sizes=[128, 512])
    assert all(m._h is None for m in ms)


def test_driver_picks_the_mlp_kind_for_general_variants():
    from robosuite_benchmark_amd.group import runs_general_step
    assert runs_general_step(sac(hidden=(512, 512)))
    assert runs_general_step(sac(hidden=(256, 256, 256)))
    assert runs_general_step(sac(hidden=(256, 256), hidden_q=(1024, 1024)))
    assert not runs_general_step(sac(hidden=(256, 256)))
    assert not runs_general_step(sac(hidden=(128, 64)))


def test_mlp_group_symbols_declared_and_bound():
    from tests.test_abi_library import declared_symbols
    names = declared_symbols()
    for n in ("sac_group_create_mlp", "td3_group_create_mlp", "sac_group_train_loop", "sac_group_destroy"):
        assert n in names and n in _lib.SYMBOLS
        assert hasattr(_lib.load(), n)
