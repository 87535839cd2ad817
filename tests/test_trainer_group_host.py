"""CPU: trainer groups refuse members that cannot share grouped launches from their host metadata alone, before any
handle exists, and the group's C entry points are declared and bound."""
import pytest

from robosuite_benchmark_amd import FlattenMlp, SACTrainer, SACTrainerGroup, TanhGaussianPolicy, TanhMlpPolicy, TD3Trainer
from robosuite_benchmark_amd import _lib


def sac(O=42, A=7, hidden=(256, 256), hidden_q=None):
    hq = list(hidden_q or hidden)
    return SACTrainer(policy=TanhGaussianPolicy(list(hidden), O, A), qf1=FlattenMlp(hq, 1, O + A),
                      qf2=FlattenMlp(hq, 1, O + A), target_qf1=FlattenMlp(hq, 1, O + A), target_qf2=FlattenMlp(hq, 1, O + A))


def td3(O=42, A=7):
    return TD3Trainer(policy=TanhMlpPolicy([256, 256], A, O), qf1=FlattenMlp([256, 256], 1, O + A),
                      qf2=FlattenMlp([256, 256], 1, O + A), target_qf1=FlattenMlp([256, 256], 1, O + A),
                      target_qf2=FlattenMlp([256, 256], 1, O + A), target_policy=TanhMlpPolicy([256, 256], A, O))


def test_mismatched_members_are_refused_before_any_handle():
    with pytest.raises(RuntimeError, match="has dims"):
        SACTrainerGroup([sac(), sac(O=43)])
    with pytest.raises(RuntimeError, match="has dims"):
        SACTrainerGroup([sac(), sac(A=6)])
    with pytest.raises(RuntimeError, match="policy hidden sizes"):
        SACTrainerGroup([sac(), sac(hidden=(128, 256), hidden_q=(256, 256))])
    with pytest.raises(RuntimeError, match="qf1 hidden sizes"):
        SACTrainerGroup([sac(), sac(hidden_q=(256, 64))])
    with pytest.raises(RuntimeError, match="SAC trainers only"):
        SACTrainerGroup([sac(), td3()])
    with pytest.raises(RuntimeError, match="SAC trainers only"):
        SACTrainerGroup([td3()])
    t = sac()
    with pytest.raises(RuntimeError, match="twice"):
        SACTrainerGroup([t, t])
    with pytest.raises(RuntimeError, match="1..16"):
        SACTrainerGroup([])
    with pytest.raises(RuntimeError, match="1..16"):
        SACTrainerGroup([sac() for _ in range(17)])


def test_matching_members_make_a_group_without_a_gpu():
    ms = [sac(), sac()]
    g = SACTrainerGroup(ms)
    assert len(g) == 2 and all(m._h is None for m in ms)


def test_group_symbols_declared_and_bound():
    from tests.test_abi_library import declared_symbols
    names = declared_symbols()
    for n in ("sac_group_create", "sac_group_destroy", "sac_group_train_loop"):
        assert n in names and n in _lib.SYMBOLS
        assert hasattr(_lib.load(), n)
