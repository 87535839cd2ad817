"""GPU: the step schedule (step_schedule, csrc/sac_step_plan.h) as its three readers walk it -- the solo step, the
profiling pass, which walks the same list with events between the stages, and the trainer groups of the fused kernels'
shapes."""
import os

import numpy as np
import pytest

from robosuite_benchmark_amd import SACTrainerGroup, TD3TrainerGroup
from tests.helpers import make_pair, make_td3_pair, plain_buffer

pytestmark = pytest.mark.gpu

STEP_ENV = ("SAC_FUSED", "SAC_CHAIN_BWD")


def _pair_under(env, O, A, B):
    """two trainers with the same seeds, created under `env` (the step plan reads the environment at creation)"""
    old = {k: os.environ.get(k) for k in STEP_ENV}
    try:
        for k in STEP_ENV:
            os.environ.pop(k, None)
        for k, v in env.items():
            os.environ[k] = str(v)
        return [make_pair(O, A, B, seed=6, noise_seed=11)[1] for _ in range(2)]
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _words(x):
    return np.ascontiguousarray(x).view(np.uint32)


# the smallest shapes that reach each sequence: k_abc + dW (three row-blocks, eight padding rows), A + B + C + dW,
# chained + C + dW, chained with the backward inside + dW
@pytest.mark.parametrize("O,A,B,env,kind", [(42, 7, 40, {}, 1), (42, 7, 40, {"SAC_FUSED": 0}, 0), (46, 7, 544, {}, 2),
                                            (46, 7, 544, {"SAC_CHAIN_BWD": 1}, 4)])
def test_the_profiled_step_is_the_step(O, A, B, env, kind):
    steps = 6
    profiled, looped = _pair_under(env, O, A, B)
    assert profiled.fused_mode() == kind and looped.fused_mode() == kind
    bufs = [plain_buffer(2000, O, A, 8), plain_buffer(2000, O, A, 8)]
    for b in bufs:
        b.seed(31)
    ms = list(profiled.profile_loop(bufs[0], steps, batch_size=B).values())
    looped.train_loop(bufs[1], steps, batch_size=B)
    assert profiled.fused_mode() == kind and looped.fused_mode() == kind
    assert len(ms) == 9 and all(np.isfinite(v) and v >= 0 for v in ms) and ms[8] > 0, ms
    sa, sb = profiled.state_dict(), looped.state_dict()
    assert set(sa["params"]) == {"policy", "qf1", "qf2", "target_qf1", "target_qf2"}
    for k in sa["params"]:
        assert np.array_equal(_words(sa["params"][k]), _words(sb["params"][k])), k
    for k in sa["opt"]:
        for i in range(2):
            assert np.array_equal(_words(sa["opt"][k][i]), _words(sb["opt"][k][i])), (k, i)
    assert np.array_equal(_words(sa["scalars"]), _words(sb["scalars"]))
    assert sa["scalars"][4] == steps and sa["scalars"][3] == steps


def test_the_groups_list_is_the_solo_list():
    """A, B, C, dW for SAC; TD3: the critic pass's four, then B2, C2, dW of the actor pass"""
    O, A, B = 42, 7, 32
    sac = SACTrainerGroup([make_pair(O, A, B, seed=3 + i)[1] for i in range(2)])
    assert sac.stage_count() == 4
    td3 = TD3TrainerGroup([make_td3_pair(O, A, B, seed=3 + i)[1] for i in range(2)])
    assert td3.stage_count() == 7
