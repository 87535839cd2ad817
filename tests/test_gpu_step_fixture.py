"""GPU: every step path held to the frozen float64 steps of tests/golden/step_fixtures.npz.  Per case of
tests/step_fixture_cases.py and per path that takes its shape: a trainer, the case uploaded through load_state_dict (nets,
Adam moments, scalars), one train(batch, eps=...), and what it computed and wrote back against the FILE under the rule of
tests/test_step_fixture_host.py hold_to_fixture -- diagnostics, per-row outputs, every gradient tensor, and for the narrow
cases the update of every parameter and target tensor, both Adam moments, log_alpha and its moments; the counters and
what a case leaves unchanged exactly.  No oracle runs here: a reference computed now could follow the code under test.
tests/test_step_fixture_host.py holds the oracles to the same file on the CPU."""
import numpy as np
import pytest

from tests import step_fixture_cases as cases
from tests.test_gpu_step_edges import ENV, PATHS
from tests.test_step_fixture_host import WORST, case, fixture, hold_to_fixture

pytestmark = pytest.mark.gpu

_ENV_OF = {p[0]: p[2] for p in PATHS}
# label -> (environment, SAC: fused_mode(); TD3: is_fused(), None: the general step)
SAC_NARROW = {"sac kind 1": (_ENV_OF["sac kind 1"], 1), "sac kind 0": (_ENV_OF["sac kind 0"], 0),
              "sac kind 3": (_ENV_OF["sac kind 3"], 3)}
TD3_NARROW = {"td3 fused critic": (_ENV_OF["td3 fused critic"], True),
              "td3 four-launch critic": (_ENV_OF["td3 four-launch critic"], False),
              "td3 general": (_ENV_OF["sac kind 3"], None)}
# (34 row-blocks: without the fused launch the plan still chains -- SAC_CHAIN=0 gives the four launches)
CHAINED = {"sac kind 2": (_ENV_OF["sac kind 2"], 2), "sac kind 4": (_ENV_OF["sac kind 4"], 4),
           "sac kind 0": (dict(_ENV_OF["sac kind 0"], SAC_CHAIN=0), 0)}
RUNS = ([(n, l, *v) for n in ("sac on-period", "sac off-period", "sac early", "sac fixed alpha") for l, v in SAC_NARROW.items()]
        + [(n, l, *v) for n in ("td3 policy step", "td3 critic step") for l, v in TD3_NARROW.items()]
        + [("sac chained", l, *v) for l, v in CHAINED.items()]
        + [("sac deep", "sac kind 3 native", {}, 3), ("td3 deep", "td3 general native", {}, None)]
        # the full-size cases on their default plan
        + [("lift full", "default plan", {}, 1), ("door full", "default plan", {}, 4), ("twoarmlift full", "default plan", {}, 1),
           ("td3 lift full", "default plan", {}, True)])
assert {r[0] for r in RUNS} == set(cases.NAMES)


def _trainer(c):
    from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy, TanhMlpPolicy, TD3Trainer
    qs = {n: FlattenMlp(list(c.hidden_q), 1, c.O + c.A) for n in ("qf1", "qf2", "target_qf1", "target_qf2")}
    if c.td3:
        pols = dict(policy=TanhMlpPolicy(list(c.hidden), c.A, c.O), target_policy=TanhMlpPolicy(list(c.hidden), c.A, c.O))
        hip = TD3Trainer(batch_size=c.B, device=0, noise_seed=0, **pols, **qs, **c.kw)
    else:
        hip = SACTrainer(policy=TanhGaussianPolicy(list(c.hidden), c.O, c.A), batch_size=c.B, device=0, noise_seed=0, **qs,
                         **c.kw)
    hip.load_state_dict(dict(params={n: c.params[n].copy() for n in c.nets},
                             opt={n: (m.copy(), v.copy()) for n, (m, v) in c.opt.items()}, scalars=c.scalars.copy()))
    return hip


@pytest.mark.parametrize("name,label,env,kind", RUNS, ids=[f"{r[0]}-{r[1]}" for r in RUNS])
def test_step_against_the_frozen_fixture(name, label, env, kind, monkeypatch):
    from robosuite_benchmark_amd._lib import DIAG_NAMES, TD3_DIAG_NAMES
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    c, fx = case(name), fixture()
    assert dict(c.checksums()) == fx.meta["cases"][name]["inputs"], "the inputs are not the ones the file was computed from"
    hip = _trainer(c)
    if not c.td3:
        assert hip.fused_mode() == kind, (label, hip.fused_mode())
    elif kind is None:
        assert hip.fused_mode() == 3, (label, hip.fused_mode())
    else:
        assert hip.is_fused() == kind, (label, hip.fused_mode())
    diag = hip.train(c.train_batch(), eps=c.eps[0] if c.td3 else c.eps)
    names = TD3_DIAG_NAMES if c.td3 else DIAG_NAMES
    wide = ("a_new", "mu", "log_std", "a_next")
    got = dict(diag={n: float(diag[i]) for i, n in enumerate(names)},
               rows={n: hip.debug_fetch(n, c.B * (c.A if n in wide else 1)) for n in cases.ROW_NAMES[c.algo]},
               grads={net: hip.debug_fetch("g_" + net, c.count(net)) for net in c.stepped()})
    for n, x in got["rows"].items():
        assert x.size == c.B * (c.A if n in wide else 1), (n, x.size)
    after = hip.state_dict()
    got.update(params=after["params"], opt=after["opt"], scalars=after["scalars"])
    path = f"{label} | {name}"
    hold_to_fixture(c, fx, got, path)
    rows = cases.terminal_rows(c)               # a terminal row bootstraps nothing: y = reward_scale * r, exactly
    want = (np.float32(c.kw["reward_scale"]) * c.batch["rewards"].ravel()[rows]).astype(np.float32)
    assert rows.size and np.array_equal(got["rows"]["q_target"][rows], want), (path, "terminal rows")
    frac, tensor = WORST[path]
    print(f"STEP FIXTURE {path}: largest kernel error {frac:.3f} of its bound ({tensor})")
