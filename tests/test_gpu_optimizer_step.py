"""GPU: what a step writes back into the trainer's state -- new parameters, both Adam moments, the Polyak targets, log_alpha
and its Adam state, the counters -- per named tensor against the float64 restatement of tests/helpers.py
(check_optimizer_step), on every step path: from init, from injected states (random moments, large and TD3-split
counters, on and off the averaging period) and at non-default hyperparameters.  Then the loop's per-step tables
(bias corrections, period, policy-step plan built on the host) against the same steps taken one by one."""
import numpy as np
import pytest

from tests.helpers import check_optimizer_step, make_pair, make_td3_pair, optimizer_cfg, synth_transitions
from tests.test_gpu_step_edges import ENV, PATHS

pytestmark = pytest.mark.gpu

# every path of the step-edge tests, and one wide general shape: ragged 16-row tiles and the bias column in the
# general step's Adam epilogue
OPT_PATHS = PATHS + [("sac kind 3 wide", "sac", {}, (42, 7, 255), (513, 257), 3)]
IDS = [p[0] for p in OPT_PATHS]


def _env(path, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in path[2].items():
        monkeypatch.setenv(k, str(v))


def _trainer(path, monkeypatch, seed=5, **kw):
    label, algo, env, (O, A, B), hidden, kind = path
    _env(path, monkeypatch)
    hip = (make_pair if algo == "sac" else make_td3_pair)(O, A, B, seed=seed, hidden=hidden, **kw)[1]
    if algo == "sac":
        assert hip.fused_mode() == kind, (label, hip.fused_mode())
    elif kind is None:
        assert hip.fused_mode() == 3
    else:
        assert hip.is_fused() == kind
    return hip


def _batch(O, A, B, seed, term_frac=0.1):
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=900 + seed, term_frac=term_frac)
    rs = np.random.RandomState(1900 + seed)
    eps = (rs.normal(0, 1, (B, A)).astype(np.float32), rs.normal(0, 1, (B, A)).astype(np.float32))
    return dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs), eps


def _step(hip, path, seed):
    """One stepwise train(batch, eps=...) and the check of everything it wrote back."""
    O, A, B = path[3]
    before = hip.state_dict()
    batch, eps = _batch(O, A, B, seed)
    hip.train(batch, eps=eps if path[1] == "sac" else eps[0])
    after = hip.state_dict()
    check_optimizer_step(hip, before, after, optimizer_cfg(hip), path[0])
    return before, after


def _inject(hip, rs, adam_t, n_steps, adam_t_pi=None):
    """Random nonzero moments with v0 on the scale of g^2 (g: the last step's gradients), the counters given."""
    st = hip.state_dict()
    for net, (m, v) in st["opt"].items():
        g = hip.debug_fetch("g_" + net, m.size).astype(np.float64)
        s = np.maximum(np.abs(g), 1e-3 * np.max(np.abs(g)))
        st["opt"][net] = ((s * rs.uniform(-2, 2, m.size)).astype(np.float32),
                          (s * s * rs.uniform(0.2, 5, m.size)).astype(np.float32))
    sc = st["scalars"]
    sc[3], sc[4] = adam_t, n_steps
    if adam_t_pi is not None:
        sc[0] = adam_t_pi
    else:
        sc[1], sc[2] = rs.uniform(-0.5, 0.5), rs.uniform(0.1, 2.0)          # log_alpha's moments, float32-representable
        sc[1], sc[2] = float(np.float32(sc[1])), float(np.float32(sc[2]))
    hip.load_state_dict(st)


@pytest.mark.parametrize("path", OPT_PATHS, ids=IDS)
def test_steps_from_init(path, monkeypatch):
    hip = _trainer(path, monkeypatch)
    for s in range(1, 4):
        _step(hip, path, s)


# (adam_t, n_train_steps_total, TD3 adam_t_pi): t = 1000 on the period (SAC 5, TD3 2: a policy step), then t = 2^31 off it
INJECTED = [(999, 1000, 499), (2 ** 31 - 1, 2 ** 31 + 1, 2 ** 30 - 1)]


@pytest.mark.parametrize("path", OPT_PATHS, ids=IDS)
def test_steps_from_injected_states(path, monkeypatch):
    hip = _trainer(path, monkeypatch)
    rs = np.random.RandomState(11)
    td3 = path[1] == "td3"
    _step(hip, path, 9)                                       # (gradients to scale the injected moments by)
    for i, (t, n, tp) in enumerate(INJECTED):
        _inject(hip, rs, t, n, tp if td3 else None)
        _step(hip, path, 10 + i)
        assert (int(n) % (2 if td3 else 5) == 0) == (i == 0)


@pytest.mark.parametrize("path", OPT_PATHS, ids=IDS)
def test_tau_and_period_one(path, monkeypatch):
    kw = dict(soft_target_tau=0.3, target_update_period=1) if path[1] == "sac" else dict(tau=0.3,
                                                                                          policy_and_target_update_period=1)
    hip = _trainer(path, monkeypatch, seed=6, **kw)
    rs = np.random.RandomState(12)
    _step(hip, path, 20)
    _inject(hip, rs, 999, 1003, 998 if path[1] == "td3" else None)
    _step(hip, path, 21)


@pytest.mark.parametrize("path", [p for p in OPT_PATHS if p[0] in ("sac kind 1", "sac kind 3 deep")], ids=lambda p: p[0])
def test_fixed_alpha(path, monkeypatch):
    hip = _trainer(path, monkeypatch, seed=7, use_automatic_entropy_tuning=False)
    rs = np.random.RandomState(13)
    _step(hip, path, 30)
    _inject(hip, rs, 999, 1000)
    _step(hip, path, 31)


# ---- the loop's per-step tables -------------------------------------------------------------------------------------------
def _buffer(O, A, seed):
    from robosuite_benchmark_amd import EnvReplayBuffer
    obs, act, rew, term, nobs = synth_transitions(3000, O, A, seed=seed, term_frac=0.1)
    buf = EnvReplayBuffer(3000, obs_dim=O, action_dim=A)
    buf.add_block(obs, act, rew, nobs, term)
    buf.seed(seed + 1)
    return buf


N0 = 2 ** 32 - 3          # steps 2^32 - 3 .. 2^32 + 3: the counter crosses 2^32; 2^32 - 1 is on the SAC period (5), TD3's (2)
STEPS = 6


def _counters(hip, rs, n0, t, tp):
    st = hip.state_dict()
    for net, (m, v) in st["opt"].items():
        g = np.abs(rs.standard_normal(m.size)) * 1e-3
        st["opt"][net] = ((g * rs.uniform(-2, 2, m.size)).astype(np.float32), (g * g).astype(np.float32))
    st["scalars"][3], st["scalars"][4] = t, n0
    if hasattr(hip, "target_policy"):
        st["scalars"][0] = tp
    hip.load_state_dict(st)


def _same_state(a, b, where):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa["params"]:
        assert np.array_equal(sa["params"][k], sb["params"][k]), (where, k)
    for k in sa["opt"]:
        for x, y in zip(sa["opt"][k], sb["opt"][k]):
            assert np.array_equal(x, y), (where, "adam", k)
    assert np.array_equal(sa["scalars"], sb["scalars"]), (where, sa["scalars"], sb["scalars"])


LOOP_PATHS = [p for p in OPT_PATHS if p[0] in ("sac kind 1", "sac kind 3 deep", "td3 fused critic")]


@pytest.mark.parametrize("path", LOOP_PATHS, ids=lambda p: p[0])
def test_loop_tables_equal_stepwise_across_2_32(path, monkeypatch):
    label, algo, env, (O, A, B), hidden, kind = path
    _env(path, monkeypatch)
    make = make_pair if algo == "sac" else make_td3_pair
    loop, stepw = (make(O, A, B, seed=8, hidden=hidden, noise_seed=31)[1] for _ in range(2))
    for t in (loop, stepw):
        _counters(t, np.random.RandomState(3), N0, 2 ** 32 - 7, 2 ** 31 + 5)
    ba, bb = _buffer(O, A, 40), _buffer(O, A, 40)
    first, last = loop.train_loop(ba, STEPS, batch_size=B)
    diags = [stepw.train(bb.random_batch(B, lazy=False)) for _ in range(STEPS)]     # (host rows: diagnostics every step)
    assert np.array_equal(first, diags[0]) and np.array_equal(last, diags[-1]), label
    _same_state(loop, stepw, label)
    sc = loop.state_dict()["scalars"]
    assert sc[4] == N0 + STEPS and sc[3] == 2 ** 32 - 7 + STEPS
    if algo == "td3":                                        # policy steps at 2^32 - 2, 2^32, 2^32 + 2
        assert sc[0] == 2 ** 31 + 5 + 3


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_group_members_with_different_counters(algo, monkeypatch):
    from robosuite_benchmark_amd import SACTrainerGroup, TD3TrainerGroup
    _env(OPT_PATHS[0], monkeypatch)
    O, A, B = 42, 7, 128
    make = make_pair if algo == "sac" else make_td3_pair
    counters = [(N0, 2 ** 32 - 7, 2 ** 31 + 5), (N0 + 1, 998, 499)]            # member 1 one step out of phase
    members, twins, bufs, tbufs = [], [], [], []
    for r, c in enumerate(counters):
        for lst in (members, twins):
            t = make(O, A, B, seed=20 + r, noise_seed=50 + r)[1]
            _counters(t, np.random.RandomState(r), *c)
            lst.append(t)
        bufs.append(_buffer(O, A, 60 + r))
        tbufs.append(_buffer(O, A, 60 + r))
    group = (SACTrainerGroup if algo == "sac" else TD3TrainerGroup)(members)
    first, last = group.train_loop(bufs, STEPS, batch_size=B)
    for r, (tw, tb) in enumerate(zip(twins, tbufs)):
        f, l = tw.train_loop(tb, STEPS, batch_size=B)
        assert np.array_equal(first[r], f) and np.array_equal(last[r], l), (algo, r)
        _same_state(members[r], tw, (algo, r))

