"""GPU: the inference kernels on trained-regime weights (tests/trained_states.py: the networks of a shipped run with
lagged target networks, 42/7 and inflated to 126/14; Q about -114, saturated actions, log_std on its clamp) under the
checks each kernel already has at init -- no new reference, no new bound:

  evaluate / evaluate_td3 (k_eval, k_eval_td3; with SAC_GENERAL=1 k_eval_layer, k_eval_y, k_eval_layer_td3): every column
    under helpers.check_f64 against tests/eval_reference*.py and tests/td3_eval_reference*.py; the identities of
    test_gpu_evaluate.test_bitwise_against_the_existing_entries, where tq* == q_values(..., TARGETS) now tells the target
    nets from the online ones; the device statistics (k_eval_moments, k_eval_moments_td3) within eval_stats_bound /
    td3_eval_stats_bound of the columns;
  evaluate_replay / evaluate_td3_replay (k_eval_rows): bit for bit evaluate on the gathered rows;
  param_moments (k_param_moments): the bytes of tests/param_reference.py;
  general-shape acting and Q values (k_act_layer, k_act_layer_session, k_qval_layer): helpers.check_act,
    test_gpu_q_values_general.check_against_oracle, session rows bit for bit the one-shot entry's.

Rows: 1, 17 and 256."""
import numpy as np
import pytest
import torch

from robosuite_benchmark_amd import infer
from robosuite_benchmark_amd.sac import eval_target
from tests import eval_reference, eval_reference_general, td3_eval_reference, td3_eval_reference_general
from tests import trained_states as ts
from tests.helpers import ACT_ERRORS, act_reference, check_act, make_pair, make_td3_pair, synth_transitions

pytestmark = pytest.mark.gpu
ROWS = (1, 17, 256)
TARGETS = ("target_qf1", "target_qf2")
# label, algo, environment, (ko, ka), general step
CASES = [("sac 42/7", "sac", {}, (1, 1), False), ("sac 126/14", "sac", {}, (3, 2), False),
         ("sac general", "sac", dict(SAC_GENERAL=1), (1, 1), True),
         ("td3 42/7", "td3", {}, (1, 1), False), ("td3 126/14", "td3", {}, (3, 2), False),
         ("td3 general", "td3", dict(SAC_GENERAL=1), (1, 1), True)]
IDS = [c[0] for c in CASES]
EVAL_ERRORS = {}            # label -> {column: largest |K - f64| / max|R| seen}


def trainer(case, monkeypatch):
    label, algo, env, (ko, ka), general = case
    for k in ts.ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    nets = ts.inflate(ts.trained_nets(algo), ko, ka, seed=1)
    t = (make_td3_pair if algo == "td3" else make_pair)(ts.O0 * ko, ts.A0 * ka, 32, nets=nets, noise_seed=3)[1]
    assert t.runs_general_step() == general and (t.fused_mode() == 3) == general, (label, t.fused_mode())
    return t


def inputs(case, n, seed):
    """(batch, eps): n trained rows (terminal fraction 0.1) as the tuple the references take, and the N(0, 1) draws."""
    ko, ka = case[3]
    batch = ts.trained_rows(n, ko, ka, seed, term_frac=0.1)
    rs = np.random.RandomState(seed + 7)
    A = ts.A0 * ka
    e = rs.standard_normal((n, A)).astype(np.float32), rs.standard_normal((n, A)).astype(np.float32)
    return batch, (e if case[1] == "sac" else e[0])


def bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def act_device(t, obs, det, eps):
    return (t.policy_act_general if t.runs_general_step() else t.policy_act_device)(obs, det, eps)


def evaluate(t, td3, batch, eps, **kw):
    bd = eval_reference.batch_dict(batch)
    return (t.evaluate_td3 if td3 else t.evaluate)(bd, eps=eps, rows=True, general="device", **kw)


# ---- evaluate: columns, identities, device statistics -----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_evaluate_columns_identities_and_statistics(case, monkeypatch):
    from tests.test_gpu_evaluate_stats import check as sac_stats_check
    from tests.test_gpu_td3_evaluate_stats import check as td3_stats_check
    label, algo, env, (ko, ka), general = case
    td3 = algo == "td3"
    t = trainer(case, monkeypatch)
    ref = {(False, False): eval_reference, (False, True): eval_reference_general, (True, False): td3_eval_reference,
           (True, True): td3_eval_reference_general}[(td3, general)]
    errors = EVAL_ERRORS.setdefault(label, {})
    for n in ROWS:
        batch, eps = inputs(case, n, 300 + n)
        obs, act, rew, term, nobs = batch
        stats, c = evaluate(t, td3, batch, eps, stats="device")
        ref.check_columns(c, t, batch, eps, (label, n), errors)
        # the statistics reduced on the device, within the bound of the columns' own; the columns are stats="host"'s
        h_stats, h = evaluate(t, td3, batch, eps)
        assert all(bits(c[k], h[k]) for k in ref.COLUMNS), n
        want = (td3_stats_check if td3 else sac_stats_check)(t, stats, c, (label, n))
        assert want == h_stats, n
        assert abs(stats["Q1 Predictions Mean"]) > 1.0
        # bit for bit what the other entries give; with lagged targets tq* tells the target nets from the online ones
        q = t.q_values(obs, act, general="device")
        assert bits(c["q1"], q[0]) and bits(c["q2"], q[1]), n
        r, d = rew.reshape(-1), term.reshape(-1)
        if td3:
            assert bits(c["a_pi"], act_device(t, obs, True, None)), n
            assert bits(c["q_pi"], t.q_values(obs, c["a_pi"], ("qf1",), general="device")[0]), n
            assert bits(c["a_smooth"], infer.td3_smooth(c["a_target"], eps, t.target_policy_noise, t.target_policy_noise_clip)), n
            a_next = c["a_smooth"]
            assert not bits(c["a_target"], act_device(t, nobs, True, None)), n          # the target policy, not the policy
            y = infer.td3_eval_target(r, d, c["tq1"], c["tq2"], t.reward_scale, t.discount)
        else:
            assert bits(c["a_new"], act_device(t, obs, False, eps[0])), n
            assert bits(c["a_next"], act_device(t, nobs, False, eps[1])), n
            qn = t.q_values(obs, c["a_new"], general="device")
            assert bits(c["q1_new"], qn[0]) and bits(c["q2_new"], qn[1]), n
            a_next = c["a_next"]
            y = eval_target(r, d, c["tq1"], c["tq2"], c["log_pi_next"], c["alpha"], t.reward_scale, t.discount)
        tq = t.q_values(nobs, a_next, TARGETS, general="device")
        assert bits(c["tq1"], tq[0]) and bits(c["tq2"], tq[1]), n
        online = t.q_values(nobs, a_next, general="device")
        assert not bits(tq[0], online[0]) and not bits(tq[1], online[1]), n
        assert y.dtype == np.float32 and bits(c["y"], y), n
    print(f"trained {label}: largest |K - f64| / max|R|: " + "  ".join(f"{k} {errors[k]:.3g}" for k in ref.COLUMNS))


# ---- evaluate_replay: the buffer's rows in place ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_evaluate_replay_equals_evaluate_on_the_gathered_rows(case, monkeypatch):
    from robosuite_benchmark_amd import EnvReplayBuffer
    label, algo, env, (ko, ka), general = case
    td3 = algo == "td3"
    t = trainer(case, monkeypatch)
    obs, act, rew, term, nobs = ts.trained_rows(300, ko, ka, 41, term_frac=0.1)
    buf = EnvReplayBuffer(400, obs_dim=t.obs_dim, action_dim=t.act_dim)
    buf.add_block(obs, act, rew, nobs, term)
    rs = np.random.RandomState(9)
    for n in ROWS:
        idx = rs.randint(0, 300, n)
        _, eps = inputs(case, n, 500 + n)
        for kw in (dict(), dict(stats="device")):
            if td3:
                stats, c = t.evaluate_td3_replay(buf, indices=idx, eps=eps, rows=True, general="device", **kw)
                w_stats, w = t.evaluate_td3(buf.gather(idx), eps=eps, rows=True, general="device", **kw)
                columns = td3_eval_reference.COLUMNS
            else:
                stats, c = t.evaluate_replay(buf, indices=idx, eps=eps, rows=True, general="device", **kw)
                w_stats, w = t.evaluate(buf.gather(idx), eps=eps, rows=True, general="device", **kw)
                columns = eval_reference.COLUMNS
            assert all(bits(c[k], w[k]) for k in columns), (n, kw)
            assert stats == w_stats and np.array_equal(c["indices"], idx), (n, kw)
        assert np.array_equal(buf.gather(idx)["observations"], obs[idx])
        assert abs(stats["Q1 Predictions Mean"]) > 1.0


# ---- param_moments: the trained parameters, then behind a step ---------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[3] == (1, 1)], ids=lambda c: c[0])
def test_param_moments_are_the_reference_of_the_getters(case, monkeypatch):
    from tests.param_reference import F
    from tests.test_gpu_param_moments import check
    t = trainer(case, monkeypatch)
    got = check(t, what="trained")
    assert np.max(got["policy"][:, F["absmax"]]) > 30.0                        # the fixture's weights reach 39
    assert all(np.all(got[net][:, F["gap_sumsq"]] > 0) for net in ("qf1", "qf2"))       # lagged targets: a gap in every tensor
    assert np.all(got["policy"][:, F["gap_sumsq"]] > 0) == (case[1] == "td3")
    batch, eps = ts.trained_batch(ts.O0, ts.A0, 32)
    t.train(batch, eps=eps if case[1] == "sac" else eps[0])
    got = check(t, what="trained, one step")
    assert all(np.all(got[net][:, F["m_sumsq"]] > 0) for net in ("policy", "qf1", "qf2"))


# ---- general-shape acting and Q values ---------------------------------------------------------------------------------------
GENERAL = [c for c in CASES if c[4]]
ACT_MARGIN = 2.0e-6         # rows are taken where the fp32 oracle is within this of float64 (check_act asserts 2.5e-6)


def conditioned_observations(layers, td3, n):
    """(obs, eps): the first n rows of the obs_scale = 0.25 batch of tests/test_gpu_trained_weights.py (synth_transitions
    seed 77, here 1024 rows of it) on which the fp32 oracle is within ACT_MARGIN of the float64 one, deterministic and
    stochastic.  Chosen from the two REFERENCES alone, never from a kernel's result."""
    obs = synth_transitions(1024, ts.O0, ts.A0, seed=77)[0] * np.float32(0.25)
    eps = np.random.RandomState(5).normal(size=(1024, ts.A0)).astype(np.float32)
    e = np.zeros(1024)
    for det in (True, False):
        p, r = (act_reference(layers, td3, obs, det, eps, dt) for dt in (torch.float32, torch.float64))
        e = np.maximum(e, np.max(np.abs(p - r), axis=1))
    keep = np.flatnonzero(e <= ACT_MARGIN)[:n]
    assert keep.size == n, (n, keep.size)
    return np.ascontiguousarray(obs[keep]), np.ascontiguousarray(eps[keep])


@pytest.mark.parametrize("case", GENERAL, ids=lambda c: c[0])
def test_general_acting_and_its_session(case, monkeypatch):
    """helpers.check_act first asserts that the fp32 oracle is well conditioned (8 |P - R| <= 2e-5).  On trained weights
    that fails on rows of full-scale observations (|P - R| reaches 5.5e-6 at 256 rows) and on some rows of the
    obs_scale = 0.25 batch of tests/test_gpu_trained_weights.py too (3.5e-6), so the rows are chosen FROM that batch where
    the two references agree to 2e-6 (conditioned_observations); the check itself is as it stands."""
    from tests.test_gpu_general_acting import act_g, policy_layers
    from tests.test_gpu_general_acting_session import Session, fill
    label, algo = case[0], case[1]
    t = trainer(case, monkeypatch)
    layers = policy_layers(t)
    sess = Session([t], [max(ROWS)])
    try:
        for n in ROWS:
            obs, eps = conditioned_observations(layers, algo == "td3", n)
            for det in (True, False):
                got = act_g(t, obs, det, eps, extra=2)
                check_act(t, got, layers, obs, det, eps, (label, n, "deterministic" if det else "stochastic"), tag=("trained", label))
                assert bits(got, act_device(t, obs, det, None if (det or algo == "td3") else eps)), (n, det)
                fill(sess, 0, obs.astype(np.float64), eps)
                sess.tick([n], [det])
                assert bits(sess.act[0][:n], got), (label, n, det, "session rows differ from the one-shot entry's")
            assert n == 1 or np.any(np.abs(got) > 0.999), label               # saturated actions among them
    finally:
        sess.close()
    print(f"trained {label}: largest |K - f64|, the fp32 oracle's, the call: {ACT_ERRORS.get(('trained', label))}")


@pytest.mark.parametrize("case", GENERAL, ids=lambda c: c[0])
def test_general_q_values(case, monkeypatch):
    from tests.test_gpu_q_values_general import Q_ERRORS, Q_NETS, assert_nets_differ, check_against_oracle, q_g, q_params
    label = case[0]
    t = trainer(case, monkeypatch)
    params = q_params(t)
    for n in ROWS:
        (obs, act, _, _, _), _ = inputs(case, n, 700 + n)
        got = q_g(t, obs, act, 15, extra=3)
        refs = check_against_oracle(t, params, got, Q_NETS, obs, act, "trained " + label)
        assert bits(got, t.q_values(obs, act, Q_NETS, general="device")), n
        assert abs(float(np.mean(refs[0]))) > 1.0
        if n > 1:
            assert_nets_differ(refs, (label, n))
    print(f"trained {label}: largest |K - f64| / max|R| = {Q_ERRORS['trained ' + label]:.3g}")
