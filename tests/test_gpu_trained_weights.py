"""GPU parity on REALISTIC weights: the trained networks of a shipped run (raw fp32 blobs of
log/runs/Lift-Panda-OSC-POSE-SEED129/*/params.pkl, tests/golden/make_trained_weights_fixture.py).
Q values are O(10-100) and the policy saturates log_std clamps and tanh -- the regime where a
relative 1e-5 on the losses is a real constraint."""
import os

import numpy as np
import pytest

from robosuite_benchmark_amd._lib import DIAG_NAMES
from tests.helpers import check_step_f64, make_pair_from_flat, rel_err, synth_transitions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_flats():
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_weights_lift_seed129.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("B,obs_scale", [(256, 1.0), (128, 0.25)])
def test_step_parity_on_trained_weights(B, obs_scale):
    O, A = 42, 7
    oracle, hip, o64 = make_pair_from_flat(load_flats(), O, A, B, with_f64=True)
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=77)
    obs, nobs = obs * obs_scale, nobs * obs_scale
    rs = np.random.RandomState(5)
    eps = (rs.normal(size=(B, A)).astype(np.float32), rs.normal(size=(B, A)).astype(np.float32))
    batch = dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32),
                 next_observations=nobs)
    want = oracle.step(obs, act, rew, term.astype(np.float32), nobs, *eps)
    got = hip.train(batch, eps=eps)
    for i, name in enumerate(DIAG_NAMES):
        assert abs(got[i] - want[name]) <= 1e-5 * max(1.0, abs(want[name])), (name, got[i], want[name])
    L = oracle.last
    # per-element: |weights| reach 39 and hidden activations O(100), so a Q value near zero is a
    # cancellation of O(100) terms -- its fp32 summation-order noise is ~1e-5 absolute
    for name, ref in (("q1", L["q1"]), ("q2", L["q2"]), ("q_target", L["y"]), ("log_pi", L["log_pi"])):
        assert rel_err(hip.debug_fetch(name, B), ref.detach().numpy().ravel()) < 1e-4, name
    assert abs(want["Q1 Predictions Mean"]) > 1.0            # really the large-magnitude regime
    # gradients, rows and statistics per tensor against float64: near-saturated tanh rows make the fp32 oracle itself
    # ill-conditioned here, the bound follows it (8x its own error)
    want64 = o64.step(obs, act, rew, term.astype(np.float32), nobs, *eps)
    check_step_f64(hip, oracle, o64, got, want, want64, path="sac trained weights")


def test_acting_path_matches_the_oracle_policy():
    """sac_policy_act (C ABI) and TanhGaussianPolicy.get_action / MakeDeterministic -- which act THROUGH it once a
    trainer owns the weights -- against oracle.PolicyNet (tanh(mean) for evaluation,
    tanh(mean + exp(clamp(log_std)) * eps) for exploration) on the trained weights of a shipped run, before and after
    a training block (the library re-mirrors the policy D2H by itself)."""
    import torch
    from robosuite_benchmark_amd import MakeDeterministic, _lib
    O, A, B = 42, 7, 64
    oracle, hip = make_pair_from_flat(load_flats(), O, A, B)
    lib = _lib.load()
    rs = np.random.RandomState(1)

    def check(policy_net):
        for _ in range(5):
            o = rs.normal(0, 0.3, O).astype(np.float32)
            with torch.no_grad():
                mean, log_std = policy_net.trunk(torch.from_numpy(o[None]))
            out = np.empty(A, np.float32)
            _lib.check(lib.sac_policy_act(hip._h, _lib.ptr(o), 1, None, _lib.ptr(out)), "sac_policy_act")
            assert np.allclose(out, torch.tanh(mean)[0].numpy(), atol=2e-5)
            eps = rs.normal(size=A).astype(np.float32)
            _lib.check(lib.sac_policy_act(hip._h, _lib.ptr(o), 0, _lib.ptr(eps), _lib.ptr(out)), "sac_policy_act")
            want = torch.tanh(mean + torch.exp(log_std) * torch.from_numpy(eps))[0].numpy()
            assert np.allclose(out, want, atol=2e-5)
            # the Python duck types: MakeDeterministic(policy).get_action(obs) / policy.get_action(obs)
            a_det, info = MakeDeterministic(hip.policy).get_action(o)
            assert info == {} and np.allclose(a_det, torch.tanh(mean)[0].numpy(), atol=2e-5)
            hip.policy._noise = np.random.RandomState(9)
            a_sto, _ = hip.policy.get_action(o)
            e9 = np.random.RandomState(9).standard_normal((1, A)).astype(np.float32)
            assert np.allclose(a_sto, torch.tanh(mean + torch.exp(log_std) * torch.from_numpy(e9))[0].numpy(), atol=2e-5)
        assert lib.sac_policy_act(hip._h, _lib.ptr(o), 0, None, _lib.ptr(out)) < 0     # stochastic needs eps

    check(oracle.policy)
    assert float(oracle.policy.trunk(torch.zeros(1, O))[1].max()) <= 2.0
    # after a training block acting follows the UPDATED policy (the library re-mirrors it by itself): the oracle's
    # forward on the parameters the device now holds
    from oracle.sac_step_torch import PolicyNet
    from tests.helpers import layers_from_flat
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=12)
    before = hip.state_dict()["params"]["policy"].copy()
    for _ in range(3):
        hip.train(dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32), next_observations=nobs))
    now = hip.state_dict()["params"]["policy"]
    assert not np.array_equal(before, now)
    check(PolicyNet(layers_from_flat(now, [(256, O), (256, 256), (A, 256), (A, 256)])))


def test_two_handles_are_independent():
    """Distinct handles on one GPU do not share state (one process may host several replicas)."""
    O, A, B = 42, 7, 64
    flats = load_flats()
    _, a = make_pair_from_flat(flats, O, A, B, noise_seed=1)
    _, b = make_pair_from_flat(flats, O, A, B, noise_seed=1)
    _, solo = make_pair_from_flat(flats, O, A, B, noise_seed=1)
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=3)
    batch = dict(observations=obs, actions=act, rewards=rew, terminals=term.astype(np.float32),
                 next_observations=nobs)
    outs = []
    for _ in range(4):                  # interleave a and b
        outs.append((a.train(batch), b.train(batch)))
    ref = [solo.train(batch) for _ in range(4)]
    for (da, db), dr in zip(outs, ref):
        assert np.array_equal(da, dr) and np.array_equal(db, dr)
