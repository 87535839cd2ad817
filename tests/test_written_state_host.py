"""Host: the recipe of tests/written_state.py oracles_from_state is exact, and its checkers see what they must.

An oracle takes 6 steps; its state leaves it as plain numbers -- flat float32 vectors in the library's layout and Python
floats, the shape of a trainer's state_dict(), nothing cloned -- and a float32 oracle rebuilt from them takes the 7th step
bit for bit as the continued one does: every diagnostic, every gradient, every per-row output.  Without log_alpha's Adam
state (SAC) or qf1's (TD3) it does not, so a reference rebuilt from a trainer's state carries everything that enters the
compared step, and nothing is compared along two trajectories."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.sac_step_torch import RlkitEquivalentSAC, init_sac_params
from oracle.td3_step_torch import RlkitEquivalentTD3, init_td3_params
from tests.helpers import SAC_ROWS, TD3_ROWS, flat_of, oracle_flat_grad, synth_transitions
from tests.written_state import copy_differences, oracles_from_state, pad_labels, pad_report

SAC_KW = dict(policy_lr=1e-3, qf_lr=5e-4, soft_target_tau=0.005, target_update_period=5)
TD3_KW = dict(policy_learning_rate=1e-3, qf_learning_rate=5e-4, policy_and_target_update_period=2, tau=0.005)
# (O, A, B), hidden, hidden_q
SHAPES = [((42, 7, 48), (256, 256), None), ((13, 3, 33), (24, 40), (7, 31))]


def _batch(B, O, A, seed, td3):
    obs, act, rew, term, nobs = synth_transitions(B, O, A, seed=seed, term_frac=0.1)
    rs = np.random.RandomState(seed + 1)
    eps = [rs.normal(0, 1, (B, A)).astype(np.float32) for _ in range(1 if td3 else 2)]
    return (obs, act, rew, term.astype(np.float32), nobs, *eps)


def _holder(hidden):
    return SimpleNamespace(hidden_sizes=list(hidden))


def _moments(opt, net):
    """An oracle net's Adam moments as two flat float32 vectors in library layout (W0 b0 W1 b1 ...)."""
    def flat(key):
        return np.concatenate([np.concatenate([opt.state[w][key].detach().numpy().ravel(),
                                               opt.state[b][key].detach().numpy().ravel()])
                               for w, b in zip(net.ws, net.bs)]).astype(np.float32)
    return flat("exp_avg"), flat("exp_avg_sq")


def _exported(o, O, A, B, hidden, hidden_q, td3):
    """(a stand-in for the trainer: the host attributes optimizer_cfg and oracles_from_state read; the oracle's state in
    the form of state_dict())."""
    nets = o.export_nets()
    params = {k: flat_of(v) for k, v in nets.items()}
    opt = {k: _moments(getattr(o, k + "_opt"), getattr(o, k)) for k in ("policy", "qf1", "qf2")}
    t_q = int(o.qf1_opt.state[o.qf1.ws[0]]["step"])
    if td3:
        t_pi = int(o.policy_opt.state[o.policy.ws[0]]["step"])
        scalars = [float(t_pi), 0.0, 0.0, float(t_q), float(o.n_train_steps_total), 0.0]
        hip = SimpleNamespace(obs_dim=O, act_dim=A, _batch=B, policy=_holder(hidden), qf1=_holder(hidden_q or hidden),
                              target_policy=_holder(hidden), target_policy_noise=o.noise, target_policy_noise_clip=o.clip,
                              discount=o.discount, reward_scale=o.reward_scale,
                              policy_learning_rate=TD3_KW["policy_learning_rate"], qf_learning_rate=TD3_KW["qf_learning_rate"],
                              policy_and_target_update_period=o.period, tau=o.tau)
    else:
        st = o.alpha_opt.state[o.log_alpha]
        assert int(st["step"]) == t_q
        scalars = [float(o.log_alpha.detach()), float(st["exp_avg"]), float(st["exp_avg_sq"]), float(t_q),
                   float(o.n_train_steps_total), float(o.log_alpha.detach().exp())]
        hip = SimpleNamespace(obs_dim=O, act_dim=A, _batch=B, policy=_holder(hidden), qf1=_holder(hidden_q or hidden),
                              discount=o.discount, reward_scale=o.reward_scale, policy_lr=SAC_KW["policy_lr"],
                              qf_lr=SAC_KW["qf_lr"], soft_target_tau=o.tau, target_update_period=o.period,
                              use_automatic_entropy_tuning=True, target_entropy=o.target_entropy)
    return hip, dict(params=params, opt=opt, scalars=np.asarray(scalars, np.float64))


def _seventh_steps(algo, shape, with_optimizer_state=True):
    (O, A, B), hidden, hidden_q = shape
    td3 = algo == "td3"
    if td3:
        o = RlkitEquivalentTD3(init_td3_params(O, A, hidden=hidden, seed=3), A, **TD3_KW)
    else:
        o = RlkitEquivalentSAC(init_sac_params(O, A, hidden=hidden, seed=3, hidden_q=hidden_q), A, **SAC_KW)
    for s in range(6):
        o.step(*_batch(B, O, A, 100 + s, td3))
    hip, state = _exported(o, O, A, B, hidden, None if td3 else hidden_q, td3)
    r32, r64 = oracles_from_state(hip, state, with_optimizer_state=with_optimizer_state)
    x = _batch(B, O, A, 200, td3)
    return o, o.step(*x), r32, r32.step(*x), r64, r64.step(*x)


def _differences(o, d, r, dr, td3):
    """Names of the diagnostics, gradients and per-row outputs of the last step that differ between two oracles."""
    out = [k for k in d if not (d[k] == dr[k] or (np.isnan(d[k]) and np.isnan(dr[k])))]
    for k in ("g_policy", "g_qf1", "g_qf2"):
        if o.last[k] is None and r.last[k] is None:
            continue
        if copy_differences(oracle_flat_grad(o.last[k]), oracle_flat_grad(r.last[k])).size:
            out.append(k)
    for key in (TD3_ROWS if td3 else SAC_ROWS).values():
        if copy_differences(o.last[key].detach().numpy(), r.last[key].detach().numpy()).size:
            out.append(key)
    return out


# (TD3's oracle builds all nets at one hidden size)
REBUILT = [("sac", s) for s in SHAPES] + [("td3", SHAPES[0]), ("td3", (SHAPES[1][0], SHAPES[1][1], None))]


@pytest.mark.parametrize("algo,shape", REBUILT, ids=[f"{a}-{'x'.join(map(str, s[0]))}" for a, s in REBUILT])
def test_the_rebuilt_oracle_takes_the_seventh_step_bit_for_bit(algo, shape):
    o, d, r32, d32, r64, d64 = _seventh_steps(algo, shape)
    assert o.n_train_steps_total == r32.n_train_steps_total == r64.n_train_steps_total == 7
    assert d.keys() == d32.keys() == d64.keys()
    assert _differences(o, d, r32, d32, algo == "td3") == []
    if algo == "td3":
        assert o.last["policy_step"] and o.last["g_policy"] is not None         # step 6 is a policy step (period 2)
    # the float64 twin of the same state: the same step to float32 accuracy, not another trajectory
    for k in ("g_qf1", "g_qf2", "g_policy"):
        g, h = oracle_flat_grad(r32.last[k]).astype(np.float64), oracle_flat_grad(r64.last[k])
        assert np.max(np.abs(g - h)) <= 1e-5 * np.max(np.abs(h)), k
    assert r64.last["q1"].dtype == torch.float64


def test_without_log_alphas_adam_state_the_sac_step_differs():
    o, d, r32, d32, _, _ = _seventh_steps("sac", SHAPES[0], with_optimizer_state=False)
    diff = _differences(o, d, r32, d32, False)
    assert "Alpha" in diff and "g_policy" in diff and "y" in diff, diff


def test_without_qf1s_adam_state_the_td3_policy_step_differs():
    o, d, r32, d32, _, _ = _seventh_steps("td3", SHAPES[0], with_optimizer_state=False)
    diff = _differences(o, d, r32, d32, True)
    assert "g_policy" in diff and "q_pi" in diff, diff
    assert "g_qf1" not in diff and "g_qf2" not in diff                         # (the critic pass reads no optimizer state)


# ---- the checkers on synthetic arrays ------------------------------------------------------------------------------------
def test_copy_differences_compares_bit_patterns():
    a = np.array([1.0, -0.0, np.nan, 3.0, np.inf], np.float32)
    assert copy_differences(a, a.copy()).size == 0                              # (a NaN is its own copy)
    b = a.copy()
    b[1] = 0.0                                                                  # -0 -> +0: equal as numbers, not as copies
    b[3] = np.nextafter(np.float32(3.0), np.float32(4.0))                       # one ulp
    assert copy_differences(a, b).tolist() == [1, 3]
    with pytest.raises(AssertionError):
        copy_differences(a, a[:-1])


@pytest.mark.parametrize("td3,general,n", [(False, False, 14), (True, False, 15), (False, True, 11), (True, True, 12)])
def test_pad_report_names_the_array_of_each_count(td3, general, n):
    labels = pad_labels(td3, general)
    assert len(labels) == n == len(set(labels))
    assert labels[0] == "policy P" and labels[-1] == ("target_policy P" if td3 else "target_qf2 P")
    assert labels[1] == ("policy M" if general else "policy PT")
    assert pad_report(np.zeros(n, np.float32), td3, general) == {}
    counts = np.zeros(n, np.float32)
    counts[5], counts[n - 2] = 3, np.nan                                        # (a count that is not a number is not zero)
    bad = pad_report(counts, td3, general)
    assert list(bad) == [labels[5], labels[n - 2]]
    assert labels[5] == ("qf1 V" if general else "qf1 PT")
    with pytest.raises(AssertionError):
        pad_report(np.zeros(n + 1, np.float32), td3, general)
