"""CPU: the float64 restatement of what a step writes back (tests/helpers.py adam_ref, polyak_ref, alpha_ref and
check_optimizer_step) -- pinned to torch.optim.Adam and to rlkit's soft update in torch float32, and shown to REJECT
after-states that carry each of the mistakes the GPU tests (test_gpu_optimizer_step.py) are there to catch."""
import numpy as np
import pytest
import torch

from tests.helpers import (U32, _f, adam_param_ref, adam_ref, adam_scalars, alpha_ref, check_optimizer_step,
                           named_tensors, polyak_ref, ulp32)

# torch keeps Adam's `step` as a float32 tensor and adds 1 in float32: the count it applies after a stored step s
STEPS = [0, 1, 9, 999, 2 ** 31 - 1, 2 ** 32 + 4]


def _applied_t(s):
    return float(np.float32(np.float32(s) + np.float32(1)))


def _grads(rs, n, scale=1e-3):
    """Gradient-like values: signed, over five decades, a few exact zeros."""
    g = rs.standard_normal(n) * scale * 10.0 ** rs.uniform(-3, 1, n)
    g[rs.rand(n) < 0.02] = 0.0
    return g.astype(np.float32)


@pytest.mark.parametrize("s", STEPS)
@pytest.mark.parametrize("injected", [False, True])
def test_adam_ref_matches_torch_adam(s, injected):
    rs = np.random.RandomState(s % 1000 + 7 * injected)
    n, lr = 4096, 1e-3
    p0 = (rs.standard_normal(n) * 0.05).astype(np.float32)
    g = _grads(rs, n)
    if injected:
        m0 = (g * rs.uniform(-2, 2, n)).astype(np.float32)
        v0 = (g.astype(np.float64) ** 2 * rs.uniform(0.2, 5, n)).astype(np.float32)
    else:
        m0 = v0 = np.zeros(n, np.float32)
    w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([w], lr=lr)
    w.grad = torch.from_numpy(g.copy())
    if injected or s:
        opt.state[w] = {"step": torch.tensor(float(s)), "exp_avg": torch.from_numpy(m0.copy()),
                        "exp_avg_sq": torch.from_numpy(v0.copy())}
    opt.step()
    st = opt.state[w]
    t = _applied_t(s)
    assert float(st["step"]) == t
    P, M, V = w.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
    pr, mr, vr = adam_ref(p0, m0, v0, g, lr, t)
    c1 = adam_scalars(lr, t)[0]
    assert np.all(np.abs(M - mr) <= 2 * ulp32(mr) + 2 * U32 * np.abs(c1 * (g.astype(np.float64) - m0))), "exp_avg"
    assert np.all(np.abs(V - vr) <= 2 * ulp32(vr)), "exp_avg_sq"
    # the parameter from torch's own moments (as check_optimizer_step takes it from the kernel's)
    pr2, d = adam_param_ref(p0, M, V, lr, t)
    assert np.all(np.abs(P - pr2) <= ulp32(pr2) + 6 * U32 * np.abs(d)), "param"
    # and from the reference's moments, at the same bound plus what the moments' own roundings move the update
    assert np.all(np.abs(P - pr) <= ulp32(pr) + 12 * U32 * np.abs(d)), "param (float64 moments)"


@pytest.mark.parametrize("tau", [0.005, 0.01, 0.3, 1.0])
def test_polyak_ref_matches_rlkit_soft_update(tau):
    rs = np.random.RandomState(int(tau * 1000))
    t_old = (rs.standard_normal(8192) * 0.05).astype(np.float32)
    p_new = (t_old + rs.standard_normal(8192) * 1e-3).astype(np.float32)
    tgt, src = torch.from_numpy(t_old.copy()), torch.from_numpy(p_new)
    tgt.copy_(tgt * (1.0 - tau) + src * tau)              # rlkit.torch.pytorch_util.soft_update_from_to
    r = polyak_ref(t_old, p_new, tau)
    b = ulp32(r) + 2 * U32 * (np.abs(t_old * _f(1 - tau)) + np.abs(p_new * _f(tau)))
    assert np.all(np.abs(tgt.numpy() - r) <= b)
    if tau == 1.0:
        assert np.array_equal(r, p_new)


def test_alpha_ref_matches_torch():
    rs = np.random.RandomState(3)
    B, H = 255, -7.0
    lp = (rs.standard_normal(B) * 2 - 3).astype(np.float32)
    la = torch.nn.Parameter(torch.tensor(-0.37))
    opt = torch.optim.Adam([la], lr=1e-3)
    opt.state[la] = {"step": torch.tensor(999.0), "exp_avg": torch.tensor(0.21), "exp_avg_sq": torch.tensor(0.05)}
    loss = -(la * (torch.from_numpy(lp) + H).detach()).mean()
    loss.backward()
    opt.step()
    st = opt.state[la]
    r_la, r_m, r_v, gr = alpha_ref(-0.37, float(np.float32(0.21)), float(np.float32(0.05)), lp, H, 1e-3, 1000)
    assert abs(float(la.grad) - gr) <= (B + 4) * U32 * (np.mean(np.abs(lp)) + abs(H))
    assert abs(float(st["exp_avg"]) - r_m) <= 1e-6 * abs(r_m)
    assert abs(float(st["exp_avg_sq"]) - r_v) <= 1e-6 * abs(r_v)
    assert abs(float(la.detach()) - r_la) <= 2 * float(ulp32(r_la))


# ---- check_optimizer_step on synthetic states ---------------------------------------------------------------------------
O, A, HID = 5, 3, (20, 12)


def _cfg(td3, **over):
    pol = [(HID[0], O), (HID[1], HID[0]), (A, HID[1])] + ([] if td3 else [(A, HID[1])])
    q = [(HID[0], O + A), (HID[1], HID[0]), (1, HID[1])]
    pn = ["fc0", "fc1", "last_fc"] + ([] if td3 else ["last_fc_log_std"])
    qn = ["fc0", "fc1", "last_fc"]
    cfg = dict(td3=td3, nets={"policy": (pol, pn), "qf1": (q, qn), "qf2": (q, qn)}, B=37,
               lr={"policy": 1e-3, "qf1": 5e-4, "qf2": 5e-4}, tau=0.005, period=2 if td3 else 5,
               targets={"target_qf1": "qf1", "target_qf2": "qf2"})
    if td3:
        cfg["targets"]["target_policy"] = "policy"
    else:
        cfg.update(auto_alpha=True, target_entropy=-float(A), alpha_lr=1e-3)
    cfg.update(over)
    return cfg


class FakeTrainer:
    """debug_fetch of the step's gradients and log_pi rows, as a trainer's after train()."""

    def __init__(self, fetch):
        self.fetch = fetch

    def debug_fetch(self, name, n):
        x = self.fetch[name]
        assert x.size == n, (name, x.size, n)
        return x


def _size(shapes):
    return sum(a * b + a for a, b in shapes)


def _before(cfg, rs, adam_t, n_steps, adam_t_pi=0, zero_moments=False):
    st = dict(params={}, opt={})
    for net, (shapes, _) in cfg["nets"].items():
        n = _size(shapes)
        st["params"][net] = (rs.standard_normal(n) * 0.1).astype(np.float32)
        g = _grads(rs, n)
        st["opt"][net] = ((np.zeros(n, np.float32), np.zeros(n, np.float32)) if zero_moments else
                          ((g * rs.uniform(-2, 2, n)).astype(np.float32),
                           (g.astype(np.float64) ** 2 * rs.uniform(0.2, 5, n)).astype(np.float32)))
    for tgt, src in cfg["targets"].items():
        p = st["params"][src]
        st["params"][tgt] = (p + rs.standard_normal(p.size) * 1e-2).astype(np.float32)
    if cfg["td3"]:
        st["scalars"] = np.array([adam_t_pi, 0, 0, adam_t, n_steps, 0], np.float64)
    else:
        la = np.float32(-0.3)
        st["scalars"] = np.array([la, np.float32(0.0 if zero_moments else 0.4),
                                  np.float32(0.0 if zero_moments else 0.9), adam_t, n_steps, np.exp(la)], np.float64)
    return st


def _fetch(cfg, rs):
    f = {"g_" + net: _grads(rs, _size(shapes)) for net, (shapes, _) in cfg["nets"].items()}
    f["log_pi"] = (rs.standard_normal(cfg["B"]) - 1.0).astype(np.float32)
    return f


def _adam32(p, m, v, g, lr, t, eps_inside=False, bc2_t=None):
    """One Adam step in float32 arithmetic as the kernels write it (adam_update), with the mutants' knobs."""
    f = np.float32
    m = (m + f(0.1) * (g - m)).astype(f)
    v = (v * f(0.999) + f(0.001) * g * g).astype(f)
    ss, bc2s = f(lr / (1.0 - 0.9 ** t)), f(np.sqrt(1.0 - 0.999 ** (t if bc2_t is None else bc2_t)))
    with np.errstate(divide="ignore", invalid="ignore"):          # (bc2s from t - 1 is 0 at the first step)
        denom = np.sqrt(v + f(1e-8)) / bc2s if eps_inside else np.sqrt(v) / bc2s + f(1e-8)
        return (p + (-ss * m) / denom).astype(f), m, v


def _after(cfg, before, fetch, mut=None):
    """The state a correct step leaves -- or one with mistake `mut` in it."""
    f = np.float32
    sb = before["scalars"]
    n0, t0 = int(sb[4]), int(sb[3])
    avg = n0 % cfg["period"] == 0
    td3 = cfg["td3"]
    tp = int(sb[0]) + 1 if td3 else t0 + 1
    if mut == "td3_policy_adam_t":
        tp = t0 + 1
    after = dict(params={k: v.copy() for k, v in before["params"].items()},
                 opt={k: (m.copy(), v.copy()) for k, (m, v) in before["opt"].items()}, scalars=sb.copy())
    trained = ["qf1", "qf2"] + (["policy"] if (avg or not td3 or mut == "td3_policy_every_step") else [])
    for net in trained:
        t = tp if net == "policy" else t0 + 1
        if mut == "t_off_by_one":
            t -= 1
        p, m, v = _adam32(before["params"][net], *before["opt"][net], fetch["g_" + net], cfg["lr"][net], t,
                          eps_inside=mut == "eps_inside_sqrt", bc2_t=t - 1 if mut == "bc2s_from_t_minus_1" else None)
        shapes, names = cfg["nets"][net]
        for x, x0 in ((p, before["params"][net]), (m, before["opt"][net][0]), (v, before["opt"][net][1])):
            X, X0 = named_tensors(x, shapes, names, net), named_tensors(x0, shapes, names, net)
            for k in X:
                if mut == "bias_skipped" and k.endswith(".bias"):
                    X[k][...] = X0[k]
                if mut == "ragged_tile_skipped" and k == f"{net} fc0.weight":
                    X[k][16:] = X0[k][16:]                 # rows 16-19: the second, ragged 16-row tile
        after["params"][net] = p
        after["opt"][net] = (m, v)
    for tgt, src in cfg["targets"].items():
        if src not in trained or not (avg or mut == "target_every_step"):
            continue
        pn = before["params"][src] if mut == "polyak_pre_update" else after["params"][src]
        after["params"][tgt] = (before["params"][tgt] * f(1 - cfg["tau"]) + pn * f(cfg["tau"])).astype(f)
    after["scalars"][3] += 1
    after["scalars"][4] += 1
    if td3:
        after["scalars"][0] += 1 if avg else 0
        return after
    if cfg["auto_alpha"]:
        la, am, av = (f(x) for x in sb[:3])
        rows = cfg["B"] + 11 if mut == "alpha_padded_rows" else cfg["B"]
        gr = -(f(np.sum(fetch["log_pi"], dtype=f) / f(rows)) + f(cfg["target_entropy"]))
        if mut == "alpha_grad_doubled":
            gr = f(2) * gr
        t = t0 + 1
        am = f(am + f(0.1) * (gr - am))
        av = f(av * f(0.999) + f(0.001) * gr * gr)
        denom = f(np.sqrt(av) / f(np.sqrt(1.0 - 0.999 ** t)) + f(1e-8))
        la_new = f(la + (-f(cfg["alpha_lr"] / (1.0 - 0.9 ** t)) * am) / denom)
        after["scalars"][:3] = (la_new, am, av)
        after["scalars"][5] = np.exp(la if mut == "alpha_pre_step" else la_new).astype(f)
    else:
        after["scalars"][5] = 1.0
    return after


SAC_STATES = {"init": dict(adam_t=0, n_steps=0, zero_moments=True), "t1000 on period": dict(adam_t=999, n_steps=1000),
              "t2^31 off period": dict(adam_t=2 ** 31 - 1, n_steps=2 ** 31 + 1)}
TD3_STATES = {"init": dict(adam_t=0, n_steps=0, zero_moments=True),
              "policy step": dict(adam_t=999, n_steps=1000, adam_t_pi=499),
              "critic-only step": dict(adam_t=2 ** 31 - 1, n_steps=2 ** 31 + 1, adam_t_pi=2 ** 30 - 1)}


def _case(td3, state, seed=0, **over):
    cfg = _cfg(td3, **over)
    rs = np.random.RandomState(seed)
    before = _before(cfg, rs, **(TD3_STATES if td3 else SAC_STATES)[state])
    fetch = _fetch(cfg, rs)
    return cfg, before, fetch


@pytest.mark.parametrize("td3,state", [(False, s) for s in SAC_STATES] + [(True, s) for s in TD3_STATES])
def test_correct_step_is_accepted(td3, state):
    cfg, before, fetch = _case(td3, state)
    check_optimizer_step(FakeTrainer(fetch), before, _after(cfg, before, fetch), cfg, "synthetic")


def test_fixed_alpha_and_zero_lr_are_accepted():
    cfg, before, fetch = _case(False, "t1000 on period", auto_alpha=False, lr={"policy": 0.0, "qf1": 5e-4, "qf2": 5e-4})
    after = _after(cfg, before, fetch)
    assert np.array_equal(after["params"]["policy"], before["params"]["policy"])
    check_optimizer_step(FakeTrainer(fetch), before, after, cfg, "synthetic")


# mistake -> the states where it must be seen (SAC / TD3)
MUTANTS = [("polyak_pre_update", False, "t1000 on period"), ("polyak_pre_update", True, "policy step"),
           ("td3_policy_adam_t", True, "policy step"), ("td3_policy_every_step", True, "critic-only step"),
           ("bc2s_from_t_minus_1", False, "init"), ("bc2s_from_t_minus_1", False, "t1000 on period"),
           ("bc2s_from_t_minus_1", True, "policy step"), ("t_off_by_one", False, "t1000 on period"),
           ("eps_inside_sqrt", False, "init"), ("eps_inside_sqrt", True, "critic-only step"),
           ("bias_skipped", False, "init"), ("bias_skipped", True, "policy step"),
           ("ragged_tile_skipped", False, "t2^31 off period"), ("target_every_step", False, "t2^31 off period"),
           ("target_every_step", True, "critic-only step"), ("alpha_padded_rows", False, "init"),
           ("alpha_padded_rows", False, "t1000 on period"), ("alpha_grad_doubled", False, "t2^31 off period"),
           ("alpha_pre_step", False, "t1000 on period")]


@pytest.mark.parametrize("mut,td3,state", MUTANTS, ids=[f"{m}-{'td3' if t else 'sac'}-{s}" for m, t, s in MUTANTS])
def test_each_mistake_is_rejected(mut, td3, state):
    cfg, before, fetch = _case(td3, state)
    with pytest.raises(AssertionError):
        check_optimizer_step(FakeTrainer(fetch), before, _after(cfg, before, fetch, mut), cfg, "synthetic")


def test_exact_cases_are_exact():
    """A last-bit change where g == m0 == v0 == 0, or of the parameters at lr 0, is refused though inside the ulp bound."""
    cfg, before, fetch = _case(False, "init")
    fetch["g_qf1"][:50] = 0.0
    after = _after(cfg, before, fetch)
    after["params"]["qf1"][3] = np.nextafter(after["params"]["qf1"][3], np.float32(1))
    with pytest.raises(AssertionError, match="bit-unchanged"):
        check_optimizer_step(FakeTrainer(fetch), before, after, cfg, "synthetic")
    cfg, before, fetch = _case(False, "t1000 on period", lr={"policy": 1e-3, "qf1": 0.0, "qf2": 5e-4})
    after = _after(cfg, before, fetch)
    after["params"]["qf1"][-1] = np.nextafter(after["params"]["qf1"][-1], np.float32(1))
    with pytest.raises(AssertionError, match="lr 0"):
        check_optimizer_step(FakeTrainer(fetch), before, after, cfg, "synthetic")
