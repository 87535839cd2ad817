"""Shared helpers for the parity tests (test infrastructure; may import oracle/)."""
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle.sac_step_torch import RlkitEquivalentSAC, init_sac_params

TASK_DIMS = {"Lift": (42, 7), "Door": (46, 7), "Stack": (55, 7), "TwoArmLift": (89, 14), "Wipe": (379, 6),
             "TwoArmPegInHole": (73, 12), "TwoArmHandoff": (86, 14), "PickPlaceCan": (46, 7),
             "NutAssemblyRound": (46, 7), "LiftModded": (64, 4), "LiftJaco": (50, 4), "WipeJV": (379, 7)}


def synth_transitions(n, O, A, seed=1234, term_frac=0.0, reward_scale=1.0):
    """SURVEY.md section 8d synthetic data: obs ~ N(0, .5^2), act ~ U(-1,1), rew ~ U(0,1)."""
    rs = np.random.RandomState(seed)
    obs = rs.normal(0, 0.5, (n, O)).astype(np.float32)
    nobs = rs.normal(0, 0.5, (n, O)).astype(np.float32)
    act = rs.uniform(-1, 1, (n, A)).astype(np.float32)
    rew = (rs.uniform(0, 1, (n, 1)) * reward_scale).astype(np.float32)
    term = (rs.uniform(0, 1, (n, 1)) < term_frac).astype(np.uint8)
    return obs, act, rew, term, nobs


def flat_of(layers):
    return np.concatenate([np.concatenate([w.ravel(), b.ravel()]) for w, b in layers]).astype(np.float32)


def make_pair(O, A, B, seed=3, device=0, with_f64=False, nets=None, **kw):
    """An oracle and a HIP trainer holding identical parameters (with_f64: and the oracle's float64 twin, third;
    nets: these parameters instead of init_sac_params', at the sizes `hidden` / `hidden_q` name)."""
    from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy
    kw.setdefault("policy_lr", 1e-3)
    kw.setdefault("qf_lr", 5e-4)
    kw.setdefault("soft_target_tau", 0.005)
    kw.setdefault("target_update_period", 5)
    hidden, hidden_q = tuple(kw.pop("hidden", (256, 256))), kw.pop("hidden_q", None)
    hidden_q = tuple(hidden_q) if hidden_q else hidden
    nets = nets or init_sac_params(O, A, hidden=hidden, seed=seed, hidden_q=hidden_q)
    noise_seed = kw.pop("noise_seed", 0)
    oracle = RlkitEquivalentSAC(nets, A, **kw)
    twin = RlkitEquivalentSAC(nets, A, dtype=torch.float64, **kw) if with_f64 else None
    pol = TanhGaussianPolicy(list(hidden), O, A)
    qs = [FlattenMlp(list(hidden_q), 1, O + A) for _ in range(4)]
    pol.load_flat(flat_of(nets["policy"]))
    for q, name in zip(qs, ("qf1", "qf2", "target_qf1", "target_qf2")):
        q.load_flat(flat_of(nets[name]))
    hip = SACTrainer(policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], batch_size=B,
                     device=device, noise_seed=noise_seed, **kw)
    return (oracle, hip, twin) if with_f64 else (oracle, hip)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def layers_from_flat(flat, shapes):
    """flat nn.Linear vector (W, b per layer) -> [(W, b), ...] for the oracle."""
    out, off = [], 0
    for (n, k) in shapes:
        w = np.asarray(flat[off:off + n * k], np.float32).reshape(n, k).copy(); off += n * k
        b = np.asarray(flat[off:off + n], np.float32).copy(); off += n
        out.append((w, b))
    assert off == len(flat)
    return out


def make_pair_from_flat(flats, O, A, B, device=0, with_f64=False, **kw):
    """Oracle + HIP trainer from flat parameter vectors {policy, qf1, qf2[, target_qf1, target_qf2]} (with_f64: and the
    oracle's float64 twin, third).  Without targets in `flats` the target nets ALIAS the critics; tests/trained_states.py
    is the variant with distinct (lagged) ones."""
    from collections import OrderedDict
    from robosuite_benchmark_amd import FlattenMlp, SACTrainer, TanhGaussianPolicy
    kw.setdefault("policy_lr", 1e-3)
    kw.setdefault("qf_lr", 5e-4)
    kw.setdefault("soft_target_tau", 0.005)
    kw.setdefault("target_update_period", 5)
    qs, ps = [(256, O + A), (256, 256), (1, 256)], [(256, O), (256, 256), (A, 256), (A, 256)]
    nets = OrderedDict()
    for name in ("qf1", "qf2", "target_qf1", "target_qf2"):
        nets[name] = layers_from_flat(flats.get(name, flats[name.replace("target_", "")]), qs)
    nets["policy"] = layers_from_flat(flats["policy"], ps)
    noise_seed = kw.pop("noise_seed", 0)
    oracle = RlkitEquivalentSAC(nets, A, **kw)
    twin = RlkitEquivalentSAC(nets, A, dtype=torch.float64, **kw) if with_f64 else None
    pol = TanhGaussianPolicy([256, 256], O, A)
    pol.load_flat(flat_of(nets["policy"]))
    qn = [FlattenMlp([256, 256], 1, O + A) for _ in range(4)]
    for q, name in zip(qn, ("qf1", "qf2", "target_qf1", "target_qf2")):
        q.load_flat(flat_of(nets[name]))
    hip = SACTrainer(policy=pol, qf1=qn[0], qf2=qn[1], target_qf1=qn[2], target_qf2=qn[3], batch_size=B,
                     device=device, noise_seed=noise_seed, **kw)
    return (oracle, hip, twin) if with_f64 else (oracle, hip)


def make_td3_pair(O, A, B, seed=3, device=0, with_f64=False, nets=None, **kw):
    """A TD3 oracle and a HIP TD3 trainer holding identical parameters (with_f64: and the oracle's float64 twin, third;
    nets: these parameters instead of init_td3_params')."""
    from oracle.td3_step_torch import RlkitEquivalentTD3, init_td3_params
    from robosuite_benchmark_amd import FlattenMlp, TanhMlpPolicy, TD3Trainer
    kw.setdefault("policy_learning_rate", 1e-3)
    kw.setdefault("qf_learning_rate", 5e-4)
    hidden = tuple(kw.pop("hidden", (256, 256)))
    nets = nets or init_td3_params(O, A, hidden=hidden, seed=seed)
    noise_seed = kw.pop("noise_seed", 0)
    oracle = RlkitEquivalentTD3(nets, A, **kw)
    twin = RlkitEquivalentTD3(nets, A, dtype=torch.float64, **kw) if with_f64 else None
    pols = [TanhMlpPolicy(list(hidden), A, O) for _ in range(2)]
    qs = [FlattenMlp(list(hidden), 1, O + A) for _ in range(4)]
    for p, name in zip(pols, ("policy", "target_policy")):
        p.load_flat(flat_of(nets[name]))
    for q, name in zip(qs, ("qf1", "qf2", "target_qf1", "target_qf2")):
        q.load_flat(flat_of(nets[name]))
    hip = TD3Trainer(policy=pols[0], qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3], target_policy=pols[1],
                     batch_size=B, device=device, noise_seed=noise_seed, **kw)
    return (oracle, hip, twin) if with_f64 else (oracle, hip)


# ---- per-tensor comparison against the float64 oracle ------------------------------------------------------------------
# For every tensor, with R the float64 oracle's value, P the float32 oracle's and K the kernel's, s = max|R|:
#     max|K - R| / s  <=  max(F64_FACTOR * max|P - R| / s, F64_FLOOR)
# and K == 0 exactly where R is exactly 0.  The fp32 oracle's own distance to float64 carries the conditioning of each
# tensor (saturated tanh rows, cancelling sums); the floor is what fp32 arithmetic in another order costs at init.
F64_FACTOR, F64_FLOOR = 8.0, 1e-5
F64_ERRORS = {}             # path -> (largest kernel error seen, max|K - R| / s; its tensor; the fp32 oracle's), for reporting


def _np64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().numpy()
    return np.asarray(x, np.float64).ravel()


def check_f64(name, got, p32, r64, path=None, scale=None, factor=F64_FACTOR, floor=F64_FLOOR):
    """Assert the per-tensor rule above for one tensor (`scale`: s when it is not max|R|); returns the kernel's error."""
    K, P, R = _np64(got), _np64(p32), _np64(r64)
    assert K.shape == R.shape == P.shape, (name, K.shape, P.shape, R.shape)
    s = float(np.max(np.abs(R))) if scale is None else float(scale)
    return check_f64_e32(name, K, R, s, float(np.max(np.abs(P - R))) / s if s else 0.0, path, factor, floor)


def check_f64_e32(name, got, r64, s, e32, path=None, factor=F64_FACTOR, floor=F64_FLOOR):
    """The per-tensor rule with the fp32 oracle's error given as a number: s = max|R| (or the tensor's stated scale) and
    e32 = max|P - R| / s, computed when R was (check_f64: now; a frozen fixture: when it was written, over the whole
    tensor, of which `got` and `r64` may be the same sample).  Returns the kernel's error."""
    K, R = _np64(got), _np64(r64)
    assert K.shape == R.shape, (name, K.shape, R.shape)
    if s == 0.0:
        assert np.all(K == 0.0), f"{name}: the float64 reference is exactly 0, the kernel has max|K| = {np.max(np.abs(K)):.3g}"
        return 0.0
    eK, eP = float(np.max(np.abs(K - R))) / s, float(e32)
    if path is not None and eK >= F64_ERRORS.get(path, (0.0,))[0]:
        F64_ERRORS[path] = (eK, name, eP)
    bound = max(factor * eP, floor)
    assert eK <= bound, f"{name}: kernel error {eK:.3g} of max|R| = {s:.3g} > {bound:.3g} (fp32 oracle: {eP:.3g})"
    return eK


def layer_names(n_layers, heads):
    """fc0, fc1, ... for the hidden layers, then the heads' names."""
    return [f"fc{i}" for i in range(n_layers - len(heads))] + list(heads)


NET_HEADS = {"sac_policy": ("last_fc", "last_fc_log_std"), "td3_policy": ("last_fc",), "q": ("last_fc",)}


def named_tensors(flat, shapes, names, prefix):
    """Flat vector in library layout (W0 b0 W1 b1 ...) -> {"<prefix> fc0.weight": W0, "<prefix> fc0.bias": b0, ...}."""
    flat = np.asarray(flat).ravel()
    out, off = OrderedDict(), 0
    for (n, k), nm in zip(shapes, names):
        out[f"{prefix} {nm}.weight"] = flat[off:off + n * k].reshape(n, k); off += n * k
        out[f"{prefix} {nm}.bias"] = flat[off:off + n]; off += n
    assert off == flat.size, (prefix, off, flat.size)
    return out


def oracle_flat_grad(g):
    """An oracle gradient in library layout: SAC keeps [W0, W1, ..., b0, b1, ...], TD3 the flat vector already."""
    if isinstance(g, np.ndarray):
        return g
    nl = len(g) // 2
    return np.concatenate([np.concatenate([np.ravel(g[l]), np.ravel(g[nl + l])]) for l in range(nl)])


def _net_info(oracle, net):
    m = getattr(oracle, net)
    shapes = [tuple(w.shape) for w in m.ws]
    heads = NET_HEADS["q"] if net.startswith("qf") else NET_HEADS["td3_policy" if hasattr(oracle, "target_policy") else "sac_policy"]
    return shapes, layer_names(len(shapes), heads)


def check_grads_f64(hip, o32, o64, path, nets=("policy", "qf1", "qf2")):
    """Every weight and bias gradient of `nets` after one step from identical state, per tensor."""
    for net in nets:
        shapes, names = _net_info(o32, net)
        R = named_tensors(oracle_flat_grad(o64.last["g_" + net]), shapes, names, net)
        P = named_tensors(oracle_flat_grad(o32.last["g_" + net]), shapes, names, net)
        K = named_tensors(hip.debug_fetch("g_" + net, sum(n * k + n for n, k in shapes)), shapes, names, net)
        for key in R:
            check_f64("gradient of " + key, K[key], P[key], R[key], path)


# debug_fetch name -> oracle.last key of the per-row outputs
SAC_ROWS = {"q1": "q1", "q2": "q2", "q1_new": "q1_new", "q2_new": "q2_new", "q_target": "y", "log_pi": "log_pi",
            "log_pi_next": "log_pi2", "a_new": "a_new", "mu": "mu", "log_std": "log_std", "a_next": "a2"}
TD3_ROWS = {"q1": "q1", "q2": "q2", "q_target": "y", "tq1": "tq1", "tq2": "tq2", "q1_new": "q_pi", "a_new": "pa",
            "a_next": "noisy"}


def check_rows_f64(hip, o32, o64, path, skip=()):
    rows = TD3_ROWS if hasattr(o32, "target_policy") else SAC_ROWS
    for name, key in rows.items():
        if name in skip:
            continue
        R = _np64(o64.last[key])
        check_f64(name, hip.debug_fetch(name, R.size), o32.last[key], R, path)


def _row_quantities(o, td3):
    """The per-row values each logged statistic / loss summarises (its scale is their max |.|)."""
    L = o.last
    q = {"Q1 Predictions": L["q1"], "Q2 Predictions": L["q2"], "Q Targets": L["y"]}
    if td3:
        q.update({"Bellman Errors 1": (L["q1"] - L["y"]) ** 2, "Bellman Errors 2": (L["q2"] - L["y"]) ** 2,
                  "Policy Action": L["pa"], "QF1 Loss": (L["q1"] - L["y"]) ** 2, "QF2 Loss": (L["q2"] - L["y"]) ** 2,
                  "Policy Loss": -L["q_pi"]})
    else:
        q_new = torch.min(L["q1_new"], L["q2_new"])
        alpha = float(o.log_alpha.detach().exp()) if o.auto_alpha else 1.0
        q.update({"Log Pis": L["log_pi"], "Policy mu": L["mu"], "Policy log std": L["log_std"],
                  "QF1 Loss": (L["q1"] - L["y"]) ** 2, "QF2 Loss": (L["q2"] - L["y"]) ** 2,
                  "Policy Loss": L["log_pi"] - q_new, "Actor Loss": alpha * L["log_pi"] - q_new})
    return {k: float(np.max(np.abs(_np64(v)))) for k, v in q.items()}


def check_diag_f64(diag, names, want32, want64, o64, path):
    """Every diagnostic of one step: a statistic at the scale of its rows, Alpha / Alpha Loss at their own."""
    scales = diag_scales(want64, o64)
    for i, name in enumerate(names):
        if name not in want64:
            continue
        check_f64(name, [diag[i]], [want32[name]], [want64[name]], path, scale=scales[name])


def diag_scales(want64, o64):
    """{diagnostic: its scale}: a statistic's is the largest |.| of the rows it summarises, Alpha's / Alpha Loss's their own."""
    scales = _row_quantities(o64, hasattr(o64, "target_policy"))
    out = {}
    for name in want64:
        quantity = name.rsplit(" ", 1)[0] if name.rsplit(" ", 1)[-1] in ("Mean", "Std", "Max", "Min") else name
        out[name] = scales.get(quantity, abs(want64[name]))
    return out


def check_step_f64(hip, o32, o64, diag, want32, want64, path=None, skip_rows=()):
    """Gradients, per-row outputs and diagnostics of one step from identical state against the float64 oracle."""
    from robosuite_benchmark_amd._lib import DIAG_NAMES, TD3_DIAG_NAMES
    td3 = hasattr(o32, "target_policy")
    path = path or f"{'td3' if td3 else 'sac'} kind {hip.fused_mode()}"
    check_grads_f64(hip, o32, o64, path, nets=("qf1", "qf2") + (("policy",) if not td3 or o32.last["policy_step"] else ()))
    check_rows_f64(hip, o32, o64, path, skip=skip_rows)
    check_diag_f64(diag, TD3_DIAG_NAMES if td3 else DIAG_NAMES, want32, want64, o64, path)


# ---- what a step writes back: Adam, Polyak and the entropy coefficient against a float64 restatement -------------------
def _adam_f32(p, m, v, g, lr, t):
    """torch.optim.Adam (fp32 tensors, double bias corrections) restated in NumPy float32."""
    f = np.float32
    m = m + f(1.0 - 0.9) * (g - m)                                  # exp_avg.lerp_(grad, 1 - beta1)
    v = v * f(0.999) + f(1.0 - 0.999) * g * g                       # mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    bc1, bc2s = 1.0 - 0.9 ** t, np.sqrt(1.0 - 0.999 ** t)
    denom = np.sqrt(v) / f(bc2s) + f(1e-8)
    p = p + (f(-(lr / bc1)) * m) / denom                            # addcdiv_(exp_avg, denom, value=-step_size)
    return p.astype(f), m.astype(f), v.astype(f)


U32 = 2.0 ** -24                     # unit roundoff of float32: |fl(x) - x| <= U32 |x| (normal range)
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def _f(x):
    """A double scalar as torch applies it to float32 tensors: rounded to float32 once."""
    return float(np.float32(x))


def adam_scalars(lr, t):
    """The float32 scalars of torch Adam at optimizer step t (1-based): 1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2),
    eps.  torch forms bias corrections and step size in double and each reaches the tensor ops as one float32."""
    b1, b2 = ADAM_BETAS
    bc1, bc2s = 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5
    return _f(1.0 - b1), _f(b2), _f(1.0 - b2), _f(lr / bc1), _f(bc2s), _f(ADAM_EPS)


def adam_moments_ref(m0, v0, g, t):
    """exp_avg.lerp_(g, 1 - beta1) and exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2) in float64."""
    c1, b2, c2 = adam_scalars(0.0, t)[:3]
    m0, v0, g = (np.asarray(x, np.float64) for x in (m0, v0, g))
    return m0 + c1 * (g - m0), v0 * b2 + c2 * g * g


def adam_param_ref(p0, m, v, lr, t):
    """param.addcdiv_(m, sqrt(v) / sqrt(bc2) + eps, value=-lr / bc1) in float64, from the moments AFTER the step.
    Returns the new parameter and the update it added."""
    _, _, _, ss, bc2s, eps = adam_scalars(lr, t)
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    d = (-ss * m) / (np.sqrt(v) / bc2s + eps)
    return np.asarray(p0, np.float64) + d, d


def adam_ref(p0, m0, v0, g, lr, t):
    """One step of torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, no weight decay) at optimizer step t, in float64 from
    float32 inputs with torch's float32 scalars: (p, m, v)."""
    m, v = adam_moments_ref(m0, v0, g, t)
    return adam_param_ref(p0, m, v, lr, t)[0], m, v


def polyak_ref(t_old, p_new, tau):
    """rlkit soft_update_from_to: target * (1 - tau) + param * tau, float64 with the two float32 scalars."""
    return np.asarray(t_old, np.float64) * _f(1.0 - tau) + np.asarray(p_new, np.float64) * _f(tau)


def alpha_grad_ref(log_pi, target_entropy):
    """d/d log_alpha of -(log_alpha * (log_pi + H)).mean() = -mean(log_pi + H), float64 over the B rows."""
    return -float(np.mean(np.asarray(log_pi, np.float64) + float(np.float32(target_entropy))))


def alpha_ref(log_alpha, a_m, a_v, log_pi, target_entropy, lr, t):
    """One Adam step of log_alpha (torch Adam on a 0-dim float32 tensor) on the gradient of mean(log_pi + H):
    (log_alpha, exp_avg, exp_avg_sq, gradient)."""
    gr = alpha_grad_ref(log_pi, target_entropy)
    p, m, v = adam_ref(log_alpha, a_m, a_v, gr, lr, t)
    return float(p), float(m), float(v), gr


def ulp32(x):
    """The float32 ulp at |x| (the spacing above the float32 nearest to |x|; 2^-149 at 0)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def ulp_distance(got, ref):
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / ulp32(ref)


OPT_ULPS = {}               # path -> {quantity: largest |K - R| / ulp(R) seen, "<quantity> of bound": largest |K - R| / bound}


def _within(what, got, ref, bound, path, quantity):
    """Assert |K - R| <= bound per element; record the largest ulp distance of (path, quantity)."""
    K, R = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert K.shape == R.shape, (what, K.shape, R.shape)
    bound = np.broadcast_to(np.asarray(bound, np.float64), R.shape).ravel()
    K, R = K.ravel(), R.ravel()
    ul = ulp_distance(K, R)
    if ul.size:
        rec = OPT_ULPS.setdefault(path, {})
        rec[quantity] = max(rec.get(quantity, 0.0), float(np.max(ul)))
        use = np.abs(K - R) / np.maximum(bound, 1e-300)
        rec[quantity + " of bound"] = max(rec.get(quantity + " of bound", 0.0), float(np.max(use)))
    bad = ~(np.abs(K - R) <= bound)                     # (NaN counts as bad)
    if np.any(bad):
        i = int(np.argmax(np.where(bad, ul, -1.0)))
        raise AssertionError(f"{path}: {what}: {int(bad.sum())} of {R.size} elements beyond the bound; worst at [{i}]: "
                             f"kernel {K[i]:.9g}, reference {R[i]:.9g} ({ul[i]:.3g} ulp, bound {bound[i] / ulp32(R[i]):.3g} ulp)")


def _bit_equal(what, got, want, path):
    a, b = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    same = a.view(np.uint32) == b.view(np.uint32)
    assert np.all(same), f"{path}: {what} must be bit-unchanged: {int((~same).sum())} of {a.size} elements differ"


def optimizer_cfg(hip):
    """What check_optimizer_step needs of a SACTrainer / TD3Trainer, from its host attributes only."""
    td3 = hasattr(hip, "target_policy")
    O, A = hip.obs_dim, hip.act_dim
    hp = [int(h) for h in hip.policy.hidden_sizes]
    hq = [int(h) for h in hip.qf1.hidden_sizes]

    def mlp(k, hs, heads):
        dims = [k] + hs
        return [(dims[i + 1], dims[i]) for i in range(len(hs))] + [(n, hs[-1]) for n in heads]

    pol = mlp(O, hp, [A] if td3 else [A, A])
    q = mlp(O + A, hq, [1])
    nets = {"policy": (pol, layer_names(len(pol), NET_HEADS["td3_policy" if td3 else "sac_policy"])),
            "qf1": (q, layer_names(len(q), NET_HEADS["q"])), "qf2": (q, layer_names(len(q), NET_HEADS["q"]))}
    if td3:
        return dict(td3=True, nets=nets, B=hip._batch, lr={"policy": hip.policy_learning_rate, "qf1": hip.qf_learning_rate,
                    "qf2": hip.qf_learning_rate}, tau=hip.tau, period=hip.policy_and_target_update_period,
                    targets={"target_qf1": "qf1", "target_qf2": "qf2", "target_policy": "policy"})
    return dict(td3=False, nets=nets, B=hip._batch, lr={"policy": hip.policy_lr, "qf1": hip.qf_lr, "qf2": hip.qf_lr},
                tau=hip.soft_target_tau, period=hip.target_update_period, targets={"target_qf1": "qf1", "target_qf2": "qf2"},
                auto_alpha=hip.use_automatic_entropy_tuning, target_entropy=hip.target_entropy, alpha_lr=hip.policy_lr)


def check_optimizer_step(hip, before, after, cfg, path):
    """What one stepwise train(batch, eps=...) wrote back -- parameters, Adam moments, Polyak targets, log_alpha and its
    Adam state, counters -- per named tensor, each quantity from the kernel's OWN inputs to its stage (so errors do not
    compound): `before` / `after` are state_dict()s around the step, `hip` the trainer (debug_fetch "g_*", "log_pi").

    Bounds, u = 2^-24 the float32 unit roundoff, ulp(R) >= u |R| at the float64 reference R:
      m = m0 + c1 (g - m0): fl(g - m0), fl(c1 .), fl(m0 + .) (a fused multiply-add drops one) -- at most 1/2 ulp(R) for the
        last rounding and u |c1 (g - m0)| for the two inside, where (g - m0) may cancel against m0.  Bound: 2 ulp(R) +
        2 u |c1 (g - m0)|.
      v = v0 b2 + c2 g g: every term >= 0, so four roundings stay inside 2 u |R| <= 2 ulp(R).  Bound: 2 ulp(R).
      p = p0 + d, d = (-s m) / (sqrt(v) / bc2s + eps) from the kernel's own m and v: the float32 step size s (one rounding
        of lr / bc1 in double; the kernel's float lr may move it one more), the product, the square root (1 ulp where it is
        not correctly rounded), the scaling, eps and the quotient put at most ~4.5 u |d| into d, and the sum rounds once.
        Bound: 1 ulp(R) + 6 u |d|.
      target = t (1 - tau) + p tau from `before`'s target and the kernel's own new p: the scalar 1 - tau (one more
        rounding where it is formed in float32), two products and the sum.  Bound: 1 ulp(R) + 2 u (|t (1 - tau)| + |p tau|).
      log_alpha: gr = -mean(log_pi + H) summed in float32 over B rows -- at most (B + 4) u (mean|log_pi| + |H|) =: E from
        the float64 value (recursive summation of B terms, the division, adding H).  a_m: the m bound + c1 E; a_v: 2 ulp(R)
        + c2 E (2 |gr| + E); log_alpha from the kernel's own a_m, a_v: the p bound; Alpha = exp(log_alpha) to 2 ulp.
    Exact: where g == 0 and m0 == v0 == 0, p stays bit-unchanged and m, v stay 0; with lr == 0, p stays bit-unchanged.
    A target off its period, the TD3 policy and its moments off a policy step stay bit-unchanged; without automatic
    entropy tuning so do log_alpha, a_m and a_v, and Alpha is 1."""
    td3 = cfg["td3"]
    sb, sa = np.asarray(before["scalars"], np.float64), np.asarray(after["scalars"], np.float64)
    n0, t0 = int(sb[4]), int(sb[3])
    step = f"step {n0}"
    assert sa[4] == n0 + 1 and sa[3] == t0 + 1, (path, step, "counters", sb, sa)
    avg = n0 % cfg["period"] == 0                        # rlkit: soft update where _n_train_steps_total % period == 0
    t_of = {"qf1": t0 + 1, "qf2": t0 + 1, "policy": t0 + 1}
    trained = ["qf1", "qf2", "policy"]
    if td3:
        tp0 = int(sb[0])                                 # TD3: scalars[0] counts the (delayed) policy's optimizer steps
        assert sa[0] == tp0 + (1 if avg else 0), (path, step, "adam_t_pi", sb, sa)
        t_of["policy"] = tp0 + 1
        if not avg:
            trained = ["qf1", "qf2"]
            _bit_equal(f"{step} policy (no policy step)", after["params"]["policy"], before["params"]["policy"], path)
            for i, q in enumerate(("m", "v")):
                _bit_equal(f"{step} policy {q} (no policy step)", after["opt"]["policy"][i], before["opt"]["policy"][i],
                           path)
    for net in trained:
        shapes, names = cfg["nets"][net]
        lr, t = cfg["lr"][net], t_of[net]
        c1 = adam_scalars(lr, t)[0]
        n = sum(a * b + a for a, b in shapes)
        T = lambda x: named_tensors(np.asarray(x), shapes, names, net)     # noqa: E731
        P0, M0, V0 = T(before["params"][net]), T(before["opt"][net][0]), T(before["opt"][net][1])
        P1, M1, V1 = T(after["params"][net]), T(after["opt"][net][0]), T(after["opt"][net][1])
        G = T(hip.debug_fetch("g_" + net, n))
        for k in P0:
            g, m0, v0 = (x[k].astype(np.float64) for x in (G, M0, V0))
            mr, vr = adam_moments_ref(m0, v0, g, t)
            _within(f"{step} exp_avg of {k} (t = {t})", M1[k], mr, 2 * ulp32(mr) + 2 * U32 * np.abs(c1 * (g - m0)), path,
                    "m")
            _within(f"{step} exp_avg_sq of {k} (t = {t})", V1[k], vr, 2 * ulp32(vr), path, "v")
            pr, d = adam_param_ref(P0[k], M1[k], V1[k], lr, t)
            _within(f"{step} {k} (t = {t})", P1[k], pr, ulp32(pr) + 6 * U32 * np.abs(d), path, "p")
            z = (g == 0) & (m0 == 0) & (v0 == 0)
            if np.any(z):                                # (a moment of -0 may come back +0: m0 + c1 (0 - m0))
                _bit_equal(f"{step} {k} where g == m0 == v0 == 0", P1[k][z], P0[k][z], path)
                assert np.all(M1[k][z] == 0) and np.all(V1[k][z] == 0), f"{path}: {step} {k}: moments must stay 0 where g == m0 == v0 == 0"

            if lr == 0:
                _bit_equal(f"{step} {k} at lr 0", P1[k], P0[k], path)
    for tgt, src in cfg["targets"].items():
        if src not in trained:
            _bit_equal(f"{step} {tgt} (no policy step)", after["params"][tgt], before["params"][tgt], path)
            continue
        if not avg:
            _bit_equal(f"{step} {tgt} (off its period {cfg['period']})", after["params"][tgt], before["params"][tgt], path)
            continue
        shapes, names = cfg["nets"][src]
        T = lambda x: named_tensors(np.asarray(x), shapes, names, tgt)     # noqa: E731
        T0, T1, P1 = T(before["params"][tgt]), T(after["params"][tgt]), T(after["params"][src])
        tau = cfg["tau"]
        for k in T0:
            r = polyak_ref(T0[k], P1[k], tau)
            t64, p64 = T0[k].astype(np.float64), P1[k].astype(np.float64)
            b = ulp32(r) + 2 * U32 * (np.abs(t64 * _f(1 - tau)) + np.abs(p64 * _f(tau)))
            _within(f"{step} {k} (Polyak, tau {tau})", T1[k], r, b, path, "target")
    if td3:
        return
    la0, am0, av0 = (float(np.float32(x)) for x in sb[:3])
    la1, am1, av1, alpha = (float(np.float32(x)) for x in sa[(0, 1, 2, 5),])
    if not cfg["auto_alpha"]:
        _bit_equal(f"{step} log_alpha, a_m, a_v (fixed alpha)", [la1, am1, av1], [la0, am0, av0], path)
        assert alpha == 1.0, (path, step, "Alpha with fixed alpha", alpha)
        return
    t = t0 + 1
    lp = hip.debug_fetch("log_pi", cfg["B"])
    H = float(np.float32(cfg["target_entropy"]))
    E = (cfg["B"] + 4) * U32 * (float(np.mean(np.abs(lp.astype(np.float64)))) + abs(H))
    c1, _, c2 = adam_scalars(0.0, t)[:3]
    gr = alpha_grad_ref(lp, H)
    mr, vr = adam_moments_ref(am0, av0, gr, t)
    _within(f"{step} log_alpha exp_avg (t = {t})", am1, mr, 2 * ulp32(mr) + 2 * U32 * abs(c1 * (gr - am0)) + c1 * E, path,
            "a_m")
    _within(f"{step} log_alpha exp_avg_sq (t = {t})", av1, vr, 2 * ulp32(vr) + c2 * E * (2 * abs(gr) + E), path, "a_v")
    pr, d = adam_param_ref(la0, am1, av1, cfg["alpha_lr"], t)
    _within(f"{step} log_alpha (t = {t})", la1, pr, ulp32(pr) + 6 * U32 * np.abs(d), path, "log_alpha")
    ea = np.float32(np.exp(la1))
    assert ulp_distance(alpha, ea) <= 2, (path, step, "Alpha != exp(log_alpha)", alpha, float(ea))
    rec = OPT_ULPS.setdefault(path, {})
    rec["alpha"] = max(rec.get("alpha", 0.0), float(ulp_distance(alpha, ea)))


# ---- trainers and buffers several GPU test files share -------------------------------------------------------------------
def pair_of_hip(O, A, B, seed, noise_seed, **env):
    """(fused, four-launch) trainers with identical parameters."""
    old = {k: os.environ.get(k) for k in ("SAC_FUSED", "SAC_FUSED_TEST_STALL")}
    try:
        os.environ.pop("SAC_FUSED", None)
        for k, v in env.items():
            os.environ[k] = str(v)
        _, fused = make_pair(O, A, B, seed=seed, noise_seed=noise_seed)
        os.environ.pop("SAC_FUSED_TEST_STALL", None)
        os.environ["SAC_FUSED"] = "0"
        _, plain = make_pair(O, A, B, seed=seed, noise_seed=noise_seed)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return fused, plain


def _td3_pair_of_hip(O, A, B, seed, noise_seed, **env):
    """(fused critic pass, four-launch critic pass) TD3 trainers with identical parameters."""
    old = {k: os.environ.get(k) for k in ("SAC_FUSED", "SAC_FUSED_TEST_STALL")}
    try:
        os.environ.pop("SAC_FUSED", None)
        for k, v in env.items():
            os.environ[k] = str(v)
        _, fused = make_td3_pair(O, A, B, seed=seed, noise_seed=noise_seed)
        os.environ.pop("SAC_FUSED_TEST_STALL", None)
        os.environ["SAC_FUSED"] = "0"
        _, plain = make_td3_pair(O, A, B, seed=seed, noise_seed=noise_seed)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return fused, plain


def plain_buffer(n, O, A, seed):
    from robosuite_benchmark_amd import EnvReplayBuffer
    obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=seed, term_frac=0.05)
    buf = EnvReplayBuffer(n, obs_dim=O, action_dim=A)
    buf.add_block(obs, act, rew, nobs, term)
    return buf


def filled_buffer(n, O, A, seed):
    from robosuite_benchmark_amd import EnvReplayBuffer
    obs, act, rew, term, nobs = synth_transitions(n, O, A, seed=seed, term_frac=0.1)
    buf = EnvReplayBuffer(n, obs_dim=O, action_dim=A)
    buf.add_block(obs, act, rew, nobs, term)
    buf.seed(seed)
    return buf


# ---- acting: the policy's forward against oracle.sac_step_torch.PolicyNet ----------------------------------------------
def act_reference(layers, td3, obs, deterministic, eps, dtype):
    """policy.get_actions of the oracle: tanh(mean) or tanh(mean + exp(clamp(log_std)) * eps) on `layers` (the oracle's
    layer list; TD3: the TanhMlpPolicy's, tanh(last_fc)) in `dtype`."""
    from oracle.sac_step_torch import PolicyNet
    if td3:                                         # TanhMlpPolicy = PolicyNet's mean head (its log_std head is unused)
        layers, deterministic = list(layers) + [layers[-1]], True
    net = PolicyNet(layers, dtype=dtype)
    with torch.no_grad():
        mean, log_std = net.trunk(torch.from_numpy(obs).to(dtype))
        z = mean if deterministic else mean + torch.exp(log_std) * torch.from_numpy(eps).to(dtype)
        return torch.tanh(z).numpy()


ACT_ATOL, ACT_F64_FACTOR = 2e-5, 8.0        # the constants of test_gpu_device_acting.check_against_oracle
ACT_ERRORS = {}             # tag -> [largest |K - f64|, the fp32 oracle's |P - f64| of that call, the call], for reporting


def check_act(trainer, got, layers, obs, det, eps, where, tag=None):
    """One acting call of either implementation (k_act or the host forward) against PolicyNet on `layers`:
    max|K - R| <= max(2e-5, 8 max|P - R|) with R the float64 and P the fp32 oracle, and atol 2e-5 against P.  The
    second holds only where the fp32 oracle is well conditioned, 8 max|P - R| <= 2e-5: that is asserted first, so the
    fp32 check never drops out silently (tests/test_acting_edges_host.py asserts it for every case of the edge matrix;
    at init and on trained weights P is closer still).  Returns the float64 bound of this call."""
    td3 = "target_policy" in trainer.NETS
    w32, w64 = act_reference(layers, td3, obs, det, eps, torch.float32), act_reference(layers, td3, obs, det, eps, torch.float64)
    e_k32, e_k64 = float(np.max(np.abs(got - w32))), float(np.max(np.abs(got.astype(np.float64) - w64)))
    e_32 = float(np.max(np.abs(w32.astype(np.float64) - w64)))
    print(f"{where}: |K - fp32 oracle| {e_k32:.3g}  |K - f64| {e_k64:.3g}  |fp32 oracle - f64| {e_32:.3g}")
    if tag is not None and not e_k64 < ACT_ERRORS.get(tag, [-1.0])[0]:
        ACT_ERRORS[tag] = [e_k64, e_32, str(where)]
    bound = max(ACT_ATOL, ACT_F64_FACTOR * e_32)
    assert ACT_F64_FACTOR * e_32 <= ACT_ATOL, (where, "the fp32 oracle is not well conditioned here", e_32)
    assert got.shape == w64.shape and np.all(np.isfinite(got)), (where, got.shape)
    assert e_k64 <= bound, (where, e_k64, e_32)
    assert np.allclose(got, w32, atol=ACT_ATOL), (where, e_k32)
    return bound


def is_td3(t):
    return "target_policy" in t.NETS


def draws(rs, n, O, A):
    return rs.normal(0, 0.4, (n, O)).astype(np.float32), rs.normal(size=(n, A)).astype(np.float32)


def act_c(t, obs, deterministic, eps):
    """sac_policy_act_device through the C ABI."""
    from robosuite_benchmark_amd import _lib
    out = np.full((obs.shape[0], t.act_dim), 7.0, np.float32)
    _lib.check(_lib.load().sac_policy_act_device(t._h, obs.shape[0], _lib.ptr(obs), int(deterministic), _lib.ptr(eps),
                                                 _lib.ptr(out)), "sac_policy_act_device")
    return out


ACT_NETS = ("policy", "qf1", "qf2", "target_qf1", "target_qf2")


def full_state(t, buf):
    st = t.state_dict()
    k, p = buf.rng_state()
    return ([st["params"][n] for n in ACT_NETS] + [x for n in ("policy", "qf1", "qf2") for x in st["opt"][n]]
            + [st["scalars"], np.asarray(k), np.asarray([p])])
