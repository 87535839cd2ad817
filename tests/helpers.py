"""Shared helpers for the parity tests (test infrastructure; may import oracle/)."""
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
    oracle's float64 twin, third)."""
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
    if s == 0.0:
        assert np.all(K == 0.0), f"{name}: the float64 reference is exactly 0, the kernel has max|K| = {np.max(np.abs(K)):.3g}"
        return 0.0
    eK, eP = float(np.max(np.abs(K - R))) / s, float(np.max(np.abs(P - R))) / s
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
    scales = _row_quantities(o64, hasattr(o64, "target_policy"))
    for i, name in enumerate(names):
        if name not in want64:
            continue
        quantity = name.rsplit(" ", 1)[0] if name.rsplit(" ", 1)[-1] in ("Mean", "Std", "Max", "Min") else name
        s = scales.get(quantity, abs(want64[name]))
        check_f64(name, [diag[i]], [want32[name]], [want64[name]], path, scale=s)


def check_step_f64(hip, o32, o64, diag, want32, want64, path=None, skip_rows=()):
    """Gradients, per-row outputs and diagnostics of one step from identical state against the float64 oracle."""
    from robosuite_benchmark_amd._lib import DIAG_NAMES, TD3_DIAG_NAMES
    td3 = hasattr(o32, "target_policy")
    path = path or f"{'td3' if td3 else 'sac'} kind {hip.fused_mode()}"
    check_grads_f64(hip, o32, o64, path, nets=("qf1", "qf2") + (("policy",) if not td3 or o32.last["policy_step"] else ()))
    check_rows_f64(hip, o32, o64, path, skip=skip_rows)
    check_diag_f64(diag, TD3_DIAG_NAMES if td3 else DIAG_NAMES, want32, want64, o64, path)
